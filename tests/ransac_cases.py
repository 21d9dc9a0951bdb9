"""Cases of okvis_fe_ransac, shared by test_ransac_host.py and test_gpu_ransac.py: the sampler's shapes, the constructed loop
cases, the scenes (those of sac_solve_cases.py and sac_abs_cases.py with the stated sampler instead of numpy's generator), the
float64 statement of a whole run, and the stand-alone probe (tests/ransac_probe.cpp).

Everything the device is held to here is exact: samples and loop decisions are integers and float64 comparisons stated in
tests/ransac_statement.py, hypotheses and counts are compared bit for bit with the existing entries' on the same samples."""
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ransac_statement as R  # noqa: E402
import sac_abs_cases as AC  # noqa: E402
import sac_abs_statement as AS  # noqa: E402
import sac_solve_cases as SC  # noqa: E402
import sac_solve_statement as SS  # noqa: E402

ABSOLUTE, ROTATION_ONLY, RELATIVE = 0, 1, 2
KINDS = (ABSOLUTE, ROTATION_ONLY, RELATIVE)
SEEDS = (0, 2 ** 64 - 1, 0x243F6A8885A308D3)
SLOTS = (1, 64, 65, 1024)


def sample_sizes(s):
    return (s, s + 1, 64, 65, 300, 65536)


# ---- the constructed loop cases --------------------------------------------------------------------------------------------------------
def first_done(c, n, s, p=0.99, upto=2000):
    """the least it with done(it, c), or None"""
    return next((it for it in range(1, upto) if R.done(it, c, n, s, p)), None)


def loop_cases():
    """-> list of dicts: name, n, s, max_iterations, p, counts, valid and `expect`, the fields of the result the case is built to
    produce (the statement's whole result is what the probe is compared with)"""
    C = R  # the stop constants
    cases = []

    def add(name, n, s, counts, valid=None, max_iterations=50, p=0.99, **expect):
        counts = np.asarray(counts, np.int32)
        valid = np.ones(len(counts), np.int32) if valid is None else np.asarray(valid, np.int32)
        cases.append({"name": name, "n": n, "s": s, "max_iterations": max_iterations, "p": p, "counts": counts, "valid": valid, "expect": expect})

    for s in (2, 4, 8):
        n = 300
        add(f"tie_s{s}", n, s, [150, 150, 150, 149] + [0] * 60, best=0)                      # a tie must not replace the best
        add(f"full_count_first_valid_s{s}", n, s, [7, n, 0, 0], [0, 1, 1, 1], best=1, iterations=1, skipped=1, stop=C.STOP_CONVERGED)
        add(f"all_zero_s{s}", n, s, [0] * 64, best=0, n_inliers=0, iterations=51, stop=C.STOP_MAX_ITERATIONS)
        add(f"exhausted_s{s}", n, s, [3] * 8, best=0, iterations=8, stop=C.STOP_EXHAUSTED)
        add(f"all_invalid_s{s}", n, s, [9] * 64, [0] * 64, max_iterations=5, best=-1, n_inliers=0, iterations=0, skipped=50, stop=C.STOP_SKIPS)
        add(f"all_invalid_too_few_s{s}", n, s, [9] * 49, [0] * 49, max_iterations=5, best=-1, skipped=49, stop=C.STOP_EXHAUSTED)
        add(f"interleaved_s{s}", n, s, [5, 200, 6, 250, 7, 250, 8, 100] * 8, [0, 1] * 32, best=3)
        add(f"skips_after_iterations_s{s}", n, s, [4, 0, 0, 4] + [0] * 30, [1, 0, 0, 1] + [0] * 30, max_iterations=2, best=0, iterations=2,
            skipped=20, stop=C.STOP_SKIPS)
        add(f"max_iterations_1_zero_s{s}", n, s, [0, 0, 0], max_iterations=1, iterations=2, stop=C.STOP_MAX_ITERATIONS)
        add(f"max_iterations_1_full_s{s}", n, s, [n, 0, 0], max_iterations=1, iterations=1, stop=C.STOP_CONVERGED)
        add(f"late_best_s{s}", n, s, [10] * 70 + [n], max_iterations=1000, best=70, iterations=71, stop=C.STOP_CONVERGED)   # past a wave
        # both sides of done: the least count that converges at iteration `it`, and one below it
        for it in (1, 2, 3, 7, 20, 50, 51):
            c = next((c for c in range(n + 1) if R.done(it, c, n, s, 0.99)), None)
            assert c is not None and c > 0 and not R.done(it, c - 1, n, s, 0.99)
            lead = [0] * (it - 1)
            add(f"edge_s{s}_it{it}_at", n, s, lead + [c, 0, 0], max_iterations=60, best=it - 1, iterations=it, stop=C.STOP_CONVERGED)
            add(f"edge_s{s}_it{it}_below", n, s, lead + [c - 1, 0, 0], max_iterations=60)
    return cases


def done_sweep(s, n=300, p=0.99, its=range(1, 53)):
    """every (it, c) of the sweep the decision function is compared over"""
    return [(it, c) for it in its for c in range(n + 1)]


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
SLOTS_E2E = 64
E2E_SEEDS = {ABSOLUTE: 1, ROTATION_ONLY: 1, RELATIVE: 1}          # test_ransac_host.py shows that the float64 run returns the truth


def ransac_job(kind, fields, **kw):
    """a job of Frontend.ransac from the fields of a sac_solve / sac_solve_absolute job"""
    names = (("points", "bearing", "sigma", "cam_index", "cam_offsets", "cam_rotations") if kind == ABSOLUTE else
             ("bearing1", "bearing2", "sigma1", "sigma2"))
    return dict({k: fields[k] for k in names}, kind=kind, **kw)


@functools.lru_cache(maxsize=None)
def end_to_end(kind):
    """the 345-correspondence scenes with 15 % gross outliers -> (job, the true inlier indices ascending)"""
    fields, truth = AC.end_to_end() if kind == ABSOLUTE else SC.end_to_end(kind)
    return ransac_job(kind, fields, threshold=9.0, n_slots=SLOTS_E2E, max_iterations=50, probability=0.99, seed=E2E_SEEDS[kind]), truth


def job_n(job):
    return len(job["points"] if job["kind"] == ABSOLUTE else job["bearing1"])


def slot_float64(job, q):
    """one slot in float64 numpy: the hypothesis of sample q and its scores -> (valid, scores [n])"""
    kind, n = job["kind"], job_n(job)
    if kind == ABSOLUTE:
        ev = AS.gp3p(*AC.sample_inputs(job, q), ctx=AS.NP)
        if not ev["valid"]:
            return False, np.full(n, np.nan)
        return True, AS.score_absolute(ev["R"], ev["t"], job["points"], job["bearing"], job["cam_index"], job["cam_offsets"],
                                       job["cam_rotations"]) / job["sigma"]
    b1, b2, s1, s2 = job["bearing1"], job["bearing2"], job["sigma1"], job["sigma2"]
    if kind == RELATIVE:
        ev = SS.five_point(b1[q], b2[q], s1[q], s2[q], ctx=SS.NP)
        if not ev["valid"]:
            return False, np.full(n, np.nan)
        return True, SS.score_relative(ev["R"], ev["t"], b1, b2, s1, s2)
    Rm, ok = SS.two_point(b1, b2, q[0], q[1])
    return (True, SS.score_rotation_only(Rm, b1, b2, s1, s2)) if ok else (False, np.full(n, np.nan))


def run_float64(job):
    """the float64 statement of a whole run: the stated samples, numpy hypotheses and scores, `<`, the loop rule, slot by slot until
    the rule stops -> the rule's result with `inliers`"""
    n, s = job_n(job), R.SAMPLE_SIZE[job["kind"]]
    if n < s:
        return dict(R.NO_SAMPLE, inliers=np.zeros(0, np.int32))
    q = R.samples(job["seed"], job["n_slots"], n, s)
    counts, valid, sets = [], [], []
    res = None
    for m in range(job["n_slots"]):
        ok, sc = slot_float64(job, q[m])
        with np.errstate(invalid="ignore"):
            inl = np.nonzero(sc < job["threshold"])[0].astype(np.int32)
        counts.append(len(inl)), valid.append(ok), sets.append(inl)
        res = R.loop(counts, valid, n, s, job["max_iterations"], job["probability"])
        if res["stop"] != R.STOP_EXHAUSTED:
            break
    return dict(res, inliers=sets[res["best"]] if res["best"] >= 0 else np.zeros(0, np.int32))


def random_fields(kind, n, seed):
    """n correspondences without any geometry behind them (unit bearings, points in a box): for the sampler's shapes"""
    rng = np.random.default_rng(seed)
    unit = lambda: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    sig = lambda: rng.uniform(0.5e-6, 2e-6, n)
    if kind == ABSOLUTE:
        off, rot = AC.rig(rng, 2)
        return {"points": rng.uniform(-5, 5, (n, 3)), "bearing": unit(), "sigma": sig(), "cam_index": rng.integers(0, 2, n).astype(np.int32),
                "cam_offsets": off, "cam_rotations": rot}
    return {"bearing1": unit(), "bearing2": unit(), "sigma1": sig(), "sigma2": sig()}


def exact_fields(kind, n, seed, outliers=0.0):
    """an exact scene of n correspondences; `outliers`: the fraction (at the end) whose second bearing belongs to another point"""
    rng = np.random.default_rng(seed)
    if kind == ABSOLUTE:
        c = AC.scene(rng, n)
        f = {k: c[k] for k in ("points", "bearing", "cam_index", "cam_offsets", "cam_rotations")}
        f["sigma"], key = rng.uniform(0.5e-6, 2e-6, n), "bearing"
    else:
        _, _, b1, b2 = SC.scene(rng, n, baseline=0.0 if kind == ROTATION_ONLY else None)
        f = {"bearing1": b1, "bearing2": b2, "sigma1": rng.uniform(0.5e-6, 2e-6, n), "sigma2": rng.uniform(0.5e-6, 2e-6, n)}
        key = "bearing2"
    k = int(round(outliers * n))
    if k:
        f[key] = f[key].copy()
        f[key][n - k:] = np.roll(f[key][n - k:], 1, axis=0)
    return f


def multi_chunk_cases():
    """Scenes whose run goes past the first 64 slots, so that the loop kernel's wave carries its state (iterations, skips, best)
    from one step of 64 slots into the next.  -> list of (name, job, expect): `expect` holds the fields of the result the scene was
    chosen for, on the float64 statement (test_ransac_host.py shows that it produces them)."""
    def job(kind, n, scene, outliers, **kw):
        return ransac_job(kind, exact_fields(kind, n, scene, outliers), **dict({"threshold": 9.0, "probability": 0.99}, **kw))

    cases = [
        # 8 inliers of 40: the two-point bound needs 113 iterations; under this seed the first clean sample is slot 84
        ("best_and_stop_in_the_second_step", job(ROTATION_ONLY, 40, 200, 0.8, n_slots=130, max_iterations=1000, seed=18),
         {"best": 84, "iterations": 113, "skipped": 0, "stop": R.STOP_CONVERGED}),
        # 4 inliers of 40: the bound needs 459 iterations, the loop gives up after 201, in the fourth step of sixteen
        ("max_iterations_in_a_later_step", job(ROTATION_ONLY, 40, 201, 0.9, n_slots=1024, max_iterations=200, seed=2),
         {"iterations": 201, "skipped": 0, "stop": R.STOP_MAX_ITERATIONS}),
        # 65 slots: the second step holds one slot; 16 inliers of 40 under the three-point solver never meet the bound in 65
        ("slots_run_out_in_a_step_of_one", job(ABSOLUTE, 40, 202, 0.6, n_slots=65, max_iterations=1000, seed=2),
         {"iterations": 62, "skipped": 3, "stop": R.STOP_EXHAUSTED}),
        # 20 inliers of 40 and p = 1 - 2^-53, so that the bound needs 128 iterations: every clean sample counts 20, in every step;
        # the first of them (slot 5) has to stay the best against the ties behind the edge
        ("tie_across_the_edge", job(ROTATION_ONLY, 40, 203, 0.5, n_slots=130, max_iterations=1000, seed=1, probability=1.0 - 2.0 ** -53),
         {"best": 5, "n_inliers": 20, "iterations": 128, "skipped": 0, "stop": R.STOP_CONVERGED}),
    ]
    # 97 of 100 first bearings equal: 94 % of the samples are invalid, the valid ones lie between them in every step; 500 skips
    # are reached in the ninth step, before 51 iterations
    f = exact_fields(ROTATION_ONLY, 100, 204)
    f["bearing1"] = f["bearing1"].copy()
    f["bearing1"][:97] = f["bearing1"][0]
    cases.append(("skips_add_up_across_steps", ransac_job(ROTATION_ONLY, f, threshold=9.0, probability=0.99, n_slots=1024, max_iterations=50, seed=2),
                  {"best": 103, "iterations": 24, "skipped": 500, "stop": R.STOP_SKIPS}))
    # every sample invalid: 100 skips end the run in the second step
    g = exact_fields(ROTATION_ONLY, 40, 205)
    g["bearing1"] = np.repeat(g["bearing1"][:1], 40, axis=0)
    cases.append(("all_invalid_past_the_first_step", ransac_job(ROTATION_ONLY, g, threshold=9.0, probability=0.99, n_slots=130, max_iterations=10, seed=3),
                  {"best": -1, "n_inliers": 0, "iterations": 0, "skipped": 100, "stop": R.STOP_SKIPS}))
    return cases


# ---- the stand-alone probe (tests/ransac_probe.cpp) ------------------------------------------------------------------------------------
def build_probe(out_dir, sanitize=True):
    """the probe with the sanitizers' runtimes linked statically (the CPU tests), or plain"""
    exe = os.path.join(str(out_dir), "ransac_probe")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, os.path.join(HERE, "ransac_probe.cpp"), "-o", exe], check=True)
    return exe


def run_probe(exe, out_dir, philox=(), sample=(), loop=(), done=(), tag="p"):
    """philox: (counter [4], key [2]); sample: (seed, n, n_slots, s); loop: dicts of loop_cases(); done: (it, c, n, s, p)
    -> (blocks [k][4] uint32, a list of [n_slots][s] int32 arrays, a list of result dicts, decisions [k] bool)"""
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    with open(src, "wb") as f:
        np.array([len(philox), len(sample), len(loop), len(done)], np.int32).tofile(f)
        for ctr, key in philox:
            np.array(list(ctr) + list(key), np.uint32).tofile(f)
        for seed, n, n_slots, s in sample:
            np.array([seed], np.uint64).tofile(f)
            np.array([n, n_slots, s, 0], np.int32).tofile(f)
        for c in loop:
            np.array([c["n"], len(c["counts"]), c["s"], c["max_iterations"]], np.int32).tofile(f)
            np.array([c["p"]], np.float64).tofile(f)
            np.asarray(c["counts"], np.int32).tofile(f), np.asarray(c["valid"], np.int32).tofile(f)
        for it, c, n, s, p in done:
            np.array([it, c, n, s], np.int32).tofile(f)
            np.array([p], np.float64).tofile(f)
    subprocess.run([exe, src, dst], check=True)
    raw = np.fromfile(dst, np.int32)
    at = 4 * len(philox)
    blocks = raw[:at].view(np.uint32).reshape(-1, 4)
    tables = []
    for seed, n, n_slots, s in sample:
        tables.append(raw[at:at + n_slots * s].reshape(n_slots, s))
        at += n_slots * s
    results = [dict(zip(("best", "n_inliers", "iterations", "skipped", "stop"), (int(x) for x in raw[at + 5 * i:at + 5 * i + 5])))
               for i in range(len(loop))]
    at += 5 * len(loop)
    assert len(raw) == at + len(done)
    return blocks, tables, results, raw[at:] != 0
