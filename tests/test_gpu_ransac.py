"""GPU: okvis_fe_ransac against the statement of its sampler and loop (tests/ransac_statement.py) and against the existing solver
entries.  Everything compared here is exact, so no sample is left out of any comparison.

  - samples: over the shapes of the CPU test (n in {s, s+1, 64, 65, 300, 65536} x n_slots in {1, 64, 65, 1024} x three seeds, the
    full product) and across n = 63 / 64 / 65 / 257 and n_slots = 4 / 5 (samples per wave of the three-point kernel), 8 / 9
    (consensus tile), the referee `samples` equal the numpy statement, and the loop's outputs of every one of these jobs equal
    the numpy rule on the job's referee counts and valid;
  - the chain: the returned samples through okvis_fe_sac_solve / okvis_fe_sac_solve_absolute give the referee models, valid and
    counts bit for bit; the numpy loop statement on those counts and valid gives best, iterations, skipped, stop and n_inliers;
    inliers is the row of `scores < threshold` of hypothesis best; model is models[best] byte for byte;
  - runs past the first 64 slots (65, 130 and 1024 slots): the loop kernel carries its state from one step of 64 slots to the
    next; the best and the stop in a later step, a step of one slot, a tie across the edge, skips adding up over nine steps;
  - every stop reason from a scene, the smallest that produces it;
  - end to end: the scenes and seeds of tests/test_ransac_host.py return exactly the true inlier set;
  - independence: a mixed batch of 130 jobs equals each job run alone, the same call twice gives the same bytes, leaving out any
    optional output changes none of the others."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC  # noqa: E402
import ransac_statement as R  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
MAIN = ("best", "n_inliers", "iterations", "skipped", "stop")
REFEREE = ("samples", "valid", "counts", "models")


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


def _bytes(r, names=MAIN + ("inliers", "model") + REFEREE):
    return {k: np.asarray(r[k]).tobytes() for k in names if k in r}


def _solve_entry(fe, job, samples, want_scores=True):
    """the job's hypotheses and counts on these samples through the existing entries"""
    if job["kind"] == RC.ABSOLUTE:
        fields = {k: job[k] for k in ("points", "bearing", "sigma", "cam_index", "cam_offsets", "cam_rotations")}
        return fe.sac_solve_absolute([dict(fields, samples=samples, threshold=job["threshold"])], want_scores=want_scores)[0]
    fields = {k: job[k] for k in ("kind", "bearing1", "bearing2", "sigma1", "sigma2")}
    return fe.sac_solve([dict(fields, samples=samples, threshold=job["threshold"])], want_scores=want_scores)[0]


def _check_against_the_entries(fe, job, got):
    """the whole chain of one job with referee outputs; -> the statement's loop result"""
    n, s = RC.job_n(job), R.SAMPLE_SIZE[job["kind"]]
    assert np.array_equal(got["samples"], R.samples(job["seed"], job["n_slots"], n, s))
    ref = _solve_entry(fe, job, got["samples"])
    assert ref["models"].tobytes() == got["models"].tobytes()
    assert np.array_equal(ref["valid"], got["valid"]) and np.array_equal(ref["counts"], got["counts"])
    want = R.loop(got["counts"], got["valid"], n, s, job["max_iterations"], job["probability"])
    assert {k: got[k] for k in MAIN} == want, (got, want)
    if want["best"] >= 0:
        with np.errstate(invalid="ignore"):
            row = np.nonzero(ref["scores"][want["best"]] < job["threshold"])[0]
        assert np.array_equal(got["inliers"], row) and len(row) == want["n_inliers"]
        assert got["model"].tobytes() == got["models"][want["best"]].tobytes()
    else:
        assert len(got["inliers"]) == 0 and np.isnan(got["model"]).all()
    return want


# ---- samples --------------------------------------------------------------------------------------------------------------------------
def _check_loop(job, got):
    """the loop's outputs of one job against the numpy rule on the job's own referee counts and valid"""
    n, s = RC.job_n(job), R.SAMPLE_SIZE[job["kind"]]
    want = R.loop(got["counts"], got["valid"], n, s, job["max_iterations"], job["probability"])
    assert {k: got[k] for k in MAIN} == want, (got, want)
    return want


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_samples_equal_the_statement(fe, seed):
    """the full product of the CPU test's shapes, one call per seed; the scenes have no geometry behind them, so the loop's
    outputs (checked too, at 1, 64, 65 and 1024 slots) show runs without a consensus and with many invalid samples"""
    shapes = [(kind, n, n_slots) for kind in RC.KINDS for n in RC.sample_sizes(R.SAMPLE_SIZE[kind]) for n_slots in RC.SLOTS]
    if seed == RC.SEEDS[2]:
        shapes += [(kind, n, 9) for kind in RC.KINDS for n in (63, 64, 65, 257)]
        shapes += [(kind, 257, n_slots) for kind in RC.KINDS for n_slots in (4, 5, 8, 9)]
    fields = {(kind, n): RC.random_fields(kind, n, 900 + n) for kind, n, _ in shapes}
    jobs = [RC.ransac_job(kind, fields[kind, n], n_slots=n_slots, seed=seed, max_iterations=50, probability=0.99, threshold=9.0)
            for kind, n, n_slots in shapes]
    longest = 0
    for (kind, n, n_slots), job, got in zip(shapes, jobs, fe.ransac(jobs, want_referee=True)):
        assert np.array_equal(got["samples"], R.samples(seed, n_slots, n, R.SAMPLE_SIZE[kind])), (kind, n, n_slots, seed)
        want = _check_loop(job, got)
        longest = max(longest, want["iterations"] + want["skipped"])
    assert longest > 64          # some of these runs end behind the first 64 slots (test_runs_past_the_first_64_slots has the scenes for it)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
def test_chain_equals_the_existing_entries_and_the_loop_statement(fe, kind):
    job, _ = RC.end_to_end(kind)
    got, = fe.ransac([job], want_referee=True)
    want = _check_against_the_entries(fe, job, got)
    print(f"kind {kind}: {want}")
    small = RC.ransac_job(kind, RC.exact_fields(kind, 65, 31 + kind, outliers=0.3), n_slots=9, seed=5, max_iterations=50, probability=0.99,
                          threshold=9.0)          # a second ballot word of one bit, a second consensus tile of one hypothesis
    _check_against_the_entries(fe, small, fe.ransac([small], want_referee=True)[0])


def _stop_slot(got):
    return got["iterations"] + got["skipped"] - 1          # the slot the run ended at


def test_runs_past_the_first_64_slots(fe):
    """the loop kernel walks 64 slots per step and carries iterations, skips and the best from step to step: runs that end, and
    find their best, behind the first step, against the numpy rule and the existing entries; a batch of them equals each alone"""
    cases = RC.multi_chunk_cases()
    batch = fe.ransac([job for _, job, _ in cases], want_referee=True)
    by_name = {}
    for (name, job, expect), got in zip(cases, batch):
        want = _check_against_the_entries(fe, job, got)
        print(f"{name}: {want}")
        assert got["stop"] == expect["stop"] and _stop_slot(got) >= 64, (name, got)
        assert _bytes(fe.ransac([job], want_referee=True)[0]) == _bytes(got), name
        by_name[name] = got
    g = by_name["best_and_stop_in_the_second_step"]
    assert g["best"] >= 64 and _stop_slot(g) > g["best"]
    g = by_name["max_iterations_in_a_later_step"]
    assert g["iterations"] == 201 and _stop_slot(g) >= 192
    g = by_name["slots_run_out_in_a_step_of_one"]
    assert _stop_slot(g) == 64
    g = by_name["tie_across_the_edge"]
    ties = np.nonzero(g["valid"] & (g["counts"] == g["counts"][g["best"]]))[0]
    assert g["best"] == ties[0] < 64 and ((ties >= 64) & (ties <= _stop_slot(g))).any()          # equal counts behind the edge did not replace it
    g = by_name["skips_add_up_across_steps"]
    assert g["skipped"] == 500 and 0 < g["iterations"] < 51 and _stop_slot(g) >= 512
    assert all(g["valid"][64 * k:64 * k + 64].any() and not g["valid"][64 * k:64 * k + 64].all() for k in range(8))          # both kinds in every step
    g = by_name["all_invalid_past_the_first_step"]
    assert (g["best"], g["iterations"], g["skipped"], _stop_slot(g)) == (-1, 0, 100, 99)


# ---- every stop reason ----------------------------------------------------------------------------------------------------------------
def _scene_job(kind, n, seed, outliers=0.0, **kw):
    return RC.ransac_job(kind, RC.exact_fields(kind, n, seed, outliers), **dict({"n_slots": 64, "max_iterations": 50, "probability": 0.99,
                                                                                  "threshold": 9.0, "seed": 3}, **kw))


@pytest.mark.parametrize("kind", RC.KINDS)
def test_all_inlier_scene_converges_in_one_iteration(fe, kind):
    job = _scene_job(kind, 40, 70 + kind)
    got, = fe.ransac([job], want_referee=True)
    assert got["valid"][0] and got["counts"][0] == 40          # the scene is exact: the first hypothesis explains all of it
    assert (got["stop"], got["iterations"], got["skipped"], got["best"], got["n_inliers"]) == (F.RANSAC_STOP_CONVERGED, 1, 0, 0, 40)
    assert np.array_equal(got["inliers"], np.arange(40))
    _check_against_the_entries(fe, job, got)


@pytest.mark.parametrize("kind", RC.KINDS)
def test_outlier_scene_converges_where_the_statement_does(fe, kind):
    job, truth = RC.end_to_end(kind)
    got, = fe.ransac([job], want_referee=True)
    want = R.loop(got["counts"], got["valid"], 345, R.SAMPLE_SIZE[kind], 50, 0.99)
    assert got["stop"] == F.RANSAC_STOP_CONVERGED and got["iterations"] == want["iterations"] > 1
    assert {k: got[k] for k in MAIN} == want


def test_no_consensus_stops_at_max_iterations(fe):
    job = _scene_job(RC.ROTATION_ONLY, 40, 75, outliers=1.0, max_iterations=5, n_slots=16)          # every bearing is another point's
    got, = fe.ransac([job], want_referee=True)
    assert got["valid"][:6].all()
    assert (got["stop"], got["iterations"], got["skipped"]) == (F.RANSAC_STOP_MAX_ITERATIONS, 6, 0)          # max_iterations + 1
    _check_against_the_entries(fe, job, got)


def test_eight_slots_run_out(fe):
    job = dict(RC.end_to_end(RC.RELATIVE)[0], n_slots=8)          # eight five-point samples at 87 % inliers: the bound needs twelve
    got, = fe.ransac([job], want_referee=True)
    assert got["stop"] == F.RANSAC_STOP_EXHAUSTED and got["iterations"] + got["skipped"] == 8
    _check_against_the_entries(fe, job, got)


def test_all_invalid_samples_stop_on_skips(fe):
    job = _scene_job(RC.ROTATION_ONLY, 40, 76, max_iterations=5)
    job["bearing1"] = np.repeat(job["bearing1"][:1], 40, axis=0)          # every cross product of two of them is zero
    got, = fe.ransac([job], want_referee=True)
    assert not got["valid"].any() and not got["counts"].any() and np.isnan(got["models"]).all()
    assert {k: got[k] for k in MAIN} == {"best": -1, "n_inliers": 0, "iterations": 0, "skipped": 50, "stop": F.RANSAC_STOP_SKIPS}
    assert len(got["inliers"]) == 0 and np.isnan(got["model"]).all()
    _check_against_the_entries(fe, job, got)


@pytest.mark.parametrize("kind", RC.KINDS)
def test_too_few_correspondences(fe, kind):
    s = R.SAMPLE_SIZE[kind]
    job = _scene_job(kind, 40, 77)
    for k in ("points", "bearing", "sigma", "cam_index", "bearing1", "bearing2", "sigma1", "sigma2"):
        if k in job:
            job[k] = job[k][:s - 1]
    got, = fe.ransac([job], want_referee=True)
    assert {k: got[k] for k in MAIN} == {k: R.NO_SAMPLE[k] for k in MAIN}
    assert len(got["inliers"]) == 0 and np.isnan(got["model"]).all()
    assert not got["samples"].any() and not got["counts"].any()          # the referee outputs of such a job are not written


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
def test_end_to_end_returns_exactly_the_true_inliers(fe, kind):
    job, truth = RC.end_to_end(kind)
    got, = fe.ransac([job])
    print(f"kind {kind}: {got['iterations']} iterations, {got['skipped']} skipped, best {got['best']}, stop {got['stop']}")
    assert got["stop"] == F.RANSAC_STOP_CONVERGED and got["n_inliers"] == 300
    assert np.array_equal(got["inliers"], truth)


# ---- independence ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch():
    rng = np.random.default_rng(2024)
    jobs = []
    sizes = [0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 600]
    for j in range(130):
        kind = RC.KINDS[j % 3]
        n = sizes[j // 3] if j < 3 * len(sizes) else int(rng.integers(0, 601))          # every size under every kind
        jobs.append(RC.ransac_job(kind, RC.exact_fields(kind, n, 3000 + j, outliers=(0.0, 0.2, 0.5)[(j // 3) % 3]),
                                  n_slots=int(rng.choice([1, 4, 5, 8, 9, 16, 24])), max_iterations=int(rng.choice([1, 3, 50])),
                                  probability=float(rng.choice([0.5, 0.99])), threshold=9.0, seed=int(rng.integers(0, 2 ** 63))))
    dead = RC.ransac_job(RC.ROTATION_ONLY, RC.exact_fields(RC.ROTATION_ONLY, 50, 4000), n_slots=16, max_iterations=1, probability=0.99,
                          threshold=9.0, seed=9)
    dead["bearing1"] = np.repeat(dead["bearing1"][:1], 50, axis=0)          # all samples invalid: SKIPS at ten
    jobs[40] = dead
    assert any(RC.job_n(j) < R.SAMPLE_SIZE[j["kind"]] for j in jobs) and max(RC.job_n(j) for j in jobs) == 600
    return jobs


def test_batch_equals_each_job_alone_and_repeats(fe, mixed_batch):
    batch = fe.ransac(mixed_batch, want_referee=True)
    again = fe.ransac(mixed_batch, want_referee=True)
    assert [_bytes(a) for a in again] == [_bytes(b) for b in batch]
    stops = set()
    for j, (job, b) in enumerate(zip(mixed_batch, batch)):
        alone, = fe.ransac([job], want_referee=True)
        assert _bytes(alone) == _bytes(b), j
        stops.add(b["stop"])
        if RC.job_n(job) >= R.SAMPLE_SIZE[job["kind"]]:
            want = R.loop(b["counts"], b["valid"], RC.job_n(job), R.SAMPLE_SIZE[job["kind"]], job["max_iterations"], job["probability"])
            assert {k: b[k] for k in MAIN} == want, j
    assert batch[40]["stop"] == F.RANSAC_STOP_SKIPS and batch[40]["skipped"] == 10
    assert stops == set(range(5)), stops
    plain = fe.ransac(mixed_batch)          # without the referee outputs: the counts and the rest stay on the device
    assert [_bytes(p) for p in plain] == [_bytes(b, MAIN + ("inliers", "model")) for b in batch]


def test_leaving_out_an_output_changes_none_of_the_others(fe, mixed_batch):
    jobs = [mixed_batch[j] for j in (17, 40, 60, 61, 62, 0)]          # all kinds, the all-invalid job and one without a sample
    full = fe.ransac(jobs, want_referee=True)
    names = MAIN + ("inliers", "model") + REFEREE
    for left_out in names:
        table, keep, out = F.ransac_job_table(jobs, want_referee=True)
        for t in table:
            setattr(t, left_out, None)
        fe._call("ransac", len(jobs), table)
        for o, want in zip(out, full):
            got = F.ransac_result(o)
            if left_out == "n_inliers":
                got["inliers"] = o["inliers"][:want["n_inliers"]].copy()          # ransac_result cuts the list by the field left out
            rest = tuple(k for k in names if k != left_out)
            assert _bytes(got, rest) == _bytes(want, rest), left_out
