"""Seeded cases of okvis_fe_sac_solve and their stated results, shared by test_sac_solve_host.py and test_gpu_sac_solve.py.

Scene family: rotation 0.01-0.3 rad about a random axis, baseline 0.05-0.5 m, points in x +-2 m, y +-1.5 m, z 2-8 m (frame 1),
exact bearings.  A point of frame 2 is R12 p2 + t12 in frame 1.

The bound on a five-point hypothesis, per sample: d = max(|R - R_st|_F, |t - t_st|) <= 4 max(e64, e_in), with e64 the float64
numpy evaluation's distance to the statement and e_in the largest distance between the statement's result and its result when
every bearing component is multiplied by 1 +- 2^-53, over 8 seeded draws.  A sample whose separation is below 1e-3 or whose
margin is below 1e-6 stays out of the root-count and hypothesis comparison (at most 2 % of a case); it stays in every property
check.

The statement costs about half a second per sample in mpmath, so the samples of a case are stated once per process, on a pool of
worker processes that never see a GPU (spawned, not forked), and the cases share samples: the 130 samples of the large case begin
with the 50 of the middle one, which begin with the single one."""
import concurrent.futures
import functools
import multiprocessing
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sac_solve_statement as S  # noqa: E402

BOUND_FACTOR = 4.0
DRAWS = 8
MAIN_SEED, SMALL_SEED = 20, 21          # n = 400 (1, 50, 130 samples) and n = 8 (one sample)
ORTHO_TOL = 1e-14                        # |R^T R - I|_F, ||t| - 1|: some 45 roundings of unit-size 3-vector products


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene(rng, n, angle=None, baseline=None):
    """-> R12, t12, bearing1 [n][3], bearing2 [n][3]"""
    R = rotation(rng.normal(size=3), rng.uniform(0.01, 0.3) if angle is None else angle)
    t = rng.normal(size=3)
    t *= (rng.uniform(0.05, 0.5) if baseline is None else baseline) / np.linalg.norm(t)
    p1 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], axis=1)
    p2 = (p1 - t) @ R          # R^T (p1 - t)
    return R, t, p1 / np.linalg.norm(p1, axis=1, keepdims=True), p2 / np.linalg.norm(p2, axis=1, keepdims=True)


def samples(rng, n, k, size):
    return np.stack([rng.choice(n, size, replace=False) for _ in range(k)]).astype(np.int32)


def case(seed, n, k):
    """one problem with k samples of each kind; the samples of a smaller k are a prefix of those of a larger one"""
    rng = np.random.default_rng(seed)
    R, t, b1, b2 = scene(rng, n)
    s1, s2 = rng.uniform(0.5e-6, 2e-6, n), rng.uniform(0.5e-6, 2e-6, n)
    q5 = samples(np.random.default_rng(seed + 1000), n, 130, 8)[:k]
    q2 = samples(np.random.default_rng(seed + 2000), n, 130, 2)[:k]
    return {"R": R, "t": t, "bearing1": b1, "bearing2": b2, "sigma1": s1, "sigma2": s2, "samples5": q5, "samples2": q2, "n": n}


def relative_job(c, q5=None, **kw):
    return dict({"kind": 2, "bearing1": c["bearing1"], "bearing2": c["bearing2"], "sigma1": c["sigma1"], "sigma2": c["sigma2"],
                 "samples": c["samples5"] if q5 is None else q5}, **kw)


def rotation_job(c, q2=None, **kw):
    return dict({"kind": 1, "bearing1": c["bearing1"], "bearing2": c["bearing2"], "sigma1": c["sigma1"], "sigma2": c["sigma2"],
                 "samples": c["samples2"] if q2 is None else q2}, **kw)


# ---- the stated results ----------------------------------------------------------------------------------------------------------------
def state_one(args):
    """one sample: the statement, the numpy evaluation, e64 and e_in"""
    f1, f2, s1, s2, seed = args
    st = S.five_point(f1, f2, s1, s2, ctx=S.MP)
    ev = S.five_point(f1, f2, s1, s2, ctx=S.NP)
    out = {k: st[k] for k in ("valid", "R", "t", "n_roots", "essentials", "separation", "margin")}
    out["np"] = {k: ev[k] for k in ("valid", "R", "t", "n_roots", "essentials")}
    out["e64"] = S.pose_distance(ev["R"], ev["t"], st["R"], st["t"]) if st["valid"] and ev["valid"] else np.inf
    e_in = 0.0
    if st["valid"]:
        rng = np.random.default_rng(seed)
        for _ in range(DRAWS):
            g1 = f1 * (1.0 + rng.choice([-1.0, 1.0], f1.shape) * 2.0 ** -53)
            g2 = f2 * (1.0 + rng.choice([-1.0, 1.0], f2.shape) * 2.0 ** -53)
            R, t = S.five_point_near(g1, g2, st)
            e_in = max(e_in, S.pose_distance(R, t, st["R"], st["t"]))
    out["e_in"] = e_in
    out["bound"] = BOUND_FACTOR * max(out["e64"], e_in)
    out["excluded"] = S.excluded(st)
    return out


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        workers = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
        _POOL = concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn"))
    return _POOL


def state(b1, b2, s1, s2, q5, seed=0):
    """the stated results of the samples q5 [k][8], in order"""
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    args = [(b1[q], b2[q], None if s1 is None else np.asarray(s1)[q], None if s2 is None else np.asarray(s2)[q], seed + 7919 * m)
            for m, q in enumerate(np.asarray(q5))]
    if len(args) <= 2:
        return [state_one(a) for a in args]
    return list(pool().map(state_one, args, chunksize=2))


@functools.lru_cache(maxsize=None)
def stated(seed, n, k=None):
    """the stated results of all samples of case(seed, n, .) (130, or 1 for n = 8): stated once, sliced by the callers"""
    c = case(seed, n, 130 if n > 8 else 1)
    return state(c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], c["samples5"], seed)


@functools.lru_cache(maxsize=None)
def most_roots(seed=33, count=20000):
    """-> (case, sample [8]): the first sample with the most real roots among `count` seeded samples of one scene (float64 count)"""
    c = case(seed, 400, 1)
    q = samples(np.random.default_rng(seed + 3000), 400, count, 8)
    roots = S.count_real_roots(c["bearing1"][q[:, :5]], c["bearing2"][q[:, :5]])
    return c, q[int(np.argmax(roots))], int(roots.max())


def pure_rotation_case(seed=41, n=40, k=16):
    rng = np.random.default_rng(seed)
    R, t, b1, b2 = scene(rng, n, baseline=0.0)
    return {"R": R, "t": t, "bearing1": b1, "bearing2": b2, "sigma1": np.full(n, 1e-6), "sigma2": np.full(n, 1e-6),
            "samples5": samples(rng, n, k, 8), "samples2": samples(rng, n, k, 2), "n": n}


def planar_case(seed=42, n=40, k=16):
    """every point on one plane through both camera centres (the plane spanned by the baseline and one more direction)"""
    rng = np.random.default_rng(seed)
    R = rotation(rng.normal(size=3), 0.1)
    t = np.array([0.3, 0.0, 0.0])
    u = np.array([0.0, 0.2, 1.0])
    p1 = np.outer(rng.uniform(-2, 2, n), t / 0.3) + np.outer(rng.uniform(2, 8, n), u)
    p2 = (p1 - t) @ R
    b1, b2 = p1 / np.linalg.norm(p1, axis=1, keepdims=True), p2 / np.linalg.norm(p2, axis=1, keepdims=True)
    return {"R": R, "t": t, "bearing1": b1, "bearing2": b2, "sigma1": np.full(n, 1e-6), "sigma2": np.full(n, 1e-6),
            "samples5": samples(rng, n, k, 8), "samples2": samples(rng, n, k, 2), "n": n}


# seeds under which no gross outlier lies by chance within the threshold of its epipolar plane: test_sac_solve_host.py shows that
# on the float64 statement before the device is asked
E2E_SEEDS = {1: 51, 2: 53}


@functools.lru_cache(maxsize=None)
def end_to_end(kind):
    """300 exact inlier correspondences and 15 % gross outliers (45 random bearing pairs), shuffled; 50 seeded samples.  The
    rotation-only scene has no baseline.  -> (job fields, the true inlier indices ascending)"""
    rng = np.random.default_rng(E2E_SEEDS[kind])
    R, t, b1, b2 = scene(rng, 300, baseline=0.0 if kind == 1 else None)
    o1, o2 = scene(rng, 45)[2], scene(rng, 45)[3]
    rng.shuffle(o2)
    b1, b2 = np.concatenate([b1, o1]), np.concatenate([b2, o2])
    order = rng.permutation(345)
    b1, b2 = b1[order], b2[order]
    truth = np.sort(np.nonzero(order < 300)[0]).astype(np.int32)
    s1, s2 = rng.uniform(0.5e-6, 2e-6, 345), rng.uniform(0.5e-6, 2e-6, 345)
    q = samples(rng, 345, 50, 8 if kind == 2 else 2)
    return {"kind": kind, "bearing1": b1, "bearing2": b2, "sigma1": s1, "sigma2": s2, "samples": q, "threshold": 9.0}, truth


def end_to_end_float64(kind):
    """the float64 statement of the whole rejection: numpy hypotheses, numpy scores, `<` and the first-best rule -> inliers"""
    job, _ = end_to_end(kind)
    b1, b2, s1, s2 = job["bearing1"], job["bearing2"], job["sigma1"], job["sigma2"]
    best, best_set = -1, None
    for q in job["samples"]:
        if kind == 2:
            ev = S.five_point(b1[q], b2[q], s1[q], s2[q], ctx=S.NP)
            sc = S.score_relative(ev["R"], ev["t"], b1, b2, s1, s2) if ev["valid"] else np.full(len(b1), np.nan)
        else:
            R, ok = S.two_point(b1, b2, q[0], q[1])
            sc = S.score_rotation_only(R, b1, b2, s1, s2)
        with np.errstate(invalid="ignore"):
            inl = np.nonzero(sc < job["threshold"])[0]
        if len(inl) > best:
            best, best_set = len(inl), inl.astype(np.int32)
    return best_set


def check_five_point(c, q5, st_list, valid, n_roots, T, Es, label):
    """The comparison and the properties of one case.  Prints the figures, then asserts.  -> (largest d / bound, excluded)"""
    problems, worst, n_ex, worst_res = [], 0.0, 0, 0.0
    for m, st in enumerate(st_list):
        f1, f2 = c["bearing1"][q5[m]], c["bearing2"][q5[m]]
        k = int(n_roots[m])
        if not 0 <= k <= 10:
            problems.append((m, "n_roots", k))
            continue
        E = Es[m][:k]
        if not np.isfinite(E).all() or (k and np.abs(np.linalg.norm(E, axis=1) - 1).max() > 4e-16 * 4):
            problems.append((m, "essentials not unit", E))
        ref = [essential_residuals(e, f1, f2) for e in st["np"]["essentials"]]
        ref_epi, ref_cub = max([r[0] for r in ref], default=0.0), max([r[1] for r in ref], default=0.0)
        for e in E:
            epi, cub = essential_residuals(e, f1, f2)
            worst_res = max(worst_res, epi / ref_epi if ref_epi else np.inf, cub / ref_cub if ref_cub else np.inf)
            if epi > 4 * ref_epi or cub > 4 * ref_cub:
                problems.append((m, "residual", epi, ref_epi, cub, ref_cub))
        if valid[m]:
            R, t = T[m][:, :3], T[m][:, 3]
            if not np.isfinite(T[m]).all() or np.linalg.norm(R.T @ R - np.eye(3)) > ORTHO_TOL or abs(np.linalg.norm(t) - 1) > ORTHO_TOL:
                problems.append((m, "not a pose", T[m]))
        elif not np.isnan(T[m]).all():
            problems.append((m, "invalid but not NaN", T[m]))
        if st["excluded"]:
            n_ex += 1
            continue
        if k != st["n_roots"] or bool(valid[m]) != st["valid"]:
            problems.append((m, "roots / valid", k, st["n_roots"], bool(valid[m]), st["valid"]))
        elif st["valid"]:
            d = S.pose_distance(T[m][:, :3], T[m][:, 3], st["R"], st["t"])
            worst = max(worst, d / st["bound"])
            if d > st["bound"]:
                problems.append((m, "distance", d, st["bound"], st["e64"], st["e_in"]))
            if k and match_essentials(E, st["essentials"]) > 1e3 * st["bound"] + 1e-12:
                problems.append((m, "essentials do not match the statement's", match_essentials(E, st["essentials"])))
    print(f"{label}: {len(st_list)} samples, {n_ex} excluded, largest d / bound {worst:.3f}, largest residual / numpy's {worst_res:.3f}")
    assert n_ex <= S.MAX_EXCLUDED * len(st_list), (label, n_ex)
    assert not problems, (label, problems[:5])
    return worst, n_ex


# ---- the device's (or the probe's) results against them -------------------------------------------------------------------------------
def match_essentials(got, want):
    """got, want [k][9] up to sign and order -> the largest distance of a wanted matrix to its nearest reported one"""
    worst = 0.0
    for w in want:
        worst = max(worst, min(min(np.linalg.norm(g - w), np.linalg.norm(g + w)) for g in got))
    return worst


def essential_residuals(E, f1, f2):
    """(largest |f1^T E f2| over the five correspondences, |2 E E^T E - tr(E E^T) E|_F) of one 3x3"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    epi = max(abs(f1[k] @ E @ f2[k]) for k in range(5))
    return epi, float(np.linalg.norm(2 * E @ E.T @ E - np.trace(E @ E.T) * E))


# ---- the stand-alone probe (tests/sac_solve_probe.cpp) ---------------------------------------------------------------------------------
def build_probe(out_dir):
    exe = os.path.join(str(out_dir), "sac_solve_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(HERE, "sac_solve_probe.cpp"), "-o", exe], check=True)
    return exe


def run_probe(exe, out_dir, b1, b2, s1, s2, q5, q2, tag="p"):
    """-> (valid5, n_roots, models [k][3][4], essentials [k][10][9]), (valid2, R [k][3][3])"""
    b1, b2 = np.ascontiguousarray(b1, np.float64), np.ascontiguousarray(b2, np.float64)
    q5, q2 = np.ascontiguousarray(q5, np.int32).reshape(-1, 8), np.ascontiguousarray(q2, np.int32).reshape(-1, 2)
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    with open(src, "wb") as f:
        np.array([len(b1), len(q5), len(q2), 0 if s1 is None else 1], np.int32).tofile(f)
        b1.tofile(f), b2.tofile(f)
        if s1 is not None:
            np.ascontiguousarray(s1, np.float64).tofile(f), np.ascontiguousarray(s2, np.float64).tofile(f)
        q5.tofile(f), q2.tofile(f)
    subprocess.run([exe, src, dst], check=True)
    raw = np.fromfile(dst, np.float64)
    five, two = raw[:104 * len(q5)].reshape(-1, 104), raw[104 * len(q5):].reshape(-1, 10)
    return ((five[:, 0] != 0, five[:, 1].astype(np.int32), five[:, 2:14].reshape(-1, 3, 4), five[:, 14:].reshape(-1, 10, 9)),
            (two[:, 0] != 0, two[:, 1:].reshape(-1, 3, 3)))
