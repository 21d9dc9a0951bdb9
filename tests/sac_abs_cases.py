"""Seeded cases of okvis_fe_sac_solve_absolute and their stated results, shared by test_sac_abs_host.py and test_gpu_sac_abs.py.

Scene family (the 2D-2D cases' family seen from a rig): the body's pose in the world is a rotation of 0.01-0.3 rad about a
random axis and a translation of 0-3 m; the cameras sit at x = +-0.055 m in the body (eight cameras: between those two) under
random rotations of up to 0.05 rad; every correspondence is a point at x +-2 m, y +-1.5 m, z 2-8 m in its camera (the far scene:
z 50-100 m, x and y in proportion), with the exact bearing.  A body point p is R p + t in the world.

The bound on a hypothesis, per sample: d = max(|R - R_st|_F, |t - t_st|) <= 4 max(e64, e_in), with e64 the float64 numpy
evaluation's distance to the statement and e_in the largest distance between the statement's result and its result when every
component of the sample's bearings and points is multiplied by 1 +- 2^-53, over 8 seeded draws.  A sample whose separation is
below 1e-3 or whose margin is below 1e-6 stays out of the root-count and hypothesis comparison (at most 2 % of a case); it stays
in every property check.

The samples of a case are stated once per process, on a pool of worker processes that never see a GPU (spawned, not forked),
and the cases share samples: the 130 samples of the large case begin with the 50 of the middle one, which begin with the single
one."""
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sac_abs_statement as S  # noqa: E402
from sac_solve_cases import BOUND_FACTOR, DRAWS, ORTHO_TOL, pool, rotation  # noqa: E402

MAIN_SEED, SMALL_SEED, FAR_SEED = 60, 61, 62          # n = 400 (1, 50, 130 samples), n = 4 (one sample), the far scene
MAPPED_TOL = 1e-12          # |R p_k + t - X_k| over max(1, |X_k|, depth): 2^-52 times the few hundred roundings of a candidate and
                            # the 1 / sin of the thinnest triangle of a random sample (above 1e-2)


def rig(rng, n_cams):
    """-> offsets [n_cams][3], rotations [n_cams][3][3]"""
    x = np.linspace(-0.055, 0.055, n_cams) if n_cams > 1 else np.array([0.055])
    off = np.stack([x, np.zeros(n_cams), np.zeros(n_cams)], axis=1)
    rot = np.stack([rotation(rng.normal(size=3), rng.uniform(0.0, 0.05)) for _ in range(n_cams)])
    return off, rot


def scene(rng, n, n_cams=2, far=False, cams_used=None):
    """-> dict: R, t (the true pose), points, bearing [n][3], cam_index [n], cam_offsets, cam_rotations"""
    R = rotation(rng.normal(size=3), rng.uniform(0.01, 0.3))
    t = rng.normal(size=3)
    t *= rng.uniform(0.0, 3.0) / np.linalg.norm(t)
    off, rot = rig(rng, n_cams)
    used = np.arange(n_cams) if cams_used is None else np.asarray(cams_used)
    ci = used[rng.integers(0, len(used), n)].astype(np.int32)
    z = rng.uniform(50, 100, n) if far else rng.uniform(2, 8, n)
    s = z / 5.0 if far else np.ones(n)
    pc = np.stack([rng.uniform(-2, 2, n) * s, rng.uniform(-1.5, 1.5, n) * s, z], axis=1)
    body = off[ci] + np.einsum("nij,nj->ni", rot[ci], pc)
    return {"R": R, "t": t, "points": body @ R.T + t, "bearing": pc / np.linalg.norm(pc, axis=1, keepdims=True), "cam_index": ci,
            "cam_offsets": off, "cam_rotations": rot, "n": n}


def samples(rng, n, k, size=4):
    return np.stack([rng.choice(n, size, replace=False) for _ in range(k)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(seed, n, k, n_cams=2, far=False, cams_used=None):
    """one problem with k samples; the samples of a smaller k are a prefix of those of a larger one"""
    rng = np.random.default_rng(seed)
    c = scene(rng, n, n_cams, far, cams_used)
    c["sigma"] = rng.uniform(0.5e-6, 2e-6, n)
    c["samples"] = samples(np.random.default_rng(seed + 1000), n, 130 if n > 4 else 1)[:k]
    return c


def job(c, q=None, **kw):
    return dict({"points": c["points"], "bearing": c["bearing"], "sigma": c["sigma"], "cam_index": c["cam_index"],
                 "cam_offsets": c["cam_offsets"], "cam_rotations": c["cam_rotations"], "samples": c["samples"] if q is None else q}, **kw)


def sample_inputs(c, q):
    """the four correspondences of the sample q as the statement takes them"""
    ci = c["cam_index"][q]
    return c["points"][q], c["bearing"][q], c["cam_offsets"][ci], c["cam_rotations"][ci]


# ---- the stated results ----------------------------------------------------------------------------------------------------------------
def state_one(args):
    """one sample: the statement, the numpy evaluation, e64 and e_in"""
    X, f, off, rot, seed = args
    st = S.gp3p(X, f, off, rot, ctx=S.MP)
    ev = S.gp3p(X, f, off, rot, ctx=S.NP)
    out = {k: st[k] for k in ("valid", "R", "t", "n_roots", "n_real", "candidates", "separation", "margin")}
    out["np"] = {k: ev[k] for k in ("valid", "R", "t", "n_roots", "candidates")}
    out["e64"] = S.pose_distance(ev["R"], ev["t"], st["R"], st["t"]) if st["valid"] and ev["valid"] else np.inf
    e_in = 0.0
    if st["valid"]:
        rng = np.random.default_rng(seed)
        for _ in range(DRAWS):
            g = f * (1.0 + rng.choice([-1.0, 1.0], f.shape) * 2.0 ** -53)
            Y = X * (1.0 + rng.choice([-1.0, 1.0], X.shape) * 2.0 ** -53)
            R, t = S.gp3p_near(Y, g, off, rot, st)
            e_in = max(e_in, S.pose_distance(R, t, st["R"], st["t"]))
    out["e_in"] = e_in
    out["bound"] = BOUND_FACTOR * max(out["e64"], e_in)
    out["excluded"] = S.excluded(st)
    return out


def state(c, q, seed=0):
    """the stated results of the samples q [k][4] of the problem c, in order"""
    args = [sample_inputs(c, s) + (seed + 7919 * m,) for m, s in enumerate(np.asarray(q))]
    if len(args) <= 2:
        return [state_one(a) for a in args]
    return list(pool().map(state_one, args, chunksize=2))


@functools.lru_cache(maxsize=None)
def stated(seed, n, n_cams=2, far=False, cams_used=None, k=None):
    """the stated results of all samples of case(seed, n, .) (130, or 1 for n = 4; or the first k): stated once, sliced by the callers"""
    c = case(seed, n, (130 if n > 4 else 1) if k is None else k, n_cams, far, cams_used)
    return state(c, c["samples"], seed)


@functools.lru_cache(maxsize=None)
def most_roots(seed=73, count=20000):
    """-> (case, sample [4], candidates, real solutions): the first sample with the most candidates (real solutions with three
    positive depths) among `count` seeded samples of one scene (float64 count)"""
    c = case(seed, 400, 1)
    q = samples(np.random.default_rng(seed + 3000), 400, count)
    ci = c["cam_index"][q[:, :3]]
    d = np.einsum("nkij,nkj->nki", c["cam_rotations"][ci], c["bearing"][q[:, :3]])
    real, pos = S.count_candidates(c["points"][q[:, :3]], c["cam_offsets"][ci], d)
    m = int(np.argmax(pos))
    return c, q[m], int(pos[m]), int(real.max())


def degenerate_case(seed=81, n=40):
    """-> (case, samples): a repeated index, three collinear world points (correspondences 1, 2, 3 of the scene), and two world
    points on one ray of one camera (correspondences 4, 5), next to a plain sample"""
    c = dict(case(seed, n, 1))
    c["points"], c["bearing"], c["cam_index"] = c["points"].copy(), c["bearing"].copy(), c["cam_index"].copy()
    c["points"][1:3] = c["points"][1:3].astype(np.float32)          # short mantissas, so that the next line is exact:
    c["points"][3] = 2.0 * c["points"][2] - c["points"][1]          # collinear in double, the cross product an exact zero
    body = (c["points"][4] - c["t"]) @ c["R"]
    cam = c["cam_index"][4]
    far = c["cam_offsets"][cam] + 1.5 * (body - c["cam_offsets"][cam])          # on the same ray, half as far again
    c["points"][5], c["bearing"][5], c["cam_index"][5] = far @ c["R"].T + c["t"], c["bearing"][4], cam
    q = np.array([[10, 11, 12, 13], [10, 11, 10, 13], [10, 11, 12, 12], [1, 2, 3, 13], [4, 5, 12, 13]], np.int32)
    return c, q


E2E_SEED = 91          # no gross outlier lies by chance within the threshold: test_sac_abs_host.py shows that on the float64 statement


@functools.lru_cache(maxsize=None)
def end_to_end():
    """300 exact inlier correspondences over two cameras and 15 % gross outliers (45 correspondences whose bearings belong to other
    points), shuffled; 50 seeded samples.  -> (job fields, the true inlier indices ascending)"""
    rng = np.random.default_rng(E2E_SEED)
    c = scene(rng, 345)
    wrong = 300 + rng.permutation(45)
    while (wrong == 300 + np.arange(45)).any():
        wrong = 300 + rng.permutation(45)
    c["bearing"][300:] = c["bearing"][wrong]
    order = rng.permutation(345)
    for k in ("points", "bearing", "cam_index"):
        c[k] = c[k][order]
    truth = np.sort(np.nonzero(order < 300)[0]).astype(np.int32)
    c["sigma"] = rng.uniform(0.5e-6, 2e-6, 345)
    c["samples"] = samples(rng, 345, 50)
    return job(c, threshold=9.0), truth


def end_to_end_float64():
    """the float64 statement of the whole rejection: numpy hypotheses, numpy scores, `<` and the first-best rule -> inliers"""
    j, _ = end_to_end()
    best, best_set = -1, None
    for q in j["samples"]:
        ev = S.gp3p(*sample_inputs(j, q), ctx=S.NP)
        sc = (S.score_absolute(ev["R"], ev["t"], j["points"], j["bearing"], j["cam_index"], j["cam_offsets"], j["cam_rotations"]) / j["sigma"]
              if ev["valid"] else np.full(len(j["sigma"]), np.nan))
        with np.errstate(invalid="ignore"):
            inl = np.nonzero(sc < j["threshold"])[0]
        if len(inl) > best:
            best, best_set = len(inl), inl.astype(np.int32)
    return best_set


# ---- the device's (or the probe's) results against them -------------------------------------------------------------------------------
def match_candidates(got, want):
    """got, want [k][3][4] in any order -> the largest distance of a wanted transformation to its nearest reported one"""
    return max([min(S.pose_distance(g[:, :3], g[:, 3], w[:, :3], w[:, 3]) for g in got) for w in want], default=0.0)


def mapped_residual(c, q, T):
    """the largest distance, over the sample's first three correspondences, of R^T (X_k - t) to the ray of correspondence k at a
    positive depth, over max(1, |X_k|, depth)"""
    X, f, off, rot = sample_inputs(c, q)
    worst = 0.0
    for k in range(3):
        d = rot[k] @ f[k]
        body = T[:, :3].T @ (X[k] - T[:, 3]) - off[k]
        lam = (body @ d) / (d @ d)
        if not lam > 0:
            return np.inf
        worst = max(worst, np.linalg.norm(body - lam * d) / max(1.0, np.linalg.norm(X[k]), lam))
    return worst


def check(c, q, st_list, valid, n_roots, T, cands, label):
    """The comparison and the properties of one case.  Prints the figures, then asserts.  -> (largest d / bound, excluded)"""
    problems, worst, n_ex, worst_map = [], 0.0, 0, 0.0
    for m, st in enumerate(st_list):
        k = int(n_roots[m])
        if not 0 <= k <= 8:
            problems.append((m, "n_roots", k))
            continue
        if not np.isfinite(cands[m][:k]).all() or not np.isnan(cands[m][k:]).all():
            problems.append((m, "candidates are not the first n_roots", cands[m]))
            continue
        for g in cands[m][:k]:
            R = g[:, :3]
            res = mapped_residual(c, q[m], g)
            worst_map = max(worst_map, res)
            if np.linalg.norm(R.T @ R - np.eye(3)) > ORTHO_TOL or np.linalg.det(R) < 0 or res > MAPPED_TOL:
                problems.append((m, "not a pose that maps the three points", g, res))
        if bool(valid[m]) != (k > 0):
            problems.append((m, "valid but no candidate, or the reverse", k))
        if valid[m]:
            if not any(np.array_equal(T[m], g) for g in cands[m][:k]):
                problems.append((m, "the hypothesis is none of the candidates", T[m]))
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
            far = match_candidates(cands[m][:k], st["candidates"])
            if far > 1e3 * st["bound"] + 1e-12:
                problems.append((m, "candidates do not match the statement's", far))
    print(f"{label}: {len(st_list)} samples, {n_ex} excluded, largest d / bound {worst:.3f}, largest mapping residual {worst_map:.3e}")
    assert n_ex <= S.MAX_EXCLUDED * len(st_list), (label, n_ex)
    assert not problems, (label, problems[:5])
    return worst, n_ex


# ---- the stand-alone probe (tests/sac_abs_probe.cpp) -----------------------------------------------------------------------------------
def build_probe(out_dir, sanitize=True):
    """the probe with the sanitizers' runtimes linked statically (the CPU tests), or plain (next to the device, for the bits)"""
    exe = os.path.join(str(out_dir), "sac_abs_probe")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, os.path.join(HERE, "sac_abs_probe.cpp"), "-o", exe], check=True)
    return exe


def run_probe(exe, out_dir, c, q, tag="p"):
    """-> valid [k], n_roots [k], models [k][3][4], candidates [k][8][3][4]"""
    q = np.ascontiguousarray(q, np.int32).reshape(-1, 4)
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    with open(src, "wb") as f:
        np.array([len(c["points"]), len(c["cam_offsets"]), len(q), 0], np.int32).tofile(f)
        for name, dtype in (("points", np.float64), ("bearing", np.float64), ("cam_index", np.int32), ("cam_offsets", np.float64),
                            ("cam_rotations", np.float64)):
            np.ascontiguousarray(c[name], dtype).tofile(f)
        q.tofile(f)
    subprocess.run([exe, src, dst], check=True)
    raw = np.fromfile(dst, np.float64).reshape(-1, 110)
    return raw[:, 0] != 0, raw[:, 1].astype(np.int32), raw[:, 2:14].reshape(-1, 3, 4), raw[:, 14:].reshape(-1, 8, 3, 4)
