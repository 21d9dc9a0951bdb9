"""Inputs of the sample-consensus tests (tests/test_sac_consensus_host.py, tests/test_gpu_sac_consensus.py): the problems recorded in
tests/golden/sac_consensus.npz as job dicts, and seeded random problems larger than the golden file can hold.  TEST INFRASTRUCTURE
ONLY: imports nothing from the product.

Tolerances.  REF_* is the largest distance (sac_statement.distance: relative, with an absolute floor of 1e-3 for scores near zero)
of the reference's own double results in the golden file from the long double statement, as tests/golden/make_sac_consensus_golden.py
measured and printed it; the host test measures it again.  The GPU gets 10 times that, the project's standing convention.  The
relative-pose figure is the largest because one golden case has next to no translation between its frames (4 mm against 2..12 m
of depth): the midpoint triangulation is then ill-conditioned in double, for the reference as for anyone."""
import os

import numpy as np

import sac_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sac_consensus.npz")

KINDS = {"abs": S.ABSOLUTE, "rot": S.ROTATION_ONLY, "rel": S.RELATIVE}
# reference (double) against the statement (long double) on the golden cases, measured
REF_SCORE = {S.ABSOLUTE: 6.023e-12, S.ROTATION_ONLY: 5.490e-13, S.RELATIVE: 3.549e-08}
REF_BEARING = 2.748e-16   # absolute, per component of the unit vector
REF_SIGMA = 4.939e-16     # relative
# what the GPU gets
GPU_FACTOR = 10.0
GPU_SCORE = {k: GPU_FACTOR * v for k, v in REF_SCORE.items()}
GPU_BEARING, GPU_SIGMA = GPU_FACTOR * REF_BEARING, GPU_FACTOR * REF_SIGMA
MAX_EXCLUDED = 0.005      # of a random job's cells may lie within GPU_SCORE of the threshold and stay out of the exact comparison

PROBLEMS = ("abs", "rot0", "rel0", "rot1", "rel1")


def golden():
    return np.load(GOLDEN)


def golden_job(g, i, name):
    """problem `name` of case i as the dict Frontend.sac_consensus takes, plus the recorded results under ref_*"""
    pre = f"c{i}_{name}_"
    kind = KINDS[name[:3]]
    job = {"kind": kind, "threshold": float(g["threshold"]), "models": g[pre + "models"]}
    if kind == S.ABSOLUTE:
        for k in ("points", "bearing", "sigma", "cam_index", "cam_offsets", "cam_rotations", "kp_index"):
            job[k] = g[pre + k]
    else:
        src = f"c{i}_rot{name[3]}_"    # the relative-pose problem of a camera runs on the rotation-only problem's adapter
        for k in ("bearing1", "bearing2", "sigma1", "sigma2", "idx_a", "idx_b"):
            job[k] = g[src + k]
    for k in ("scores", "counts", "best", "inliers", "pinned"):
        job["ref_" + k] = g[pre + k]
    return job


def golden_jobs():
    g = golden()
    return [(i, name, golden_job(g, i, name)) for i in range(int(g["n_cases"])) for name in PROBLEMS]


# ---- random problems ----------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, float)
    x, y, z = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _models(rng, R, t, k, with_translation):
    out = []
    for j in range(k):
        u = rng.random()
        if u < 0.1:
            Rm, tm = R, t
        elif u < 0.9:
            mag = 10.0 ** rng.uniform(-7, -0.5)
            Rm, tm = _rot(rng.normal(size=3), mag) @ R, t + mag * rng.normal(size=3)
        else:
            Rm, tm = _rot(rng.normal(size=3), rng.uniform(0.5, 3.0)) @ R, t + rng.normal(size=3)
        out.append(np.concatenate([Rm, tm[:, None]], axis=1) if with_translation else Rm)
    return np.array(out)


def random_job(rng, kind, n, k):
    """a problem with a true pose, correspondences that agree with it up to noise (a fifth of them does not), and k hypotheses from
    the true pose to far off"""
    sigma = lambda: np.sqrt(2.0) * (0.8 * rng.uniform(5.0, 20.0, n) / 12.0) ** 2 / rng.uniform(300.0, 600.0) ** 2   # noqa: E731
    noise = lambda: rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3.5, -2.5)                                      # noqa: E731
    z = rng.uniform(2.0, 12.0, n)
    p = np.stack([0.5 * z * rng.uniform(-1, 1, n), 0.35 * z * rng.uniform(-1, 1, n), z], axis=1)      # in the first camera
    wrong = rng.random(n) < 0.2
    R, t = _rot(rng.normal(size=3), rng.uniform(0.0, 0.3)), rng.uniform(0.1, 0.5) * _unit(rng.normal(size=(1, 3)))[0]
    if kind == S.ABSOLUTE:
        n_cams = int(rng.integers(1, 9))
        C = np.array([_rot(rng.normal(size=3), rng.uniform(0, 0.2)) for _ in range(n_cams)])
        off = rng.normal(size=(n_cams, 3)) * 0.05
        ci = rng.integers(0, n_cams, n).astype(np.int32)
        R_WS, r_WS = _rot(rng.normal(size=3), rng.uniform(0, 1.0)), rng.normal(size=3)
        # p is in the correspondence's own camera: world = T_WS T_SC p
        body = np.einsum("nij,nj->ni", C[ci], p) + off[ci] if n else p
        world = body @ R_WS.T + r_WS
        f = _unit(p + noise() * z[:, None]) if n else p
        f[wrong] = _unit(rng.normal(size=(int(wrong.sum()), 3)) + [0, 0, 2.0])
        return {"kind": kind, "threshold": 9.0, "models": _models(rng, R_WS, r_WS, k, True), "points": world, "bearing": f, "sigma": sigma(),
                "cam_index": ci, "cam_offsets": off, "cam_rotations": C}
    # p1 = R p2 + t
    p2 = (p - t) @ R
    f1, f2 = (_unit(p + noise() * z[:, None]), _unit(p2 + noise() * z[:, None])) if n else (p, p2)
    f2[wrong] = _unit(rng.normal(size=(int(wrong.sum()), 3)) + [0, 0, 2.0])
    return {"kind": kind, "threshold": 9.0, "models": _models(rng, R, t, k, kind == S.RELATIVE), "bearing1": f1, "bearing2": f2,
            "sigma1": sigma(), "sigma2": sigma()}


# n, K of the jobs of one call: mixed kinds, n not a multiple of 64, n = 0 and 1, K from 1 to 1024
RANDOM_SHAPES = [(0, 5), (1, 1024), (1, 1), (63, 7), (64, 64), (65, 65), (127, 1), (128, 63), (255, 50), (256, 50), (257, 129), (300, 50),
                 (5000, 40), (3001, 200), (4099, 64), (2049, 128), (700, 1024), (1000, 300), (64, 1), (0, 1), (150, 50), (150, 50),
                 (333, 17), (1, 3), (2, 2), (999, 99), (512, 512), (4000, 65), (191, 33), (6000, 20), (31, 1000), (1536, 70)]
RANDOM_SEEDS = (11,)


def random_jobs(seed):
    """2 x len(RANDOM_SHAPES) = 64 jobs: every shape twice, with kinds that go round"""
    rng = np.random.default_rng(seed)
    jobs = []
    for r in range(2):
        for j, (n, k) in enumerate(RANDOM_SHAPES):
            jobs.append(random_job(rng, (j + r + seed) % 3, n, k))
    order = rng.permutation(len(jobs))
    return [jobs[i] for i in order]


_stated = {}


def stated(seed):
    """per job of random_jobs(seed): the statement's scores (long double), the cells too close to the threshold to call, and the
    consensus with those cells left out: counts_lo (the uncertain cells counted as outliers)"""
    if seed not in _stated:
        res = []
        for job in random_jobs(seed):
            sc = S.scores(job)
            near = S.near_threshold(sc, job["threshold"], GPU_SCORE[job["kind"]])
            res.append({"scores": sc, "near": near, "inlier": (sc < job["threshold"]) & ~near})
        _stated[seed] = res
    return _stated[seed]
