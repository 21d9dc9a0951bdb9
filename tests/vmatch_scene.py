"""Scenes for the verified matcher (okvis_fe_match_verified): two views of clustered points with look-alike descriptors, so that
the geometric verification, not the descriptor distance, decides most rows.

Geometry as _stereo_case of tests/test_gpu_frontend.py: camera B = camera A moved by T_AB (baseline 0.11 m, a small rotation), points
0.6 ... 25 m in front of A, keypoints = projections + 0.5 px noise, sizes from {4, 8, 12, 31}.  About 35 % of the points sit at the
position of an earlier point (a cluster: several keypoints of B verify against one of A).  Descriptors (48 bytes) are one of 12 base
descriptors with 0 ... 5 flipped bits, a cluster shares its base; B's descriptor is A's with 0 ... 5 more flips; B is permuted.  For
the 3D-2D step the landmarks are the A-frame points plus 1 cm noise (world = frame A), T_CbW the inverse of T_AB, P3 = 1.69e-2 I."""
import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import DIST_EQUIDISTANT, DIST_RADTAN

INTR = {DIST_EQUIDISTANT: synthetic.TEST_INTR_EQUI, DIST_RADTAN: synthetic.TEST_INTR_RADTAN}
THRESHOLD, NUM_BEST, WIDTH = 60.0, 4, 48
KIND_3D2D, KIND_2D2D = 1, 2


def _quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.r_[axis * np.sin(angle / 2), np.cos(angle / 2)]


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _flip(rng, d, lo, hi):
    d = d.copy()
    for _ in range(rng.integers(lo, hi + 1)):
        d[rng.integers(0, len(d))] ^= np.uint8(1 << rng.integers(0, 8))
    return d


def scene(model, seed, n_a, n_b, skipped=0.0):
    """-> dict: model, intr, T_AB, UOplus, T_CbW, P3, kp_a [n_a][3], kp_b [n_b][3] float32, desc_a, desc_b uint8, hp_W [n_a][4],
    skip_a, skip_b (bool arrays, or None without `skipped`), partner [n_b] (the point of B's keypoint; its keypoint in A where < n_a)"""
    rng = np.random.default_rng(seed)
    n = max(n_a, n_b, 1)
    intr = INTR[model]
    T_AB = np.r_[0.11 * np.array([1.0, 0.05, -0.02]), _quat(rng.normal(size=3), 0.02)]
    depth = rng.uniform(0.6, 25.0, n)
    p_A = np.c_[rng.uniform(-0.55, 0.55, n) * depth, rng.uniform(-0.4, 0.4, n) * depth, depth]
    base = rng.integers(0, 256, (12, WIDTH)).astype(np.uint8)
    which = rng.integers(0, len(base), n)
    for k in range(1, n):
        if rng.random() < 0.35:
            j = rng.integers(0, k)
            p_A[k], which[k] = p_A[j], which[j]
    C_AB = _rot(T_AB[3:])
    p_B = (p_A - T_AB[:3]) @ C_AB                    # C_AB^T (p - r)
    uvA, okA = synthetic.project_points(intr, model, p_A)
    uvB, okB = synthetic.project_points(intr, model, p_B)
    uvA = np.where(okA[:, None], uvA, 100.0) + rng.normal(size=(n, 2)) * 0.5
    uvB = np.where(okB[:, None], uvB, 100.0) + rng.normal(size=(n, 2)) * 0.5
    sizes = [4.0, 8.0, 12.0, 31.0]
    kpA = np.c_[uvA, rng.choice(sizes, n)].astype(np.float32)
    kpB = np.c_[uvB, rng.choice(sizes, n)].astype(np.float32)
    descA = np.stack([_flip(rng, base[which[k]], 0, 5) for k in range(n)])
    descB = np.stack([_flip(rng, descA[k], 0, 5) for k in range(n)])
    perm = rng.permutation(n)
    hp_W = np.c_[p_A + rng.normal(size=(n, 3)) * 0.01, np.ones(n)]
    q = T_AB[3:]
    T_CbW = np.r_[-(C_AB.T @ T_AB[:3]), -q[0], -q[1], -q[2], q[3]]
    s = {"model": model, "intr": intr, "T_AB": T_AB, "UOplus": np.diag([1.69e-2] * 3 + [1e-8] * 3), "T_CbW": T_CbW,
         "P3": np.eye(3) * 1.69e-2, "kp_a": np.ascontiguousarray(kpA[:n_a]), "kp_b": np.ascontiguousarray(kpB[perm][:n_b]),
         "desc_a": np.ascontiguousarray(descA[:n_a]), "desc_b": np.ascontiguousarray(descB[perm][:n_b]),
         "hp_W": np.ascontiguousarray(hp_W[:n_a]), "partner": perm[:n_b], "skip_a": None, "skip_b": None}
    if skipped:
        s["skip_a"], s["skip_b"] = rng.random(n_a) < skipped, rng.random(n_b) < skipped
    return s


def ray_sigmas(kp, fu):
    """raySigmasA_ / raySigmasB_ (VioKeyframeWindowMatchingAlgorithm.cpp:210-221, :251-261), in double, in the reference's order"""
    sd = 0.8 * kp[:, 2].astype(np.float64) / 12.0
    return np.sqrt(np.sqrt(2.0)) * sd / fu


def pair_sigmas(s, pairs):
    """sigma of stereoTriangulate for each pair: max(raySigmaA[a], raySigmaB[b]) (:313)"""
    sa, sb = ray_sigmas(s["kp_a"], s["intr"][0]), ray_sigmas(s["kp_b"], s["intr"][0])
    return np.maximum(sa[pairs[:, 0]], sb[pairs[:, 1]])
