"""TEST INFRASTRUCTURE.  The seeded cases of okvis_fe_keyframe_decision: the smallest shapes at which each mechanism of the kernel
(okvis_amd/csrc/fe_keyframe.hpp) can fail.  A case is a list of jobs in the form Frontend.keyframe_decision takes; stated(name) is
what tests/keyframe_statement.py says about them, computed once per process and shared by the tests.

  skips        n = 0, 2, 3; m = 2, 3; a triangle whose three vertices are the only matches (inside 0, ratio +inf, decision 0)
  degenerate   all keypoints collinear (0/0 = NaN) before and after a regular camera: the two orders differ under the std::max
               rule; matched points collinear (hull size 2, inside 0); all matched points coincident (size 1); duplicate
               coordinates under different indices (the lowest index is reported)
  on_edges     integer and half-integer coordinates: keypoints exactly on hull edges and at hull vertices are not inside
  adversarial  the near-collinear family on which plain double arithmetic returns wrong signs: such a c as a would-be hull vertex
               and as a would-be inside point
  convex       y = x^2 on integers, n = 64, 65, 512: every point is a vertex, more vertices than lanes
  regular      400 uniform keypoints on 752 x 480 at 2^-4 pixel, 10-60 % matched inside a sub-rectangle, two cameras, thresholds
               0.6 and 0.2; only seeds whose exact overlap and ratio lie at least 1e-6 (relative) from their thresholds
  limit        one image of 8192 keypoints, the most an image may hold (the whole of the wave's 64 KB of LDS)
  mixed        130 jobs of 1..8 cameras, empty images, jobs with num_frames < 2 and initialized = 0 among them"""
import functools
from fractions import Fraction

import numpy as np

import keyframe_statement as S

NAMES = ("skips", "degenerate", "on_edges", "adversarial", "convex", "regular", "limit", "mixed")
THRESHOLDS = (0.6, 0.2)        # the reference's comments at Frontend.hpp:312, 319
REGULAR_GENERATED = 20         # seeds generated for `regular`; at most 1 in 20 may be dropped
MARGIN = Fraction(1, 10 ** 6)


def kp3(xy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    return np.concatenate([xy, np.full((len(xy), 1), 6.0, np.float32)], axis=1)


def im(xy, matched):
    xy = kp3(xy)
    m = np.zeros(len(xy), np.uint8)
    if isinstance(matched, str) and matched == "all":
        m[:] = 1
    else:
        m[np.asarray(matched, np.int64)] = 1
    return xy, m


# ---- the near-collinear family ---------------------------------------------------------------------------------------------------
def exact_array(x):
    """float32 array -> object array of the Python integers x * 2^149"""
    m, e = np.frexp(np.asarray(x, np.float32).astype(np.float64))
    M = np.array([int(v) for v in (m * 2.0 ** 24).ravel()], dtype=object)
    sh = np.array([int(v) for v in e.ravel()], dtype=object) - 24 + S.SCALE
    out = np.array([(a << s) if s >= 0 else (a >> -s) for a, s in zip(M, sh)], dtype=object)
    return out.reshape(np.shape(x))


def exact_signs(a, b, c):
    """orient over [N][2] float32 arrays, exact"""
    A, B, Cc = exact_array(a), exact_array(b), exact_array(c)
    d = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (Cc[:, 0] - A[:, 0])
    return np.array([(v > 0) - (v < 0) for v in d], np.int32)


def naive_signs(a, b, c):
    """the plain double expression (numpy float64: one rounding per operation)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    d = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    return np.sign(d).astype(np.int32)


@functools.lru_cache(maxsize=None)
def family(n=100000, seed=20240):
    """a = (1 + i 2^-23, 1 + j 2^-23), b = a + (700 + k 2^-14, 700 + l 2^-14), c = a + (350 + p 2^-15, 350 + q 2^-15), b and c
    rounded to float, i..q small integers -> a, b, c [n][2] float32"""
    rng = np.random.default_rng(seed)
    i, j, k, l, p, q = (rng.integers(-4, 5, n).astype(np.float64) for _ in range(6))      # about 1 in 4000 then goes wrong
    a = np.stack([1 + i * 2.0 ** -23, 1 + j * 2.0 ** -23], 1).astype(np.float32)
    a64 = a.astype(np.float64)
    b = (a64 + np.stack([700 + k * 2.0 ** -14, 700 + l * 2.0 ** -14], 1)).astype(np.float32)
    c = (a64 + np.stack([350 + p * 2.0 ** -15, 350 + q * 2.0 ** -15], 1)).astype(np.float32)
    return a, b, c


@functools.lru_cache(maxsize=None)
def random_triples(n=100000, seed=20241):
    """finite float32 of every exponent and sign, by bit pattern; a third of the triples share coordinates, so that zeros occur"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (3, n, 2), dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = np.where(np.isfinite(v), v, np.float32(1.5))
    a, b, c = v[0].copy(), v[1].copy(), v[2].copy()
    third = n // 3
    b[:third, 0] = a[:third, 0]           # a vertical edge
    c[:third // 2, 0] = a[:third // 2, 0]  # and c on its line
    c[third:third + 100] = b[third:third + 100]
    return a, b, c


@functools.lru_cache(maxsize=None)
def family_signs():
    a, b, c = family()
    return exact_signs(a, b, c), naive_signs(a, b, c)


def wrong_triples(per_sign=4):
    """triples of the family on which the naive sign is wrong, some for each exact sign that occurs"""
    a, b, c = family()
    ex, nv = family_signs()
    out = []
    for s in (-1, 0, 1):
        for t in np.nonzero((ex != nv) & (ex == s))[0][:per_sign]:
            out.append((a[t], b[t], c[t], s))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def regular_image(rng):
    xy = rng.integers(0, [752 * 16, 480 * 16], (400, 2)).astype(np.float32) / np.float32(16)
    lo = rng.uniform([0, 0], [200, 120])
    hi = lo + rng.uniform([300, 200], [752, 480])     # (clipped by the image: the overlap comes out between 0.2 and 0.9)
    box = np.nonzero(((xy >= lo) & (xy <= hi)).all(1))[0]
    m = rng.permutation(box)[:int(rng.uniform(0.10, 0.60) * 400)]
    return im(xy, m)


def regular_job(seed):
    rng = np.random.default_rng(7000 + seed)
    return {"images": [regular_image(rng), regular_image(rng)], "overlap_threshold": THRESHOLDS[0], "ratio_threshold": THRESHOLDS[1]}


def far_from_thresholds(st):
    o, r = S.exact_scores(st["images"])
    if o is None:
        return False
    t_o, t_r = (Fraction(float(np.float32(t))) for t in THRESHOLDS)
    return abs(o - t_o) >= MARGIN * t_o and abs(r - t_r) >= MARGIN * t_r


@functools.lru_cache(maxsize=None)
def regular_kept():
    """-> (the kept jobs, their statements, how many seeds were generated)"""
    jobs = [regular_job(s) for s in range(REGULAR_GENERATED)]
    stated_ = [S.job(j) for j in jobs]
    keep = [i for i, st in enumerate(stated_) if far_from_thresholds(st)]
    return [jobs[i] for i in keep], [stated_[i] for i in keep], len(jobs)


def square_with_edge_points():
    """corners (0,0) (8,0) (8,8) (0,8) matched, with matched and unmatched points on the edges (half-integers too), duplicates of
    the corners under later indices, and points strictly inside"""
    xy = [(8, 8), (0, 0), (8, 0), (0, 8),                   # 0-3 corners, not in hull order
          (4, 0), (8, 2.5), (3.5, 8), (0, 7.5),               # 4-7 on the edges, matched: never vertices of the strict hull
          (0.5, 0), (8, 7.5), (0, 0.5), (7.5, 8),             # 8-11 on the edges, unmatched: not inside
          (0, 0), (8, 8), (8, 0),                             # 12-14 duplicates of corners, unmatched: not inside
          (4, 4), (0.5, 0.5), (7.5, 7.5), (1, 7), (4, 0.5),   # 15-19 inside
          (9, 4), (-1, -1), (4, 8.5)]                         # 20-22 outside
    return im(xy, [0, 1, 2, 3, 4, 5, 6, 7, 15])


def diamond_on_diagonals():
    """edges that are not axis-parallel: (0,0) (6,2) (8,8) (2,6); (3,1) and (7,5) lie on edges, (4,4) on the diagonal inside"""
    xy = [(2, 6), (8, 8), (6, 2), (0, 0), (3, 1), (7, 5), (4, 4), (1, 3), (5, 7), (4.5, 1.5), (1.5, 0.5)]
    return im(xy, [0, 1, 2, 3, 4, 6])


def collinear_image(n=9, matched="all"):
    t = np.arange(n, dtype=np.float64)[np.array([3, 0, 8, 5, 1, 7, 2, 6, 4])[:n]]
    return im(np.stack([10 + 3 * t, 20 + 1.5 * t], 1), matched)


def small_regular():
    rng = np.random.default_rng(99)
    xy = rng.integers(0, 64 * 16, (40, 2)).astype(np.float32) / np.float32(16)
    return im(xy, rng.permutation(40)[:20])


@functools.lru_cache(maxsize=None)
def cases(name):
    th = {"overlap_threshold": THRESHOLDS[0], "ratio_threshold": THRESHOLDS[1]}
    if name == "skips":
        tri = [(0, 0), (4, 0), (0, 4)]
        return [{"images": [im(np.zeros((0, 2)), []), im(tri[:2], "all"), im(tri, [0, 1])], **th},        # n = 0, 2; n = 3 with m = 2
                {"images": [im(tri, "all")], **th},                                                       # inside 0, ratio +inf, decision 0
                {"images": [im(tri + [(1, 1), (1, 2), (5, 5)], [0, 1, 2])], **th},                        # m = 3 among n = 6
                {"images": [im(tri + [(1, 1)], [0, 3])], **th},                                           # m = 2 among n = 4
                {"images": [im(tri[:2], "all"), im(tri, "all")], **th}]                                   # a skipped camera first
    if name == "degenerate":
        line, reg = collinear_image(), small_regular()
        dup = im([(5, 5), (0, 0), (5, 0), (0, 0), (5, 5), (0, 5), (5, 0), (2, 2), (0, 5)], [0, 2, 3, 4, 5, 6, 8])
        return [{"images": [line, reg], **th},                       # NaN first: the regular camera replaces it
                {"images": [reg, line], **th},                       # NaN last: it stays
                {"images": [line], **th},
                {"images": [im(np.concatenate([collinear_image()[0][:, :2], [[0, 50], [40, 0]]]), list(range(9)))], **th},   # matched collinear
                {"images": [im([(3, 3), (0, 0), (3, 3), (9, 1), (3, 3), (2, 7), (3, 3)], [0, 2, 4, 6])], **th},          # matched coincident
                {"images": [im([(1, 1)] * 5, "all")], **th},         # everything coincident
                {"images": [dup], **th},
                {"images": [im([(0.0, 1), (-0.0, 1), (3, 1), (2, 5), (1, 2)], "all")], **th}]      # -0 and +0 are one coordinate
    if name == "on_edges":
        return [{"images": [square_with_edge_points(), diamond_on_diagonals()], **th}, {"images": [diamond_on_diagonals()], **th}]
    if name == "adversarial":
        jobs = []
        for a, b, c, s in wrong_triples():
            d = a + np.array([0, 700], np.float32)                   # to the left of a -> b
            e = a + np.array([700, 0], np.float32)                   # to the right
            xy = np.stack([b, c, d, a])
            jobs.append({"images": [im(xy, "all"),                   # c as a would-be vertex of the hull (it is one iff orient(a, b, c) < 0)
                                    im(xy, [0, 2, 3]),               # c as a would-be inside point of the hull a, b, d
                                    im(np.stack([c, e, b, a, d]), [0, 1, 2, 3])], **th})   # and with the hull on the other side
        return jobs
    if name == "convex":
        jobs = []
        for n in (64, 65, 512):
            x = np.arange(n, dtype=np.float64) - n // 2
            xy = np.stack([x, x * x], 1)[np.random.default_rng(n).permutation(n)]
            jobs.append({"images": [im(xy, "all"), im(xy, list(range(0, n, 3)))], **th})
        return jobs
    if name == "regular":
        return regular_kept()[0]
    if name == "limit":
        rng = np.random.default_rng(8192)
        xy = rng.integers(0, [752 * 16, 480 * 16], (8192, 2)).astype(np.float32) / np.float32(16)
        return [{"images": [im(xy, np.nonzero((xy[:, 0] > 100) & (xy[:, 0] < 600) & (xy[:, 1] > 80) & (rng.random(8192) < 0.35))[0])], **th}]
    if name == "mixed":
        rng = np.random.default_rng(130)
        jobs = []
        for j in range(130):
            images = []
            for _ in range(1 + j % 8):
                n = int(rng.choice([0, 0, 1, 2, 3, 5, 17, 63, 64, 65, 100, 130]))
                xy = rng.integers(0, 128 * 4, (n, 2)).astype(np.float32) / np.float32(4)       # a coarse grid: collinear triples and duplicates occur
                images.append(im(xy, np.nonzero(rng.random(n) < rng.choice([0.0, 0.35, 0.8, 1.0]))[0]))
            jobs.append({"images": images, "num_frames": int(rng.choice([0, 1, 2, 5])), "initialized": bool(rng.random() < 0.8),
                         "overlap_threshold": float(rng.choice([0.6, 0.3, 0.9])), "ratio_threshold": float(rng.choice([0.2, 0.5, 1.5]))})
        return jobs
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stated(name):
    if name == "regular":
        return regular_kept()[1]
    return [S.job(j) for j in cases(name)]


# ---- comparing an implementation's result with the statement ----------------------------------------------------------------------
def bits(x):
    return np.float64(x).tobytes()


def check(got, want, where):
    """one job's result (the dict shape Frontend.keyframe_decision returns, hulls included) against the statement's: the integers
    and index lists equal, the doubles equal byte for byte (NaN and inf included)"""
    assert len(got["images"]) == len(want["images"]), where
    for c, (g, w) in enumerate(zip(got["images"], want["images"])):
        at = (where, "camera", c)
        assert (g["flags"], g["n_matched"]) == (w["flags"], w["n_matched"]), at
        assert list(g["hull_all"]) == list(w["hull_all"]) and g["hull_all_size"] == len(w["hull_all"]), at
        assert list(g["hull_matched"]) == list(w["hull_matched"]) and g["hull_matched_size"] == len(w["hull_matched"]), at
        assert g["n_inside"] == w["n_inside"], at
        assert bits(g["area_all"]) == bits(w["area_all"]) and bits(g["area_matched"]) == bits(w["area_matched"]), at
    assert bits(got["overlap"]) == bits(want["overlap"]) and bits(got["ratio"]) == bits(want["ratio"]), where
    assert bool(got["decision"]) == bool(want["decision"]), where
