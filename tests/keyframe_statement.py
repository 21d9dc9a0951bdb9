"""TEST INFRASTRUCTURE.  The statement of okvis_fe_keyframe_decision (include/okvis_amd_frontend.h) in exact arithmetic: what
Frontend::doWeNeedANewKeyframe (okvis_frontend/src/Frontend.cpp:295-369) computes, with cv::convexHull, cv::contourArea and
cv::pointPolygonTest stated from their definitions.

Keypoints are float32.  Every finite float32 is an integer multiple of 2^-149, so a coordinate becomes the Python integer
x * 2^149 and orient() is integer arithmetic: no rounding anywhere.  The hull comes from Andrew's monotone chain (sort, lower and
upper chain), which shares no algorithm with the kernel's gift wrapping.  The area is evaluated twice: as the IEEE double sequence
of the header (numpy float64, one rounding per operation, no fused multiply-add) and exactly, as a Fraction."""
from fractions import Fraction

import numpy as np

FEW_POINTS, FEW_MATCHES = 1, 2
SCALE = 149


def exact(v):
    """a finite float32 as the integer v * 2^149"""
    num, den = float(np.float32(v)).as_integer_ratio()
    q, r = divmod(num << SCALE, den)
    assert r == 0
    return q


def rows(kp):
    """kp [n][2 or 3] as a float32 array with one row per keypoint (n = 0 included)"""
    kp = np.asarray(kp, np.float32)
    return kp.reshape(len(kp), -1) if kp.size else np.zeros((0, 2), np.float32)


def exact_points(kp):
    kp = rows(kp)
    return [(exact(x), exact(y)) for x, y in kp[:, :2]]


def orient(a, b, c):
    """the sign of (bx-ax)(cy-ay) - (by-ay)(cx-ax), exact"""
    d = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (d > 0) - (d < 0)


def hull(P, idx):
    """the strict convex hull of the points P[k], k in idx, as keypoint indices: from the lowest (y, then x) point, counter-clockwise;
    every vertex the lowest index with its coordinates"""
    first = {}
    for k in idx:
        first.setdefault(P[k], k)      # idx ascends: the first holder of a coordinate pair is the lowest index
    pts = sorted(first)                # by x, then y
    if len(pts) <= 1:
        return [first[p] for p in pts]

    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and orient(out[-2], out[-1], p) <= 0:
                out.pop()
            out.append(p)
        return out

    lower, upper = chain(pts), chain(pts[::-1])
    ring = lower[:-1] + upper[:-1]     # counter-clockwise from the leftmost point; two points where all are collinear
    start = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
    ring = ring[start:] + ring[:start]
    return [first[p] for p in ring]


def area_double(kp, h):
    """the header's sequence in IEEE double: a += (double)prev.x * p.y - (double)prev.y * p.x over the hull in order; fabs(a * 0.5)"""
    if len(h) < 3:
        return np.float64(0.0)
    xy = rows(kp)[:, :2].astype(np.float64)
    a = np.float64(0.0)
    prev = xy[h[-1]]
    for k in h:
        p = xy[k]
        a = a + (prev[0] * p[1] - prev[1] * p[0])
        prev = p
    return np.abs(a * np.float64(0.5))


def area_exact(P, h):
    """-> (the exact area, the sum of |x_i y_i+1| + |x_i+1 y_i| over the edges) as Fractions"""
    if len(h) < 3:
        return Fraction(0), Fraction(0)
    s = mag = 0
    for i in range(len(h)):
        p, q = P[h[i - 1]], P[h[i]]
        s += p[0] * q[1] - p[1] * q[0]
        mag += abs(p[0] * q[1]) + abs(p[1] * q[0])
    return Fraction(abs(s), 2 << (2 * SCALE)), Fraction(mag, 1 << (2 * SCALE))


def image(kp, matched):
    """one camera image -> dict: n_matched, hull_all, hull_matched (index lists), area_all, area_matched (float64), n_inside, flags,
    and the exact rationals (exact_all, exact_matched, mag_all, mag_matched)"""
    kp = rows(kp)
    matched = np.asarray(matched).reshape(-1) != 0
    n, m = len(kp), int(matched.sum())
    r = {"n_matched": m, "hull_all": [], "hull_matched": [], "area_all": np.float64(0), "area_matched": np.float64(0), "n_inside": 0,
         "flags": 0, "exact_all": Fraction(0), "exact_matched": Fraction(0), "mag_all": Fraction(0), "mag_matched": Fraction(0)}
    if n < 3:
        r["flags"] = FEW_POINTS
        return r
    if m < 3:
        r["flags"] = FEW_MATCHES
        return r
    P = exact_points(kp)
    ha, hm = hull(P, range(n)), hull(P, [k for k in range(n) if matched[k]])
    r["hull_all"], r["hull_matched"] = ha, hm
    r["area_all"], r["area_matched"] = area_double(kp, ha), area_double(kp, hm)
    r["exact_all"], r["mag_all"] = area_exact(P, ha)
    r["exact_matched"], r["mag_matched"] = area_exact(P, hm)
    if len(hm) >= 3:
        V = [P[k] for k in hm]
        E = list(zip(V, V[1:] + V[:1]))
        r["n_inside"] = sum(all(orient(a, b, p) > 0 for a, b in E) for p in P)
    return r


def fold(images, num_frames=2, initialized=True, overlap_threshold=0.6, ratio_threshold=0.2):
    """Frontend.cpp:307-368 over the images' results in camera order -> (decision, overlap, ratio), the two as float64"""
    overlap = ratio = np.float64(0.0)
    with np.errstate(all="ignore"):
        for r in images:
            if r["flags"]:
                continue
            overlap_area = np.float64(r["area_matched"]) / np.float64(r["area_all"])
            matching_ratio = np.float64(r["n_matched"]) / np.float64(r["n_inside"])
            overlap = overlap if overlap_area < overlap else overlap_area       # std::max(overlapArea, overlap)
            ratio = ratio if matching_ratio < ratio else matching_ratio
    if num_frames < 2:
        return 1, overlap, ratio
    if not initialized:
        return 0, overlap, ratio
    t_o, t_r = np.float64(np.float32(overlap_threshold)), np.float64(np.float32(ratio_threshold))
    return int(not (overlap > t_o and ratio > t_r)), overlap, ratio


def exact_scores(images):
    """the fold over the EXACT areas, for judging a case's distance from the thresholds: (overlap, ratio) as Fractions, None where
    an image's quotient is not a number (0/0) or infinite"""
    overlap = ratio = Fraction(0)
    for r in images:
        if r["flags"]:
            continue
        if r["exact_all"] == 0 or r["n_inside"] == 0:
            return None, None
        overlap = max(overlap, r["exact_matched"] / r["exact_all"])
        ratio = max(ratio, Fraction(r["n_matched"], r["n_inside"]))
    return overlap, ratio


def job(j):
    """a job dict of Frontend.keyframe_decision -> the same dict shape it returns (hulls always), plus the exact rationals"""
    ims = [image(kp, m) for kp, m in j["images"]]
    d, o, r = fold(ims, j.get("num_frames", 2), j.get("initialized", True), j.get("overlap_threshold", 0.6), j.get("ratio_threshold", 0.2))
    return {"decision": bool(d), "overlap": o, "ratio": r, "images": ims}
