"""An independent statement of what okvis_fe_bearing_vectors and okvis_fe_sac_consensus compute, in numpy's long double (the x87
80-bit format where the platform has it).  TEST INFRASTRUCTURE ONLY: imports nothing from the product.

Stated from the reference (paths relative to the okvis tree):
  bearing_vectors      okvis_frontend/src/FrameNoncentralAbsoluteAdapter.cpp:96-149, FrameRelativeAdapter.cpp:168-244; backProject =
                       okvis_cv/include/okvis/cameras/implementation/PinholeCamera.hpp:426-446 with the distortion classes' undistort
                       (Gauss-Newton on distort, at most 5 steps, left early below 1e-15)
  score_absolute       okvis_frontend/include/opengv/sac_problems/absolute_pose/FrameAbsolutePoseSacProblem.hpp:129-161
  score_rotation_only  .../relative_pose/FrameRotationOnlySacProblem.hpp:122-144
  score_relative       .../relative_pose/FrameRelativePoseSacProblem.hpp:126-161; the point it reprojects comes from
                       opengv::triangulation::triangulate2, whose source is not in the reference tree: `midpoint` states the published
                       two-view midpoint method and is not pinned to reference lines
  consensus            countWithinDistance / selectWithinDistance by the strict `<`, and the loop's rule that a hypothesis replaces
                       the best one only with strictly more inliers (so: the lowest index among the largest counts)

Everything is vectorised over the correspondences; the hypotheses are a Python loop."""
import numpy as np

LD = np.longdouble
ABSOLUTE, ROTATION_ONLY, RELATIVE = 0, 1, 2
DIST_NONE, DIST_RADTAN, DIST_EQUI, DIST_RADTAN8 = 0, 1, 2, 3


def _ld(a):
    return np.asarray(a, dtype=LD)


# ---- the adapters ------------------------------------------------------------------------------------------------------------------
def _distort(model, k, x, y):
    """distorted point and the Jacobian entries (d xd / d x, d xd / d y, d yd / d x, d yd / d y), elementwise"""
    one = np.ones_like(x)
    if model == DIST_NONE:
        return x, y, (one, 0 * one, 0 * one, one)
    if model == DIST_RADTAN:
        k1, k2, p1, p2 = k[:4]
        mx2, my2, mxy = x * x, y * y, x * y
        rho = mx2 + my2
        rad = k1 * rho + k2 * rho * rho
        xd = x + x * rad + 2 * p1 * mxy + p2 * (rho + 2 * mx2)
        yd = y + y * rad + 2 * p2 * mxy + p1 * (rho + 2 * my2)
        drad_dx = k1 * 2 * x + k2 * 4 * x * rho
        drad_dy = k1 * 2 * y + k2 * 4 * y * rho
        return xd, yd, (1 + rad + x * drad_dx + 2 * p1 * y + 6 * p2 * x, x * drad_dy + 2 * p1 * x + 2 * p2 * y,
                        y * drad_dx + 2 * p2 * y + 2 * p1 * x, 1 + rad + y * drad_dy + 2 * p2 * x + 6 * p1 * y)
    if model == DIST_RADTAN8:
        k1, k2, p1, p2, k3, k4, k5, k6 = k[:8]
        mx2, my2, mxy = x * x, y * y, x * y
        rho = mx2 + my2
        num = 1 + k1 * rho + k2 * rho ** 2 + k3 * rho ** 3
        den = 1 + k4 * rho + k5 * rho ** 2 + k6 * rho ** 3
        rad = num / den
        dnum = k1 + 2 * k2 * rho + 3 * k3 * rho ** 2
        dden = k4 + 2 * k5 * rho + 3 * k6 * rho ** 2
        drad = (dnum * den - num * dden) / (den * den)   # d rad / d rho
        xd = x * rad + 2 * p1 * mxy + p2 * (rho + 2 * mx2)
        yd = y * rad + 2 * p2 * mxy + p1 * (rho + 2 * my2)
        return xd, yd, (rad + x * drad * 2 * x + 2 * p1 * y + 6 * p2 * x, x * drad * 2 * y + 2 * p1 * x + 2 * p2 * y,
                        y * drad * 2 * x + 2 * p2 * y + 2 * p1 * x, rad + y * drad * 2 * y + 2 * p2 * x + 6 * p1 * y)
    if model == DIST_EQUI:
        k1, k2, k3, k4 = k[:4]
        r = np.sqrt(x * x + y * y)
        small = r < 1e-8
        rs = np.where(small, one, r)
        th = np.arctan(rs)
        th2 = th * th
        poly = 1 + k1 * th2 + k2 * th2 ** 2 + k3 * th2 ** 3 + k4 * th2 ** 4
        thd = th * poly
        s = np.where(small, one, thd / rs)
        dthd_dth = 1 + 3 * k1 * th2 + 5 * k2 * th2 ** 2 + 7 * k3 * th2 ** 3 + 9 * k4 * th2 ** 4
        ds_dr = np.where(small, 0 * one, (dthd_dth / (1 + rs * rs) * rs - thd) / (rs * rs))
        ds_dx, ds_dy = ds_dr * x / rs, ds_dr * y / rs
        return x * s, y * s, (s + x * ds_dx, x * ds_dy, y * ds_dx, s + y * ds_dy)
    raise ValueError(model)


def undistort(model, k, xd, yd):
    """-> x, y, success, steps (per point)"""
    k = _ld(k)
    x, y = xd.copy(), yd.copy()
    n = len(x)
    ok_below = 1e-2 if model == DIST_EQUI else 1e-4
    success = np.zeros(n, bool)
    running = np.ones(n, bool)
    steps = np.zeros(n, np.int32)
    if model == DIST_NONE:
        return x, y, np.ones(n, bool), steps
    for _ in range(5):
        dx, dy, (e00, e01, e10, e11) = _distort(model, k, x, y)
        r0, r1 = xd - dx, yd - dy
        a, b, c = e00 * e00 + e10 * e10, e00 * e01 + e10 * e11, e01 * e01 + e11 * e11
        det = a * c - b * b
        g0, g1 = e00 * r0 + e10 * r1, e01 * r0 + e11 * r1
        x = np.where(running, x + (c * g0 - b * g1) / det, x)
        y = np.where(running, y + (a * g1 - b * g0) / det, y)
        chi2 = r0 * r0 + r1 * r1
        steps += running
        success |= running & (chi2 < ok_below)
        running &= ~(chi2 < 1e-15)
    return x, y, success, steps


def bearing_vectors(intr, model, kp):
    """intr = fu fv cu cv d0..; kp [n][3] float32 (x, y, size) -> bearing [n][3], sigma_angle [n] (long double), ok [n], steps [n]"""
    intr = _ld(intr)
    kp = np.asarray(kp, np.float32).reshape(-1, 3)
    u, v, size = _ld(kp[:, 0]), _ld(kp[:, 1]), _ld(kp[:, 2])
    fu, fv, cu, cv = intr[:4]
    x, y, ok, steps = undistort(model, intr[4:], (u - cu) / fu, (v - cv) / fv)
    d = np.stack([x, y, np.ones_like(x)], axis=1)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    sd = _ld(0.8) * size / 12       # 0.8 is the double constant of the source, not 4/5
    sigma = np.sqrt(LD(2)) * sd * sd / (fu * fu)
    return d, sigma, ok, steps


# ---- the three score functions -------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _sq(v):
    return (v * v).sum(axis=1)


def score_absolute(model, points, bearing, sigma, cam_index, cam_offsets, cam_rotations):
    """model [3][4]; -> [n]"""
    T = _ld(model).reshape(3, 4)
    Ri = T[:, :3].T
    ti = -(Ri @ T[:, 3])
    body = _ld(points) @ Ri.T + ti
    ci = np.asarray(cam_index, np.int64)
    d = body - _ld(cam_offsets).reshape(-1, 3)[ci]
    C = _ld(cam_rotations).reshape(-1, 3, 3)[ci]        # [n][3][3]
    r = _unit(np.einsum("nji,nj->ni", C, d))          # C^T d
    return _sq(r - _ld(bearing)) / _ld(sigma)


def score_rotation_only(model, bearing1, bearing2, sigma1, sigma2):
    R = _ld(model).reshape(3, 3)
    f1, f2 = _ld(bearing1), _ld(bearing2)
    return _sq(f2 @ R.T - f1) * 0.5 / _ld(sigma1) + _sq(f1 @ R - f2) * 0.5 / _ld(sigma2)


def midpoint(R12, t12, f1, f2):
    """The two-view midpoint method: the closest points lambda1 f1 and t12 + lambda2 R12 f2 of the two rays, then their mean."""
    g = f2 @ R12.T
    b0, b1 = f1 @ t12, g @ t12
    a00, a10, a11 = _sq(f1), (f1 * g).sum(axis=1), -_sq(g)
    a01 = -a10
    det = a00 * a11 - a01 * a10
    l0, l1 = (a11 * b0 - a01 * b1) / det, (a00 * b1 - a10 * b0) / det
    return (l0[:, None] * f1 + (t12 + l1[:, None] * g)) / 2


def score_relative(model, bearing1, bearing2, sigma1, sigma2):
    T = _ld(model).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    f1, f2 = _ld(bearing1), _ld(bearing2)
    p = midpoint(R, t, f1, f2)
    q = p @ R + (-(R.T @ t))                          # R^T p - R^T t
    return _sq(_unit(p) - f1) * 0.5 / _ld(sigma1) + _sq(_unit(q) - f2) * 0.5 / _ld(sigma2)


def scores(job):
    """job: the dict okvis_amd.frontend.Frontend.sac_consensus takes -> [n_models][n] long double"""
    kind = int(job["kind"])
    width = 9 if kind == ROTATION_ONLY else 12
    models = np.asarray(job["models"], np.float64).reshape(-1, width)
    rows = []
    for m in models:
        if kind == ABSOLUTE:
            rows.append(score_absolute(m, job["points"], job["bearing"], job["sigma"], job["cam_index"], job["cam_offsets"],
                                       job["cam_rotations"]))
        elif kind == ROTATION_ONLY:
            rows.append(score_rotation_only(m, job["bearing1"], job["bearing2"], job["sigma1"], job["sigma2"]))
        elif kind == RELATIVE:
            rows.append(score_relative(m, job["bearing1"], job["bearing2"], job["sigma1"], job["sigma2"]))
        else:
            raise ValueError(kind)
    n = len(np.asarray(job["sigma"] if kind == ABSOLUTE else job["sigma1"]).reshape(-1))
    return np.array(rows, dtype=LD).reshape(len(models), n)


def consensus(score_matrix, threshold):
    """-> counts [K] int32, best, inliers (ascending int32) of the best hypothesis"""
    inl = np.asarray(score_matrix) < threshold
    counts = inl.sum(axis=1).astype(np.int32)
    best = int(np.argmax(counts))                     # argmax returns the first of equal maxima
    return counts, best, np.nonzero(inl[best])[0].astype(np.int32)


# ---- how two sets of scores are compared ----------------------------------------------------------------------------------------------
SCORE_FLOOR = 1e-3


def distance(got, want, floor=SCORE_FLOOR):
    """|got - want| relative to |want|, with an absolute floor: the scores are squared differences of unit vectors over a sigma of
    about 1e-6, so their error relative to themselves grows without bound as they approach zero.  Below SCORE_FLOOR (four orders of
    magnitude under the thresholds in use, 9 in the reference) the difference is measured against the floor instead."""
    got, want = _ld(got), _ld(want)
    return np.abs(got - want) / np.maximum(np.abs(want), floor)


def near_threshold(score_matrix, threshold, band):
    """the cells whose inlier decision a relative error of `band` could change"""
    return distance(_ld(threshold), score_matrix) <= band
