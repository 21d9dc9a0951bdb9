"""An independent statement of what okvis_fe_stereo_triangulate, okvis_fe_project_landmarks and okvis_fe_gate_3d2d compute, in
numpy's long double (the x87 80-bit format where the platform has it).  TEST INFRASTRUCTURE ONLY: imports nothing from the product.

Stated from the reference (paths relative to the okvis tree):
  back_project   okvis_cv/include/okvis/cameras/implementation/PinholeCamera.hpp:426-446 with the distortion classes' undistort
                 (Gauss-Newton on distort, at most 5 steps, success below 1e-4, equidistant 1e-2, left early below 1e-15); distort is
                 sac_statement._distort, the loop is sac_statement.undistort's with the chi2 of every step kept
  project        PinholeCamera.hpp:109-146 (status rules), :148-226 (the 2x3 point Jacobian), :345-378 (projectHomogeneous: w < 0 ->
                 project(-head), the Jacobian's sign kept); CameraBase.hpp:95-104 (isInImage); RadialTangentialDistortion8.hpp:113
                 (distort fails above rho = 9)
  triangulate_fast  okvis_frontend/src/stereo_triangulation.cpp:50-137 with p1 = 0
  stereo         okvis_frontend/src/ProbabilisticStereoTriangulator.cpp:127-166 (resetFrames: H_ and sigmaRay_), :178-236
                 (stereoTriangulate), :239-250 (the overload with uncertainty), :253-355 (getUncertainty), :358-385
                 (computeReprojectionError4); the Jacobians are okvis_ceres/include/okvis/ceres/implementation/ReprojectionError.hpp
                 :95-206 (with its rule that a point nearer than 0.2 in front of the camera gets zero Jacobians)
  project_landmarks, gate   okvis_frontend/src/VioKeyframeWindowMatchingAlgorithm.cpp:177-205, :320-337, :494-512

Every comparison against a threshold goes through Ctx.lt / Ctx.gt, which keeps the compared quantity, its threshold and the scale the
distance between the two is measured in: how far a candidate sat from a decision is then a number.  The same code runs in float64
(Ctx(np.float64)) and in float64 with every sum taken in the opposite order (Ctx(np.float64, order=1)): the spread of those twins
around the long double statement is what a correct double precision evaluation may differ by.  `shift` moves every threshold by that
many bands, so that a candidate inside a band is evaluated with either outcome and everything that depends on it.  `mut` names a
deliberately wrong statement (MUTATIONS), for the sensitivity test only."""
import numpy as np

from sac_statement import DIST_EQUI, DIST_NONE, DIST_RADTAN8, _distort

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
TRI_VALID, TRI_NOT_PARALLEL, TRI_CAN_INIT, TRI_RANK_DEFICIENT = 1, 2, 4, 8
PROJ_SUCCESSFUL, PROJ_OUTSIDE_IMAGE, PROJ_MASKED, PROJ_BEHIND, PROJ_INVALID = range(5)
GATE_VERIFIED, GATE_ACCEPTED, GATE_UNCERTAIN = 1, 2, 4
MUTATIONS = ("no_pull", "jac_b_at_hp", "no_half_baseline", "size_b_for_a", "a01_sign", "fu_a_only", "p3_diagonal", "u_offdiag_once",
             "gate_floor", "gate_le")


def camera(intr, model, width=752, height=480):
    k = np.zeros(12)
    k[:len(intr)] = intr
    return {"intr": k, "model": int(model), "width": int(width), "height": int(height)}


class Ctx:
    def __init__(self, dtype=LD, order=0, bands=None, shift=0.0, mut=None):
        self.T, self.order, self.bands, self.shift, self.mut = dtype, order, bands or {}, shift, mut
        self.dec = {}

    def c(self, a):
        return np.asarray(a, dtype=self.T)

    def sum(self, terms):
        terms = list(terms)[::-1] if self.order else list(terms)
        s = terms[0]
        for t in terms[1:]:
            s = s + t
        return s

    def dot(self, a, b):
        return self.sum([a[..., i] * b[..., i] for i in range(a.shape[-1])])

    def _cmp(self, name, q, thr, active, floor, scale, op):
        q = self.c(q)
        thr = self.c(thr) + 0 * q
        if scale is None:
            scale = np.maximum(np.maximum(np.abs(thr), np.abs(q)), floor)
        scale = self.c(scale) + 0 * q
        active = np.ones(q.shape, bool) if active is None else np.asarray(active, bool) & np.ones(q.shape, bool)
        self.dec[name] = {"q": q, "thr": thr, "scale": scale, "active": active}
        t = thr + self.c(self.shift * np.asarray(self.bands.get(name, 0.0), np.float64)) * scale if self.shift else thr
        with np.errstate(invalid="ignore"):
            return op(q, t)

    def lt(self, name, q, thr, active=None, floor=0.0, scale=None):
        return self._cmp(name, q, thr, active, floor, scale, np.less)

    def gt(self, name, q, thr, active=None, floor=0.0, scale=None):
        return self._cmp(name, q, thr, active, floor, scale, np.greater)


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def undistort_steps(cx, model, k, xd, yd, tag, active):
    """sac_statement.undistort with the chi2 of every step against the exit threshold on record -> x, y, success"""
    n = len(xd)
    if model == DIST_NONE:
        return xd.copy(), yd.copy(), np.ones(n, bool)
    k = cx.c(k)
    x, y = xd.copy(), yd.copy()
    ok_below = 1e-2 if model == DIST_EQUI else 1e-4
    success, running = np.zeros(n, bool), np.ones(n, bool)
    for s in range(5):
        with np.errstate(all="ignore"):      # rows that have left the loop are computed along and thrown away
            dx, dy, (e00, e01, e10, e11) = _distort(model, k, x, y)
            r0, r1 = xd - dx, yd - dy
            a, b, c = cx.sum([e00 * e00, e10 * e10]), cx.sum([e00 * e01, e10 * e11]), cx.sum([e01 * e01, e11 * e11])
            det = a * c - b * b
            g0, g1 = cx.sum([e00 * r0, e10 * r1]), cx.sum([e01 * r0, e11 * r1])
            x = np.where(running, x + (c * g0 - b * g1) / det, x)
            y = np.where(running, y + (a * g1 - b * g0) / det, y)
        chi2 = cx.sum([r0 * r0, r1 * r1])
        # backProject's success is not read by stereoTriangulate (:192-197): no decision of these entries hangs on ok_below
        success |= running & (chi2 < ok_below)
        running &= ~cx.lt(f"{tag}undistort_exit{s}", chi2, 1e-15, active & running)
    return x, y, success


def back_project(cx, cam, kp, tag, active):
    """kp [n][3] float32 -> direction [n][3] (not normalised), success [n]"""
    fu, fv, cu, cv = cx.c(cam["intr"][:4])
    u, v = cx.c(kp[:, 0]), cx.c(kp[:, 1])
    x, y, ok = undistort_steps(cx, cam["model"], cam["intr"][4:], (u - cu) / fu, (v - cv) / fv, tag, active)
    return np.stack([x, y, np.ones_like(x)], axis=1), ok


def project(cx, cam, p, w, tag, active, want_jacobian=False):
    """projectHomogeneous of (p [n][3], w [n]) -> status [n], uv [n][2] (zeros where INVALID), J [n][2][3] (zeros where |z| < 1e-12)"""
    n = len(p)
    fu, fv, cu, cv = cx.c(cam["intr"][:4])
    sign = np.where(w < 0, -1.0, 1.0).astype(cx.T)       # the sign of an input: no rounding to consider
    x, y, z = sign * p[:, 0], sign * p[:, 1], sign * p[:, 2]
    with np.errstate(all="ignore"):
        singular = cx.lt(tag + "z_small", np.abs(z), 1.0e-12, active)
        rz = 1 / np.where(singular, cx.c(1), z)
        xn, yn = x * rz, y * rz
        dist_ok = np.ones(n, bool)
        if cam["model"] == DIST_RADTAN8:
            dist_ok = ~cx.gt(tag + "rho", cx.sum([xn * xn, yn * yn]), 9.0, active & ~singular)
        xs, ys = np.where(dist_ok, xn, 0 * xn), np.where(dist_ok, yn, 0 * yn)
        xd, yd, (e00, e01, e10, e11) = _distort(cam["model"], cx.c(cam["intr"][4:]), xs, ys)
        u, v = fu * xd + cu, fv * yd + cv
        live = active & ~singular & dist_ok
        outside = cx.lt(tag + "u_low", u, 0.0, live, floor=float(cam["intr"][2]))
        outside |= cx.lt(tag + "v_low", v, 0.0, live, floor=float(cam["intr"][3]))
        outside |= ~cx.lt(tag + "u_high", u, float(cam["width"]), live)
        outside |= ~cx.lt(tag + "v_high", v, float(cam["height"]), live)
        status = np.where(z > 0, PROJ_SUCCESSFUL, PROJ_BEHIND)   # |z| >= 1e-12 here: the sign is not in doubt
        status = np.where(outside, PROJ_OUTSIDE_IMAGE, status)
        status = np.where(singular | ~dist_ok, PROJ_INVALID, status).astype(np.uint8)
        good = (~singular & dist_ok)[:, None]
        uv = np.where(good, np.stack([u, v], axis=1), cx.c(0))
        J = None
        if want_jacobian:
            rz2 = rz * rz
            J = np.stack([np.stack([fu * e00 * rz, fu * e01 * rz, -fu * cx.sum([x * e00, y * e01]) * rz2], axis=1),
                          np.stack([fv * e10 * rz, fv * e11 * rz, -fv * cx.sum([x * e10, y * e11]) * rz2], axis=1)], axis=1)
            J = np.where(good[:, :, None], J, cx.c(0))
    return status, uv, J


def rotation(cx, q):
    """C of a Transformation built from q = (x, y, z, w), which the reference normalises"""
    q = cx.c(q)
    x, y, z, w = q / np.sqrt(cx.dot(q, q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=cx.T)


def matvec(cx, M, v):
    """rows of v [n][3] through M [3][3]"""
    return np.stack([cx.sum([M[r, c] * v[:, c] for c in range(3)]) for r in range(3)], axis=1)


# ---- triangulateFast ---------------------------------------------------------------------------------------------------------------
def triangulate_fast(cx, e1, t12, e2, sigma, active):
    """-> hp [n][4], is_valid [n], is_parallel [n]"""
    t = np.broadcast_to(t12, e1.shape)
    b0, b1 = cx.dot(t, e1), cx.dot(t, e2)
    a00, a10, a11 = cx.dot(e1, e1), cx.dot(e1, e2), -cx.dot(e2, e2)
    a01 = -a10
    wrong = cx.lt("a10_negative", a10, 0.0, active, floor=1.0)
    a10 = np.where(wrong, -a10, a10)
    if cx.mut != "a01_sign":
        a01 = np.where(wrong, -a01, a01)
    det = a00 * a11 - a01 * a10
    with np.errstate(all="ignore"):
        parallel = ~cx.gt("det", np.abs(det), 1.0e-6, active)
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        valid_par = cx.lt("cross", np.sqrt(cx.dot(cr, cr)), 6 * sigma, active & parallel)
        hpar = np.concatenate([(e1 + e2) / 2, np.full((len(e1), 1), 1e-3, dtype=cx.T)], axis=1)
        hpar = hpar / np.sqrt(cx.dot(hpar, hpar))[:, None]
        l0 = (a11 / det) * b0 + (-a01 / det) * b1
        l1 = (-a10 / det) * b0 + (a00 / det) * b1
        xm, xn = l0[:, None] * e1, l1[:, None] * e2 + t
        mid = (xm + xn) / 2
        err = mid - xm
        diff = mid if cx.mut == "no_half_baseline" else mid - t / 2
        diff2 = cx.dot(diff, diff)
        chi2 = cx.dot(err, err) * (1 / (diff2 * sigma * sigma))
        valid_np = ~cx.gt("chi2", chi2, 9.0, active & ~parallel)
        flip = cx.lt("dot", cx.dot(diff, e1), 0.0, active & ~parallel, scale=np.sqrt(diff2))
        mid = np.where(flip[:, None], t / 2 - diff, mid)
        hnp = np.concatenate([mid, np.ones((len(e1), 1), dtype=cx.T)], axis=1)
        hnp = hnp / np.sqrt(cx.dot(hnp, hnp))[:, None]
    return np.where(parallel[:, None], hpar, hnp), np.where(parallel, valid_par, valid_np), parallel


# ---- the 60-digit inverses -----------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def _to_mp(a):
    mp = _mp()
    a = np.asarray(a)
    hi = a.astype(np.float64)
    lo = (a - hi.astype(a.dtype)).astype(np.float64)
    return mp.matrix([[mp.mpf(float(h)) + mp.mpf(float(l)) for h, l in zip(rh, rl)] for rh, rl in zip(hi, lo)])


def _from_mp(M, rows, cols, dtype):
    mp = _mp()
    out = np.zeros((len(rows), len(cols)), dtype=dtype)
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            hi = float(M[r, c])
            out[i, j] = dtype(hi) + dtype(float(M[r, c] - mp.mpf(hi)))
    return out


def inverse60(A, dtype=LD, rows=None, cols=None):
    """the inverse of A with 60 significant digits, rounded to dtype (the listed rows / columns of it)"""
    n = len(A)
    return _from_mp(_to_mp(A) ** -1, range(n) if rows is None else rows, range(n) if cols is None else cols, dtype)


def gauss_jordan_inverse(A):
    """the inverse of a small matrix by Gauss-Jordan elimination with partial pivoting, in A's own type and in elementwise numpy
    operations only: what the twins invert with, so that their figures do not depend on a linear algebra library"""
    n = len(A)
    M = np.concatenate([np.array(A, copy=True), np.eye(n, dtype=A.dtype)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for r in range(n):
            if r != k:
                M[r] = M[r] - M[r, k] * M[k]
    return M[:, n:]


def referee_cov(gn):
    """bottom-right 3x3 block of the inverse of a 9x9 Gauss-Newton matrix, 60 significant digits"""
    return inverse60(gn, np.float64, range(6, 9), range(6, 9))


# ---- getUncertainty's rank decision ----------------------------------------------------------------------------------------------------
def qr_diagonal(cx, H):
    """|R_ii| of the column-pivoted Householder QR of H [n][9][9] (the pivot = the largest remaining column norm) -> [n][9]"""
    A = H.copy()
    n, m = A.shape[0], A.shape[1]
    diag = np.zeros((n, m), dtype=cx.T)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(m):
            norms = cx.sum([A[:, r, k:] * A[:, r, k:] for r in range(k, m)])            # [n][m - k]
            big = k + np.argmax(norms, axis=1)
            ck, cb = A[rows, :, k].copy(), A[rows, :, big].copy()
            A[rows, :, k], A[rows, :, big] = cb, ck
            x = A[:, k:, k]
            tail = cx.sum([x[:, r] * x[:, r] for r in range(1, m - k)]) if k < m - 1 else 0 * x[:, 0]
            c0 = x[:, 0]
            beta = np.where(c0 >= 0, -1, 1) * np.sqrt(c0 * c0 + tail)
            flat = tail == 0
            beta = np.where(flat, c0, beta)
            v = np.where(flat[:, None], 0 * x, x / np.where(flat, 1, c0 - beta)[:, None])
            v[:, 0] = 1
            tau = np.where(flat, 0 * c0, (beta - c0) / np.where(beta == 0, 1, beta))
            diag[:, k] = np.abs(beta)
            for c in range(k + 1, m):
                tcol = tau * cx.sum([v[:, r] * A[:, k + r, c] for r in range(m - k)])
                A[:, k:, c] -= tcol[:, None] * v
    return diag


# ---- stereoTriangulate and getUncertainty --------------------------------------------------------------------------------------------
def stereo(cx, cam_a, cam_b, T_AB, UOplus, kp_a, kp_b, pairs, sigma_ray=None, want_uncertainty=True):
    """-> dict: hp [n][4], cov [n][3][3], flags [n], gn [n][9][9] in cx's type; cov is the 60-digit inverse's block for the long
    double statement and two double precision inversions of the twins' own gn for the twins"""
    kp_a, kp_b = np.asarray(kp_a, np.float32).reshape(-1, 3), np.asarray(kp_b, np.float32).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    ka, kb = kp_a[pairs[:, 0]], kp_b[pairs[:, 1]]
    T_AB = cx.c(T_AB)
    r, C = T_AB[:3], rotation(cx, T_AB[3:])
    fu_min = cx.c(cam_a["intr"][0]) if cx.mut == "fu_a_only" else min(cx.c(cam_a["intr"][0]), cx.c(cam_b["intr"][0]))
    sigma = np.full(n, cx.c(0.5) / fu_min, dtype=cx.T)
    if sigma_ray is not None:
        given = cx.c(sigma_ray).reshape(n)
        sigma = np.where(given == -1.0, sigma, given)
    every = np.ones(n, bool)
    dA, _ = back_project(cx, cam_a, ka, "A_", every)
    dB, _ = back_project(cx, cam_b, kb, "B_", every)
    dBA = matvec(cx, C, dB)
    e1, e2 = dA / np.sqrt(cx.dot(dA, dA))[:, None], dBA / np.sqrt(cx.dot(dBA, dBA))[:, None]
    hp, valid, parallel = triangulate_fast(cx, e1, r, e2, sigma, every)
    sdA, sdB = cx.c(0.8) * cx.c(ka[:, 2]) / 12, cx.c(0.8) * cx.c(kb[:, 2]) / 12
    # computeReprojectionError4 in A, then in B
    stA, uvA, _ = project(cx, cam_a, hp[:, :3], hp[:, 3], "A_", valid)
    okA = valid & (stA == PROJ_SUCCESSFUL)
    dyA = uvA - np.stack([cx.c(ka[:, 0]), cx.c(ka[:, 1])], axis=1)
    sd_for_a = sdB if cx.mut == "size_b_for_a" else sdA
    with np.errstate(all="ignore"):
        errA = cx.dot(dyA, dyA / (sd_for_a * sd_for_a)[:, None])
        pB = matvec(cx, C.T, hp[:, :3] - r[None, :] * hp[:, 3:4])
        stB, uvB, _ = project(cx, cam_b, pB, hp[:, 3], "B_", okA)
        okB = okA & (stB == PROJ_SUCCESSFUL)
        dyB = uvB - np.stack([cx.c(kb[:, 0]), cx.c(kb[:, 1])], axis=1)
        errB = cx.dot(dyB, dyB / (sdB * sdB)[:, None])
        bad = cx.gt("errA", errA, 4.0, okB) | cx.gt("errB", errB, 4.0, okB)
    assigned = okB
    valid = okB & ~bad
    flags = np.where(valid, TRI_VALID, 0) | np.where(parallel, 0, TRI_NOT_PARALLEL)
    hp_out = np.where(assigned[:, None], hp, cx.c(0))
    gn, cov = np.zeros((n, 9, 9), dtype=cx.T), np.zeros((n, 3, 3), dtype=cx.T)
    if want_uncertainty and valid.any():
        with np.errstate(all="ignore"):
            w = hp[:, 3]
            # A at the identity pose: J_hpA_min = -sqrt(info) Jh
            _, _, JA = project(cx, cam_a, hp[:, :3], w, "JA_", np.zeros(n, bool), True)
            nearA = cx.lt("A_near", hp[:, 2] / w, 0.2, valid & (np.abs(w) > 1.0e-8))
            JlA = np.where(nearA[:, None, None], cx.c(0), -JA / sdA[:, None, None])
            # B at T_AB, at the point pulled 20 % towards the centre of the baseline
            half = r[None, :] / 2 * w[:, None]
            pull = cx.c(1.0) if cx.mut == "no_pull" else cx.c(0.8)
            hc = pull * (hp[:, :3] - half) + half
            dW = hc - r[None, :] * w[:, None]
            pC = matvec(cx, C.T, dW)
            _, uvC, JB = project(cx, cam_b, pC, w, "JB_", np.zeros(n, bool), True)
            resB = (np.stack([cx.c(kb[:, 0]), cx.c(kb[:, 1])], axis=1) - uvC) / sdB[:, None]
            can_init = ~cx.lt("rB", cx.dot(resB, resB), 4.0, valid)
            nearB = cx.lt("B_near", pC[:, 2] / w, 0.2, valid & (np.abs(w) > 1.0e-8))
            if cx.mut == "jac_b_at_hp":
                dW = hp[:, :3] - r[None, :] * w[:, None]
                _, _, JB = project(cx, cam_b, matvec(cx, C.T, dW), w, "JBm_", np.zeros(n, bool), True)
            Aw = np.stack([matvec(cx, C, JB[:, i, :]) for i in range(2)], axis=1) / sdB[:, None, None]    # sqrt(info) Jh C_SW
            JlB = -Aw
            rot = np.stack([np.stack([JlB[:, i, 1] * dW[:, 2] - JlB[:, i, 2] * dW[:, 1], JlB[:, i, 2] * dW[:, 0] - JlB[:, i, 0] * dW[:, 2],
                                      JlB[:, i, 0] * dW[:, 1] - JlB[:, i, 1] * dW[:, 0]], axis=1) for i in range(2)], axis=1)
            JB9 = np.concatenate([Aw * w[:, None, None], rot, JlB], axis=2)                              # [n][2][9]
            JB9 = np.where(nearB[:, None, None], cx.c(0), JB9)
            info6 = inverse60(np.asarray(UOplus, np.float64).reshape(6, 6), cx.T)
            H = np.zeros((n, 9, 9), dtype=cx.T)
            H[:, :6, :6] = info6
            H += cx.sum([JB9[:, i, :, None] * JB9[:, i, None, :] for i in range(2)])
            H[:, 6:, 6:] += cx.sum([JlA[:, i, :, None] * JlA[:, i, None, :] for i in range(2)])
            d = qr_diagonal(cx, H)
            dmax = d.max(axis=1)
            deficient = ~cx.gt("rank", d.min(axis=1) / np.where(dmax > 0, dmax, 1) / (9 * EPS64), 1.0, valid, scale=1.0)
        gn = np.where(valid[:, None, None], H, cx.c(0))
        flags = flags | np.where(valid & deficient, TRI_RANK_DEFICIENT, 0) | np.where(valid & ~deficient & can_init & ~parallel, TRI_CAN_INIT, 0)
        for i in np.flatnonzero(valid & ~deficient):
            if cx.T == LD:
                cov[i] = inverse60(H[i], LD, range(6, 9), range(6, 9))
            elif cx.order == 0:
                cov[i] = gauss_jordan_inverse(H[i])[6:, 6:]
            else:   # the Schur complement of the point block
                X = gauss_jordan_inverse(H[i, :6, :6])
                XB = np.stack([cx.sum([X[:, k] * H[i, k, 6 + c] for k in range(6)]) for c in range(3)], axis=1)
                Sc = H[i, 6:, 6:] - np.stack([cx.sum([H[i, 6:, k] * XB[k, c] for k in range(6)]) for c in range(3)], axis=1)
                cov[i] = gauss_jordan_inverse(Sc)
    return {"hp": hp_out, "cov": cov, "flags": flags.astype(np.uint8), "gn": gn}


# ---- 3D-2D -------------------------------------------------------------------------------------------------------------------------
def project_landmarks(cx, cam, T_CbW, P3, hp_W):
    """-> dict: uv [n][2] (zeros where INVALID), U [n][2][2], status [n]"""
    h = cx.c(hp_W).reshape(-1, 4)
    T = cx.c(T_CbW)
    C = rotation(cx, T[3:])
    p = matvec(cx, C, h[:, :3]) + T[None, :3] * h[:, 3:4]
    status, uv, J = project(cx, cam, p, h[:, 3], "", np.ones(len(h), bool), True)
    P = cx.c(P3).reshape(3, 3)
    if cx.mut == "p3_diagonal":
        P = np.diag(np.diag(P))
    JP = np.stack([np.stack([cx.sum([J[:, r, k] * P[k, c] for k in range(3)]) for c in range(3)], axis=1) for r in range(2)], axis=1)
    U = np.stack([np.stack([cx.sum([JP[:, r, k] * J[:, c, k] for k in range(3)]) for c in range(2)], axis=1) for r in range(2)], axis=1)
    return {"uv": uv, "U": U, "status": status}


def gate(cx, uv, U, kp_b, pairs):
    """-> dict: chi2 [n], flags [n]"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    uv, U = cx.c(uv).reshape(-1, 2)[pairs[:, 0]], cx.c(U).reshape(-1, 2, 2)[pairs[:, 0]]
    kb = np.asarray(kp_b, np.float32).reshape(-1, 3)[pairs[:, 1]]
    sd = cx.c(0.8) * cx.c(kb[:, 2]) / 12
    s2 = sd * sd
    u00, u01, u10, u11 = s2 + U[:, 0, 0], U[:, 0, 1], U[:, 1, 0], s2 + U[:, 1, 1]
    if cx.mut == "u_offdiag_once":
        u10 = u01
    e0, e1 = uv[:, 0] - cx.c(kb[:, 0]), uv[:, 1] - cx.c(kb[:, 1])
    det = u00 * u11 - u01 * u10
    # err^T U^-1 err with U^-1 = [u11 -u01; -u10 u00] / det
    chi2 = cx.sum([e0 * cx.sum([u11 / det * e0, -u01 / det * e1]), e1 * cx.sum([-u10 / det * e0, u00 / det * e1])])
    # verifyMatch: `const int chi2 = ...; if (chi2 < 4.0)`: the conversion truncates towards zero, and every negative integer is < 4
    below = cx.lt("gate_chi2_lt", chi2, 4.0) if cx.mut != "gate_le" else ~cx.gt("gate_chi2_lt", chi2, 4.0)
    if cx.mut == "gate_floor":
        below &= chi2 > -1.0
    accepted = ~cx.gt("gate_chi2_gt", chi2, 4.0)
    norm = np.sqrt(cx.sum([u00 * u00, u01 * u01, u10 * u10, u11 * u11]))
    uncertain = cx.gt("gate_norm", norm, 25.0 / (s2 * np.sqrt(cx.c(2))))
    flags = np.where(below, GATE_VERIFIED, 0) | np.where(accepted, GATE_ACCEPTED, 0) | np.where(uncertain, GATE_UNCERTAIN, 0)
    return {"chi2": chi2, "flags": flags.astype(np.uint8)}


# ---- how a result is compared with the statement -------------------------------------------------------------------------------------
ULP_FLOOR = 8 * EPS64      # where the twins agree with the statement to the last bit, the bound is a few ulp


def evaluate(fn, *args, **kw):
    """the statement and its two double precision twins -> (stmt, twin0, twin1), each (result dict, decisions)"""
    out = []
    for cx in (Ctx(LD), Ctx(np.float64), Ctx(np.float64, order=1)):
        res = fn(cx, *args, **kw)
        out.append((res, cx.dec))
    return out


def block_error(got, want, block_axes):
    """|got - want| relative to the largest |want| of each candidate's block, per candidate"""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    if not block_axes:
        return np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    scale = np.abs(want).max(axis=block_axes)
    err = np.abs(got - want).max(axis=block_axes)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))


def bands(evals, per_candidate=("rank",)):
    """4 x the twins' deviation from the statement for every decision quantity, in units of its scale: one number per decision
    (the largest over the candidates of the case whose three evaluations ran the same decisions), with ULP_FLOOR as the least.
    `rank` is banded per candidate: its quantity has an absolute error of about one unit whatever its size (the smallest |R_ii|
    inherits eps64 of the largest), so one candidate near the threshold would otherwise put every candidate inside the band."""
    (_, d0), (_, d1), (_, d2) = evals
    out = {}
    for name, s in d0.items():
        e = np.zeros(s["q"].shape, LD)
        for tw in (d1, d2):
            if name in tw:
                both = s["active"] & tw[name]["active"]
                with np.errstate(all="ignore"):
                    dev = np.abs(np.asarray(tw[name]["q"], LD) - s["q"]) / s["scale"]
                e = np.maximum(e, np.where(both & np.isfinite(dev), dev, 0))
        if name in per_candidate:
            out[name] = np.maximum(4 * e, 0.5).astype(np.float64)
        else:
            out[name] = max(4 * float(e.max()) if e.size else 0.0, ULP_FLOOR)
    return out


def distances(dec):
    """per decision: how far each active candidate sits from the threshold, in units of the scale (inf where not active)"""
    out = {}
    for name, s in dec.items():
        with np.errstate(all="ignore"):
            d = np.abs(s["q"] - s["thr"]) / s["scale"]
        out[name] = np.where(s["active"], np.where(np.isfinite(d), d, np.inf), np.inf)
    return out


def compared(dec, band):
    """the candidates whose every decision lies further from its threshold than the band"""
    keep = None
    for name, d in distances(dec).items():
        k = d > band[name]
        keep = k if keep is None else keep & k
    return keep


# ---- the verdict ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = {"stereo": {"hp": (1,), "gn": (1, 2), "cov": (1, 2)}, "project": {"uv": (1,), "U": (1, 2)}, "gate": {"chi2": ()}}
FLAGS = {"stereo": "flags", "project": "status", "gate": "flags"}
FUNCTIONS = {"stereo": stereo, "project": project_landmarks, "gate": gate}


def live_rows(entry, stmt, name, of_reference=False):
    """the candidates whose output `name` the contract defines"""
    if entry == "project" and (name == "U" or of_reference):
        # the reference leaves the Jacobian of an INVALID projection unset, and writes a pixel the entry's contract keeps at zero
        return stmt["status"] != PROJ_INVALID
    return np.ones(len(stmt[FLAGS[entry]]), bool)


def judge(entry, args, got, recorded=None, kw=None, evals=None, of_reference=False, exact_rows=None):
    """`got` (the outputs of a kernel, or of whatever stands in for it) against the statement of fn(*args).
    -> dict: e_ref / figure / bound per output, keep (the candidates compared exactly), band, failures (a list of strings, empty when
    `got` passes).  recorded: outputs of the reference build for the same arguments; they widen e_ref where present."""
    kw = kw or {}
    fn = FUNCTIONS[entry]
    evals = evals or evaluate(fn, *args, **kw)
    (stmt, dec), (t0, _), (t1, _) = evals
    band = bands(evals)
    keep = compared(dec, band)
    if exact_rows is not None:       # rows built so that no arithmetic rounds: compared even on a threshold
        keep[np.asarray(exact_rows)] = True
    fl = FLAGS[entry]
    n = len(stmt[fl])
    out = {"keep": keep, "band": band, "n": n, "left_out": int((~keep).sum()), "failures": [], "e_ref": {}, "figure": {}, "bound": {},
           "stmt": stmt, "dec": dec, "twins": (t0, t1)}
    # e_ref is measured wherever the three evaluations took the same decisions, inside a band or not
    same_path = (t0[fl] == stmt[fl]) & (t1[fl] == stmt[fl])
    for name, axes in OUTPUTS[entry].items():
        if name not in got:
            continue
        rows = live_rows(entry, stmt, name)
        e = 0.0
        for other in (t0, t1, recorded):
            ref_rows = same_path & rows & (live_rows(entry, stmt, name, True) if other is recorded else True)
            if other is not None and name in other and ref_rows.any():
                e = max(e, float(block_error(other[name], stmt[name], axes)[ref_rows].max()))
        out["e_ref"][name] = e
        out["bound"][name] = max(4 * e, ULP_FLOOR)
    wrong = keep & (np.asarray(got[fl]) != stmt[fl])
    if wrong.any():
        out["failures"].append(f"{fl} differ at compared candidates {np.flatnonzero(wrong)[:8].tolist()}: "
                               f"got {np.asarray(got[fl])[wrong][:8].tolist()} want {stmt[fl][wrong][:8].tolist()}")
    for name, axes in OUTPUTS[entry].items():
        if name not in got:
            continue
        rows = keep & live_rows(entry, stmt, name, of_reference)
        err = block_error(got[name], stmt[name], axes)
        out["figure"][name] = float(err[rows].max()) if rows.any() else 0.0
        if out["figure"][name] > out["bound"][name]:
            out["failures"].append(f"{name}: {out['figure'][name]:.3e} above the bound {out['bound'][name]:.3e} (e_ref {out['e_ref'][name]:.3e}) "
                                   f"at candidate {int(np.flatnonzero(rows)[np.argmax(err[rows])])}")
    # inside a band: one of the outcomes the statement allows on either side, with everything that depends on it
    inside = np.flatnonzero(~keep)
    if len(inside):
        variants = [stmt, t0, t1]
        for shift in (-1.0, 1.0):
            cx = Ctx(LD, bands=band, shift=shift)
            variants.append(fn(cx, *args, **kw))
        for i in inside:
            fits = False
            for v in variants:
                if np.asarray(got[fl])[i] != v[fl][i]:
                    continue
                fits = True
                for name, axes in OUTPUTS[entry].items():
                    if name in got and live_rows(entry, v, name, of_reference)[i]:
                        if float(block_error(np.asarray(got[name])[i:i + 1], np.asarray(v[name])[i:i + 1], axes)[0]) > out["bound"][name]:
                            fits = False
                if fits:
                    break
            if not fits:
                out["failures"].append(f"candidate {int(i)} inside a band fits no allowed outcome ({fl} {int(np.asarray(got[fl])[i])})")
    return out
