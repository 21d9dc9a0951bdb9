"""An independent statement of the reprojection factor and of the landmark-side linearisation arrays, parametrised by the
number format — TEST INFRASTRUCTURE, host only (numpy).

One observation (reference okvis_ceres/include/okvis/ceres/implementation/ReprojectionError.hpp:87-242, in its matrix form):

    hp_S = T_SW hp_W,  hp_C = T_CS hp_S,  kp = projectHomogeneous(hp_C),  r = sqrtInfo (z - kp)
    J_pose = Jh T_CS [ C_SW w | -C_SW [hp_W - r_WS w]x ]          (:156-167)
    J_lm   = -Jh T_CS T_SW  (first three columns)                 (:188-206)
    J_ext  = Jh [ C_CS w_S | -C_CS [hp_S - r_SC w_S]x ]           (:208-219)

with Jh = sqrtInfo * d(kp)/d(p_C) of the pinhole projection (okvis_cv PinholeCamera.hpp project / projectHomogeneous: a point with
negative scale is projected as -head, the Jacobian keeps its sign) and the distortion models none, radial-tangential,
equidistant and radial-tangential with eight coefficients.  The distortion Jacobians are derived here by the chain rule from the
models' definitions.

dtype = numpy.float64 restates the CPU oracle.  dtype = numpy.float32 follows the documented design of the mixed-precision
linearisation (okvis_amd/csrc/ba_math.hpp, "reduced-precision linearisation"): the translation hp_W - r_WS w and the
measurement minus the principal point are differences formed in float64 and then rounded; every other operation — rotations, the
second translation p_S - r_SC w_S (|r_SC| ~ 0.1 m), projection, distortion, Jacobians, the Cauchy weight, the sums over
observations — is float32.  All constants are wrapped in the dtype, so no operation is silently promoted.

`mutate` deliberately breaks one term (tests/test_fp32_statement_host.py proves that the referee's inputs would notice):

    "radtan_j00"   6 p2 u0 -> 2 p2 u0 in the radial-tangential dd0/du0
    "equi_dpoly"   the 9 k4 theta^8 term of the equidistant d(theta_d)/d(theta) dropped
    "je_sign"      one sign in the rotation columns of J_ext
    "jp_trans"     the translation columns of J_pose (= -w J_lm) taken with +

and, in the sums of window_arrays (what a kernel's reduction or robustifier could get wrong; tests/test_fp64_statement_host.py):

    "drop_last_obs"  the last observation of one landmark (drop_landmark(w)) left out of V, b, H_l and W
    "rho_prime"      the Jacobians scaled by rho' instead of sqrt(rho')
    "hq_robust"      LM_HQ summed from the robustified Jacobians

dtype = numpy.longdouble (x87 extended) evaluates everything, the two differences included, in long double; keep_dtype = True then
returns the arrays unrounded.  scales = True adds, per refereed array, what every entry is a sum OF in absolute values (as
tests/schur_statement.py does for S): sum over the observations of a_A^T a_B for LM_V, LM_HQ, LM_B, PAIR_W, and
s (|z - c| + f a_d) for OBS_RESIDUAL.  The plain |J| and |f d| do not serve as a_J and a_d: the Jacobian entries and the projected
point are themselves cancelling sums (products of rotations with differences), and with the plain scale the deviation of two
correct fp64 evaluations reaches 1.7e-13 = 1500 x 2^-53 (OBS_RESIDUAL of a point that projects next to the principal point,
PAIR_W).  So the scale is built from the operands' magnitudes, the way the Schur statement does: a_Jl = |Jh| |C_CS| |C_SW|, a_Jp =
|Jh| |C_CS| [ |C_SW| |w| , |C_SW| |[dW]x| ], a_Je = |Jh| [ |C_CS| |w| , |C_CS| |[eS]x| ] with |Jh| = s f |Jd| |du|, and a_d = |d| +
|Jd| (a_pC_xy + |u| a_pC_z) / |z| with a_pC = |C_CS| (|C_SW| |dW| + |r_SC w|).  An entry whose scale is zero had nothing added.
"""
from __future__ import annotations

import numpy as np

DIST_NONE, DIST_RADTAN, DIST_EQUIDISTANT, DIST_RADTAN8 = 0, 1, 2, 3
MUTATIONS = ("radtan_j00", "equi_dpoly", "je_sign", "jp_trans")
SUM_MUTATIONS = ("drop_last_obs", "rho_prime", "hq_robust")
ARRAYS = ("OBS_RESIDUAL", "LM_V", "LM_B", "LM_HQ", "PAIR_W")
MIN_DEPTH = 0.2      # ReprojectionError.hpp:147


def _rotation(q, T):
    """C of the Hamilton quaternion (x, y, z, w) as Eigen's toRotationMatrix forms it (no normalisation)."""
    x, y, z, w = (T(v) for v in q)
    one, two = T(1), T(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=T)


def _cross(p, T):
    z = T(0)
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=T)


def distort(model, k, u0, u1, T, mutate=None):
    """(d0, d1, J 2x2) of the distortion model at the normalised point (u0, u1), or None where the model is undefined."""
    one, two = T(1), T(2)
    if model == DIST_NONE:
        return u0, u1, np.array([[one, T(0)], [T(0), one]], dtype=T)
    if model == DIST_RADTAN:
        # d = u (1 + k1 rho + k2 rho^2) + tangential(p1, p2),  rho = |u|^2
        k1, k2, p1, p2 = k[0], k[1], k[2], k[3]
        rho = u0 * u0 + u1 * u1
        rad = k1 * rho + k2 * rho * rho
        drad = k1 + two * k2 * rho                       # d(rad)/d(rho); d(rho)/du_i = 2 u_i
        d0 = u0 + u0 * rad + two * p1 * u0 * u1 + p2 * (rho + two * u0 * u0)
        d1 = u1 + u1 * rad + two * p2 * u0 * u1 + p1 * (rho + two * u1 * u1)
        c00 = T(2) if mutate == "radtan_j00" else T(6)
        j00 = one + rad + two * u0 * u0 * drad + two * p1 * u1 + c00 * p2 * u0
        j01 = two * u0 * u1 * drad + two * p1 * u0 + two * p2 * u1
        j11 = one + rad + two * u1 * u1 * drad + T(6) * p1 * u1 + two * p2 * u0
        return d0, d1, np.array([[j00, j01], [j01, j11]], dtype=T)
    if model == DIST_EQUIDISTANT:
        # d = u f(r) / r,  f = theta (1 + k1 theta^2 + ... + k4 theta^8),  theta = atan r
        k1, k2, k3, k4 = k[0], k[1], k[2], k[3]
        r2 = u0 * u0 + u1 * u1
        r = np.sqrt(r2)
        if not r > T(1e-8):
            return u0, u1, np.array([[one, T(0)], [T(0), one]], dtype=T)
        th = np.arctan(r)
        t2 = th * th
        t4, t6, t8 = t2 * t2, t2 * t2 * t2, t2 * t2 * t2 * t2
        f = th * (one + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8)
        dpoly = one + T(3) * k1 * t2 + T(5) * k2 * t4 + T(7) * k3 * t6
        if mutate != "equi_dpoly":
            dpoly = dpoly + T(9) * k4 * t8
        df = dpoly / (one + r2)                          # f'(r): d(theta)/dr = 1 / (1 + r^2)
        s = f / r
        g = (df - s) / r2                                # J = s I + u u^T (f' r - f) / r^3
        return s * u0, s * u1, np.array([[s + u0 * u0 * g, u0 * u1 * g], [u0 * u1 * g, s + u1 * u1 * g]], dtype=T)
    if model == DIST_RADTAN8:
        # d = u N(rho) / D(rho) + tangential(p1, p2); undefined beyond rho = 9 (RadialTangentialDistortion8.hpp)
        k1, k2, p1, p2, k3, k4, k5, k6 = (k[i] for i in range(8))
        rho = u0 * u0 + u1 * u1
        if rho > T(9):
            return None
        num = one + rho * (k1 + rho * (k2 + rho * k3))
        den = one + rho * (k4 + rho * (k5 + rho * k6))
        rad = num / den
        dnum = k1 + rho * (two * k2 + T(3) * k3 * rho)
        dden = k4 + rho * (two * k5 + T(3) * k6 * rho)
        drad = (dnum * den - num * dden) / (den * den)
        d0 = u0 * rad + two * p1 * u0 * u1 + p2 * (rho + two * u0 * u0)
        d1 = u1 * rad + two * p2 * u0 * u1 + p1 * (rho + two * u1 * u1)
        j00 = rad + two * u0 * u0 * drad + two * p1 * u1 + T(6) * p2 * u0
        j01 = two * u0 * u1 * drad + two * p1 * u0 + two * p2 * u1
        j11 = rad + two * u1 * u1 * drad + T(6) * p1 * u1 + two * p2 * u0
        return d0, d1, np.array([[j00, j01], [j01, j11]], dtype=T)
    raise ValueError(model)


def observation(pose, ext, lm, intr, model, uv, sqrt_w, dtype=np.float64, mutate=None):
    """One observation: dict(r [2], Jp [2,6], Jl [2,3], Je [2,6], depth, defined, valid).  `r` is the weighted, NOT robustified
    residual; an undefined projection gives zeros throughout, an invalid one (depth below 0.2 m) keeps r and zeroes the
    Jacobians.  depth = p_C.z / w (inf when |w| <= 1e-8: the reference then makes no validity check)."""
    T = dtype
    D = np.result_type(T, np.float64).type                            # the two differences: float64, or long double under it
    pose, ext, lm, intr = (np.asarray(a, np.float64) for a in (pose, ext, lm, intr))
    out = dict(r=np.zeros(2, T), Jp=np.zeros((2, 6), T), Jl=np.zeros((2, 3), T), Je=np.zeros((2, 6), T), depth=np.inf,
               defined=False, valid=False, r_scale=np.zeros(2, T), aJp=np.zeros((2, 6), T), aJl=np.zeros((2, 3), T),
               aJe=np.zeros((2, 6), T))
    with np.errstate(all="ignore"):
        C_WS, C_SC = _rotation(pose[3:7], T), _rotation(ext[3:7], T)
        C_SW, C_CS = C_WS.T, C_SC.T
        w64 = lm[3]
        w = T(w64)
        dW = (lm[:3].astype(D) - pose[:3].astype(D) * D(w64)).astype(T)   # float64 difference, then rounded
        pS = C_SW @ dW
        eS = pS - ext[:3].astype(T) * w                               # sensor-scale coordinates: dtype arithmetic
        pC = C_CS @ eS
        x, y, z = (-pC if w64 < 0 else pC)
        if abs(w64) > 1.0e-8:
            out["depth"] = float(pC[2] / w)
        if not abs(z) >= T(1.0e-12):
            return out
        u0, u1 = x / z, y / z
        k = intr[4:12].astype(T)
        dist = distort(model, k, u0, u1, T, mutate)
        if dist is None:
            return out
        out["defined"] = True
        d0, d1, Jd = dist
        fu, fv, s = T(intr[0]), T(intr[1]), T(sqrt_w)
        z0, z1 = T(D(uv[0]) - D(intr[2])), T(D(uv[1]) - D(intr[3]))
        out["r"] = np.array([s * (z0 - fu * d0), s * (z1 - fv * d1)], dtype=T)
        # the operands' magnitudes: p_C is a sum of rotated differences, a_pC = |C_CS| (|C_SW| |dW| + |r_SC w|) what it is a sum of;
        # u = p / z and the distortion hand that on to first order: a_d = |d| + |Jd| (a_pC_xy + |u| a_pC_z) / |z|
        a_pC = np.abs(C_CS) @ (np.abs(C_SW) @ np.abs(dW) + np.abs(ext[:3].astype(T) * w))
        a_u = np.array([a_pC[0] + abs(u0) * a_pC[2], a_pC[1] + abs(u1) * a_pC[2]], dtype=T) / abs(z)
        a_d = np.array([abs(d0), abs(d1)], dtype=T) + np.abs(Jd) @ a_u
        out["r_scale"] = np.array([s * (abs(z0) + fu * a_d[0]), s * (abs(z1) + fv * a_d[1])], dtype=T)
        if abs(w64) > 1.0e-8 and pC[2] / w < T(MIN_DEPTH):
            return out
        out["valid"] = True
        # Jh = sqrtInfo diag(fu, fv) Jd d(u)/d(p),  d(u)/d(p) = [ I / z | -u / z ]
        du = np.array([[T(1) / z, T(0), -u0 / z], [T(0), T(1) / z, -u1 / z]], dtype=T)
        Jh = np.array([[s * fu], [s * fv]], dtype=T) * (Jd @ du)
        Jh_CS = Jh @ C_CS
        out["Jl"] = -(Jh_CS @ C_SW)
        out["Jp"] = Jh_CS @ np.concatenate([C_SW * w, -(C_SW @ _cross(dW, T))], axis=1)
        out["Je"] = Jh @ np.concatenate([C_CS * w, -(C_CS @ _cross(eS, T))], axis=1)
        aJh = np.abs(np.array([[s * fu], [s * fv]], dtype=T)) * (np.abs(Jd) @ np.abs(du))
        aJh_CS = aJh @ np.abs(C_CS)
        out["aJl"] = aJh_CS @ np.abs(C_SW)
        out["aJp"] = aJh_CS @ np.concatenate([np.abs(C_SW) * abs(w), np.abs(C_SW) @ np.abs(_cross(dW, T))], axis=1)
        out["aJe"] = aJh @ np.concatenate([np.abs(C_CS) * abs(w), np.abs(C_CS) @ np.abs(_cross(eS, T))], axis=1)
        if mutate == "jp_trans":
            out["Jp"][:, :3] = -out["Jp"][:, :3]
        if mutate == "je_sign":
            out["Je"][0, 4] = -out["Je"][0, 4]
    return out


def pairs(w):
    """(pair_lm, pair_block): the (landmark, free pose block) pairs of a window, by landmark, then by block index."""
    free = np.asarray(w.pose_fixed).reshape(-1) == 0
    seen = set()
    for l, ip, ie in zip(np.asarray(w.obs_lm), np.asarray(w.obs_pose), np.asarray(w.obs_ext)):
        for blk in (int(ip), int(ie)):
            if free[blk]:
                seen.add((int(l), blk))
    ordered = sorted(seen)
    return np.array([p[0] for p in ordered], np.int32), np.array([p[1] for p in ordered], np.int32)


_UT = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def drop_landmark(w):
    """the landmark whose last observation the mutation "drop_last_obs" leaves out: the last one with two observations or more"""
    counts = np.bincount(np.asarray(w.obs_lm), minlength=w.n_lm)
    return int(np.flatnonzero(counts >= 2)[-1])


def window_arrays(w, dtype=np.float64, mutate=None, keep_dtype=False, scales=False, reverse=False):
    """The landmark-side linearisation of a whole Window at its state, laid out as WindowBatch.array / OracleWindow.array return
    them (flat float64): OBS_RESIDUAL [n_obs, 2], LM_V [n_lm, 6] and LM_HQ [n_lm, 6] (upper triangles; LM_HQ without the robust
    weight: Map::getLhs), LM_B [n_lm, 3], PAIR_W [n_pair, 6, 3]; plus `pairs`, and per observation `depth`, `defined`, `valid`.
    Sums run in observation order (reverse: last observation first) in `dtype`; the Cauchy corrector scales r and J by sqrt(rho')
    (Ceres Corrector, rho'' <= 0).  keep_dtype: the arrays stay in `dtype`; scales: a dict `scale` of float64 arrays, see above."""
    T = dtype
    pose = np.asarray(w.pose, np.float64).reshape(-1, 7)
    lm = np.asarray(w.lm, np.float64).reshape(-1, 4)
    intr = np.asarray(w.cam_intr, np.float64).reshape(-1, 12)
    model = np.asarray(w.cam_model).reshape(-1)
    uv = np.asarray(w.obs_uv, np.float64).reshape(-1, 2)
    n_obs, n_lm = w.n_obs, w.n_lm
    pair_lm, pair_block = pairs(w)
    pair_of = {(int(l), int(b)): p for p, (l, b) in enumerate(zip(pair_lm, pair_block))}
    R = np.zeros((n_obs, 2), T)
    V, Hq, B = np.zeros((n_lm, 6), T), np.zeros((n_lm, 6), T), np.zeros((n_lm, 3), T)
    W = np.zeros((len(pair_lm), 6, 3), T)
    aR, aV, aHq, aB, aW = (np.zeros(a.shape, T) for a in (R, V, Hq, B, W))
    dropped = -1
    if mutate == "drop_last_obs":
        dropped = int(np.flatnonzero(np.asarray(w.obs_lm) == drop_landmark(w))[-1])
    ut = lambda m: np.array([m[i, j] for i, j in _UT], dtype=T)      # noqa: E731
    depth, defined, valid = np.full(n_obs, np.inf), np.zeros(n_obs, bool), np.zeros(n_obs, bool)
    bb = T(float(w.cauchy_b) * float(w.cauchy_b))
    for o in (range(n_obs - 1, -1, -1) if reverse else range(n_obs)):
        l, ip, ie, c = int(w.obs_lm[o]), int(w.obs_pose[o]), int(w.obs_ext[o]), int(w.obs_cam[o])
        ob = observation(pose[ip], pose[ie], lm[l], intr[c], int(model[c]), uv[o], float(w.obs_sqrtw[o]), T, mutate)
        depth[o], defined[o], valid[o] = ob["depth"], ob["defined"], ob["valid"]
        r, Jp, Jl, Je = ob["r"], ob["Jp"], ob["Jl"], ob["Je"]
        R[o] = r
        aR[o] = ob["r_scale"]
        if o == dropped:
            continue
        sr = T(1)
        if w.cauchy_b > 0:
            sr = np.sqrt(T(1) / (T(1) + (r[0] * r[0] + r[1] * r[1]) / bb))
        sj = sr * sr if mutate == "rho_prime" else sr
        rs, Jps, Jls, Jes = sr * r, sj * Jp, sj * Jl, sj * Je
        Hq[l] += ut(Jls.T @ Jls if mutate == "hq_robust" else Jl.T @ Jl)
        V[l] += ut(Jls.T @ Jls)
        B[l] += Jls.T @ rs
        if (l, ip) in pair_of:
            W[pair_of[(l, ip)]] += Jps.T @ Jls
        if (l, ie) in pair_of:
            W[pair_of[(l, ie)]] += Jes.T @ Jls
        if scales:
            mJp, mJl, mJe = ob["aJp"], ob["aJl"], ob["aJe"]
            aHq[l] += ut(mJl.T @ mJl)
            aV[l] += ut((sj * mJl).T @ (sj * mJl))
            aB[l] += (sj * mJl).T @ (sr * ob["r_scale"])
            if (l, ip) in pair_of:
                aW[pair_of[(l, ip)]] += (sj * mJp).T @ (sj * mJl)
            if (l, ie) in pair_of:
                aW[pair_of[(l, ie)]] += (sj * mJe).T @ (sj * mJl)
    for a in (R, V, Hq, B, W):
        assert a.dtype == T
    f = lambda a: np.asarray(a, T if keep_dtype else np.float64).reshape(-1)      # noqa: E731
    out = dict(OBS_RESIDUAL=f(R), LM_V=f(V), LM_B=f(B), LM_HQ=f(Hq), PAIR_W=f(W), pairs=(pair_lm, pair_block), depth=depth,
               defined=defined, valid=valid)
    if scales:
        g = lambda a: np.asarray(a, np.float64).reshape(-1)      # noqa: E731
        out["scale"] = dict(OBS_RESIDUAL=g(aR), LM_V=g(aV), LM_B=g(aB), LM_HQ=g(aHq), PAIR_W=g(aW))
    return out


def deviation_entrywise(a, ref, scale):
    """max |a - ref| / scale over scale > 0 (float); where the scale is zero nothing was added and `a` must equal `ref` (asserted)"""
    a, ref, scale = (np.asarray(v, np.float64) for v in (a, ref, scale))
    assert a.shape == ref.shape == scale.shape, (a.shape, ref.shape, scale.shape)
    assert np.array_equal(a[scale == 0.0], ref[scale == 0.0]), "an entry nothing sums into differs"
    on = scale > 0.0
    return float((np.abs(a - ref)[on] / scale[on]).max()) if on.any() else 0.0


def deviation(a, ref):
    """max |a - ref| / max |ref| (0 for an empty or all-zero reference that `a` matches)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    scale = np.abs(ref).max()
    err = np.abs(a - ref).max()
    return 0.0 if err == 0.0 else float(err / scale) if scale > 0 else np.inf
