"""ImuError restated in plain numpy, with the number type as a parameter — TEST INFRASTRUCTURE, host only.

Written from okvis_ceres/src/ImuError.cpp: redoPreintegration (:76-284) and EvaluateWithMinimalJacobians (:514-685), and the
helpers they call (okvis_kinematics operators.hpp, implementation/Transformation.hpp:45-82).  It shares no code with oracle/ nor
with the kernel (okvis_amd/csrc/ba_imu.hpp): it is the second opinion of the IMU referee (tests/imu_cases.py).

Kept as the reference has them:
  * a step whose dt <= 0 is skipped with `continue` before anything is integrated (:140-142) — samples at or before t0, repeated
    timestamps;
  * the first integrated step interpolates its first sample to t0, the last its second sample to t1 (:131-150);
  * a saturated step multiplies its LOCAL sigma_g_c / sigma_a_c by 100 (:156-173);
  * dalpha_db_g += C_1 * rightJacobian(omega dt) * dt and sigma2_v = dt sigma_a_c^2 (:200, :234): redoPreintegration's variant,
    where ImuError::propagation has dt * C_1 (:412);
  * the weight is the Cholesky factor of the INVERSE covariance: P symmetrised, inverted, symmetrised, LLT, L^T (:271-279);
  * the double constants of the source stay doubles in every number type (1e-9 of Duration::toSec, 1.0 / 6.0 ...), as they do where
    the oracle's sources are built in long double.
Free choices are made differently from oracle/orc_factors.cpp on purpose: numpy's matrix products (BLAS order in float64),
P <- F (P F^T), a Gauss-Jordan inverse, a column Cholesky, H and g summed over the residual rows in descending order.

`mutate` names one deliberately wrong variant (tests/test_imu_statement_host.py shows that the referee notices each):
  no_t0_interpolation, drop_step_32, no_saturation, propagation_dalpha, integrate_non_advancing, transposed_F_block,
  wrong_permutation."""
from __future__ import annotations

import numpy as np

F64 = np.float64
MUTATIONS = ("no_t0_interpolation", "drop_step_32", "no_saturation", "propagation_dalpha", "integrate_non_advancing",
             "transposed_F_block", "wrong_permutation")
COLS = ((0, 6), (6, 15), (15, 21), (21, 30))     # the factor's own columns: pose0 | sb0 | pose1 | sb1


def sec(ns, T):
    """okvis::Duration::toSec of a normalised duration: sec + 1e-9 * nsec, 0 <= nsec < 1e9"""
    s, n = divmod(int(ns), 10 ** 9)
    return T(s) + T(F64(1e-9)) * T(n)


def cross_mx(v, T):
    x, y, z = v
    o = T(0)
    return np.array([[o, -z, y], [z, o, -x], [-y, x, o]], dtype=T)


def qmul(a, b):
    """Eigen's quaternion product; coefficients x, y, z, w"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], dtype=a.dtype)


def qinv(q):
    """Eigen::Quaternion::inverse: conjugate / squaredNorm"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=q.dtype) / n2


def rot(q, T):
    """Eigen's toRotationMatrix (no normalisation)"""
    x, y, z, w = q
    two = T(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = T(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=T)


def sinc(x, T):
    if abs(x) > 1e-6:
        return np.sin(x) / x
    c2, c4, c6 = T(F64(1.0) / F64(6.0)), T(F64(1.0) / F64(120.0)), T(F64(1.0) / F64(5040.0))
    x2 = x * x
    x4 = x2 * x2
    x6 = x2 * x2 * x2
    return T(1) - c2 * x2 + c4 * x4 - c6 * x6


def norm3(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def delta_q(dalpha, T):
    h = T(0.5) * norm3(dalpha)
    v = sinc(h, T) * T(0.5) * dalpha
    return np.array([v[0], v[1], v[2], np.cos(h)], dtype=T)


def right_jacobian(phi, T):
    n = norm3(phi)
    X = cross_mx(phi, T)
    X2 = X @ X
    R = np.eye(3, dtype=T)
    if n < 1.0e-4:
        return R + T(-0.5) * X + T(F64(1.0) / F64(6.0)) * X2
    n2 = n * n
    n3 = n2 * n
    return R + (-(T(1) - np.cos(n)) / n2) * X + ((n - np.sin(n)) / n3) * X2


def plus_mat(q, T):
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]], dtype=T)


def oplus_mat(q, T):
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]], dtype=T)


def inverse(A, T):
    """Gauss-Jordan with partial pivoting on [A | I]"""
    n = A.shape[0]
    M = np.concatenate([A.astype(T), np.eye(n, dtype=T)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, n:].copy()


def llt_lower(A, T):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=T)
    with np.errstate(invalid="ignore", divide="ignore"):      # (a wrong variant's matrix need not be positive definite: NaN)
        for j in range(n):
            d = A[j, j] - np.dot(L[j, :j], L[j, :j])
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def preintegrate(t, gyr, acc, prm, t0, t1, sb, dtype=np.float64, mutate=None):
    """redoPreintegration at the speed and biases sb: the record (a dict) with n_steps; None where the reference returns -1"""
    T = dtype
    t = np.asarray(t, np.int64)
    gyr, acc, sb = np.asarray(gyr, T), np.asarray(acc, T), np.asarray(sb, T)
    n = t.size
    if n == 0 or not t[-1] >= t1:
        return None
    half, quarter = T(0.5), T(0.25)
    Dq = np.array([0, 0, 0, 1], dtype=T)
    C_int, C_dint = np.zeros((3, 3), T), np.zeros((3, 3), T)
    a_int, a_dint = np.zeros(3, T), np.zeros(3, T)
    cross = np.zeros((3, 3), T)
    dalpha, dv, dp = np.zeros((3, 3), T), np.zeros((3, 3), T), np.zeros((3, 3), T)
    P = np.zeros((15, 15), T)
    I3 = np.eye(3, dtype=T)
    g_max, a_max = T(F64(prm.g_max)), T(F64(prm.a_max))
    time, Delta_t, started, steps = int(t0), T(0), False, 0
    for it in range(n):
        w0, a0 = gyr[it].copy(), acc[it].copy()
        nx = min(it + 1, n - 1)          # (the reference reads it + 1 before its end check; the value is unused at the last sample)
        w1, a1 = gyr[nx].copy(), acc[nx].copy()
        nexttime = int(t1) if it + 1 == n else int(t[it + 1])
        dt = sec(nexttime - time, T)
        if t1 < nexttime:
            interval = sec(nexttime - int(t[it]), T)
            nexttime = int(t1)
            dt = sec(nexttime - time, T)
            r = dt / interval
            w1 = (T(1) - r) * w0 + r * w1
            a1 = (T(1) - r) * a0 + r * a1
        if dt <= 0 and not (mutate == "integrate_non_advancing" and nexttime != int(t[it])):
            continue
        if mutate == "drop_step_32" and steps == 32:
            time = nexttime
            steps += 1
            if nexttime == t1:
                break
            continue
        Delta_t = Delta_t + dt
        if not started:
            started = True
            if mutate != "no_t0_interpolation":
                r = dt / sec(nexttime - int(t[it]), T)
                w0 = r * w0 + (T(1) - r) * w1
                a0 = r * a0 + (T(1) - r) * a1
        sigma_g_c, sigma_a_c = T(F64(prm.sigma_g_c)), T(F64(prm.sigma_a_c))
        if mutate != "no_saturation":
            if max(np.abs(w0).max(), np.abs(w1).max()) > g_max:
                sigma_g_c = sigma_g_c * T(100)
            if max(np.abs(a0).max(), np.abs(a1).max()) > a_max:
                sigma_a_c = sigma_a_c * T(100)
        # orientation (:177-185)
        w_true = half * (w0 + w1) - sb[3:6]
        th = norm3(w_true) * half * dt
        v = sinc(th, T) * w_true * half * dt
        dq = np.array([v[0], v[1], v[2], np.cos(th)], dtype=T)
        Dq1 = qmul(Dq, dq)
        # rotation matrix integrals (:187-197)
        C, C1 = rot(Dq, T), rot(Dq1, T)
        a_true = half * (a0 + a1) - sb[6:9]
        CC = C + C1
        C_int1 = C_int + half * CC * dt
        a_int1 = a_int + (half * CC) @ a_true * dt
        C_dint = C_dint + (C_int * dt + quarter * CC * dt * dt)
        a_dint = a_dint + (a_int * dt + (quarter * CC) @ a_true * dt * dt)
        # Jacobian parts (:200-207)
        Jr = right_jacobian(w_true * dt, T)
        dalpha = dalpha + (dt * C1 if mutate == "propagation_dalpha" else (C1 @ Jr) * dt)
        cross1 = rot(qinv(dq), T) @ cross + Jr * dt
        ax = cross_mx(a_true, T)
        G = (C @ ax) @ cross + (C1 @ ax) @ cross1
        dv1 = dv + half * dt * G
        dp_term = dt * dv + quarter * dt * dt * G
        dp = dp + dp_term
        # covariance (:210-249)
        F = np.eye(15, dtype=T)
        F[0:3, 3:6] = -cross_mx(a_int * dt + (quarter * CC) @ a_true * dt * dt, T)
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = dp_term
        F[0:3, 12:15] = -C_int * dt + quarter * CC * dt * dt
        F[3:6, 9:12] = -dt * C1
        F[6:9, 3:6] = -cross_mx((half * CC) @ a_true * dt, T)
        F[6:9, 9:12] = half * dt * G
        F[6:9, 12:15] = -half * CC * dt
        P = F @ (P @ F.T)
        s2_dalpha = dt * sigma_g_c * sigma_g_c
        s2_v = dt * sigma_a_c * sigma_a_c
        s2_p = half * dt * dt * s2_v
        s2_bg = dt * T(F64(prm.sigma_gw_c)) * T(F64(prm.sigma_gw_c))
        s2_ba = dt * T(F64(prm.sigma_aw_c)) * T(F64(prm.sigma_aw_c))
        for k in range(3):
            P[3 + k, 3 + k] += s2_dalpha
            P[6 + k, 6 + k] += s2_v
            P[k, k] += s2_p
            P[9 + k, 9 + k] += s2_bg
            P[12 + k, 12 + k] += s2_ba
        # memory shift (:252-257)
        Dq, C_int, a_int, cross, dv = Dq1, C_int1, a_int1, cross1, dv1
        time = nexttime
        steps += 1
        if nexttime == t1:
            break
    P = half * P + half * P.T
    info = inverse(P, T)
    info = half * info + half * info.T
    sqrt_info = llt_lower(info, T).T.copy()
    return dict(Delta_q=Dq, C_integral=C_int, C_doubleintegral=C_dint, acc_integral=a_int, acc_doubleintegral=a_dint,
                dalpha_db_g=dalpha, dv_db_g=dv, dp_db_g=dp, sqrt_info=sqrt_info, sb_ref=sb.copy(), P=P, information=info,
                n_steps=steps)


def _transformation(pose, T):
    pose = np.asarray(pose, T)
    q = pose[3:7]
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])      # Transformation(r, q): q.normalized()
    return pose[0:3].copy(), q, rot(q, T)


def evaluate(t, gyr, acc, prm, t0, t1, pose0, sb0, pose1, sb1, sb_ref=None, dtype=np.float64, mutate=None):
    """EvaluateWithMinimalJacobians of a factor whose record is new (sb_ref None: redo_ = true) or was built at sb_ref.
    Returns the record's fields plus redo_count (re-preintegrations this evaluation made), F [15][30], e, J, r, H [30][30], g, cost."""
    T = dtype
    sb0, sb1 = np.asarray(sb0, T), np.asarray(sb1, T)
    r0, q0, C_WS_0 = _transformation(pose0, T)
    r1, q1, _ = _transformation(pose1, T)
    C_S0_W = C_WS_0.T
    Dt = sec(int(t1) - int(t0), T)
    redo = sb_ref is None
    rec = None
    if not redo:
        rec = preintegrate(t, gyr, acc, prm, t0, t1, sb_ref, T, mutate)
        Delta_b = sb0[3:9] - rec["sb_ref"][3:9]
        redo = bool(norm3(Delta_b[0:3]) * Dt > 0.0001)
    redo_count = 0
    if redo:
        rec = preintegrate(t, gyr, acc, prm, t0, t1, sb0, T, mutate)
        redo_count = 1
        Delta_b = np.zeros(6, T)
    half = T(0.5)
    g_W = np.array([0, 0, 1], dtype=T) * T(F64(prm.g))        # g * (0, 0, 6371009).normalized()
    dp_est = r0 - r1 + sb0[0:3] * Dt - half * g_W * Dt * Dt
    dv_est = sb0[0:3] - sb1[0:3] - g_W * Dt
    Dq = qmul(delta_q(-(rec["dalpha_db_g"] @ Delta_b[0:3]), T), rec["Delta_q"])
    q1i = qinv(q1)
    F0 = np.eye(15, dtype=T)
    F0[0:3, 0:3] = C_S0_W
    F0[0:3, 3:6] = C_S0_W @ cross_mx(dp_est, T)
    F0[0:3, 6:9] = C_S0_W * Dt
    F0[0:3, 9:12] = rec["dp_db_g"]
    F0[0:3, 12:15] = -rec["C_doubleintegral"]
    F0[3:6, 3:6] = (plus_mat(qmul(Dq, q1i), T) @ oplus_mat(q0, T))[0:3, 0:3]
    F0[3:6, 9:12] = (oplus_mat(qmul(q1i, q0), T) @ oplus_mat(Dq, T))[0:3, 0:3] @ (-rec["dalpha_db_g"])
    F0[6:9, 3:6] = C_S0_W @ cross_mx(dv_est, T)
    F0[6:9, 6:9] = C_S0_W
    F0[6:9, 9:12] = rec["dv_db_g"]
    F0[6:9, 12:15] = -rec["C_integral"]
    if mutate == "transposed_F_block":
        F0[0:3, 3:6] = F0[0:3, 3:6].T.copy()
    F1 = -np.eye(15, dtype=T)
    F1[0:3, 0:3] = -C_S0_W
    F1[3:6, 3:6] = -((plus_mat(Dq, T) @ oplus_mat(q0, T)) @ plus_mat(q1i, T))[0:3, 0:3]
    F1[6:9, 6:9] = -C_S0_W
    e = np.zeros(15, T)
    e[0:3] = C_S0_W @ dp_est + rec["acc_doubleintegral"] + F0[0:3, 9:15] @ Delta_b
    e[3:6] = T(2) * qmul(Dq, qmul(q1i, q0))[0:3]
    e[6:9] = C_S0_W @ dv_est + rec["acc_integral"] + F0[6:9, 9:15] @ Delta_b
    e[9:15] = sb0[3:9] - sb1[3:9]
    SI = rec["sqrt_info"]
    F = np.concatenate([F0, F1], axis=1)
    J = SI @ F
    r = SI @ e
    H, g = linearisation(J, r, T)
    if mutate == "wrong_permutation":
        p = np.arange(30)
        p[[14, 15]] = [15, 14]
        H, g = H[np.ix_(p, p)], g[p]
    out = dict(rec)
    out.update(redo_count=redo_count, F=F, e=e, J=J, r=r, H=H, g=g, cost=half * np.dot(r[::-1], r[::-1]))
    return out


def linearisation(J, r, T=np.longdouble):
    """H = J^T J and g = J^T r, summed over the residual rows from the last to the first"""
    J, r = np.asarray(J, T), np.asarray(r, T)
    H, g = np.zeros((J.shape[1],) * 2, T), np.zeros(J.shape[1], T)
    for k in range(J.shape[0] - 1, -1, -1):
        H = H + np.outer(J[k], J[k])
        g = g + J[k] * r[k]
    return H, g


def pack_lower(H):
    """[30][30] -> [465], index a (a + 1) / 2 + b, b <= a: the order of OKVIS_BA_ARR_IMU_LIN"""
    a, b = np.tril_indices(H.shape[0])
    return np.asarray(H)[a, b]
