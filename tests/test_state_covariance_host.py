"""okvis_ba_state_covariance, the part that needs no device: the statement and its inputs (tests/cov_statement.py,
tests/cov_cases.py), the coordinate convention of the propagation Jacobian, the symbol and its argument check."""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib, synthetic
from okvis_amd.window import CovResultC, CovSpecC

from . import cov_cases as cc
from . import cov_statement as cs


# ---- 1. the statement and its inputs ---------------------------------------------------------------
@pytest.mark.parametrize("optimized", [False, True], ids=["uploaded", "optimized"])
@pytest.mark.parametrize("name", cc.CASES)
def test_inputs_are_invertible_in_fp64(oracle, name, optimized):
    """S0 of the fp64 oracle's arrays, inverted by scipy Cholesky and by numpy LU, against the 60-digit inverse: a condition on
    the inputs, e_ref <= 1e-4, so that no bound of the GPU tests ever exceeds 4e-4."""
    w, C_, S0, inv, _ = cc.reference(oracle, name, optimized=optimized)
    assert S0.shape == (cc.DIM[name], cc.DIM[name]) and w.reduced_dim() == cc.DIM[name]
    assert np.array_equal(S0, S0.T)
    print(f"\ncov inputs {name} {'optimized' if optimized else 'uploaded'}: D {S0.shape[0]} |C| {C_.size} "
          f"e_chol {inv.e_chol:.3e} e_lu {inv.e_lu:.3e}")
    assert inv.e_ref <= cc.E_REF_MAX


def test_prior_enters_case_E(oracle):
    """E is A plus a marginalisation prior over pose 0, speed/bias 0, pose 1: HPP changes on rows 0-11 and 24-32 and nowhere else"""
    _, _, _, _, linE = cc.reference(oracle, "E")
    _, _, _, _, linA = cc.reference(oracle, "A")
    d = np.abs(np.asarray(linE["HPP"]) - np.asarray(linA["HPP"])).reshape(60, 60)
    rows = np.flatnonzero(d.max(axis=1) > 0)
    assert np.array_equal(rows, np.r_[0:12, 24:33])


def test_case_G_is_one_block_over():
    assert cc.window("G").reduced_dim() == 180 and cc.window("F").reduced_dim() == 174


# ---- 2. mutations of the statement must be seen ------------------------------------------------------
def _moved(oracle, name, S_wrong):
    _, C_, _, inv, _ = cc.reference(oracle, name)
    return cs.e(cs.inverse_block_mp(S_wrong, C_), inv.X), inv.e_ref


def test_mutation_dropped_prior(oracle):
    w, _, _, _, _ = cc.reference(oracle, "E")
    w2 = cc.no_prior(w)
    moved, e_ref = _moved(oracle, "E", cs.S0_of(w2, cs.linearized(oracle, w2)))
    print(f"\ncov mutation dropped prior (E): moved {moved:.3e} e_ref {e_ref:.3e}")
    assert moved > cc.MUTATION_MARGIN * e_ref


@pytest.mark.parametrize("name", ["A", "C"])
def test_mutation_damping(oracle, name):
    w, _, _, _, lin = cc.reference(oracle, name)
    moved, e_ref = _moved(oracle, name, cs.S0_of(w, lin, lam=1e-8))
    print(f"\ncov mutation damping 1e-8 ({name}): moved {moved:.3e} e_ref {e_ref:.3e}")
    assert moved > cc.MUTATION_MARGIN * e_ref


@pytest.mark.parametrize("name", ["A", "C"])
def test_mutation_pseudo_inverse(oracle, name):
    w, _, _, _, lin = cc.reference(oracle, name)
    moved, e_ref = _moved(oracle, name, cs.S0_of(w, lin, vinv_of=lambda l, V: cs.pinv_rank2(V) if l == 0 else None))
    print(f"\ncov mutation pinv of a rank-2 V ({name}): moved {moved:.3e} e_ref {e_ref:.3e}")
    assert moved > cc.MUTATION_MARGIN * e_ref


# ---- 3. the coordinate convention --------------------------------------------------------------------
def _right_oplus(pose, d):
    """r += dr, q = q (x) dq(alpha): the perturbation applied on the right (a wrong candidate)"""
    out = np.array(pose, np.float64)
    out[:3] += d[:3]
    out[3:] = synthetic.qmul(pose[3:], synthetic.delta_q(np.asarray(d[3:], np.float64)))
    out[3:] /= np.linalg.norm(out[3:])
    return out


def test_propagation_jacobian_is_in_the_solver_tangent_space(oracle):
    """Central differences of ImuError::propagation through the solver's own plus / minus of a pose (orc_pose_plus,
    orc_pose_minus(x, xp) = xp (-) x) against the Jacobian it returns: the 15-vector (r, alpha, v, b_g, b_a) is the tangent space of
    (pose, speed/bias).  No tolerance is fixed: the right convention has to beat each wrong candidate by 1000 x in the r, alpha and
    v row blocks.  (A candidate that leaves a row block mathematically untouched — swapping the arguments of the pose difference
    does not reach the v rows — must reproduce the right convention's figure there instead.)"""
    w = synthetic.small_window(seed=1)
    f = 0
    b, c = int(w.imu_s_begin[f]), int(w.imu_s_count[f])
    t, gyr, acc = w.imu_s_t[b:b + c], w.imu_s_gyr[b:b + c], w.imu_s_acc[b:b + c]
    t0, t1 = int(w.imu_t0[f]), int(w.imu_t1[f])
    pose0, sb0 = np.asarray(w.pose[w.imu_pose0[f]], np.float64), np.asarray(w.sb[w.imu_sb0[f]], np.float64)
    T1, s1, _, jac, steps = oracle.imu_propagation(t, gyr, acc, w.imu_params, pose0, sb0, t0, t1, want_jac=True)
    assert steps == 101
    h = 1e-6

    def fd(plus, minus, alpha_sign):
        J = np.zeros((15, 15))
        for k in range(15):
            out = []
            for sgn in (1.0, -1.0):
                d = np.zeros(15)
                d[k] = sgn * h
                dp = d[:6].copy()
                dp[3:] *= alpha_sign
                Ta, sa, _, _, _ = oracle.imu_propagation(t, gyr, acc, w.imu_params, plus(pose0, dp), sb0 + d[6:], t0, t1)
                dm = minus(T1, Ta)
                dm[3:] *= alpha_sign
                out.append(np.concatenate([dm, sa - s1]))
            J[:, k] = (out[0] - out[1]) / (2 * h)
        return J

    right_minus = lambda x, xp: oracle.pose_minus(x, xp).copy()          # noqa: E731  xp (-) x
    candidates = {
        "right": fd(oracle.pose_plus, right_minus, 1.0),
        "alpha negated": fd(oracle.pose_plus, right_minus, -1.0),
        "minus swapped": fd(oracle.pose_plus, lambda x, xp: oracle.pose_minus(xp, x).copy(), 1.0),
        "alpha on the right": fd(_right_oplus, right_minus, 1.0),
    }
    blocks = {"r": slice(0, 3), "alpha": slice(3, 6), "v": slice(6, 9), "b_g": slice(9, 12), "b_a": slice(12, 15)}
    err = {n: {bn: float(np.abs(J[bs] - jac[bs]).max()) for bn, bs in blocks.items()} for n, J in candidates.items()}
    for n in candidates:
        print(f"\ncov convention {n:>18}: " + "  ".join(f"{bn} {err[n][bn]:.3e}" for bn in blocks))
    assert err["right"]["b_g"] == 0.0 and err["right"]["b_a"] == 0.0
    untouched = {("minus swapped", "v")}
    for n in candidates:
        if n == "right":
            continue
        for bn in ("r", "alpha", "v"):
            if (n, bn) in untouched:
                assert err[n][bn] == err["right"][bn]
            else:
                assert err[n][bn] >= 1000.0 * err["right"][bn], (n, bn, err[n][bn], err["right"][bn])


# ---- 4. symbols and arguments ------------------------------------------------------------------------
def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert "okvis_ba_state_covariance" in _lib.SYMBOLS
    assert L.okvis_ba_state_covariance.argtypes is not None and len(L.okvis_ba_state_covariance.argtypes) == 5
    assert L.okvis_ba_abi_version() == 7
    spec, res = CovSpecC(), CovResultC()
    assert L.okvis_ba_state_covariance(None, 0, 1, C.byref(spec), C.byref(res)) == -1     # OKVIS_BA_ERR_ARG
    assert C.sizeof(CovSpecC) == 24 and C.sizeof(CovResultC) == 40


def test_propagated_covariance_is_the_sandwich():
    from okvis_amd.frontend import propagated_covariance
    rng = np.random.default_rng(5)
    A = rng.standard_normal((15, 15))
    P0, J, Q = A @ A.T, rng.standard_normal((15, 15)), np.eye(15) * 0.5
    assert np.array_equal(propagated_covariance(P0, J, Q), J @ P0 @ J.T + Q)
    with pytest.raises(ValueError):
        propagated_covariance(P0[:6, :6], J, Q)
