"""okvis_ba_landmark_covariance, the part that needs no device: the statement and its inputs (tests/lmcov_statement.py,
tests/lmcov_cases.py), the symbols and their argument checks, the camera-frame helper."""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib
from okvis_amd.window import LmcovResultC, LmcovSpecC

from . import cov_cases as cc
from . import cov_statement as cs
from . import lmcov_cases as lc
from . import lmcov_statement as ls


# ---- 1. the statement and its inputs ---------------------------------------------------------------
@pytest.mark.parametrize("name", lc.CASES)
def test_inputs_can_be_evaluated_in_fp64(oracle, name):
    """Sigma_l of the fp64 oracle's arrays by numpy (P by scipy Cholesky and by numpy LU) against the 60-digit statement: a
    condition on the inputs, e_ref <= 1e-4 for every landmark, so that no bound of the GPU tests ever exceeds 4e-4."""
    ref = lc.reference(oracle, name)
    assert ref.S0.shape == (lc.DIM[name], lc.DIM[name]) and ref.Dp == lc.POSE_DIM[name]
    n_pairs = np.array([t[0].size // 6 for t in ref.terms])
    tr = [np.trace(X) / np.trace(ls.sigma_np(t, None, "only")) for t, X in zip(ref.terms, ref.X) if t[0].size]
    print(f"\nlmcov inputs {name}: D {ref.S0.shape[0]} Dp {ref.Dp} landmarks {len(ref.terms)} pairs per landmark {n_pairs.min()}..{n_pairs.max()} "
          f"worst e_ref {ref.e_ref.max():.3e}  tr Sigma / tr V^-1 {min(tr):.3f}..{max(tr):.3f}")
    assert np.all(ref.e_ref <= cc.E_REF_MAX)
    assert np.array_equal(ref.X[ref.observed], np.swapaxes(ref.X[ref.observed], 1, 2))
    if name == "H":
        assert n_pairs.min() == 12 and n_pairs.max() == 12, "every landmark of H touches 72 rows: more than a wave has lanes"
    if name == "U":
        assert not ref.observed[lc.NO_PAIRS] and ref.observed.sum() == ref.observed.size - 1
        assert np.isnan(ref.X[lc.NO_PAIRS]).all()
    else:
        assert ref.observed.all()


# ---- 2. mutations of the statement must be seen ------------------------------------------------------
def _mutants(ref):
    """name -> X [n_lm, 3, 3] of a wrong definition.  Evaluated in fp64 from the 60-digit P (or an fp64 inverse of a wrong
    matrix): their own rounding is of the order of e_ref, five orders below the moves asserted."""
    w, lin, Dp = ref.w, ref.lin, ref.Dp
    S0 = np.asarray(ref.S0, np.float64)
    damped = np.asarray(cs.S0_of(w, lin, lam=1e-8), np.float64)
    return {
        "V^-1 alone": ls.sigma_all(ref.terms, None, "np", vinv="only"),
        "inverse of the pose block": ls.sigma_all(ref.terms, np.linalg.inv(S0[:Dp, :Dp]), "np"),
        "S0 damped by 1e-8 diag": ls.sigma_all(ref.terms, np.linalg.inv(damped)[:Dp, :Dp], "np"),
        "first pair dropped": ls.sigma_all(ls.landmark_terms(w, lin["LM_V"], lin["PAIR_W"], lin["pairs"], drop_first=True), ref.inv.X, "np"),
        "W read as 3 x 6": ls.sigma_all(ls.landmark_terms(w, lin["LM_V"], lin["PAIR_W"], lin["pairs"], w_3x6=True), ref.inv.X, "np"),
    }


@pytest.mark.parametrize("name", lc.CASES)
def test_mutations_move_every_landmark(oracle, name):
    ref = lc.reference(oracle, name)
    obs = ref.observed
    for what, X in _mutants(ref).items():
        moved = ls.e(X[obs], ref.X[obs])
        ratio = moved / ref.e_ref[obs]
        print(f"\nlmcov mutation {name} {what:>27}: smallest move {moved.min():.3e}  smallest move / e_ref {ratio.min():.3e}")
        assert np.all(moved > cc.MUTATION_MARGIN * ref.e_ref[obs]), (name, what)


# ---- 3. symbols and arguments ------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert "okvis_ba_landmark_covariance" in _lib.SYMBOLS and "okvis_ba_last_landmark_covariance_ms" in _lib.SYMBOLS
    assert L.okvis_ba_landmark_covariance.argtypes is not None and len(L.okvis_ba_landmark_covariance.argtypes) == 5
    assert len(L.okvis_ba_last_landmark_covariance_ms.argtypes) == 4
    assert L.okvis_ba_abi_version() == 7
    assert C.sizeof(LmcovSpecC) == 16 and C.sizeof(LmcovResultC) == 72


def test_null_arguments_return_before_any_device_is_touched():
    L = _lib.lib()
    spec, res = LmcovSpecC(), LmcovResultC()
    assert L.okvis_ba_landmark_covariance(None, 0, 1, C.byref(spec), C.byref(res)) == -1     # OKVIS_BA_ERR_ARG
    f = C.c_float()
    assert L.okvis_ba_last_landmark_covariance_ms(None, C.byref(f), C.byref(f), C.byref(f)) == -1
    assert res.n == 0 and res.info == 0 and res.min_pivot == 0.0


def test_marshalling():
    from okvis_amd.window import lmcov_marshal_batch
    specs, results, outs, keep = lmcov_marshal_batch([None, [7, 3, 3, 0], []], [40, 60, 10], [(60, 24, 40, 100), (72, 36, 60, 300), (60, 24, 10, 0)])
    assert not specs[0].lm_idx and results[0].capacity == 40 and outs[0]["cov"].shape == (40, 9)
    assert [specs[1].lm_idx[i] for i in range(4)] == [7, 3, 3, 0] and specs[1].n_lm == 4 and results[1].capacity == 4
    assert specs[2].n_lm == 0 and bool(specs[2].lm_idx) and results[2].capacity == 0
    assert outs[1]["Spp"].shape == (36, 36) and outs[1]["W"].shape == (300, 18) and outs[0]["V"].shape == (40, 6)
    assert all(bool(getattr(results[i], k)) for i in range(3) for k in ("cov", "flags", "S0", "Spp", "V", "W"))
    del keep


# ---- 4. Python ---------------------------------------------------------------------------------------
def test_landmark_covariance_in_camera():
    from okvis_amd.frontend import landmark_covariance_in_camera
    rng = np.random.default_rng(11)
    A = rng.standard_normal((5, 3, 3))
    Sigma = A @ np.swapaxes(A, 1, 2)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Q, rng.standard_normal(3)
    got = landmark_covariance_in_camera(Sigma, T)
    assert got.shape == (5, 3, 3)
    for l in range(5):
        assert np.array_equal(got[l], Q @ Sigma[l] @ Q.T)
    assert np.array_equal(landmark_covariance_in_camera(Sigma[0], Q), Q @ Sigma[0] @ Q.T)
    assert np.allclose(np.linalg.eigvalsh(got[2]), np.linalg.eigvalsh(Sigma[2]), rtol=1e-12)     # a rotation keeps the spectrum
    with pytest.raises(ValueError):
        landmark_covariance_in_camera(Sigma[:, :2, :2], T)
