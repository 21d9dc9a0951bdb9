"""okvis_ba_predicted_measurement, the part that needs no device: the statement and its inputs (tests/predcov_statement.py,
tests/predcov_cases.py) on the oracle's arrays, the definition against the dense full normal matrix and against wrong
definitions, the Jacobians against central differences, the symbols.

What test_wrong_definitions_are_seen shows (fp64 oracle's arrays, uploaded state; median over the queries of each case of
tr U_wrong / tr U): the marginal-only covariance J_l Sigma_l J_l^T is 2.2 (F) to 13.7 (C) times too large, up to 240 times on single
queries; the marginals without the cross term 3.8 (F) to 26.5 (C) times; G with the wrong sign 6.6 (F) to 51.9 (C) times.  The
correlation between a landmark and the camera that sees it cancels most of what the world-frame marginals hold.  In fp64 the block
form is 1.0 to 2.0 times (median) as far from the 60-digit value as form A on these windows."""
import ctypes as C
import functools

import numpy as np
import pytest

from okvis_amd import _lib, synthetic

from . import cov_cases as cc
from . import cov_statement as cs
from . import lmcov_cases as lc
from . import predcov_cases as pc
from . import predcov_statement as ps

EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def host(oracle, name):
    """one case on the fp64 oracle's arrays at the uploaded state: (window, queries, tags, lmcov reference, uv, jac, projects,
    U* by form A at 60 digits)"""
    w, Q, tags = pc.queries(name)
    ref = lc.reference(oracle, name)
    uv, jac, projects = ps.jacobians_all(oracle.lib(), w, Q)
    return w, Q, tags, ref, uv, jac, projects, ps.u_all(w, ref.terms, Q, jac, ref.inv.X, form="A")


# ---- 1. the two forms of the statement ---------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CASES)
def test_the_two_forms_agree_at_60_digits(oracle, name):
    w, Q, tags, ref, uv, jac, projects, UA = host(oracle, name)
    UB = ps.u_all(w, ref.terms, Q, jac, ref.inv.X, form="block")
    flags = pc.expected_flags(w, ref.terms, Q, projects)
    rows = np.array([ps.n_rows(w, ref.terms[int(q[0])], q) for q in Q])
    good = flags == 0
    print(f"\npredcov inputs {name}: queries {len(Q)} ({', '.join(f'{t} {int((tags == t).sum())}' for t in dict.fromkeys(tags))})  |R| {rows[good].min()}..{rows[good].max()}  "
          f"flagged {int((~good).sum())}")
    assert good.sum() >= len(Q) - 4 and np.all(np.isnan(UA[~good])) and np.all(np.isfinite(UA[good]))
    # both forms are rounded from 60 digits: they agree to the last bit or the one before it
    assert np.all(ps.e(UB[good], UA[good]) <= 2 * EPS)
    assert np.linalg.eigvalsh(UA[good]).min() > 0.0
    # the lists hold what tests/predcov_cases.py says
    assert set(tags) >= {"newest", "observed", "behind", "repeats"} and (name in ("D", "H") or "unseen" in tags)
    assert flags[tags == "behind"].tolist() == [2] and np.isnan(uv[tags == "behind"]).all()
    if name == "H":
        assert rows[good].max() == 72, "more rows than a wave has lanes"
    if name == "U":
        assert flags[lc.NO_PAIRS] == 1 and np.isfinite(uv[lc.NO_PAIRS]).all()
    if name == "F":
        fx = tags == "fixed"
        assert fx.sum() == 2 and all(ps.rows_x_of(w, q)[0].size == 0 for q in Q[fx]), "a fixed pose seen through fixed extrinsics"
    if name in ("C", "H"):
        assert "crossed" in tags


@pytest.mark.parametrize("name", pc.CASES)
def test_inputs_can_be_evaluated_in_fp64(oracle, name):
    """a condition on the inputs: both float64 evaluations stay below E_REF_MAX, so no bound of the GPU tests exceeds 4e-4"""
    w, Q, tags, ref, uv, jac, projects, UA = host(oracle, name)
    eA = ps.e(ps.u_all(w, ref.terms, Q, jac, ref.inv.X, "np", form="A"), UA)
    eB = ps.e(ps.u_all(w, ref.terms, Q, jac, ref.inv.X, "np", form="block"), UA)
    print(f"\npredcov fp64 {name}: form A worst {eA.max():.3e}  block form worst {eB.max():.3e}  median block / A {np.median(eB[eA > 0] / eA[eA > 0]):.1f}")
    assert max(eA.max(), eB.max()) <= cc.E_REF_MAX


# ---- 2. the definition: J H^-1 J^T of the dense full normal matrix -----------------------------------
def test_statement_is_the_block_of_the_full_inverse(oracle):
    """case A, D + 3 n_lm = 180: the columns of H^-1 the chosen queries touch, at 60 digits and rounded to double (a relative 2^-53
    on every entry of Sigma, hence at most 2^-53 |J| |Sigma| |J|^T on U, entry by entry: the bound, doubled for the rounding of
    the statement itself)"""
    w, Q, tags, ref, uv, jac, projects, UA = host(oracle, "A")
    H = ps.full_normal_matrix(w, ref.lin)
    assert np.array_equal(H, H.T) and H.shape == (180, 180)
    pick = [0, 7, int(np.flatnonzero(tags == "observed")[1]), int(np.flatnonzero(tags == "unseen")[0])]
    cols = [ps.full_jacobian(w, ref.lin["D"], Q[k], jac[k]) for k in pick]
    need = np.unique(np.concatenate([c for c, _ in cols]))
    Sigma = cs.inverse_block_mp(H, need)
    for k, (c, J) in zip(pick, cols):
        at = np.searchsorted(need, c)
        S = Sigma[np.ix_(at, at)]
        U = J @ S @ J.T
        slack = 2 * 2.0 ** -53 * (np.abs(J) @ np.abs(S) @ np.abs(J).T) + 4 * EPS * np.abs(UA[k])
        print(f"\npredcov full inverse query {Q[k].tolist()}: |U - U*| / slack {(np.abs(U - UA[k]) / slack).max():.3f}  cancellation {slack.max() / np.abs(UA[k]).max() / EPS:.0f} eps")
        assert np.all(np.abs(U - UA[k]) <= slack), (k, U, UA[k])


# ---- 3. the Jacobians are those of the projection in the solver's tangent coordinates ----------------
@pytest.mark.parametrize("name", ["B", "C"])
def test_jacobians_match_central_differences(oracle, name):
    w, Q, tags, ref, uv, jac, projects, UA = host(oracle, name)
    L = oracle.lib()
    pose0, lm0 = np.asarray(w.pose, np.float64).reshape(-1, 7), np.asarray(w.lm, np.float64).reshape(-1, 4)
    h = 1e-6
    worst = 0.0
    for k in (0, 1, int(np.flatnonzero(tags == "observed")[0]), int(np.flatnonzero(tags == "unseen")[0])):
        q = Q[k]
        num = np.zeros((2, 15))
        for c in range(15):
            side = []
            for s in (+1.0, -1.0):
                pose, lm = pose0.copy(), lm0.copy()
                if c < 3:
                    lm[q[0], c] += s * h
                else:
                    d = np.zeros(6)
                    d[(c - 3) % 6] = s * h
                    b = q[1] if c < 9 else q[2]
                    pose[b] = synthetic.pose_oplus(pose0[b], d)
                side.append(ps.jacobians(L, w, q, pose, lm)[0])
            num[:, c] = (side[0] - side[1]) / (2 * h)
        Jl, Jp, Je = ps.split(jac[k])
        ana = np.concatenate([Jl, Jp, Je], axis=1)
        # central differences: h^2 / 6 x the third derivative (below 1e-8 |J| for points metres away) plus the rounding of uv,
        # a few 2^-52 x 1e3 pixels / h = 1e-6
        tol = 1e-8 * np.abs(ana).max() + 1e-6
        worst = max(worst, np.abs(num - ana).max() / tol)
        assert np.all(np.abs(num - ana) <= tol), (k, np.abs(num - ana).max(), tol)
    print(f"\npredcov central differences {name}: worst |numeric - analytic| / tolerance {worst:.3f}")


# ---- 4. wrong definitions must be seen ---------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CASES)
def test_wrong_definitions_are_seen(oracle, name):
    """dropping the cross term, the marginal Sigma_l alone and G with the wrong sign each move U by far more than any bound the GPU
    tests can reach (BOUND_FACTOR x E_REF_MAX = 4e-4) on most queries: on every query that has rows_x."""
    w, Q, tags, ref, uv, jac, projects, UA = host(oracle, name)
    has_x = np.array([ps.rows_x_of(w, q)[0].size > 0 for q in Q]) & np.isfinite(UA[:, 0, 0])
    assert has_x.sum() >= 0.9 * len(Q)
    for what in ("no cross", "marginal", "G sign"):
        X = ps.u_all(w, ref.terms, Q, jac, ref.inv.X, "np", mutate=what)
        moved = ps.e(X[has_x], UA[has_x])
        tr = np.trace(X[has_x], axis1=1, axis2=2) / np.trace(UA[has_x], axis1=1, axis2=2)
        print(f"\npredcov wrong definition {name} {what:>9}: smallest move {moved.min():.3e}  median {np.median(moved):.3e}  "
              f"tr U_wrong / tr U  min {tr.min():.2f} median {np.median(tr):.2f} max {tr.max():.1f}")
        assert np.mean(moved > cc.MUTATION_MARGIN * cc.BOUND_FACTOR * cc.E_REF_MAX) > 0.5, (name, what)
        if what == "marginal":
            assert np.median(tr) > 1.0, "the marginal alone overstates the pixel's uncertainty"


# ---- 5. symbols --------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    from okvis_amd.window import PredResultC, PredSpecC
    L = _lib.lib()
    assert "okvis_ba_predicted_measurement" in _lib.SYMBOLS and "okvis_ba_last_predicted_measurement_ms" in _lib.SYMBOLS
    assert len(L.okvis_ba_predicted_measurement.argtypes) == 5 and len(L.okvis_ba_last_predicted_measurement_ms.argtypes) == 4
    assert L.okvis_ba_abi_version() == 7
    assert C.sizeof(PredSpecC) == 40 and C.sizeof(PredResultC) == 88


def test_null_arguments_return_before_any_device_is_touched():
    from okvis_amd.window import PredResultC, PredSpecC
    L = _lib.lib()
    spec, res = PredSpecC(), PredResultC()
    assert L.okvis_ba_predicted_measurement(None, 0, 1, C.byref(spec), C.byref(res)) == -1     # OKVIS_BA_ERR_ARG
    f = C.c_float()
    assert L.okvis_ba_last_predicted_measurement_ms(None, C.byref(f), C.byref(f), C.byref(f)) == -1
    assert res.n == 0 and res.info == 0 and res.min_pivot == 0.0


def test_marshalling():
    from okvis_amd.window import predcov_marshal_batch
    q = np.array([[7, 3, 4, 0], [7, 3, 4, 0], [1, 2, 5, 1]])
    specs, results, outs, keep = predcov_marshal_batch([q, np.zeros((0, 4), np.int32)], [(60, 24, 40, 100), (72, 36, 60, 0)])
    assert specs[0].n_q == 3 and [specs[0].q_lm[i] for i in range(3)] == [7, 7, 1] and [specs[0].q_cam[i] for i in range(3)] == [0, 0, 1]
    assert [specs[0].q_pose[i] for i in range(3)] == [3, 3, 2] and [specs[0].q_ext[i] for i in range(3)] == [4, 4, 5]
    assert specs[1].n_q == 0 and bool(specs[1].q_lm) and results[1].capacity == 0 and results[0].capacity == 3
    assert outs[0]["uv"].shape == (3, 2) and outs[0]["cov"].shape == (3, 4) and outs[0]["jac"].shape == (3, 30) and outs[1]["Spp"].shape == (36, 36)
    assert all(bool(getattr(results[i], k)) for i in range(2) for k in ("uv", "cov", "flags", "S0", "Spp", "V", "W", "jac"))
    del keep
