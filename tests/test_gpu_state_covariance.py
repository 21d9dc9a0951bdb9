"""GPU: okvis_ba_state_covariance against the 60-digit referee (cases, selections and references: tests/cov_cases.py,
tests/cov_statement.py; what the inputs can tell apart: tests/test_state_covariance_host.py).

    e(X, X*) = max_ij |X_ij - X*_ij| / sqrt(X*_ii X*_jj)

The kernel alone is judged on its own tap: e(Sigma_dev, inv_mp(S0_tap)) <= 4 max(e_chol, e_lu, D 2^-52), e_chol / e_lu the two
fp64 host inversions of that same matrix.  The assembly is judged on the tap, end to end on the long double oracle's S0."""
import ctypes as C
import functools

import numpy as np
import pytest

from okvis_amd import _lib, solver
from okvis_amd import frontend as F
from okvis_amd.window import cov_marshal_batch

from . import cov_cases as cc
from . import cov_statement as cs

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -3, -5


@functools.lru_cache(maxsize=None)
def device(name, optimized):
    """every selection of a case on the device, one call each, at the uploaded state or after optimize(5):
    (window, {selection: result}, tap, Inverse of the tap over the case's columns)"""
    w = cc.window(name)
    b = solver.WindowBatch([w])
    if optimized:
        b.optimize(cc.OPT_ITERS)
    got = {sel: b.state_covariance(blocks, want_S0=True)[0] for sel, blocks in cc.selections(name).items()}
    b.close()
    taps = [g["S0"] for g in got.values()]
    assert all(t.tobytes() == taps[0].tobytes() for t in taps), "the tap does not depend on the selection"
    return w, got, taps[0], cc.Inverse(taps[0], cc.columns(name, w))


def kernel_bound(name, optimized):
    _, _, tap, inv = device(name, optimized)
    return cc.BOUND_FACTOR * max(inv.e_chol, inv.e_lu, tap.shape[0] * 2.0 ** -52)


# ---- 5. the kernel alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("optimized", [False, True], ids=["uploaded", "optimized"])
@pytest.mark.parametrize("name", cc.CASES)
def test_kernel_inverts_its_tap(name, optimized):
    w, got, tap, inv = device(name, optimized)
    D = cc.DIM[name]
    assert tap.shape == (D, D) and np.array_equal(tap, tap.T), "the tap is bitwise symmetric"
    bound = kernel_bound(name, optimized)
    for sel, blocks in cc.selections(name).items():
        g, rows = got[sel], cs.rows_of(w, blocks)
        assert g["info"] == 0 and g["dim"] == rows.size and g["cov"].shape == (rows.size, rows.size)
        assert g["min_pivot"] > 0.0
        assert np.array_equal(g["cov"], g["cov"].T)
        err = cs.e(g["cov"], inv.block(rows))
        print(f"\ncov kernel {name} {'optimized' if optimized else 'uploaded'} {sel:>13}: device {err:.3e} host chol {inv.e_chol:.3e} "
              f"lu {inv.e_lu:.3e} bound {bound:.3e} min_pivot {g['min_pivot']:.3e}")
        assert err <= bound, (name, sel, err, bound)


@pytest.mark.parametrize("name", cc.CASES)
def test_list_order_is_a_permutation_of_the_same_bits(name):
    w, got, _, _ = device(name, False)
    a, b = got["first+newest"]["cov"], got["newest+first"]["cov"]
    p = np.r_[15:30, 0:15]
    assert a[np.ix_(p, p)].tobytes() == b.tobytes()
    # (and a sub-selection is the same rows of the same inverse, though not the same bits: another elimination order)
    assert cs.e(got["newest"]["cov"], a[15:, 15:]) <= 2 * kernel_bound(name, False)


# ---- 6. the assembly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASES)
def test_tap_is_the_statement(oracle, name):
    _, _, tap, _ = device(name, False)
    _, _, S0, _, _ = cc.reference(oracle, name, extended=True)
    S0 = np.asarray(S0, np.float64)
    d = np.abs(tap - S0).max() / np.abs(S0).max()
    print(f"\ncov assembly {name}: |tap - S0| / max |S0| = {d:.3e}")
    assert d <= 1e-12


# ---- 7. end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASES)
def test_end_to_end_against_the_long_double_oracle(oracle, name):
    w, got, _, _ = device(name, False)
    _, C_, _, ref, _ = cc.reference(oracle, name, extended=True)
    _, _, _, o64, _ = cc.reference(oracle, name)
    e_oracle = cs.e(o64.X, ref.X)
    bound = cc.BOUND_FACTOR * max(e_oracle, kernel_bound(name, False))
    for sel, blocks in cc.selections(name).items():
        err = cs.e(got[sel]["cov"], ref.block(cs.rows_of(w, blocks)))
        print(f"\ncov end to end {name} {sel:>13}: device {err:.3e} fp64 oracle {e_oracle:.3e} bound {bound:.3e}")
        assert err <= bound, (name, sel, err, bound)


# ---- 8. batch invariance -----------------------------------------------------------------------------
def test_a_mixed_range_has_the_bits_of_the_single_calls():
    names, sels = ("A", "C", "D"), ("newest", "first+newest", "sb")
    wins = [cc.window(n) for n in names]
    blocks = [cc.selections(n)[s] for n, s in zip(names, sels)]
    b = solver.WindowBatch(wins)
    got = b.state_covariance(blocks, want_S0=True)
    singles = [b.state_covariance(blocks[i], w0=i, n=1, want_S0=True)[0] for i in range(3)]
    sub = b.state_covariance([blocks[1], blocks[2]], w0=1, n=2)
    b.close()
    for n, g, one in zip(names, got, singles):
        assert g["cov"].tobytes() == one["cov"].tobytes() and g["S0"].tobytes() == one["S0"].tobytes(), n
        assert g["min_pivot"] == one["min_pivot"] and g["info"] == 0
    assert sub[0]["cov"].tobytes() == got[1]["cov"].tobytes() and sub[1]["cov"].tobytes() == got[2]["cov"].tobytes()
    # (a window's numbers against its own tap, also in this batch's layout)
    for n, s, g in list(zip(names, sels, got))[:2]:
        w, _, _, inv = device(n, False)
        assert cs.e(g["cov"], cc.Inverse(g["S0"], inv.cols, host=False).block(cs.rows_of(w, cc.selections(n)[s]))) <= kernel_bound(n, False)


def test_nine_copies_have_the_bits_of_one():
    """nine windows: above SOLVE_HELPED_MAX_WINDOWS = 8, the Schur partials are summed inside the solving workgroup"""
    b = solver.WindowBatch([cc.window("A") for _ in range(9)])
    got = b.state_covariance(want_S0=True)
    one = b.state_covariance(w0=4, n=1, want_S0=True)[0]       # (one window: with helper workgroups)
    b.close()
    for g in got:
        assert g["cov"].tobytes() == one["cov"].tobytes() and g["S0"].tobytes() == one["S0"].tobytes()


# ---- 9. the solver is untouched ----------------------------------------------------------------------
def _snapshot(b):
    out = []
    for w in range(len(b)):
        r = b.fetch_results(w)
        out.append([np.asarray(x).tobytes() for x in b.get_state(w)] + [r[k].tobytes() for k in sorted(r)] + [b.fetch_imu_caches(w).tobytes()])
    return out


@pytest.mark.parametrize("names", [("A", "B"), ("D",), ("E", "C", "A")])
def test_solver_is_left_as_it_was(names):
    def run(middle):
        b = solver.WindowBatch([cc.window(n) for n in names])
        s1 = b.optimize(3)
        before = _snapshot(b)
        if middle:
            b.state_covariance(want_S0=True)
        mid = _snapshot(b)
        s2 = b.optimize(3)
        end = _snapshot(b)
        b.close()
        return s1, before, mid, s2, end
    plain, called = run(False), run(True)
    assert called[1] == called[2], "fetch_results / fetch_imu_caches / get_state right behind the call"
    assert plain == called


def test_uploaded_state_is_left_as_it_was():
    """before the first optimisation the IMU terms have no preintegration yet: the call builds them and puts the empty records back"""
    def run(middle):
        b = solver.WindowBatch([cc.window("A"), cc.window("C")])
        if middle:
            b.state_covariance()
        first = _snapshot(b)
        s = b.optimize(4)
        end = _snapshot(b)
        b.close()
        return first, s, end
    assert run(False) == run(True)


# ---- 10. failure -------------------------------------------------------------------------------------
def test_a_singular_window_fails_alone():
    wins = [cc.window("A"), cc.singular_window(), cc.window("B")]
    blocks = [cc.selections("A")["newest"], [(cc.POSE, 3), (cc.SB, 3)], cc.selections("B")["newest"]]
    b = solver.WindowBatch(wins)
    with pytest.raises(_lib.BackendError) as err:
        b.state_covariance(blocks, want_S0=True)
    assert err.value.status == ERR_NUMERIC
    got = err.value.results
    assert [g["info"] for g in got] == [0, 1, 0]
    assert np.isnan(got[1]["cov"]).all() and got[1]["cov"].shape == (15, 15)
    Dp = 24
    assert np.all(got[1]["S0"][Dp:, :] == 0.0) and np.diag(got[1]["S0"]).min() == 0.0
    # the solver serves the next calls: the outer two alone
    for i in (0, 2):
        one = b.state_covariance(blocks[i], w0=i, n=1)[0]
        assert one["info"] == 0 and one["cov"].tobytes() == got[i]["cov"].tobytes() and one["min_pivot"] == got[i]["min_pivot"]
    b.close()


# ---- 11. arguments and state -------------------------------------------------------------------------
def _raw(b, sels, w0=0, n=None, capacity=None, null_cov=False):
    """the C entry itself on prepared structures: (status, results, outs) — every cov array starts as a pattern"""
    specs, results, outs, keep = cov_marshal_batch(sels, [0] * len(sels), False)
    for i, o in enumerate(outs):
        o["cov"][:] = -7.0
        results[i].dim, results[i].info, results[i].min_pivot = -7, -7, -7.0
        if capacity is not None:
            results[i].capacity = capacity
        if null_cov:
            results[i].cov = None
    st = b._L.okvis_ba_state_covariance(b._h, w0, len(sels) if n is None else n, specs, results)
    del keep
    return st, results, outs


def _untouched(results, outs):
    return all(np.all(o["cov"] == -7.0) for o in outs) and all(results[i].dim == -7 and results[i].info == -7 and results[i].min_pivot == -7.0
                                                                for i in range(len(outs)))


def test_arguments_and_state():
    wA, wF = cc.window("A"), cc.window("F")
    b = solver.WindowBatch([wA, wF])
    good = [cc.selections("A")["newest"], cc.selections("F")["newest"]]
    ref = b.state_covariance(good)

    def right_numbers():
        now = b.state_covariance(good)
        assert all(x["cov"].tobytes() == y["cov"].tobytes() for x, y in zip(now, ref))

    P, S = cc.POSE, cc.SB
    bad = {
        "n_blocks < 1": [[], good[1]],
        "unknown type": [[(2, 0)], good[1]],
        "pose index out of range": [[(P, len(wA.pose))], good[1]],
        "negative index": [[(S, -1)], good[1]],
        "sb index out of range": [good[0], [(S, 12)]],
        "a fixed block (extrinsics)": [[(P, 4)], good[1]],
        "a fixed block (pose 0 of F)": [good[0], [(P, 0)]],
        "a block named twice": [[(P, 1), (S, 1), (P, 1)], good[1]],
        "more than 30 rows": [[(P, 0), (P, 1), (P, 2), (P, 3), (S, 0)], good[1]],
    }
    for what, sels in bad.items():
        st, results, outs = _raw(b, sels)
        assert st == ERR_ARG, what
        assert _untouched(results, outs), what
        right_numbers()
    for what, kw in {"capacity below dim^2": dict(capacity=224), "NULL cov": dict(null_cov=True)}.items():
        st, results, outs = _raw(b, good, **kw)
        assert st == ERR_ARG and _untouched(results, outs), what
    for w0, n in ((-1, 2), (1, 2), (0, 0), (2, 1)):
        st, results, outs = _raw(b, good, w0=w0, n=n)
        assert st == ERR_ARG and _untouched(results, outs), (w0, n)
    L = b._L
    specs, results, _, keep = cov_marshal_batch(good, [0, 0], False)
    assert L.okvis_ba_state_covariance(None, 0, 2, specs, results) == ERR_ARG
    assert L.okvis_ba_state_covariance(b._h, 0, 2, None, results) == ERR_ARG
    assert L.okvis_ba_state_covariance(b._h, 0, 2, specs, None) == ERR_ARG
    right_numbers()
    # between okvis_ba_begin and okvis_ba_finish
    b.begin()
    st, results, outs = _raw(b, good)
    assert st == ERR_STATE and _untouched(results, outs)
    b.iterate(1)
    assert _raw(b, good)[0] == ERR_STATE
    b.finish()
    assert _raw(b, good)[0] == 0
    # while a marginalisation is pending
    jobs = [([1, 0, 0, 0, 0, 0], [1, 0, 0, 0], None)]
    b.marginalize_batch_begin(0, jobs)
    st, results, outs = _raw(b, good)
    assert st == ERR_STATE and _untouched(results, outs)
    b.marginalize_batch_end()
    assert _raw(b, good)[0] == 0
    b.close()
    # before upload
    h = C.c_void_p()
    _lib.check(L.okvis_ba_create(C.byref(h), 0))
    assert L.okvis_ba_state_covariance(h, 0, 1, specs, results) == ERR_STATE
    L.okvis_ba_destroy(h)
    del keep


def test_one_block_over_is_unsupported():
    wG, wA = cc.window("G"), cc.window("A")
    b = solver.WindowBatch([wA, wG])
    sels = [cc.selections("A")["newest"], cc.selections("G")["newest"]]
    st, results, outs = _raw(b, sels)
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    st, results, outs = _raw(b, sels[1:], w0=1)
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    one = b.state_covariance(sels[0], w0=0, n=1)[0]      # the window next to it is served
    b.close()
    assert one["info"] == 0 and np.all(np.isfinite(one["cov"])) and np.all(np.diag(one["cov"]) > 0)


# ---- 12. Python --------------------------------------------------------------------------------------
def test_default_selection_is_the_newest_state():
    wins = [cc.window("A"), cc.window("D")]
    b = solver.WindowBatch(wins)
    assert b.newest_state_blocks(0) == [(cc.POSE, 3), (cc.SB, 3)] and b.newest_state_blocks(1) == [(cc.POSE, 9), (cc.SB, 9)]
    a = b.state_covariance()
    e = b.state_covariance([cc.selections("A")["newest"], cc.selections("D")["newest"]])
    b.close()
    assert all(x["cov"].tobytes() == y["cov"].tobytes() and x["dim"] == 15 for x, y in zip(a, e))
    b = solver.WindowBatch([cc.singular_window()])
    with pytest.raises(ValueError):
        b.state_covariance()
    b.close()


def test_propagated_covariance_of_one_job():
    """state covariance of the first state -> okvis_fe_imu_propagate along the first IMU term -> covariance of the propagated state"""
    w = cc.window("A")
    P0 = device("A", True)[1]["first+newest"]["cov"][:15, :15]
    f = 0
    bgn, cnt = int(w.imu_s_begin[f]), int(w.imu_s_count[f])
    fe = F.Frontend()
    job = dict(s_begin=0, s_count=cnt, e_begin=0, e_count=1, t_start=int(w.imu_t0[f]), T_WS=w.pose[0], sb=w.sb[0], flags=F.IMU_COV | F.IMU_JAC)
    _, _, count, cov, jac = fe.imu_propagate([w.imu_params], w.imu_s_t[bgn:bgn + cnt], w.imu_s_gyr[bgn:bgn + cnt], w.imu_s_acc[bgn:bgn + cnt],
                                             [job], [int(w.imu_t1[f])])
    fe.close()
    assert count[0] > 0
    P = F.propagated_covariance(P0, jac[0], cov[0])
    assert np.array_equal(P, jac[0] @ P0 @ jac[0].T + cov[0])
    assert np.abs(P - P.T).max() <= 1e-12 * np.abs(P).max()
    lam = np.linalg.eigvalsh((P + P.T) / 2)
    assert lam.min() > 0.0
    # the propagation adds uncertainty to what the start state brings along
    assert np.all(np.diag(P)[:3] > np.diag(cov[0])[:3])
