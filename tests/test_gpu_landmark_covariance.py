"""GPU: okvis_ba_landmark_covariance against the 60-digit referee (cases and references: tests/lmcov_cases.py,
tests/lmcov_statement.py; what the inputs can tell apart: tests/test_landmark_covariance_host.py).  Per landmark

    e(X, X*) = max_ij |X_ij - X*_ij| / sqrt(X*_ii X*_jj)

Stage two (lmcov_kernel) is judged on its own taps V, W, Spp taken as exact doubles; stage one (cov_pose_kernel) on the S0 tap, as
cov_kernel is in tests/test_gpu_state_covariance.py, and bit for bit against okvis_ba_state_covariance; the whole against the long
double oracle's arrays.  Worst figures measured on an MI355X (stage two, device / bound): profiles/lmcov_notes.md."""
import ctypes as C
import functools

import numpy as np
import pytest

from okvis_amd import _lib, solver
from okvis_amd.frontend import landmark_covariance_in_camera
from okvis_amd.window import lmcov_marshal_batch

from . import cov_cases as cc
from . import cov_statement as cs
from . import lmcov_cases as lc
from . import lmcov_statement as ls

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -3, -5
EPS = 2.0 ** -52
STATES = pytest.mark.parametrize("optimized", [False, True], ids=["uploaded", "optimized"])


def selections(name):
    """cov_cases.selections for the two windows it does not know: U is A; H has four keyframes and free extrinsics, as B"""
    return cc.selections({"H": "B", "U": "A"}.get(name, name))


def stage_two(terms, Spp, cov):
    """(e of the device, of numpy with numpy.linalg.inv(V), of numpy with inv3sym's cofactor formula, the bound), per landmark:
    all against the 60-digit evaluation of the formula from the same taps; bound = 4 max(the two host errors, 6 n_l 2^-52)"""
    X = ls.sigma_all(terms, Spp)
    e_inv = ls.e(ls.sigma_all(terms, Spp, "np", vinv="inv"), X)
    e_cof = ls.e(ls.sigma_all(terms, Spp, "np", vinv="cofactor"), X)
    floor = np.array([t[0].size for t in terms]) * EPS
    return ls.e(cov, X), e_inv, e_cof, cc.BOUND_FACTOR * np.maximum(np.maximum(e_inv, e_cof), floor)


class Device:
    """one case on the device in one session: the all-landmarks call with taps, every state selection, the pair lists; then, on
    the host and once, the 60-digit evaluation of the formula from the taps and the two fp64 evaluations"""

    def __init__(self, name, optimized):
        self.w = w = lc.window(name)
        b = solver.WindowBatch([w])
        if optimized:
            b.optimize(cc.OPT_ITERS)
        self.got = b.landmark_covariance(want_taps=True)[0]
        self.state = {} if optimized else {sel: b.state_covariance(blocks, want_S0=True)[0] for sel, blocks in selections(name).items()}
        self.pairs = b.pairs(0)
        b.close()
        g = self.got
        self.terms = ls.landmark_terms(w, g["V"], g["W"], self.pairs)
        self.observed = np.array([t[0].size > 0 for t in self.terms])
        self.e_dev, self.e_inv, self.e_cof, self.bound2 = stage_two(self.terms, g["Spp"], g["cov"])


@functools.lru_cache(maxsize=None)
def _device(name, optimized):
    return Device(name, optimized)


def device(name, optimized=False):
    return _device(name, bool(optimized))


@functools.lru_cache(maxsize=None)
def stage_one(name):
    """(Inverse of the S0 tap over `cols`, cols, bound): all pose-type columns, or cov_cases.columns below Dp for D and F"""
    d = device(name)
    Dp = lc.POSE_DIM[name]
    cols = np.arange(Dp) if name in lc.FULL else np.array([c for c in cc.columns(name, d.w) if c < Dp])
    inv = cc.Inverse(d.got["S0"], cols)
    return inv, cols, cc.BOUND_FACTOR * max(inv.e_chol, inv.e_lu, d.got["S0"].shape[0] * EPS)


# ---- 1. stage two inverts its taps -------------------------------------------------------------------
@STATES
@pytest.mark.parametrize("name", lc.CASES)
def test_stage_two_inverts_its_taps(name, optimized):
    d = device(name, optimized)
    g = d.got
    n_lm = len(d.terms)
    assert g["info"] == 0 and g["min_pivot"] > 0.0 and g["cov"].shape == (n_lm, 3, 3) and g["flags"].shape == (n_lm,)
    assert np.array_equal(g["flags"], ~d.observed)
    obs = d.observed
    assert np.array_equal(g["cov"][obs], np.swapaxes(g["cov"][obs], 1, 2)), "bitwise symmetric"
    assert np.all(np.isnan(g["cov"][~obs]))
    ratio = np.where(obs, d.e_dev / np.where(obs, d.bound2, 1.0), 0.0)
    worst = int(np.argmax(ratio))
    print(f"\nlmcov stage two {name} {'optimized' if optimized else 'uploaded'}: device worst {d.e_dev.max():.3e}  numpy inv worst {d.e_inv.max():.3e}  "
          f"numpy cofactor worst {d.e_cof.max():.3e}  worst device / bound {ratio.max():.3f} at landmark {worst} "
          f"(device {d.e_dev[worst]:.3e} inv {d.e_inv[worst]:.3e} cofactor {d.e_cof[worst]:.3e} rows {d.terms[worst][0].size})")
    assert np.all(d.e_dev <= d.bound2), (name, worst, d.e_dev[worst], d.bound2[worst])
    lam = np.linalg.eigvalsh(g["cov"][obs])
    assert lam.min() > 0.0


# ---- 2. stage one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.CASES)
def test_stage_one_is_the_state_covariance(name):
    d = device(name)
    Spp, Dp = d.got["Spp"], lc.POSE_DIM[name]
    assert Spp.shape == (Dp, Dp) and np.array_equal(Spp, Spp.T), "the tap is bitwise symmetric"
    compared = 0
    for sel, blocks in selections(name).items():
        st = d.state[sel]
        assert st["S0"].tobytes() == d.got["S0"].tobytes(), "the S0 tap is the one state_covariance returns"
        rows = cs.rows_of(d.w, blocks)
        at = np.flatnonzero(rows < Dp)
        if at.size:
            assert Spp[np.ix_(rows[at], rows[at])].tobytes() == st["cov"][np.ix_(at, at)].tobytes(), (name, sel)
            compared += at.size
        assert st["min_pivot"] == d.got["min_pivot"]
    assert compared > 0
    inv, cols, bound = stage_one(name)
    err = cs.e(Spp[np.ix_(cols, cols)], inv.X)
    print(f"\nlmcov stage one {name}: |C| {cols.size} of Dp {Dp}  device {err:.3e} host chol {inv.e_chol:.3e} lu {inv.e_lu:.3e} bound {bound:.3e}")
    assert err <= bound


# ---- 3. end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.FULL)
def test_end_to_end_against_the_long_double_oracle(oracle, name):
    d = device(name)
    ref, o64 = lc.reference(oracle, name, extended=True), lc.reference(oracle, name)
    e_oracle = ls.e(o64.X, ref.X)
    bound = cc.BOUND_FACTOR * np.maximum(np.maximum(e_oracle, d.bound2), stage_one(name)[2])
    err = ls.e(d.got["cov"], ref.X)
    worst = int(np.argmax(err / bound))
    print(f"\nlmcov end to end {name}: device worst {err.max():.3e}  fp64 oracle worst {e_oracle.max():.3e}  worst device / bound {(err / bound).max():.2e} "
          f"at landmark {worst}")
    assert np.all(err <= bound), (name, worst, err[worst], bound[worst])


# ---- 4. bits -----------------------------------------------------------------------------------------
def test_a_selection_has_the_bits_of_the_all_landmarks_call():
    b = solver.WindowBatch([cc.window("A")])
    sel = [7, 3, 3, 0]
    got = b.landmark_covariance(sel)[0]
    one = b.landmark_covariance([3])[0]
    b.close()
    everything = device("A").got
    assert got["cov"].shape == (4, 3, 3) and not got["flags"].any()
    assert got["cov"].tobytes() == everything["cov"][sel].tobytes()
    assert got["cov"][1].tobytes() == got["cov"][2].tobytes() == one["cov"][0].tobytes()


def test_a_mixed_range_has_the_bits_of_the_single_calls():
    """(single calls on the same batch: another batch may be linearised on another launch route)"""
    names = ("A", "C", "H", "U", "F")
    b = solver.WindowBatch([lc.window(n) for n in names])
    got = b.landmark_covariance(want_taps=True)
    singles = [b.landmark_covariance(w0=i, n=1, want_taps=True)[0] for i in range(len(names))]
    sub = b.landmark_covariance(w0=1, n=3)
    sel = b.landmark_covariance([[1, 0], None, [29, 29], [lc.NO_PAIRS, 6], [59]])
    b.close()
    for i, (n, g) in enumerate(zip(names, got)):
        one = singles[i]
        for k in ("cov", "flags", "S0", "Spp", "V", "W"):
            assert g[k].tobytes() == one[k].tobytes(), (n, k)
        assert g["min_pivot"] == one["min_pivot"] and g["info"] == 0
        if 1 <= i <= 3:
            assert sub[i - 1]["cov"].tobytes() == g["cov"].tobytes() and np.array_equal(sub[i - 1]["flags"], g["flags"])
        # (a window's numbers against its own taps, also in this batch's layout)
        if n in ("A", "U"):
            d = device(n)
            e_dev, _, _, bound = stage_two(ls.landmark_terms(d.w, g["V"], g["W"], d.pairs), g["Spp"], g["cov"])
            assert np.all(e_dev <= bound), n
    assert sel[0]["cov"].tobytes() == got[0]["cov"][[1, 0]].tobytes() and sel[1]["cov"].tobytes() == got[1]["cov"].tobytes()
    assert sel[2]["cov"].tobytes() == got[2]["cov"][[29, 29]].tobytes() and sel[4]["cov"].tobytes() == got[4]["cov"][[59]].tobytes()
    assert sel[3]["cov"].tobytes() == got[3]["cov"][[lc.NO_PAIRS, 6]].tobytes() and sel[3]["flags"].tolist() == [True, False]


def test_nine_copies_have_the_bits_of_one():
    """nine windows: above SOLVE_HELPED_MAX_WINDOWS = 8, the Schur partials are summed inside the solving workgroup"""
    b = solver.WindowBatch([cc.window("A") for _ in range(9)])
    got = b.landmark_covariance(want_taps=True)
    one = b.landmark_covariance(w0=4, n=1, want_taps=True)[0]       # (one window: with helper workgroups)
    b.close()
    for g in got:
        for k in ("cov", "flags", "S0", "Spp", "V", "W"):
            assert g[k].tobytes() == one[k].tobytes(), k
    assert not one["flags"].any() and one["info"] == 0


# ---- 5. a landmark without pairs, a window without an inverse ----------------------------------------
def test_an_unobserved_landmark_fails_alone():
    d = device("U")
    g = d.got
    assert g["info"] == 0 and g["flags"].tolist() == [l == lc.NO_PAIRS for l in range(40)]
    assert np.isnan(g["cov"][lc.NO_PAIRS]).all() and np.all(np.isfinite(np.delete(g["cov"], lc.NO_PAIRS, axis=0)))
    assert np.all(np.delete(d.e_dev <= d.bound2, lc.NO_PAIRS))
    assert all(s["info"] == 0 for s in d.state.values()), "okvis_ba_state_covariance serves the window too"
    assert np.all(g["V"][lc.NO_PAIRS] == 0.0)


def test_a_singular_window_fails_alone():
    wins = [cc.window("A"), cc.singular_window(), cc.window("B")]
    b = solver.WindowBatch(wins)
    with pytest.raises(_lib.BackendError) as err:
        b.landmark_covariance(want_taps=True)
    assert err.value.status == ERR_NUMERIC
    got = err.value.results
    assert [g["info"] for g in got] == [0, 1, 0]
    assert np.isnan(got[1]["cov"]).all() and got[1]["cov"].shape == (40, 3, 3) and got[1]["flags"].all() and np.isnan(got[1]["Spp"]).all()
    assert np.diag(got[1]["S0"]).min() == 0.0
    for i in (0, 2):
        assert np.all(np.isfinite(got[i]["cov"])) and not got[i]["flags"].any()
        one = b.landmark_covariance(w0=i, n=1)[0]              # the solver serves the next calls: the outer two alone
        assert one["info"] == 0 and one["cov"].tobytes() == got[i]["cov"].tobytes()
    b.close()


# ---- 6. the solver is untouched; arguments and state -------------------------------------------------
def _snapshot(b):
    out = []
    for w in range(len(b)):
        r = b.fetch_results(w)
        out.append([np.asarray(x).tobytes() for x in b.get_state(w)] + [r[k].tobytes() for k in sorted(r)] + [b.fetch_imu_caches(w).tobytes()])
    return out


@pytest.mark.parametrize("names", [("A", "H"), ("D",), ("E", "C", "U")])
def test_solver_is_left_as_it_was(names):
    def run(middle):
        b = solver.WindowBatch([lc.window(n) for n in names])
        s1 = b.optimize(3)
        before = _snapshot(b)
        if middle:
            b.landmark_covariance(want_taps=True)
        mid = _snapshot(b)
        s2 = b.optimize(3)
        end = _snapshot(b)
        b.close()
        return s1, before, mid, s2, end
    plain, called = run(False), run(True)
    assert called[1] == called[2], "fetch_results / fetch_imu_caches / get_state right behind the call"
    assert plain == called


def test_uploaded_state_is_left_as_it_was():
    def run(middle):
        b = solver.WindowBatch([cc.window("A"), cc.window("C")])
        if middle:
            b.landmark_covariance()
        first = _snapshot(b)
        s = b.optimize(4)
        end = _snapshot(b)
        b.close()
        return first, s, end
    assert run(False) == run(True)


def _raw(b, sels, counts, w0=0, n=None, capacity=None, null=None, taps=None):
    """the C entry itself on prepared structures: (status, results, outs) — every output array starts as a pattern"""
    specs, results, outs, keep = lmcov_marshal_batch(sels, counts, taps)
    for i, o in enumerate(outs):
        o["cov"][:] = -7.0
        o["flags"][:] = 7
        for k in ("S0", "Spp", "V", "W"):
            if k in o:
                o[k][:] = -7.0
        results[i].n, results[i].info, results[i].min_pivot = -7, -7, -7.0
        if capacity is not None:
            results[i].capacity = capacity
        if null:
            setattr(results[i], null, None)
    st = b._L.okvis_ba_landmark_covariance(b._h, w0, len(sels) if n is None else n, specs, results)
    del keep
    return st, results, outs


def _untouched(results, outs):
    return (all(np.all(v == (7 if k == "flags" else -7.0)) for o in outs for k, v in o.items()) and
            all(results[i].n == -7 and results[i].info == -7 and results[i].min_pivot == -7.0 for i in range(len(outs))))


def test_arguments_and_state():
    wA, wF = cc.window("A"), cc.window("F")
    b = solver.WindowBatch([wA, wF])
    counts = [40, 60]
    taps = [(60, 24, 40, int(b.pairs(0)[0].size)), (174, 66, 60, int(b.pairs(1)[0].size))]
    good = [[7, 3, 3, 0], None]
    ref = b.landmark_covariance(good)

    def right_numbers():
        now = b.landmark_covariance(good)
        assert all(x["cov"].tobytes() == y["cov"].tobytes() for x, y in zip(now, ref))

    bad = {"index = n_lm": [[40], None], "negative index": [[0, -1], None], "index out of range in the second window": [None, [3, 60]]}
    for what, sels in bad.items():
        st, results, outs = _raw(b, sels, counts, taps=taps)
        assert st == ERR_ARG and _untouched(results, outs), what
        right_numbers()
    for what, kw in {"capacity below n": dict(capacity=3), "NULL cov": dict(null="cov"), "NULL flags": dict(null="flags")}.items():
        st, results, outs = _raw(b, good, counts, taps=taps, **kw)
        assert st == ERR_ARG and _untouched(results, outs), what
    specs, results, outs, keep = lmcov_marshal_batch(good, counts)
    specs[0].n_lm = -1
    assert b._L.okvis_ba_landmark_covariance(b._h, 0, 2, specs, results) == ERR_ARG
    specs[0].n_lm = 4
    for w0, n in ((-1, 2), (1, 2), (0, 0), (2, 1)):
        st, results_, outs_ = _raw(b, good, counts, w0=w0, n=n)
        assert st == ERR_ARG and _untouched(results_, outs_), (w0, n)
    L = b._L
    assert L.okvis_ba_landmark_covariance(None, 0, 2, specs, results) == ERR_ARG
    assert L.okvis_ba_landmark_covariance(b._h, 0, 2, None, results) == ERR_ARG
    assert L.okvis_ba_landmark_covariance(b._h, 0, 2, specs, None) == ERR_ARG
    right_numbers()
    # an empty list is served: nothing for that window
    st, results_, outs_ = _raw(b, [[], None], counts)
    assert st == 0 and results_[0].n == 0 and results_[1].n == 60 and np.all(outs_[0]["cov"] == -7.0)
    assert outs_[1]["cov"].reshape(60, 3, 3).tobytes() == ref[1]["cov"].tobytes()
    # between okvis_ba_begin and okvis_ba_finish
    b.begin()
    st, results_, outs_ = _raw(b, good, counts, taps=taps)
    assert st == ERR_STATE and _untouched(results_, outs_)
    b.iterate(1)
    assert _raw(b, good, counts)[0] == ERR_STATE
    b.finish()
    assert _raw(b, good, counts)[0] == 0
    # while a marginalisation is pending
    b.marginalize_batch_begin(0, [([1, 0, 0, 0, 0, 0], [1, 0, 0, 0], None)])
    st, results_, outs_ = _raw(b, good, counts, taps=taps)
    assert st == ERR_STATE and _untouched(results_, outs_)
    b.marginalize_batch_end()
    assert _raw(b, good, counts)[0] == 0
    f = C.c_float()
    assert L.okvis_ba_last_landmark_covariance_ms(b._h, C.byref(f), C.byref(f), None) == ERR_ARG
    ms = b.last_landmark_covariance_ms()
    assert all(ms[k] > 0.0 for k in ("assembly", "inverse", "landmark"))
    b.close()
    # before upload, and before the first call
    h = C.c_void_p()
    _lib.check(L.okvis_ba_create(C.byref(h), 0))
    assert L.okvis_ba_landmark_covariance(h, 0, 1, specs, results) == ERR_STATE
    assert L.okvis_ba_last_landmark_covariance_ms(h, C.byref(f), C.byref(f), C.byref(f)) == ERR_STATE
    L.okvis_ba_destroy(h)
    del keep


def test_one_block_over_is_unsupported():
    wG, wA = cc.window("G"), cc.window("A")
    b = solver.WindowBatch([wA, wG])
    counts = [40, 60]
    st, results, outs = _raw(b, [None, None], counts)
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    st, results, outs = _raw(b, [[0, 1]], counts[1:], w0=1)
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    one = b.landmark_covariance(w0=0, n=1)[0]      # the window next to it is served
    b.close()
    assert one["info"] == 0 and not one["flags"].any() and np.linalg.eigvalsh(one["cov"]).min() > 0.0


# ---- 7. Python ---------------------------------------------------------------------------------------
def test_default_selection_is_every_landmark_in_window_order():
    wins = [cc.window("A"), cc.window("B")]
    b = solver.WindowBatch(wins)
    a = b.landmark_covariance()
    e = b.landmark_covariance([list(range(40)), np.arange(60)])
    r = b.landmark_covariance([list(range(39, -1, -1)), None])
    b.close()
    assert a[0]["cov"].shape == (40, 3, 3) and a[1]["cov"].shape == (60, 3, 3)
    assert all(x["cov"].tobytes() == y["cov"].tobytes() for x, y in zip(a, e))
    assert r[0]["cov"][::-1].tobytes() == a[0]["cov"].tobytes()
    # into the newest camera frame: the matrix the 3D-2D gate adds to P_C
    Sigma = a[0]["cov"]
    R = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))[0]
    T = np.eye(4)
    T[:3, :3] = R
    P_C = landmark_covariance_in_camera(Sigma, T)
    assert np.array_equal(P_C, R @ Sigma @ R.T)
    assert np.allclose(np.trace(P_C, axis1=1, axis2=2), np.trace(Sigma, axis1=1, axis2=2), rtol=1e-12)
