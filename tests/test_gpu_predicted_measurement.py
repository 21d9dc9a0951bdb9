"""GPU: okvis_ba_predicted_measurement against the 60-digit referee (cases and references: tests/predcov_cases.py,
tests/predcov_statement.py; what the inputs can tell apart: tests/test_predicted_measurement_host.py).  Per query

    e(U, U*) = max_ij |U_ij - U*_ij| / sqrt(U*_ii U*_jj)

The query stage (predcov_kernel) is judged on its own taps V, W, Spp, jac taken as exact doubles; its Jacobians and uv against the
long double oracle's reprojection factor; stage one (cov_pose_kernel) bit for bit against okvis_ba_landmark_covariance; the whole
against the long double oracle's arrays.  Worst figures measured on an MI355X: profiles/predcov_notes.md."""
import ctypes as C
import functools

import numpy as np
import pytest

from okvis_amd import _lib, solver
from okvis_amd.frontend import Frontend
from okvis_amd.window import predcov_marshal_batch

from . import cov_cases as cc
from . import lmcov_cases as lc
from . import lmcov_statement as ls
from . import predcov_cases as pc
from . import predcov_statement as ps

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -3, -5
EPS = 2.0 ** -52
STATES = pytest.mark.parametrize("optimized", [False, True], ids=["uploaded", "optimized"])
KEYS = ("uv", "cov", "flags", "S0", "Spp", "V", "W", "jac")
# The projection chain rounds about twenty times between the stored state and an entry of uv or of a Jacobian (two rotations,
# the distortion polynomial, the scaling, two 3 x 3 products): 20 x 2^-53 = 10 x 2^-52 of the block's largest entry at the very
# worst.  The floor 4 x 2^-52 under the fp64 oracle's own distance gives a bound of at least 16 x 2^-52.
JAC_FLOOR = 4 * EPS


def query_stage(w, terms, Q, jac, Spp, cov):
    """(e of the device, of numpy form A, of numpy block form, the bound, |R|), per query: all against the 60-digit evaluation of
    form A from the same taps; bound = 4 max(the two host errors, |R| 2^-52)"""
    X = ps.u_all(w, terms, Q, jac, Spp, form="A")
    eA = ps.e(ps.u_all(w, terms, Q, jac, Spp, "np", form="A"), X)
    eB = ps.e(ps.u_all(w, terms, Q, jac, Spp, "np", form="block"), X)
    rows = np.array([ps.n_rows(w, terms[int(q[0])], q) for q in Q])
    return ps.e(cov, X), eA, eB, cc.BOUND_FACTOR * np.maximum(np.maximum(eA, eB), rows * EPS), rows, X


class Device:
    """one case on the device in one session: the case's query list with taps, the landmark covariance of the same batch, the state
    and the pair lists; then, on the host and once, the 60-digit evaluation of the formula from the taps and the two fp64 ones"""

    def __init__(self, name, optimized):
        self.w, self.Q, self.tags = pc.queries(name)
        b = solver.WindowBatch([self.w])
        if optimized:
            b.optimize(cc.OPT_ITERS)
        self.got = b.predicted_measurement([self.Q], want_taps=True)[0]
        self.lmcov = b.landmark_covariance(want_taps=True)[0]
        self.pose, _, self.lm = b.get_state(0)
        self.pairs = b.pairs(0)
        b.close()
        g = self.got
        self.terms = ls.landmark_terms(self.w, g["V"], g["W"], self.pairs)
        self.e_dev, self.eA, self.eB, self.bound, self.rows, self.X = query_stage(self.w, self.terms, self.Q, g["jac"], g["Spp"], g["cov"])


@functools.lru_cache(maxsize=None)
def _device(name, optimized):
    return Device(name, optimized)


def device(name, optimized=False):
    return _device(name, bool(optimized))


def _jac_distance(J, Js):
    """per query, the largest |J - J*| over a block (J_l, J_p, J_e) relative to that block's largest |J*|"""
    out = np.zeros(len(J))
    for lo, hi in ((0, 6), (6, 18), (18, 30)):
        out = np.maximum(out, np.abs(J[:, lo:hi] - Js[:, lo:hi]).max(axis=1) / np.abs(Js[:, lo:hi]).max(axis=1))
    return out


# ---- 1. the query stage on its own taps --------------------------------------------------------------
@STATES
@pytest.mark.parametrize("name", pc.CASES)
def test_query_stage_on_its_taps(oracle, name, optimized):
    d = device(name, optimized)
    g, n = d.got, len(d.Q)
    assert g["info"] == 0 and g["min_pivot"] > 0.0 and g["cov"].shape == (n, 2, 2) and g["uv"].shape == (n, 2) and g["flags"].shape == (n,)
    projects = ps.jacobians_all(oracle.lib_ld(), d.w, d.Q, d.pose, d.lm)[2]
    want = pc.expected_flags(d.w, d.terms, d.Q, projects)
    assert np.array_equal(g["flags"], want), "flags are exactly the expected ones"
    good = want == 0
    assert np.array_equal(g["cov"][good], np.swapaxes(g["cov"][good], 1, 2)), "bitwise symmetric"
    assert np.all(np.isnan(g["cov"][~good])) and np.all(np.isfinite(g["cov"][good]))
    assert np.array_equal(np.isnan(g["uv"]).any(axis=1), want & 2 != 0) and np.array_equal(np.isnan(g["jac"]).any(axis=1), want & 2 != 0)
    assert want[d.tags == "behind"].tolist() == [2]
    if name == "U":
        assert want[lc.NO_PAIRS] == 1 and np.all(np.isfinite(g["uv"][lc.NO_PAIRS]))
    ratio = np.where(good, d.e_dev / np.where(good, d.bound, 1.0), 0.0)
    worst = int(np.argmax(ratio))
    print(f"\npredcov query stage {name} {'optimized' if optimized else 'uploaded'}: device worst {d.e_dev.max():.3e}  numpy form A worst {d.eA.max():.3e}  "
          f"numpy block form worst {d.eB.max():.3e}  worst device / bound {ratio.max():.3f} at query {worst} {d.Q[worst].tolist()} "
          f"(device {d.e_dev[worst]:.3e} A {d.eA[worst]:.3e} block {d.eB[worst]:.3e} rows {d.rows[worst]})")
    assert np.all(d.e_dev <= d.bound), (name, worst, d.e_dev[worst], d.bound[worst])
    assert np.linalg.eigvalsh(g["cov"][good]).min() > 0.0, "positive definite"
    # repeats are identical rows
    rep = np.flatnonzero(d.tags == "repeats")
    assert g["cov"][rep[0]].tobytes() == g["cov"][0].tobytes() and g["uv"][rep[0]].tobytes() == g["uv"][0].tobytes()
    assert g["flags"][rep[1]] == 2


# ---- 2. Jacobians and uv -----------------------------------------------------------------------------
@STATES
@pytest.mark.parametrize("name", pc.CASES)
def test_jacobians_and_uv_against_the_long_double_oracle(oracle, name, optimized):
    d = device(name, optimized)
    uv_s, J_s, ok = ps.jacobians_all(oracle.lib_ld(), d.w, d.Q, d.pose, d.lm)
    uv_o, J_o, ok_o = ps.jacobians_all(oracle.lib(), d.w, d.Q, d.pose, d.lm)
    assert np.array_equal(ok, ok_o) and ok.sum() >= len(ok) - 2
    bound_J = cc.BOUND_FACTOR * np.maximum(_jac_distance(J_o[ok], J_s[ok]), JAC_FLOOR)
    err_J = _jac_distance(d.got["jac"][ok], J_s[ok])
    scale = np.abs(uv_s[ok]).max(axis=1)
    bound_uv = cc.BOUND_FACTOR * np.maximum(np.abs(uv_o[ok] - uv_s[ok]).max(axis=1) / scale, JAC_FLOOR)
    err_uv = np.abs(d.got["uv"][ok] - uv_s[ok]).max(axis=1) / scale
    print(f"\npredcov jacobians {name} {'optimized' if optimized else 'uploaded'}: J device worst {err_J.max() / EPS:.2f} eps, fp64 oracle worst "
          f"{_jac_distance(J_o[ok], J_s[ok]).max() / EPS:.2f} eps, worst device / bound {(err_J / bound_J).max():.3f};  uv device worst {err_uv.max() / EPS:.2f} eps, "
          f"worst device / bound {(err_uv / bound_uv).max():.3f}")
    assert np.all(err_J <= bound_J) and np.all(err_uv <= bound_uv)


# ---- 3. stage one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CASES)
def test_stage_one_has_the_bytes_of_the_landmark_entry(name):
    d = device(name)
    for k in ("S0", "Spp", "V", "W"):
        assert d.got[k].tobytes() == d.lmcov[k].tobytes(), k
    assert d.got["min_pivot"] == d.lmcov["min_pivot"]


# ---- 4. end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.FULL)
def test_end_to_end_against_the_long_double_oracle(oracle, name):
    from . import test_gpu_landmark_covariance as tl
    d = device(name)
    ref, o64 = lc.reference(oracle, name, extended=True), lc.reference(oracle, name)
    X_ref = ps.u_all(d.w, ref.terms, d.Q, ps.jacobians_all(oracle.lib_ld(), d.w, d.Q)[1], ref.inv.X)
    X_64 = ps.u_all(d.w, o64.terms, d.Q, ps.jacobians_all(oracle.lib(), d.w, d.Q)[1], o64.inv.X)
    e_oracle = ps.e(X_64, X_ref)
    bound = cc.BOUND_FACTOR * np.maximum(np.maximum(e_oracle, d.bound), tl.stage_one(name)[2])
    err = ps.e(d.got["cov"], X_ref)
    worst = int(np.argmax(err / bound))
    print(f"\npredcov end to end {name}: device worst {err.max():.3e}  fp64 oracle worst {e_oracle.max():.3e}  worst device / bound {(err / bound).max():.2e} "
          f"at query {worst} {d.Q[worst].tolist()}")
    assert np.all(err <= bound), (name, worst, err[worst], bound[worst])


# ---- 5. bits -----------------------------------------------------------------------------------------
def test_a_selection_has_the_bits_of_the_full_call():
    d = device("A")
    b = solver.WindowBatch([d.w])
    sel = [7, 3, 3, 0, len(d.Q) - 3]
    got = b.predicted_measurement([d.Q[sel]], want_taps=True)[0]
    one = b.predicted_measurement([d.Q[[3]]])[0]
    none = b.predicted_measurement([np.zeros((0, 4), np.int32)])[0]
    b.close()
    for k in ("uv", "cov", "flags", "jac"):
        assert got[k].tobytes() == d.got[k][sel].tobytes(), k
    assert got["cov"][1].tobytes() == got["cov"][2].tobytes() == one["cov"][0].tobytes() and one["uv"].tobytes() == got["uv"][1].tobytes()
    assert none["cov"].shape == (0, 2, 2) and none["info"] == 0


def test_a_mixed_range_has_the_bits_of_the_single_calls():
    """(single calls on the same batch: another batch may be linearised on another launch route)"""
    names = ("A", "C", "H", "U", "F")
    cases = [pc.queries(n) for n in names]
    b = solver.WindowBatch([c[0] for c in cases])
    Qs = [c[1] for c in cases]
    got = b.predicted_measurement(Qs, want_taps=True)
    singles = [b.predicted_measurement([Qs[i]], w0=i, n=1, want_taps=True)[0] for i in range(len(names))]
    sub = b.predicted_measurement(Qs[1:4], w0=1, n=3)
    pairs = [b.pairs(i) for i in range(len(names))]
    b.close()
    for i, (n, g) in enumerate(zip(names, got)):
        for k in KEYS:
            assert g[k].tobytes() == singles[i][k].tobytes(), (n, k)
        assert g["min_pivot"] == singles[i]["min_pivot"] and g["info"] == 0
        if 1 <= i <= 3:
            assert all(sub[i - 1][k].tobytes() == g[k].tobytes() for k in ("uv", "cov", "flags"))
        # (a window's numbers against its own taps, also in this batch's layout)
        if n in ("A", "H"):
            w, Q = cases[i][0], Qs[i]
            e_dev, _, _, bound, _, _ = query_stage(w, ls.landmark_terms(w, g["V"], g["W"], pairs[i]), Q, g["jac"], g["Spp"], g["cov"])
            assert np.all(e_dev <= bound), n


def test_nine_copies_have_the_bits_of_one():
    """nine windows: above SOLVE_HELPED_MAX_WINDOWS = 8, the Schur partials are summed inside the solving workgroup"""
    w, Q, _ = pc.queries("A")
    b = solver.WindowBatch([w for _ in range(9)])
    got = b.predicted_measurement([Q] * 9, want_taps=True)
    one = b.predicted_measurement([Q], w0=4, n=1, want_taps=True)[0]       # (one window: with helper workgroups)
    b.close()
    for g in got:
        for k in KEYS:
            assert g[k].tobytes() == one[k].tobytes(), k
    assert one["info"] == 0 and (one["flags"] == 0).sum() == len(Q) - 2


# ---- 6. next to the landmark entry, and into the gate ------------------------------------------------
def test_fixed_blocks_give_the_projected_landmark_covariance():
    """F's queries from the fixed pose through fixed extrinsics: rows_x is empty, U = J_l Sigma_l J_l^T with Sigma_l what
    okvis_ba_landmark_covariance returns.  Both are within their bounds of the same exact function of the same taps; a distance
    e on Sigma_l moves an entry of J Sigma J^T by at most e (|J| s)(|J| s)^T, s = sqrt(diag Sigma*)."""
    from . import test_gpu_landmark_covariance as tl
    d = device("F")
    fx = np.flatnonzero(d.tags == "fixed")
    assert fx.size == 2
    lms = d.Q[fx, 0]
    terms = [d.terms[int(l)] for l in lms]
    _, _, _, bound_l = tl.stage_two(terms, d.got["Spp"], d.lmcov["cov"][lms])
    S_star = ls.sigma_all(terms, d.got["Spp"])
    for k, l, bl, Ss in zip(fx, lms, bound_l, S_star):
        assert ps.rows_x_of(d.w, d.Q[k])[0].size == 0
        Jl = ps.split(d.got["jac"][k])[0]
        U = Jl @ d.lmcov["cov"][l] @ Jl.T
        s = np.abs(Jl) @ np.sqrt(np.diag(Ss))
        dd = np.sqrt(np.diag(d.X[k]))
        tol = d.bound[k] * np.outer(dd, dd) + (bl + 8 * EPS) * np.outer(s, s)
        print(f"\npredcov next to lmcov, query {d.Q[k].tolist()}: |U - J Sigma J^T| / tolerance {(np.abs(d.got['cov'][k] - U) / tol).max():.3f}")
        assert np.all(np.abs(d.got["cov"][k] - U) <= tol)


def test_uv_and_cov_go_into_the_gate():
    d = device("B")
    uv, U = d.got["uv"], d.got["cov"]
    good = np.flatnonzero(d.got["flags"] == 0)
    rng = np.random.default_rng(5)
    kp_b = np.concatenate([uv[good] + rng.normal(0, 1.5, (good.size, 2)), rng.uniform(4, 12, (good.size, 1))], axis=1).astype(np.float32)
    pairs = np.stack([good, np.arange(good.size)], 1).astype(np.int32)
    fe = Frontend()
    chi2, flags = fe.gate_3d2d(uv, U, kp_b, pairs)
    fe.close()
    s2 = (0.8 * kp_b[:, 2].astype(np.float64) / 12.0) ** 2
    err = uv[good] - kp_b[:, :2].astype(np.float64)
    want = np.einsum("ni,nij,nj->n", err, np.linalg.inv(U[good] + s2[:, None, None] * np.eye(2)), err)
    assert np.abs(chi2 - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    assert np.all(chi2 > 0.0) and flags.shape == (good.size,)


# ---- 7. a window without an inverse ------------------------------------------------------------------
def test_a_singular_window_fails_alone():
    wA, QA, _ = pc.queries("A")
    wB, QB, _ = pc.queries("B")
    ws = cc.singular_window()
    Qs = np.array([[l, 3, 4 + l % 2, l % 2] for l in range(40)], np.int32)
    b = solver.WindowBatch([wA, ws, wB])
    with pytest.raises(_lib.BackendError) as err:
        b.predicted_measurement([QA, Qs, QB], want_taps=True)
    assert err.value.status == ERR_NUMERIC
    got = err.value.results
    assert [g["info"] for g in got] == [0, 1, 0]
    assert np.isnan(got[1]["cov"]).all() and got[1]["cov"].shape == (40, 2, 2) and np.all(got[1]["flags"] & 1) and np.isnan(got[1]["Spp"]).all()
    assert np.all(np.isfinite(got[1]["uv"][got[1]["flags"] & 2 == 0]))
    for i, d in ((0, device("A")), (2, device("B"))):
        assert np.array_equal(got[i]["flags"], d.got["flags"])
        one = b.predicted_measurement([(QA, None, QB)[i]], w0=i, n=1)[0]     # the solver serves the next calls: the outer two alone
        assert one["info"] == 0 and one["cov"].tobytes() == got[i]["cov"].tobytes()
    b.close()


# ---- 8. the solver is untouched; arguments and state -------------------------------------------------
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
            b.predicted_measurement([pc.queries(n)[1] for n in names], want_taps=True)
        mid = _snapshot(b)
        s2 = b.optimize(3)
        end = _snapshot(b)
        b.close()
        return s1, before, mid, s2, end
    plain, called = run(False), run(True)
    assert called[1] == called[2], "fetch_results / fetch_imu_caches / get_state right behind the call"
    assert plain == called


def _raw(b, Qs, w0=0, n=None, capacity=None, null=None, taps=None):
    """the C entry itself on prepared structures: (status, specs, results, outs) — every output array starts as a pattern"""
    specs, results, outs, keep = predcov_marshal_batch(Qs, taps)
    for i, o in enumerate(outs):
        for k, v in o.items():
            v[:] = 7 if k == "flags" else -7.0
        results[i].n, results[i].info, results[i].min_pivot = -7, -7, -7.0
        if capacity is not None:
            results[i].capacity = capacity
        if null:
            setattr(results[i], null, None)
    st = b._L.okvis_ba_predicted_measurement(b._h, w0, len(Qs) if n is None else n, specs, results)
    del keep
    return st, results, outs


def _untouched(results, outs):
    return (all(np.all(v == (7 if k == "flags" else -7.0)) for o in outs for k, v in o.items()) and
            all(results[i].n == -7 and results[i].info == -7 and results[i].min_pivot == -7.0 for i in range(len(outs))))


def test_arguments_and_state():
    wA, QA, _ = pc.queries("A")
    wF, QF, _ = pc.queries("F")
    b = solver.WindowBatch([wA, wF])
    taps = [(60, 24, 40, int(b.pairs(0)[0].size)), (174, 66, 60, int(b.pairs(1)[0].size))]
    good = [QA[[7, 3, 3, 0]], QF]
    ref = b.predicted_measurement(good)

    def right_numbers():
        now = b.predicted_measurement(good)
        assert all(x["cov"].tobytes() == y["cov"].tobytes() and x["uv"].tobytes() == y["uv"].tobytes() for x, y in zip(now, ref))

    n_poseA = int(np.asarray(wA.pose).reshape(-1, 7).shape[0])
    bad = {"landmark = n_lm": [[[40, 3, 4, 0]], QF], "negative landmark": [[[0, 3, 4, 0], [-1, 3, 4, 0]], QF],
           "pose = n_pose": [[[0, n_poseA, 4, 0]], QF], "negative pose": [[[0, -1, 4, 0]], QF],
           "ext = n_pose": [[[0, 3, n_poseA, 0]], QF], "negative ext": [[[0, 3, -1, 0]], QF],
           "cam = n_cam": [[[0, 3, 4, 2]], QF], "negative cam": [[[0, 3, 4, -1]], QF],
           "ext and pose name the same block": [[[0, 3, 3, 0]], QF],
           "index out of range in the second window": [QA[:2], [[3, 1, 12, 0], [60, 1, 12, 0]]]}
    for what, Qs in bad.items():
        st, results, outs = _raw(b, [np.array(q, np.int32) for q in Qs], taps=taps)
        assert st == ERR_ARG and _untouched(results, outs), what
    right_numbers()
    for what, kw in {"capacity below n_q": dict(capacity=3), "NULL uv": dict(null="uv"), "NULL cov": dict(null="cov"), "NULL flags": dict(null="flags")}.items():
        st, results, outs = _raw(b, good, taps=taps, **kw)
        assert st == ERR_ARG and _untouched(results, outs), what
    specs, results, outs, keep = predcov_marshal_batch(good)
    specs[0].n_q = -1
    assert b._L.okvis_ba_predicted_measurement(b._h, 0, 2, specs, results) == ERR_ARG
    specs[0].n_q = 4
    specs[0].q_ext = None
    assert b._L.okvis_ba_predicted_measurement(b._h, 0, 2, specs, results) == ERR_ARG
    specs, results, outs, keep = predcov_marshal_batch(good)
    for w0, n in ((-1, 2), (1, 2), (0, 0), (2, 1)):
        st, results_, outs_ = _raw(b, good, w0=w0, n=n)
        assert st == ERR_ARG and _untouched(results_, outs_), (w0, n)
    L = b._L
    assert L.okvis_ba_predicted_measurement(None, 0, 2, specs, results) == ERR_ARG
    assert L.okvis_ba_predicted_measurement(b._h, 0, 2, None, results) == ERR_ARG
    assert L.okvis_ba_predicted_measurement(b._h, 0, 2, specs, None) == ERR_ARG
    right_numbers()
    # an empty list is served: nothing for that window
    st, results_, outs_ = _raw(b, [np.zeros((0, 4), np.int32), QF])
    assert st == 0 and results_[0].n == 0 and results_[1].n == len(QF) and np.all(outs_[0]["cov"] == -7.0) and np.all(outs_[0]["uv"] == -7.0)
    assert outs_[1]["cov"].reshape(-1, 2, 2).tobytes() == ref[1]["cov"].tobytes()
    # between okvis_ba_begin and okvis_ba_finish
    b.begin()
    st, results_, outs_ = _raw(b, good, taps=taps)
    assert st == ERR_STATE and _untouched(results_, outs_)
    b.iterate(1)
    assert _raw(b, good)[0] == ERR_STATE
    b.finish()
    assert _raw(b, good)[0] == 0
    # while a marginalisation is pending
    b.marginalize_batch_begin(0, [([1, 0, 0, 0, 0, 0], [1, 0, 0, 0], None)])
    st, results_, outs_ = _raw(b, good, taps=taps)
    assert st == ERR_STATE and _untouched(results_, outs_)
    b.marginalize_batch_end()
    assert _raw(b, good)[0] == 0
    f = C.c_float()
    assert L.okvis_ba_last_predicted_measurement_ms(b._h, C.byref(f), C.byref(f), None) == ERR_ARG
    ms = b.last_predicted_measurement_ms()
    assert all(ms[k] > 0.0 for k in ("assembly", "inverse", "query"))
    b.close()
    # before upload, and before the first call
    h = C.c_void_p()
    _lib.check(L.okvis_ba_create(C.byref(h), 0))
    assert L.okvis_ba_predicted_measurement(h, 0, 1, specs, results) == ERR_STATE
    assert L.okvis_ba_last_predicted_measurement_ms(h, C.byref(f), C.byref(f), C.byref(f)) == ERR_STATE
    L.okvis_ba_destroy(h)
    del keep


def test_one_block_over_is_unsupported():
    wG, wA = cc.window("G"), cc.window("A")
    QA = pc.queries("A")[1]
    QG = np.array([[0, 11, 12, 0], [1, 11, 13, 1]], np.int32)
    b = solver.WindowBatch([wA, wG])
    st, results, outs = _raw(b, [QA, QG])
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    st, results, outs = _raw(b, [QG], w0=1)
    assert st == ERR_UNSUPPORTED and _untouched(results, outs)
    one = b.predicted_measurement([QA], w0=0, n=1)[0]      # the window next to it is served
    b.close()
    assert one["info"] == 0 and np.array_equal(one["flags"], device("A").got["flags"]) and np.all(np.isfinite(one["cov"][one["flags"] == 0]))


# ---- 9. Python ---------------------------------------------------------------------------------------
def test_default_queries_are_every_landmark_into_the_newest_state():
    wA, wC = cc.window("A"), cc.window("C")
    b = solver.WindowBatch([wA, wC])
    QA, QC = b.newest_state_queries(0), b.newest_state_queries(1)
    a = b.predicted_measurement()
    e = b.predicted_measurement([QA, QC])
    b.close()
    assert QA.shape == (80, 4) and QC.shape == (120, 4)
    assert np.array_equal(QA[:40], np.stack([np.arange(40), np.full(40, 3), np.full(40, 4), np.zeros(40, int)], 1))
    assert np.array_equal(QA[40:], np.stack([np.arange(40), np.full(40, 3), np.full(40, 5), np.ones(40, int)], 1))
    assert np.all(QC[:, 1] == 2) and set(map(tuple, QC[:, 2:].tolist())) == {(3 + 2 * 2, 0), (3 + 2 * 2 + 1, 1)}, "per-frame: the newest frame's blocks"
    assert all(x["cov"].tobytes() == y["cov"].tobytes() and x["uv"].tobytes() == y["uv"].tobytes() for x, y in zip(a, e))
    # the even landmarks through camera 0 and the odd ones through camera 1 are rows of the referee's list
    d = device("A")
    rows = np.concatenate([np.arange(0, 40, 2), 40 + np.arange(1, 40, 2)])
    # (another batch may be linearised on another launch route: no bits across batches)
    assert np.allclose(a[0]["cov"][rows], d.got["cov"][np.concatenate([np.arange(0, 40, 2), np.arange(1, 40, 2)])], rtol=1e-9, atol=0.0)
