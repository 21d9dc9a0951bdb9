"""The IMU factor kernel (okvis_amd/csrc/ba_imu.hpp) refereed record by record on every launch route.

What is read: OKVIS_BA_ARR_IMU_LIN — per factor H (packed lower triangle over the factor's own 30 columns), g, r and the cost of
the accepted buffer, the device's order of H | g (W.imu_pos) undone on the host — and the preintegration records
(okvis_ba_fetch_imu_caches, decoded by tests/imu_cases.py::decode_record).  Every quantity is compared with the long-double oracle
in its entrywise scale, within BOUND_FACTOR * max(e_ref, (n_steps + 15) 2^-52); e_ref is measured on the CPU when the test runs
(tests/imu_cases.py has the yardstick, tests/test_imu_statement_host.py shows that seven wrong factors leave it by 2e9 x and more).

Routes (launch_route() is asserted every time), each with the first record built by imu_pre_kernel at upload (at most 8 new terms
in the batch: every case here) and, under OKVIS_BA_TUNE_NO_EARLY_PREINTEGRATION, by the first evaluation:
  default   fused linearise + reduce launch, piece path, the small factors inside the linearise launch (imu_factor<0>)
  separate  reserved0 bit 2: no fused launch
  staged    reserved0 bit 3: the staged linearise kernel (ba_linearize.hpp) carries the factors
  small     split_small with OKVIS_BA_TUNE_NO_SMALL_RIDE: small_kernel
  ride      split_small: small_prepare_kernel (imu_factor<1>) and, from the first iteration on, the second half riding in the Schur
            launch (imu_factor<2>); okvis_ba_begin's own evaluation is small_kernel's on this route, so the riding half is judged
            by test_record_after_iterations
Every case of tests/imu_cases.py runs on the default route, imu_cases.OTHER_ROUTES on the others.

Per factor: H, g, r, the cost and every field of the record within the bounds; H also block by block against the oracle's J (a
wrong place in the packed order shows as the block it lands in); redo_count as the oracle counts; the record's reference bias is
the bias it was evaluated at, to the bit.  Record life cycle: the inherited reference bias (flag 1) and the travelling record
(flag 2) on both sides of |db_g| Dt > 1e-4, the early record made stale by okvis_ba_set_state.  Across routes: the same bits.
After three Gauss-Newton iterations: the accepted buffer's record against the referee at the accepted state and the device's own
IMU_SB_REF.  Measured ratios: profiles/imu_referee_notes.md."""
import numpy as np
import pytest

from okvis_amd.window import TUNE_NO_EARLY_PREINTEGRATION, TUNE_NO_SMALL_RIDE, default_options, set_options

from . import imu_cases as cases
from . import imu_statement as stmt

pytestmark = pytest.mark.gpu

FLAT = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
# label: (options, what launch_route() must say)
ROUTES = {
    "default": ({}, dict(fused=1, piece_path=1, split_small=0)),
    "separate": (dict(reserved0=4), dict(fused=0, piece_path=1, split_small=0)),
    "staged": (dict(reserved0=8), dict(piece_path=0, split_small=0)),
    "small": (dict(reserved0=4, tuning_split_small_min=1, tuning_flags=TUNE_NO_SMALL_RIDE), dict(fused=0, split_small=1, small_rides=0)),
    "ride": (dict(reserved0=4, tuning_split_small_min=1), dict(fused=0, split_small=1, small_rides=1, decision_free_schur=1)),
}
EARLY = {"early": 0, "first_evaluation": TUNE_NO_EARLY_PREINTEGRATION}


@pytest.fixture(scope="module")
def ref(oracle):
    assert np.finfo(np.longdouble).eps < 2e-19, "the referee needs an extended long double"
    r = cases.Referee(oracle)
    r.runs = {}
    return r


def _batch(ws, label, early, **extra):
    from okvis_amd import solver
    options, expect = ROUTES[label]
    options = dict(FLAT, **options, **extra)
    options["tuning_flags"] = options.get("tuning_flags", 0) | EARLY[early]
    b = solver.WindowBatch(ws, options=set_options(default_options(), **options))
    route = b.launch_route()
    assert {k: route[k] for k in expect} == expect, (label, early, route, expect)
    return b


def _read(b, n_windows):
    out = []
    for i in range(n_windows):
        lin = b.array("IMU_LIN", i).reshape(-1, cases.LIN_DOUBLES)
        rec = b.fetch_imu_caches(i)
        assert lin.shape[0] == rec.shape[0]
        out.append((lin, rec))
    return out


def _blocks(fac, lin):
    """H unpacked, block by block over pose0 | sb0 | pose1 | sb1 against the referee's: [(block, deviation / bound)]"""
    a, b = np.tril_indices(30)
    H, Href, A = (np.zeros((30, 30), np.longdouble) for _ in range(3))
    H[a, b], Href[a, b], A[a, b] = lin[slice(*cases.LIN["H"])], fac.ref["H"], fac.a["H"]
    out = []
    for bi, (r0, r1) in enumerate(stmt.COLS):
        for bj, (c0, c1) in enumerate(stmt.COLS[:bi + 1]):
            rows, cols = np.tril_indices(r1 - r0) if bi == bj else np.indices((r1 - r0, c1 - c0)).reshape(2, -1)
            sel = (rows + r0, cols + c0)
            out.append(((bi, bj), cases.deviation(H[sel], Href[sel], A[sel]) / fac.bound("H")))
    return out


def judge(tag, fac, lin, rec, failures, expect_redo=None, expect_ref=None):
    """one factor of the device against its referee; prints every ratio, appends what is out of bounds"""
    dev, d = fac.judge(lin, rec)
    worst = 0.0
    for q in cases.QUANTITIES:
        ratio = dev[q] / fac.bound(q)
        worst = max(worst, ratio)
        print(f"IMUREF {tag} {q} e_kernel {dev[q]:.3e} e_ref {fac.e_ref[q]:.3e} bound {fac.bound(q):.3e} ratio {ratio:.3f}")
        if not dev[q] <= fac.bound(q):
            failures.append((tag, q, dev[q], fac.bound(q)))
    # the cost alone: r.r / 2 of the device's OWN r (15 products, 14 additions, each rounded once)
    r = lin[slice(*cases.LIN["r"])].astype(np.longdouble)
    alone = float(abs(lin[cases.LIN["cost"][0]] - 0.5 * np.dot(r, r)) / (0.5 * np.dot(r, r)))
    print(f"IMUREF {tag} cost alone {alone:.3e} bound {cases.BOUND_FACTOR * 15 * cases.EPS:.3e}")
    if not alone <= cases.BOUND_FACTOR * 15 * cases.EPS:
        failures.append((tag, "cost alone", alone))
    for block, ratio in _blocks(fac, lin):
        if not ratio <= 1.0:
            failures.append((tag, "H block", block, ratio))
    redo = fac.redo_count if expect_redo is None else expect_redo
    if d["redo_count"] != redo or d["valid"] != 1:
        failures.append((tag, "redo_count, valid", d["redo_count"], d["valid"], "expected", redo, 1))
    sb_ref = fac.record["sb_ref"] if expect_ref is None else expect_ref
    if not np.array_equal(d["sb_ref"], sb_ref):
        failures.append((tag, "sb_ref", d["sb_ref"], sb_ref))
    # the weight is upper triangular, exact zeros below
    SI = d["sqrt_info"].reshape(15, 15)
    if np.any(np.tril(SI, -1) != 0) or not np.all(np.diag(SI) > 0):
        failures.append((tag, "sqrt_info is not upper triangular with a positive diagonal"))
    return worst


def first_evaluation(ref, name, label, early):
    """upload, begin() / finish() with no iteration, read; memoised: the cross-route test compares what the route tests read"""
    key = (name, label, early)
    if key not in ref.runs:
        ws = ref.case(name)
        b = _batch(ws, label, early)
        b.begin()
        b.finish()
        ref.runs[key] = _read(b, len(ws))
        b.close()
    return ref.runs[key]


PARAMS = [("default", name, "early") for name in cases.CASES] + \
         [(label, name, early) for label in ROUTES for early in EARLY for name in cases.OTHER_ROUTES if (label, early) != ("default", "early")]


@pytest.mark.parametrize("label,name,early", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_route(ref, label, name, early):
    got = first_evaluation(ref, name, label, early)
    failures = []
    for i, (lin, rec) in enumerate(got):
        facs = ref.factors[name][i]
        assert lin.shape[0] == len(facs)
        for f, fac in enumerate(facs):
            assert np.all(np.isfinite(lin[f])) and np.all(np.isfinite(rec[f][:cases.RECORD_FLAGS])), (label, name, i, f)
            judge(f"{label} {early} {name} w{i} f{f}", fac, lin[f], rec[f], failures)
    assert not failures, failures


@pytest.mark.parametrize("name", cases.OTHER_ROUTES)
def test_records_are_bit_identical_across_routes(ref, name):
    """the same factor code in every launch, whoever built the first record: H, g, r, the cost and the record, to the bit"""
    base = first_evaluation(ref, name, "default", "early")
    different = []
    for label in ROUTES:
        for early in EARLY:
            got = first_evaluation(ref, name, label, early)
            for i, ((lin, rec), (lin0, rec0)) in enumerate(zip(got, base)):
                for what, x, y in (("IMU_LIN", lin, lin0), ("record", rec, rec0)):
                    if x.tobytes() != y.tobytes():
                        different.append((label, early, i, what, float(np.abs(x - y).max())))
    assert not different, different


def _moved_bias(w, product):
    """the gyro bias of every speed/bias block moved so that |db_g| Dt = product for the window's factors (all of one length)"""
    Dt = (int(w.imu_t1[0]) - int(w.imu_t0[0])) * 1e-9
    assert all(int(w.imu_t1[f]) - int(w.imu_t0[f]) == int(w.imu_t1[0]) - int(w.imu_t0[0]) for f in range(w.n_imu))
    d = np.array([2.0, -1.0, 2.0]) / 3.0 * product / Dt
    sb = np.array(w.sb, np.float64)
    sb[:, 3:6] += d
    return sb


@pytest.mark.parametrize("product,redone", [(0.9e-4, 0), (1.1e-4, 1)])
@pytest.mark.parametrize("label", ["default", "small"])
def test_inherited_reference_bias(ref, label, product, redone):
    """flag 1: only the reference bias travels.  The record is rebuilt AT that reference on first use (which the device counts, the
    reference's object did it in an earlier optimize()) and the factor evaluated at sb0 with the first-order correction — unless
    the bias moved past the threshold: then it is rebuilt at sb0 (ImuError.cpp:549)."""
    w = ref.case("unaligned_33")[0]
    sb_ref = _moved_bias(w, product)[np.asarray(w.imu_sb0)]
    w.imu_sb_ref, w.imu_sb_ref_valid = sb_ref, np.ones(w.n_imu, np.uint8)
    b = _batch([w], label, "early")
    b.begin()
    b.finish()
    (lin, rec), = _read(b, 1)
    b.close()
    failures = []
    for f in range(w.n_imu):
        fac = cases.Factor(ref.oracle, cases.factor_inputs(w, f), sb_ref=sb_ref[f], label=f"flag1 {product} f{f}")
        assert fac.redo_count == redone
        judge(f"flag1 {label} {product:.1e} f{f}", fac, lin[f], rec[f], failures, expect_redo=1)
        assert np.array_equal(fac.record["sb_ref"], w.sb[w.imu_sb0[f]] if redone else sb_ref[f])
    assert not failures, failures


@pytest.mark.parametrize("product,redone", [(0.9e-4, 0), (1.1e-4, 1)])
@pytest.mark.parametrize("label", ["default", "small"])
def test_travelling_record(ref, label, product, redone):
    """flag 2: the record itself travels (okvis_ba_fetch_imu_caches -> okvis_ba_window::imu_cache).  Inside the threshold it is used
    as it stands, to the bit, with the first-order correction; beyond it the factor is integrated again at the new bias."""
    (_, rec0), = first_evaluation(ref, "unaligned_33", "default", "early")
    w = ref.case("unaligned_33")[0]
    old = np.array(w.sb, np.float64)
    w.sb = _moved_bias(w, product)
    w.imu_cache, w.imu_sb_ref, w.imu_sb_ref_valid = rec0.copy(), old[np.asarray(w.imu_sb0)], np.full(w.n_imu, 2, np.uint8)
    b = _batch([w], label, "early")
    b.begin()
    b.finish()
    (lin, rec), = _read(b, 1)
    b.close()
    failures = []
    for f in range(w.n_imu):
        fac = cases.Factor(ref.oracle, cases.factor_inputs(w, f), sb_ref=old[w.imu_sb0[f]], label=f"flag2 {product} f{f}")
        assert fac.redo_count == redone
        judge(f"flag2 {label} {product:.1e} f{f}", fac, lin[f], rec[f], failures)
        if not redone:
            assert rec[f][:cases.RECORD_FLAGS].tobytes() == rec0[f][:cases.RECORD_FLAGS].tobytes(), f
    assert not failures, failures


@pytest.mark.parametrize("early", list(EARLY))
def test_early_record_made_stale_by_set_state(ref, early):
    """okvis_ba_set_state changes the bias between the upload (imu_pre_kernel integrated at the uploaded bias, valid == 3) and the
    first evaluation: the record must be the fresh one at the NEW bias, counted once — far inside the threshold, so that only the
    staleness check can have rebuilt it.  The same bits without the early record."""
    w = ref.case("unaligned_33")[0]
    sb = _moved_bias(w, 1e-6)
    sb[:, 6:9] += 1e-4
    b = _batch([w], "default", early)
    b.set_state(0, sb=sb)
    b.begin()
    b.finish()
    (lin, rec), = _read(b, 1)
    b.close()
    ref.runs["stale", early] = (lin, rec)
    failures = []
    for f in range(w.n_imu):
        fac = cases.Factor(ref.oracle, cases.factor_inputs(w, f, sb=sb), label=f"stale f{f}")
        judge(f"stale {early} f{f}", fac, lin[f], rec[f], failures, expect_redo=1, expect_ref=sb[w.imu_sb0[f]])
    assert not failures, failures
    if len([k for k in ref.runs if k[0] == "stale"]) == 2:
        a, c = ref.runs["stale", "early"], ref.runs["stale", "first_evaluation"]
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


@pytest.mark.parametrize("name", ["unaligned_33", "ragged"])
@pytest.mark.parametrize("label", list(ROUTES))
def test_record_after_iterations(ref, label, name):
    """three Gauss-Newton iterations (every evaluation is the accepted one; on `ride` they are imu_factor<1> + imu_factor<2>): the
    accepted buffer's H, g, r, cost and the record against the referee evaluated at the accepted state from a record built at the
    device's own IMU_SB_REF — which must lie inside the threshold of the accepted bias, or the device should have rebuilt it."""
    ws = ref.case(name)
    b = _batch(ws, label, "early", gauss_newton=1)
    summary = b.optimize(3)
    assert all(s["iterations"] == 3 for s in summary), summary
    got = _read(b, len(ws))
    state = [b.get_state(i) for i in range(len(ws))]
    sb_ref = [b.array("IMU_SB_REF", i).reshape(-1, 9) for i in range(len(ws))]
    b.close()
    failures = []
    for i, w in enumerate(ws):
        for f in range(w.n_imu):
            fac = cases.Factor(ref.oracle, cases.factor_inputs(w, f, pose=state[i][0], sb=state[i][1]), sb_ref=sb_ref[i][f],
                               label=f"after {label} {name} w{i} f{f}")
            assert fac.redo_count == 0, (label, name, i, f)
            d = cases.decode_record(got[i][1][f])
            judge(f"after3 {label} {name} w{i} f{f}", fac, got[i][0][f], got[i][1][f], failures, expect_redo=d["redo_count"],
                  expect_ref=sb_ref[i][f])
            assert d["redo_count"] >= 1
    assert not failures, failures
