"""The fp64 linearise kernels (the default precision) refereed entry by entry on every launch route.

linearize2_kernel<double, FUSE, SMALL, OCC, UB> as LIN2_FUSED, LIN2_FUSED_SMALL, LIN2_SMALL, LIN2_OCC3, LIN2_OCC4 (the piece path,
ba_linearize2.hpp) and linearize_kernel<EXT, double, FUSE> (the staged kernel, ba_linearize.hpp) are each reached here — the
expected launch_route() is restated from make_plan for the fp64 stage (lin64_cases.expected_route) and asserted, with the one
exception of the fp32 referee: LIN2_OCC3 and LIN2_OCC4 differ in tuning.lin2_occupancy alone — and the first linearisation of
every window is compared with the oracle built with real = long double:

  bound     deviation <= 4 x e_ref(A, scale) for the five arrays under two scales: entrywise (every entry against what it is a sum
            of in absolute values, built from the operands' magnitudes: tests/fp32_statement.py) and max |A|.  e_ref is the
            largest deviation of three correct fp64 CPU evaluations (the fp64 oracle, the numpy statement, the statement summing
            in reverse order) from the same referee over every window of tests/lin64_cases.py; measured on the CPU, never from a
            kernel.  tests/test_fp64_statement_host.py shows that seven wrong terms exceed the entrywise bound tenfold on every
            window they apply to, and that a left-out observation of the outlier window passes the earlier 1e-9 x max |A|.
  exact     the (landmark, block) pairs; every exact zero of the referee; landmark w untouched by optimize(10).
  end       optimize(10) against the fp64 oracle as tests/test_gpu_parity.py asks: cost within 1e-9, the same iteration,
            successful-step and termination numbers.
  pairs     the two routes of one kernel family give the same bits in all five arrays.
  phase A   the landmark back-substitution of the first iteration, isolated: from the GPU's own pre-step LM, LM_V, LM_B, PAIR_W,
            pairs and STEP the statement lm + delta_l in long double (lin64_cases.phase_a) must give the GPU's new landmarks within
            4 x e_ref entrywise, scale |lm| + |Vd^-1| (|b| + sum |W|^T |delta|); under LM damping with gauss_newton = 1 and under
            the default dogleg (Gauss-Newton point, mu = min_mu on the Jacobi-scaled diagonal), on all thirteen routes; one
            radius-limited dogleg run per kernel family (the explicit-step branch) against the extended oracle's landmarks.

Every comparison prints a line `FP64REF label case window array e_kernel e_ref ratio`.

Measured (CPU: e_ref; MI355X: the kernels; profiles/fp64_referee_notes.md has the tables per route and what was found):
  e_ref entrywise     OBS_RESIDUAL 1.88e-15   LM_V 9.26e-14   LM_B 7.27e-16   LM_HQ 2.07e-15   PAIR_W 1.00e-13   phase A 1.5e-14 .. 2.1e-14
  e_ref max-scaled    OBS_RESIDUAL 8.12e-15   LM_V 9.43e-14   LM_B 5.35e-14   LM_HQ 7.24e-16   PAIR_W 1.01e-13   (numpy's FMA: by machine)
  worst e_kernel / e_ref, entrywise / max-scaled, over all routes and windows (bound 4):
                      OBS_RESIDUAL 0.81 / 1.09   LM_V 0.64 / 0.61   LM_B 1.00 / 2.74   LM_HQ 1.20 / 0.94   PAIR_W 0.70 / 0.63
  optimize(10) against the fp64 oracle: cost within 2.9e-10 relative everywhere (bound 1e-9), the same bookkeeping.
  phase A: e_kernel 1.6e-16 ... 6.6e-15, at most 0.42 x e_ref (LM damping, one block per frame and camera); the radius-limited
  runs reproduce the extended oracle's landmarks to the bit.
The referee found one fault: PAIR_W of the fused piece-path kernels differed from the unfused ones' in the last bit of entries
[3][0] and [5][2] of the 6 x 3 blocks (182 of 2106 values on route_small, 170 of 1890 and 62 of 1152 on route_two; 3.3e-18 ...
4.0e-18 of max |W|): a b - c d of W = M^T Vp, which ba_linearize2.hpp spelled out in float and left to the compiler in double, and
which the two instantiations contracted differently (fused: fma(a, b, -(c d)), but fma(-c, d, a b) in [3][0]; unfused: the first
form, but both products rounded in [5][2]).  Spelled out now in one form for every double instantiation ([3][0] as the fused
kernels had it, [5][2] as the unfused ones; profiles/fp64_referee_notes.md, "Route pairs", says why this one): all five pairs
give the same bits.  No fault in phase A.
"""
import numpy as np
import pytest

from . import fp32_statement as stmt
from . import lin64_cases as cases
from . import schur_statement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle):
    r = cases.Referee(oracle)
    for line in r.table():
        print(line)
    return r


def _batch(ws, opt):
    from okvis_amd import solver
    return solver.WindowBatch(ws, options=opt)


def _route(b):
    r = b.launch_route()
    return {k: r[k] for k in ("fused", "piece_path", "split_small")}


def _r(fused, piece, split):
    return dict(fused=fused, piece_path=piece, split_small=split)


def _upload(ref, name, label, expect, opt):
    """the case's windows uploaded under opt; the route is the one make_plan names for fp64 (and `expect`, where the caller names it)"""
    ws = ref.case(name)
    derived = cases.expected_route(ws, opt)
    assert expect is None or derived == expect, (name, label, derived, expect)
    b = _batch(ws, opt)
    route = _route(b)
    assert route == derived, (name, label, route, derived)
    return ws, b, route


def first_linearisation(ref, name, label, expect=None, **options):
    """Upload the case's windows in fp64 mode, linearise once and check every window as the module docstring says (bound under both
    scales, pairs, exact zeros), then optimize(10): landmark w untouched, cost and bookkeeping as the fp64 oracle's.  Returns
    dict(route, arrays[window][name])."""
    ref.check_input_condition(name)
    ws, b, route = _upload(ref, name, label, expect, cases.options(name, debug_arrays=1, **options))
    b.begin()
    b.finish()
    got, failures = [], []
    for i, w in enumerate(ws):
        pg, po = b.pairs(i), ref.pairs[name][i]
        assert np.array_equal(pg[0], po[0]) and np.array_equal(pg[1], po[1]), (name, label, i)
        arrays = {a: b.array(a, i) for a in stmt.ARRAYS}
        for a in stmt.ARRAYS:
            want = ref.ref[name][i][a]
            assert np.isfinite(arrays[a]).all(), (name, label, i, a)
            assert np.all(arrays[a][want == 0.0] == 0.0), (name, label, i, a)
        e = ref.deviations(name, i, arrays)          # (asserts that entries nothing sums into equal the referee's)
        for a in stmt.ARRAYS:
            for k in cases.SCALES:
                e_ref = ref.e_ref[a][k]
                print(f"FP64REF {label} {name} w{i} {a} {k} e_kernel {e[a][k]:.3e} e_ref {e_ref:.3e} ratio {e[a][k] / e_ref:.2f}")
                if not e[a][k] <= ref.bound(a, k):
                    d = np.abs(arrays[a] - ref.ref[name][i][a]) / np.where(ref.scale[name][i][a] > 0, ref.scale[name][i][a], 1.0)
                    failures.append((name, label, i, a, k, e[a][k], ref.bound(a, k), "worst entry (entrywise)", int(np.argmax(d)),
                                     "entries beyond the entrywise bound", int((d > ref.bound(a, "entry")).sum()), "of", d.size))
        got.append(arrays)
    assert not failures, failures
    s = b.optimize(10)
    for i, (w, so) in enumerate(zip(ws, ref.optimized(name))):
        assert np.array_equal(b.get_state(i)[2][:, 3], np.asarray(w.lm)[:, 3]), (name, label, i)
        rel = abs(s[i]["final_cost"] - so["final_cost"]) / so["final_cost"]
        print(f"FP64REF {label} {name} w{i} optimize10 rel_cost {rel:.3e} iterations {s[i]['iterations']} oracle {so['iterations']}")
        assert rel <= 1e-9, (name, label, i, s[i], so)
        assert (s[i]["iterations"], s[i]["successful_steps"], s[i]["termination"]) == \
               (so["iterations"], so["successful_steps"], so["termination"]), (name, label, i, s[i], so)
    b.close()
    return dict(route=route, arrays=got)


SPLIT = dict(tuning_split_small_min=1)
UNFUSED_SPLIT = dict(tuning_split_small_min=1, tuning_fused_max_windows=-1)
# label: (case, options, expected route) — the thirteen labels of the fp32 referee; in fp64 the fused boundary lies at Dp <= 61
# (93 with free extrinsics), so the by-size label takes K = 11 (Dp = 66) and one block per frame and camera (Dp = 54) is fused
ROUTES = {
    "LIN2_FUSED_SMALL": ("route_small", {}, _r(1, 1, 0)),
    "LIN2_SMALL": ("route_small", dict(reserved0=4), _r(0, 1, 0)),
    "LIN2_FUSED": ("route_two", SPLIT, _r(1, 1, 1)),
    "LIN2_OCC4": ("route_two", UNFUSED_SPLIT, _r(0, 1, 1)),                                  # the 64-window benchmark's kernel
    "LIN2_OCC3": ("route_two", dict(UNFUSED_SPLIT, tuning_lin2_occupancy=3), _r(0, 1, 1)),
    "staged_fused": ("route_small", dict(reserved0=8), _r(1, 0, 0)),                         # linearize_kernel<false, double, true>
    "staged_unfused": ("route_small", dict(reserved0=8 | 4), _r(0, 0, 0)),                   # <false, double, false>
    "staged_unfused_two": ("route_two", dict(reserved0=8 | 4), _r(0, 0, 0)),
    "staged_unfused_by_size": ("boundary64_11_fixed", dict(reserved0=8), _r(0, 0, 0)),       # Dp = 66 > 61: no fused mode in fp64
    "staged_ext_fused": ("route_ext_shared", {}, _r(1, 0, 0)),                               # <true, double, true>
    "staged_ext_unfused": ("route_ext_shared", dict(reserved0=4), _r(0, 0, 0)),              # <true, double, false>
    "staged_ext_perframe": ("route_ext_perframe", {}, _r(1, 0, 0)),                          # Dp = 54 <= 93: fused in fp64
    "staged_ext_perframe_unfused": ("route_ext_perframe", dict(reserved0=4), _r(0, 0, 0)),
}


@pytest.mark.parametrize("label", list(ROUTES))
def test_route(ref, label):
    name, options, expect = ROUTES[label]
    first_linearisation(ref, name, label, expect, **options)


@pytest.mark.parametrize("name,fused,piece", [("boundary64_10_fixed", 1, 1), ("boundary64_11_fixed", 0, 1), ("boundary64_13_shared", 1, 0),
                                              ("boundary64_14_shared", 0, 0), ("boundary_5_fixed", 1, 1), ("boundary_6_fixed", 1, 1),
                                              ("boundary_5_shared", 1, 0), ("boundary_6_shared", 1, 0)])
def test_fused_mode_boundary(ref, name, fused, piece):
    """2 * SCHUR_LM_BATCH * 3 * Dp <= stage: Dp = 60 | 66 and 90 | 96 lie on the two sides in fp64; the fp32 boundary's windows are all fused"""
    first_linearisation(ref, name, "boundary_fp64", _r(fused, piece, 0))


@pytest.mark.parametrize("name", ["model_none", "model_radtan", "model_equidistant", "model_radtan8", "edge_unobserved", "edge_too_close",
                                  "edge_negative_w", "edge_radtan8_undefined", "edge_equidistant_on_axis", "outliers"])
@pytest.mark.parametrize("staged", [0, 1])
def test_models_edges_and_outliers(ref, name, staged):
    first_linearisation(ref, name, f"{'staged' if staged else 'piece'}_fused", _r(1, 1 - staged, 0), reserved0=8 * staged)


@pytest.mark.parametrize("name,piece", [("piece_monocular", 1), ("piece_odd_counts", 1), ("piece_three_and_four", 1),
                                        ("piece_beyond_128", 0), ("piece_beyond_64_poses", 1)])
def test_piece_enumeration(ref, name, piece):
    """the piece path, the fall-back to the staged kernel (a landmark of more than 128 pieces) and the split kernels"""
    first_linearisation(ref, name, "piece_shapes", _r(1, piece, 0))
    if name in ("piece_monocular", "piece_odd_counts", "piece_beyond_64_poses"):
        first_linearisation(ref, name, "piece_shapes_OCC4", _r(0, piece, 1), **UNFUSED_SPLIT)


@pytest.mark.parametrize("label,options,expect", [("ragged_FUSED_SMALL", {}, _r(1, 1, 0)), ("ragged_OCC4", UNFUSED_SPLIT, _r(0, 1, 1)),
                                                  ("ragged_staged_fused", dict(reserved0=8), _r(1, 0, 0))])
def test_ragged_batch(ref, label, options, expect):
    first_linearisation(ref, "ragged_batch", label, expect, **options)


def test_group_edge_cases_have_their_edges(ref):
    cases.check_group_edges(ref.windows)


@pytest.mark.parametrize("name,label,options", [
    ("group_obs_256", "staged_fused", {}), ("group_obs_256", "staged_unfused", dict(reserved0=8 | 4)),
    ("group_pieces_128", "LIN2_FUSED_SMALL", {}), ("group_pieces_128", "LIN2_OCC4", UNFUSED_SPLIT),
    ("group_lm_16", "LIN2_FUSED_SMALL", {}), ("group_lm_32", "LIN2_FUSED_SMALL", {}), ("group_lm_64", "LIN2_FUSED_SMALL", {}),
    ("group_lm_64", "LIN2_OCC4", UNFUSED_SPLIT), ("group_lm_64", "staged_fused", dict(reserved0=8)),
    ("group_work", "LIN2_FUSED_SMALL", {}), ("group_work", "staged_unfused", dict(reserved0=8 | 4))])
def test_group_edges(ref, name, label, options):
    """a group closed by exactly 256 observations, by exactly 128 pieces, by the landmark cap (16, 32, 64) and by the work cap"""
    first_linearisation(ref, name, f"group_{label}", None, **options)


@pytest.mark.parametrize("fused,unfused", [("LIN2_FUSED_SMALL", "LIN2_SMALL"), ("LIN2_FUSED", "LIN2_OCC4"), ("LIN2_FUSED", "LIN2_OCC3"),
                                           ("staged_fused", "staged_unfused"), ("staged_ext_fused", "staged_ext_unfused")])
def test_fused_and_unfused_routes_agree(ref, fused, unfused):
    """The two routes of one kernel family evaluate the observations with the same code: the five arrays are bit-identical"""
    name, opt_f, exp_f = ROUTES[fused]
    name_u, opt_u, exp_u = ROUTES[unfused]
    assert name == name_u
    a = first_linearisation(ref, name, fused, exp_f, **opt_f)
    c = first_linearisation(ref, name, unfused, exp_u, **opt_u)
    differ = []
    for i in range(len(a["arrays"])):
        for arr in stmt.ARRAYS:
            x, y = a["arrays"][i][arr], c["arrays"][i][arr]
            if not np.array_equal(x, y):
                where = sorted(set(int(k) % 18 for k in np.flatnonzero(x != y))) if arr == "PAIR_W" else []
                differ.append((i, arr, int((x != y).sum()), x.size, stmt.deviation(x, y), "entries of the 6 x 3 block", where))
    print(f"FP64REF pair {fused}/{unfused} {name} arrays that differ (window, array, entries, of, max relative): {differ}")
    assert not differ, (fused, unfused, differ)


def _first_iteration(ref, name, label, expect, opt):
    """begin, finish: the pre-step arrays; begin, iterate(1), finish: STEP, the summary and the new landmarks — per window"""
    ws, b, _ = _upload(ref, name, label, expect, opt)
    b.begin()
    b.finish()
    pre = [dict({a: b.array(a, i) for a in ("LM_V", "LM_B", "PAIR_W")}, LM=b.get_state(i)[2], pairs=b.pairs(i)) for i in range(len(ws))]
    b.begin()
    b.iterate(1)
    b.synchronize()
    step = [b.array("STEP", i) for i in range(len(ws))]
    summary = b.finish()
    new = [b.get_state(i)[2] for i in range(len(ws))]
    b.close()
    return ws, pre, step, summary, new


@pytest.mark.parametrize("kind", ["lm", "dl"])
@pytest.mark.parametrize("label", list(ROUTES))
def test_phase_a(ref, label, kind):
    """The back-substitution alone: the statement in long double on the GPU's own arrays and step gives the GPU's new landmarks"""
    name, options, expect = ROUTES[label]
    opt = cases.phase_a_options(kind, debug_arrays=1, fp32_linearize=0, **options)
    ws, pre, step, summary, new = _first_iteration(ref, name, f"phaseA_{kind}_{label}", expect, opt)
    failures = []
    for i, w in enumerate(ws):
        s = summary[i]
        assert s["iterations"] == 1 and s["successful_steps"] == 1, (label, kind, i, s)
        if kind == "dl":     # the Gauss-Newton point lies inside the trust region: an accepted step ON the boundary would leave
            # 3 x the radius behind (or the radius itself, at a middling step quality; the statement below then tells)
            assert s["final_radius"] < 3.0 * opt.initial_radius, (label, i, s)
        assert np.array_equal(pre[i]["LM"], np.asarray(w.lm, np.float64).reshape(-1, 4)), (label, i)
        lam, Dl2 = cases.phase_a_damping(kind, pre[i]["LM_V"])
        want, a = cases.phase_a(pre[i]["LM"], pre[i]["LM_V"], pre[i]["LM_B"], pre[i]["PAIR_W"], *pre[i]["pairs"],
                                schur_statement.pose_offsets(w), step[i], lam, Dl2, dtype=np.longdouble)
        assert np.array_equal(new[i][:, 3], pre[i]["LM"][:, 3]), (label, kind, i)
        e = cases.phase_a_deviation(new[i][:, :3], want, a)
        moved = float(np.abs(new[i][:, :3] - pre[i]["LM"][:, :3]).max())
        print(f"FP64REF phaseA_{kind}_{label} {name} w{i} LM e_kernel {e:.3e} e_ref {ref.e_ref_phase_a:.3e} ratio {e / ref.e_ref_phase_a:.2f} "
              f"(largest landmark step {moved:.3e})")
        assert moved > 1e-6, (label, kind, i)
        if not e <= cases.BOUND_FACTOR * ref.e_ref_phase_a:
            d = np.abs(new[i][:, :3] - np.asarray(want, np.float64)) / a
            failures.append((label, kind, name, i, e, cases.BOUND_FACTOR * ref.e_ref_phase_a, "worst landmark", int(np.argmax(d.max(axis=1)))))
    assert not failures, failures


@pytest.mark.parametrize("label", ["LIN2_FUSED_SMALL", "staged_fused"])
def test_phase_a_radius_limited_dogleg(ref, label):
    """initial_radius = 1: the Gauss-Newton point lies outside, the step is the explicit -cA xv + beta dGN (its scalars stay on the
    device).  The landmark steps of the first iteration against the extended oracle's, relative to the largest, within 4 x the fp64
    oracle's own deviation from the extended oracle on this window."""
    name, options, expect = ROUTES[label]
    opt = cases.phase_a_options("dl", debug_arrays=1, fp32_linearize=0, initial_radius=1.0, **options)
    ws, pre, step, summary, new = _first_iteration(ref, name, f"phaseA_radius_{label}", expect, opt)
    for i, w in enumerate(ws):
        x, o = ref.oracle.OracleWindow(w, extended=True), ref.oracle.OracleWindow(w)
        sx, so = x.optimize(1, opt), o.optimize(1, opt)
        assert summary[i]["successful_steps"] == sx["successful_steps"] == so["successful_steps"] == 1, (summary[i], sx, so)
        lm0 = np.asarray(w.lm, np.float64).reshape(-1, 4)[:, :3]
        dx, do, dg = x.get_state()[2][:, :3] - lm0, o.get_state()[2][:, :3] - lm0, new[i][:, :3] - lm0
        # not the Gauss-Newton point: the statement of the plain back-substitution must NOT reproduce these landmarks
        lam, Dl2 = cases.phase_a_damping("dl", pre[i]["LM_V"])
        gn, _ = cases.phase_a(pre[i]["LM"], pre[i]["LM_V"], pre[i]["LM_B"], pre[i]["PAIR_W"], *pre[i]["pairs"],
                              schur_statement.pose_offsets(w), step[i], lam, Dl2)
        assert np.abs(gn - new[i][:, :3]).max() > 1e-3 * np.abs(dg).max(), "the run took the Gauss-Newton point"
        e_oracle = float(np.abs(do - dx).max() / np.abs(dx).max())
        e = float(np.abs(dg - dx).max() / np.abs(dx).max())
        print(f"FP64REF phaseA_radius_{label} {name} w{i} LM_STEP e_kernel {e:.3e} e_ref {e_oracle:.3e} ratio {e / e_oracle:.2f}")
        assert e <= cases.BOUND_FACTOR * e_oracle, (label, i, e, e_oracle)
