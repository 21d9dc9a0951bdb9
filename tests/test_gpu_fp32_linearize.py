"""The fp32 linearise kernels (okvis_ba_options.fp32_linearize = 1) refereed array by array on every launch route.

Nine kernel instantiations evaluate the observations through reproj_linearize_mixed<float> with LDS layouts sized by
sizeof(REAL): linearize2_kernel<float, ...> as LIN2_FUSED, LIN2_FUSED_SMALL, LIN2_SMALL, LIN2_OCC3, LIN2_OCC4 (the piece path,
ba_linearize2.hpp) and linearize_kernel<EXT, float, FUSE> (the staged kernel, ba_linearize.hpp).  Each is reached here — the
launch_route() assertions, not the options alone, say which one ran, with one exception: the route has no field that tells
LIN2_OCC3 from LIN2_OCC4 (both are piece path, unfused, split factors); between these two only tuning.lin2_occupancy decides
(make_plan, capi_launch.inc) — and its first linearisation is compared with the fp64 CPU oracle:

  bound     for array A, e_stmt(A) = max |A_stmt32 - A_oracle| / max |A_oracle| over every window of tests/fp32_cases.py, where
            A_stmt32 is an independent float32 evaluation in numpy (tests/fp32_statement.py).  The kernel must stay within
            4 x e_stmt(A): the 4 is for what two correct float32 evaluations may differ in (summation order, FMA contraction,
            device atan / log / sqrt against numpy's), it is not tuned against the kernel.  tests/test_fp32_statement_host.py shows
            on the CPU that a wrong Jacobian term exceeds this bound tenfold on these windows.
  exact     the (landmark, block) pairs; every exact zero of the oracle (fixed poses, invalid / undefined observations,
            unobserved landmarks); IMU_RESIDUAL bit-identical to the fp64 mode (the factors stay fp64); landmark w untouched by
            optimize().
  inputs    no observation within 1e-4 of the 0.2 m validity threshold, float32 takes the branches float64 takes (asserted
            from the statement's depths, no case is skipped).

Measured on MI355X (profiles/fp32_referee_notes.md has the table per route and the route pairs):
  e_stmt              OBS_RESIDUAL 4.49e-06   LM_V 4.49e-05   LM_B 3.40e-05   LM_HQ 4.20e-07   PAIR_W 5.08e-05
  worst e_kernel      OBS_RESIDUAL 4.32e-06   LM_V 3.66e-05   LM_B 3.15e-05   LM_HQ 3.45e-07   PAIR_W 4.41e-05
  e_kernel / e_stmt                0.96            0.81            0.93             0.82              0.87     (bound: 4)
  optimize(10) against the oracle: final cost within 6.5e-06 relative on every route (bound 1e-5), the same iteration counts.
The referee found one fault: W and the block records of the UB = 14 instantiation (LIN2_OCC4) differed from the other piece-path
kernels' in the last float bit, an FMA contraction the compiler chose differently; ba_linearize2.hpp now spells both out.  With
that the five arrays are bit-identical between the two routes of every pair, and the reduced systems of LIN2_FUSED / LIN2_OCC4 are
as close in fp32 mode as in fp64 mode (REDUCED_RHS 4.7e-16 against 9.0e-16; see test_fused_and_unfused_routes_agree).
LM_QUALITY in fp32 mode is out of scope: a ratio of extreme eigenvalues of H_l, ill-conditioned by construction."""
import numpy as np
import pytest

from okvis_amd.window import default_options, set_options

from . import fp32_cases as cases
from . import fp32_statement as stmt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle):
    r = cases.Referee(oracle)
    r.oracle = oracle
    for a in stmt.ARRAYS:
        print(f"FP32REF e_stmt {a} {r.e_stmt[a]:.3e}")
    return r


def _batch(ws, **kw):
    from okvis_amd import solver
    return solver.WindowBatch(ws, options=set_options(default_options(), **kw))


def _route(b):
    r = b.launch_route()
    return {k: r[k] for k in ("fused", "piece_path", "split_small")}


def first_linearisation(ref, name, expect, label, end_to_end=False, **options):
    """Upload the case's windows in fp32 mode, linearise once, compare the five arrays of every window with the oracle (bound and
    exact checks of the module docstring), then optimize(10): landmark w must be untouched, and with end_to_end (the routes, the
    boundaries, the ragged batch) cost and iteration count are compared with the oracle's optimize(10).  Returns
    dict(route, Dp, arrays[window][name])."""
    ref.check_input_condition(name)
    ws = ref.case(name)
    b = _batch(ws, fp32_linearize=1, debug_arrays=1, **options)
    route = _route(b)
    assert route == expect, (name, label, route, expect)
    b.begin()
    b.finish()
    got, failures = [], []
    for i, w in enumerate(ws):
        pg, po = b.pairs(i), ref.oracle_pairs[name][i]
        assert np.array_equal(pg[0], po[0]) and np.array_equal(pg[1], po[1]), (name, i)
        arrays = {a: b.array(a, i) for a in stmt.ARRAYS + ("IMU_RESIDUAL",)}
        for a in stmt.ARRAYS:
            want = ref.oracle_arrays[name][i][a]
            e = stmt.deviation(arrays[a], want)
            print(f"FP32REF {label} {name} w{i} {a} e_kernel {e:.3e} e_stmt {ref.e_stmt[a]:.3e} ratio {e / ref.e_stmt[a]:.2f}")
            assert np.all(arrays[a][want == 0.0] == 0.0), (name, label, i, a)
            if not e <= cases.BOUND_FACTOR * ref.e_stmt[a]:
                failures.append((name, label, i, a, e, ref.e_stmt[a]))
        got.append(arrays)
    assert not failures, failures
    # the IMU / prior factors stay fp64: the same bits as in fp64 mode on the same route options
    b64 = _batch(ref.case(name), fp32_linearize=0, debug_arrays=1, **options)
    b64.begin()
    b64.finish()
    for i in range(len(ws)):
        assert np.array_equal(got[i]["IMU_RESIDUAL"], b64.array("IMU_RESIDUAL", i)), (name, label, i)
    b64.close()
    Dp = [b.reduced_dim(i) - 9 * int((np.asarray(w.sb_fixed) == 0).sum()) for i, w in enumerate(ws)]
    s = b.optimize(10)
    for i, w in enumerate(ws):
        assert np.array_equal(b.get_state(i)[2][:, 3], np.asarray(w.lm)[:, 3]), (name, label, i)
        if end_to_end:     # the project's mixed-precision bound (tests/test_gpu_mixed_precision.py)
            so = ref.oracle.OracleWindow(w).optimize(10)
            rel = abs(s[i]["final_cost"] - so["final_cost"]) / so["final_cost"]
            print(f"FP32REF {label} {name} w{i} optimize10 rel_cost {rel:.3e} iterations {s[i]['iterations']} oracle {so['iterations']}")
            assert rel <= 1e-5, (name, label, i, s[i], so)
            assert abs(s[i]["iterations"] - so["iterations"]) <= 2, (name, label, i, s[i], so)
    b.close()
    return dict(route=route, Dp=Dp, arrays=got)


def _r(fused, piece, split):
    return dict(fused=fused, piece_path=piece, split_small=split)


SPLIT = dict(tuning_split_small_min=1)
UNFUSED_SPLIT = dict(tuning_split_small_min=1, tuning_fused_max_windows=-1)
# label: (case, options, expected route, kernel)
ROUTES = {
    "LIN2_FUSED_SMALL": ("route_small", {}, _r(1, 1, 0)),
    "LIN2_SMALL": ("route_small", dict(reserved0=4), _r(0, 1, 0)),
    "LIN2_FUSED": ("route_two", SPLIT, _r(1, 1, 1)),
    "LIN2_OCC4": ("route_two", UNFUSED_SPLIT, _r(0, 1, 1)),                                  # the 64-window benchmark's kernel
    "LIN2_OCC3": ("route_two", dict(UNFUSED_SPLIT, tuning_lin2_occupancy=3), _r(0, 1, 1)),
    "staged_fused": ("route_small", dict(reserved0=8), _r(1, 0, 0)),                         # linearize_kernel<false, float, true>
    "staged_unfused": ("route_small", dict(reserved0=8 | 4), _r(0, 0, 0)),                   # <false, float, false>
    "staged_unfused_two": ("route_two", dict(reserved0=8 | 4), _r(0, 0, 0)),
    "staged_unfused_by_size": ("boundary_6_fixed", dict(reserved0=8), _r(0, 0, 0)),          # Dp = 36 > 30: no fused mode in fp32
    "staged_ext_fused": ("route_ext_shared", {}, _r(1, 0, 0)),                               # <true, float, true>
    "staged_ext_unfused": ("route_ext_shared", dict(reserved0=4), _r(0, 0, 0)),              # <true, float, false>
    # one block per frame and camera: 9 free pose blocks, Dp = 54 > 46: not fused in fp32 whatever the options say
    "staged_ext_perframe": ("route_ext_perframe", {}, _r(0, 0, 0)),
    "staged_ext_perframe_unfused": ("route_ext_perframe", dict(reserved0=4), _r(0, 0, 0)),
}


@pytest.mark.parametrize("label", list(ROUTES))
def test_route(ref, label):
    name, options, expect = ROUTES[label]
    first_linearisation(ref, name, expect, label, end_to_end=True, **options)


@pytest.mark.parametrize("K,ext,Dp,fused32", [(5, "fixed", 30, 1), (6, "fixed", 36, 0), (5, "shared", 42, 1), (6, "shared", 48, 0)])
def test_fused_mode_boundary(ref, K, ext, Dp, fused32):
    """2 * SCHUR_LM_BATCH * 3 * Dp <= stage: Dp <= 30 in fp32 against 61 in fp64 (stride-23 stage), 46 against 93 with free
    extrinsics — where the code says the boundary is, the layout must put it, and both sides must linearise right"""
    name = f"boundary_{K}_{ext}"
    piece = 1 if ext == "fixed" else 0
    out = first_linearisation(ref, name, _r(fused32, piece, 0), f"boundary_fp32_{K}_{ext}", end_to_end=True)
    assert out["Dp"] == [Dp]
    b = _batch(ref.case(name), fp32_linearize=0)
    assert _route(b) == _r(1, piece, 0)
    b.close()


@pytest.mark.parametrize("name", ["model_none", "model_radtan", "model_equidistant", "model_radtan8", "edge_unobserved", "edge_too_close",
                                  "edge_negative_w", "edge_radtan8_undefined", "edge_equidistant_on_axis"])
@pytest.mark.parametrize("staged", [0, 1])
def test_models_and_edges(ref, name, staged):
    first_linearisation(ref, name, _r(1, 1 - staged, 0), f"{'staged' if staged else 'piece'}_fused", reserved0=8 * staged)


@pytest.mark.parametrize("name,piece,fused", [("piece_monocular", 1, 0), ("piece_odd_counts", 1, 0), ("piece_three_and_four", 1, 1),
                                              ("piece_beyond_128", 0, 0), ("piece_beyond_64_poses", 1, 0)])
def test_piece_enumeration(ref, name, piece, fused):
    """the piece and block records are float here, at other LDS offsets than in fp64: the shapes of tests/test_gpu_piece_path.py.
    (fused only up to five free pose blocks: Dp <= 30.)"""
    first_linearisation(ref, name, _r(fused, piece, 0), "piece_shapes")
    if name in ("piece_monocular", "piece_odd_counts", "piece_beyond_64_poses"):      # and through the split kernels
        first_linearisation(ref, name, _r(0, piece, 1), "piece_shapes_OCC4", **UNFUSED_SPLIT)


@pytest.mark.parametrize("label,options,expect", [("ragged_FUSED_SMALL", {}, _r(1, 1, 0)), ("ragged_OCC4", UNFUSED_SPLIT, _r(0, 1, 1)),
                                                  ("ragged_staged_fused", dict(reserved0=8), _r(1, 0, 0))])
def test_ragged_batch(ref, label, options, expect):
    """three windows of different K, L and model in one upload (3, 5 and 4 keyframes: Dp <= 30, the batch is fused where the options allow)"""
    first_linearisation(ref, "ragged_batch", expect, label, end_to_end=True, **options)


def _reduced(ws, fp32, options):
    b = _batch(ws, fp32_linearize=fp32, debug_arrays=1, **options)
    b.begin()
    b.iterate(1)
    out = [{a: b.array(a, i) for a in ("REDUCED_S", "REDUCED_RHS", "STEP")} for i in range(len(ws))]
    b.close()
    return out


@pytest.mark.parametrize("fused,unfused", [("LIN2_FUSED_SMALL", "LIN2_SMALL"), ("LIN2_FUSED", "LIN2_OCC4"), ("LIN2_FUSED", "LIN2_OCC3"),
                                           ("staged_fused", "staged_unfused"), ("staged_ext_fused", "staged_ext_unfused")])
def test_fused_and_unfused_routes_agree(ref, fused, unfused):
    """Downstream of the linearisation.  The two routes of one kernel family evaluate the observations with the same code: the five
    arrays are bit-identical between them in fp32 mode.  The reduction is fp64 in both modes, so the precision of the
    linearisation must not change how far the two routes' reduced systems drift apart: within 10 x the fp64 deviation of the same
    two routes on the same window (floor 1e-12 relative).

    Measured on MI355X, fp64 / fp32 deviation of REDUCED_RHS: LIN2_FUSED_SMALL / LIN2_SMALL 6.0e-16 / 1.3e-16, LIN2_FUSED / LIN2_OCC4
    and LIN2_FUSED / LIN2_OCC3 alike 9.0e-16 / 4.7e-16 (first window) and 7.3e-16 / 2.7e-16 (second), staged 3.6e-16 / 1.3e-16, staged
    with extrinsics 0 / 0.  REDUCED_S: fp32 deviation 0 in every pair (fp64 up to 8.4e-25).  STEP: all within 2.1e-11, fp32 no further
    apart than fp64 x 2 (LIN2_FUSED / LIN2_OCC4: 8.1e-12 / 3.9e-12 and 1.9e-11 / 2.1e-11).  LIN2_FUSED / LIN2_OCC4 was 9.0e-16 / 2.6e-10
    (REDUCED_S 8.4e-25 / 2.0e-19) while the two kernels still contracted the a b - c d entries of the block records differently
    (ba_linearize2.hpp spells them out now)."""
    name, opt_f, exp_f = ROUTES[fused]
    name_u, opt_u, exp_u = ROUTES[unfused]
    assert name == name_u
    a = first_linearisation(ref, name, exp_f, fused, **opt_f)
    c = first_linearisation(ref, name, exp_u, unfused, **opt_u)
    differ = []
    for i in range(len(a["arrays"])):
        for arr in stmt.ARRAYS:
            x, y = a["arrays"][i][arr], c["arrays"][i][arr]
            if not np.array_equal(x, y):
                differ.append((i, arr, int((x != y).sum()), x.size, stmt.deviation(x, y)))
    print(f"FP32REF pair {fused}/{unfused} {name} arrays that differ (window, array, entries, of, max relative): {differ}")
    assert not differ, (fused, unfused, differ)
    dev = {}
    for fp32 in (0, 1):
        rf, ru = _reduced(ref.case(name), fp32, opt_f), _reduced(ref.case(name), fp32, opt_u)
        dev[fp32] = [{k: stmt.deviation(rf[i][k], ru[i][k]) for k in rf[i]} for i in range(len(rf))]
    for i in range(len(dev[0])):
        for k in ("REDUCED_S", "REDUCED_RHS", "STEP"):
            print(f"FP32REF pair {fused}/{unfused} {name} w{i} {k} dev_fp64 {dev[0][i][k]:.3e} dev_fp32 {dev[1][i][k]:.3e}")
            assert dev[1][i][k] <= max(10.0 * dev[0][i][k], 1e-12), (fused, unfused, i, k, dev[0][i][k], dev[1][i][k])
