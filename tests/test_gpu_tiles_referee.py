"""GPU: the tiled multi-workgroup Cholesky of the reduced camera system (okvis_amd/csrc/ba_chol_tiles.hpp), the solver behind every
window with D > 174, refereed at its tile edges — stand-alone through okvis_ba_dense_solve on the cases of tests/tiles_cases.py, and
in the window (large_export_kernel -> chol_tiles_window_kernel -> solve_large_tail_kernel) on windows with D = 180, 192, 195, 240.

The rule (tests/tiles_statement.py, the LDS referee's): x of the kernel against the 50-digit Cholesky solution of the same fp64
system, by e = max|x - x_ref| / max|x_ref| and the Jacobi-scaled residual rho; per family of cases both must stay within
BOUND_FACTOR = 4 times what the family's fp64 peers reach over the family's cases (tiles_cases.FAMILY_REF: e of numpy.linalg.solve,
a LAPACK Cholesky solve and the tile data flow restated in numpy, rho of the two Cholesky peers; measured on the CPU by
tests/test_tiles_statement_host.py, which also asserts that every mutation of the emulation — the chain's last update of a
diagonal tile left out, a forward term L_jk y_k left out, L_(1,0) transposed, a far tile skipped on the way back, a tile index
one column off from tile row 3 on, zero padding — leaves that bound on every case it changes).  Every run also asks for info = 0
and for the same bits from a second call: the sums of each tile run in a fixed order, the multi-workgroup schedule must not show.

The rotated family (1e16 n n^T on rows 3 .. 5, inside the first 16-block of tile 0, and on rows 46 .. 48 across the first tile
edge) cannot referee structure: its peers scatter over e = 7e-6 .. 9e-4.  It referees the claim in ct_ldl_inv48 that the tile
elimination needs no compensated products.  Held: e to the family's bound; rho, case by case, to ROTATED_RHO_FACTOR = 5e4 times
the better of the case's peers — what a CPU peer with the kernel's arithmetic restated reaches (tiles_statement.
tiled_kernel_arithmetic, 39850 at rotated3-97) plus a quarter for LAPACK's last bits in the plain peers; rho to the family's bound where that CPU peer stays inside it (rows 46 .. 48),
recorded where it does not (rows 3 .. 5: tiles_cases.ROTATED_UNCOMPENSATED), as the LDS referee does for a comp_mask that leaves
the prior's block to the plain elimination.

In the window: one LM iteration with debug arrays, OKVIS_BA_ARR_STEP against the reference solve of the downloaded REDUCED_S /
REDUCED_RHS, the bound 4 x what the peers reach on that very system (e: the worst peer, rho: the worse of the two Cholesky peers);
one dogleg iteration the same way; four iterations with debug arrays off and on to the same bits (the export's clear-on-write leaves
exactly the matrix the next assembly expects); a batch [D = 180, D = 60, D = 240] in one launch against each window alone.

RESULTS (MI355X; runs = solves compared with the reference; worst kernel / family reference, bound 4; the per-case lines are in
profiles/tiles_referee_notes.md):
  family   runs   e / e_ref   rho / rho_ref   worst case (e | rho)
  dense      23     1.47         0.98         dense-288 | dense-97
  struct     15     1.73         1.27         reverse_arrow-193
  graded      3     0.05         1.43         graded-240        (e_ref is numpy's pivoted LU; against the Cholesky peers' 8.6e-16: 1.7)
  axis       12     1.57         1.75         axis3-240
  rotated     6     0.25         1.35 | 7397  rotated46-97 | rotated3-97 (rho: the three cases across the tile edge | the three inside one
                                              16-block, recorded, not asserted against rho_ref)
  rotated  rho / the better peer's rho, case by case (3-97, 46-97, 3-193, 46-193, 3-240, 46-240): 39850, 3.1, 12963, 0.3, 602, 2.9
           (bound 5e4; the CPU peer with the kernel's arithmetic: 39850, 1.8, 33614, 0.6, 602, 3.0); e / the better peer's e: 3.85, 6.57, 4.11,
           0.57, 0.06, 4.94
  window   LM, D = 180, 192, 195, 240      4     2.48     1.47     D = 180 | D = 240  (e: the worst peer, rho: the worse Cholesky peer,
  window   dogleg, D = 195                 1     1.19     0.57                         on the window's own system)
  Every run: info = 0 and the same bits from a second call.  Four iterations with debug arrays off and on: the same bits at all four D.
  The batch [180, 60, 240]: every window on the bits it ends on alone.  A pivot of -1 and of 0 at fifteen positions and one indefinite
  matrix with a positive diagonal: all reported, x finite and zero in the pivot's row.
Found: the guard of a pivot that is not positive replaced it by 1 and x overflowed (not a number at 12 of the 15 positions and for the
indefinite matrix; the window route discards x of a failed factorisation, okvis_ba_dense_solve handed it out) — ldl16_pivot<.., GUARD> now
leaves such a pivot out of the elimination.  No fault in the tile indices, the hand-overs, the window launch or the export's
clear-on-write: no size hung or faulted, no ratio above 4.  The uncompensated elimination of ct_ldl_inv48 leaves rho 76 to 7400 times the
family's reference behind a prior inside one 16-block, exactly what its arithmetic gives on the CPU, with e inside the peers' scatter:
recorded (the kernel's comment), not closed.
"""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib, solver, synthetic
from okvis_amd.window import STRATEGY_DOGLEG, STRATEGY_LM, TUNE_SCHUR_DECIDES, TUNE_SCHUR_VALU, default_options, set_options
from tests import tiles_cases as tc
from tests import tiles_statement as ts

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
ERR_ARG = -1


def solve(S, g):
    """(status, x, info) of okvis_ba_dense_solve"""
    n = S.shape[0]
    Sc, gc, x = np.ascontiguousarray(S, np.float64), np.ascontiguousarray(g, np.float64), np.zeros(n)
    info = C.c_int32(-1)
    rc = _lib.lib().okvis_ba_dense_solve(0, n, Sc.ctypes.data_as(_dp), gc.ctypes.data_as(_dp), x.ctypes.data_as(_dp), C.byref(info))
    if rc not in (0, ERR_ARG):      # a device error: nothing more is started on that device in this session
        pytest.exit(f"okvis_ba_dense_solve(n = {n}) returned {rc}", returncode=3)
    return rc, x, info.value


def _report(tag, name, mode, ek, rk, e_ref, rho_ref):
    print(f"  referee {tag:8s} {name:24s} {mode:5s} e {ek:.2e} ({ek / e_ref:5.2f} x e_ref)  rho {rk:.2e} ({rk / rho_ref:5.2f} x rho_ref)")


@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_case_against_the_reference(case):
    S, g = tc.system(case)
    xr = tc.reference_of(case)
    rc, x, info = solve(S, g)
    assert rc == 0 and info == 0, (rc, info)
    ek, rk = ts.e(x, xr), ts.rho(S, g, x)
    e_ref, rho_ref = tc.FAMILY_REF[case.family]
    _report(case.family, case.name, "tiles", ek, rk, e_ref, rho_ref)
    rc2, x2, info2 = solve(S, g)
    assert (rc2, info2) == (0, 0) and np.array_equal(x, x2)
    be, br = tc.bound(case.family)
    if case.family != "rotated":
        assert ek <= be and rk <= br, (ek / e_ref, rk / rho_ref)
        return
    # the uncompensated tile elimination behind the rotated prior: e within the family's bound; rho, case by case, within the factor
    # the CPU peer with the kernel's arithmetic reaches against the better plain peer, and within the family's bound where that CPU
    # peer is (the other cases: recorded)
    better_e, better_r = tc.better_peer(case)
    print(f"  referee rotated  {case.name:24s} tiles e / the better peer's {ek / better_e:.2f}, rho / the better peer's {rk / better_r:.1f} "
          f"(bound {tc.ROTATED_RHO_FACTOR:g}){'  rho beyond the family bound: recorded' if rk > br else ''}")
    assert ek <= be, ek / e_ref
    assert rk <= tc.ROTATED_RHO_FACTOR * better_r, rk / better_r
    assert rk <= br or case.name in tc.ROTATED_UNCOMPENSATED, rk / rho_ref


PIVOTS = {97: (0, 15, 16, 47, 48, 95, 96), 144: (0, 15, 16, 47, 48, 95, 96, 143)}      # (n = 97: 96 is n - 1, the padded tile's only row)


@pytest.mark.parametrize("n,where", [(n, w) for n, ws in PIVOTS.items() for w in ws])
def test_a_pivot_that_is_not_positive_is_reported(n, where):
    """a reported outcome of the guarded elimination (ldl16_pivot<.., GUARD>: the pivot is left out of the elimination, its row of
    Linv_j is zero and so is its x; the tile raises the failure flag), in every 16-panel of a tile, in the chain's first, a middle
    and the last tile, with and without padding"""
    S, g = tc.system(tc.BY_NAME[f"dense-{n}"])
    for value in (-1.0, 0.0):
        Sb = S.copy()
        Sb[where, where] = value
        rc, x, info = solve(Sb, g)
        assert rc == 0 and info != 0 and np.all(np.isfinite(x)) and x[where] == 0.0, (value, rc, info, x[where])


def test_an_indefinite_matrix_with_a_positive_diagonal_is_reported():
    """the pivot turns non-positive only behind the updates: an SPD matrix minus 2 lambda_min v v^T"""
    S, g = tc.system(tc.BY_NAME["dense-97"])
    lam, V = np.linalg.eigh(S)
    Sb = S - 2.0 * lam[0] * np.outer(V[:, 0], V[:, 0])
    Sb = 0.5 * (Sb + Sb.T)
    assert np.all(np.diag(Sb) > 0) and np.linalg.eigvalsh(Sb)[0] < -0.5 * lam[0]
    rc, x, info = solve(Sb, g)
    assert rc == 0 and info != 0 and np.all(np.isfinite(x)), (rc, info)


# ---- in the window: the export, the window launch (progress counter, several windows in blockIdx.y) and the tail around the same tasks
WINDOW_D = (180, 192, 195, 240)


def _window(D):
    if D == 180:        # twelve keyframes: nT = 4, padded
        w = synthetic.make_window(12, 30, 1.0, 512, frame_dt=0.1)
    elif D == 192:      # twelve keyframes and the two shared extrinsics: nT = 4, exact
        w = synthetic.make_window(12, 30, 1.0, 612, frame_dt=0.1, estimate_extrinsics="shared")
    elif D == 195:      # thirteen keyframes: nT = 5, padded
        w = synthetic.make_window(13, 30, 1.0, 513, frame_dt=0.1)
    elif D == 240:      # sixteen keyframes: nT = 5, exact
        w = synthetic.make_window(16, 30, 1.0, 516, frame_dt=0.1)
    else:               # four keyframes: solved in LDS
        w = synthetic.make_window(4, 30, 1.0, 504, frame_dt=0.1)
    assert w.reduced_dim() == D
    return w


def _opts(strategy=None, **kw):
    return set_options(default_options(strategy), **kw)


def _stop(err):
    """no call of these tests may fail: a backend error ends the session like a device error of the stand-alone entry"""
    pytest.exit(f"the window route returned an error: {err}", returncode=3)


def _step_against_the_reference(D, strategy, tag):
    w = _window(D)
    b = solver.WindowBatch([w], options=_opts(strategy, debug_arrays=1))
    try:
        assert b.launch_route()["solve_tiled"] == 1 and b.reduced_dim() == D
        b.begin()
        b.iterate(1)
        b.synchronize()
        step, S, rhs = b.array("STEP"), b.array("REDUCED_S").reshape(D, D), b.array("REDUCED_RHS")
        b.finish()
    except _lib.BackendError as err:
        _stop(err)
    finally:
        b.close()
    assert np.array_equal(S, S.T) and np.all(np.isfinite(step)) and np.any(step != 0.0)
    xr = ts.reference(S, rhs)
    peers = {n: (ts.e(x, xr), ts.rho(S, rhs, x)) for n, x in ts.peers(S, rhs).items()}
    e_ref, rho_ref = max(v[0] for v in peers.values()), max(peers[p][1] for p in ts.CHOLESKY_PEERS)
    ek, rk = ts.e(step, xr), ts.rho(S, rhs, step)
    print(f"  referee window   D {D} peers {({n: (float(f'{a:.2g}'), float(f'{r:.2g}')) for n, (a, r) in peers.items()})}")
    _report("window", f"window-{D}", tag, ek, rk, e_ref, rho_ref)
    assert ek <= ts.BOUND_FACTOR * e_ref and rk <= ts.BOUND_FACTOR * rho_ref, (ek / e_ref, rk / rho_ref)


@pytest.mark.parametrize("D", WINDOW_D)
def test_step_in_the_window_lm(D):
    _step_against_the_reference(D, STRATEGY_LM, "lm")


def test_step_in_the_window_dogleg():
    _step_against_the_reference(195, STRATEGY_DOGLEG, "dl")


def _optimised(ws, iters=4, want_route=False, **kw):
    """(summaries, states[, launch route]) of the batch after `iters` iterations"""
    b = solver.WindowBatch(list(ws), options=_opts(**kw))
    try:
        summary = b.optimize(iters)
        out = summary, [b.get_state(i) for i in range(len(ws))]
        return out + (b.launch_route(),) if want_route else out
    except _lib.BackendError as err:
        _stop(err)
    finally:
        b.close()


def _same_bits(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("D", WINDOW_D)
def test_export_leaves_the_matrix_the_next_assembly_expects(D):
    """without debug arrays large_export_kernel clears every entry of the HBM matrix it reads and the next assembly skips its
    clearing pass; with them the assembly clears.  Four iterations either way: the same bits"""
    w = _window(D)
    s0, x0 = _optimised([w], debug_arrays=0)
    s1, x1 = _optimised([w], debug_arrays=1)
    print(f"  referee window   D {D} four iterations: {s0[0]['iterations']} iterations, {s0[0]['successful_steps']} steps, cost {s0[0]['initial_cost']:.6e} -> {s0[0]['final_cost']:.6e}")
    assert s0[0]["successful_steps"] >= 2 and s0[0]["final_cost"] < s0[0]["initial_cost"]
    assert s0 == s1, (s0, s1)
    assert _same_bits(x0[0], x1[0])


def test_windows_of_different_tile_counts_and_an_lds_window_in_one_launch():
    """[D = 180 (nT = 4), D = 60 (solved in LDS), D = 240 (nT = 5)] in one batch: the tile grid is sized for nT = 5, the solve launch
    runs both instantiations side by side; every window ends on the bits it ends on alone.
    A batch takes its Schur route as a whole (make_plan): alone, the D = 60 window is fused (the linearise workgroups reduce their own
    groups, a chunk is a group) and in this batch it is not, which groups its partial sums differently — measured: final costs
    3.5e-13 apart under the default options, the two tiled windows to the bit.  Both runs therefore pin that route where the options
    can (no fusing, schur_kernel, the deciding Schur launch): what is left to differ is what this test is about"""
    pinned = dict(tuning_fused_max_windows=-1, tuning_flags=TUNE_SCHUR_DECIDES | TUNE_SCHUR_VALU)
    ws = [_window(180), _window(60), _window(240)]
    got, state, route = _optimised(ws, want_route=True, **pinned)
    assert (route["solve_tiled"], route["fused"], route["schur_kernel"]) == (1, 0, 1) and route["solve_mode"] != 0, route
    for i, w in enumerate(ws):
        want, alone, r1 = _optimised([w], want_route=True, **pinned)
        print(f"  referee batch    window {i} D {w.reduced_dim()}: cost {got[i]['final_cost']:.17g} in the batch, {want[0]['final_cost']:.17g} alone"
              f" (route alone: fused {r1['fused']}, schur_kernel {r1['schur_kernel']}, tiled {r1['solve_tiled']})")
        assert (r1["fused"], r1["schur_kernel"], r1["solve_tiled"]) == (0, 1, int(w.reduced_dim() > 174)), r1
        assert got[i] == want[0], (i, got[i], want[0])
        assert _same_bits(state[i], alone[0]), i
