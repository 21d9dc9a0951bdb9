"""The landmark Schur kernels refereed entry by entry on every launch route.

make_plan (capi_launch.inc) can name six instantiations: schur_kernel (fp64 FMA; free extrinsics, pose parts beyond 63 rows,
OKVIS_BA_TUNE_SCHUR_VALU), schur_mfma_kernel<3> (matrix core, ring loop), schur_mfma_kernel<9> (matrix core, pose parts of
several 96-row tiles, OKVIS_BA_TUNE_SCHUR_MFMA_LARGE only), schur_ride_kernel<3>, and the serial variants of the two small-tile
kernels.  Each is reached here with its route asserted (launch_route(): fused == 0, schur_kernel, small_rides,
decision_free_schur), and the damped reduced system of the first iteration is compared with the long-double oracle:

  bound   deviation(X, ref) = max |X - ref| / a entrywise, a = what the entry is a sum of, in absolute values:
          |U_ij| + lambda Dp2_i delta_ij + sum_l (|W_l| |Vd_l^-1| |W_l|^T)_ij, unweighted (tests/schur_statement.py; weighting a
          landmark's term with cond(Vd_l) changed no e_ref and shrank what a wrong reduction shows a thousandfold).  The kernel
          must stay within 4 x e_ref(A), e_ref = the larger deviation of the fp64 oracle and of an independent numpy statement
          from the same referee over every window of tests/schur_cases.py — measured on the CPU, never from the kernels — over
          three sets of entries, each with its own e_ref:
            whole          the whole array.  Its e_ref (1.2e-6) is NOT about the reduction: it comes from pose x speed/bias entries
                           of the IMU factors' J^T J that nearly cancel, which no Schur kernel writes.
            pose_part      the rows and columns a Schur kernel writes (e_ref 1.5e-8: the IMU factors' pose x pose blocks).
            landmark_only  the entries of the pose part with U_ij = 0, where S_ij is the kernel's own sum and nothing else, against
                           the statement in long double on the GPU's OWN LM_V, LM_B, PAIR_W (e_ref 2.4e-14: fp64 against long
                           double on identical inputs).  This is the check that isolates the Schur kernel.
          tests/test_schur_statement_host.py shows that a left-out landmark, pair or V^-1 b row, omitted landmark damping or a
          transposed block exceed the first two bounds tenfold (at least 11.9 x and 76 x the bound on every window), a left-out
          landmark and the omitted damping the third by 6e8.
  exact   the (landmark, block) pairs; entries nothing sums into are exact zeros; the pose part of S is symmetric to the bit.
  alone   the statement in long double on the GPU's own landmark arrays and the referee's HPP, GRADIENT, damping: within the same
          bounds as against the referee.
  step    STEP against the referee's, relative to max |step|, within 4 x the fp64 oracle's own deviation on that window.

RESULTS (MI355X, worst e_kernel / e_ref of every route over its cases and modes; bound 4; per case: profiles/schur_referee_notes.md)
  route (schur_kernel, rides)            runs  S whole  S pose  S landmark-only  rhs    STEP
  VALU_ext       schur_kernel (1)           3    0.00    0.00       0.02         0.00   1.08
  VALU_forced    schur_kernel (1)          16    0.06    0.12       0.32         0.46   1.61
  VALU_large     schur_kernel (1)        8+2    3.21    0.59       0.54         1.00   0.89
  MFMA3          schur_mfma_kernel<3> (2)  25    0.06    0.12       0.32         0.46   1.61
  MFMA9          schur_mfma_kernel<9> (3)   8    3.21    0.59       0.54         1.00   0.89
  RIDE3          schur_ride_kernel<3> (2, 1) 18  0.06    0.12       0.32         0.42   0.88
  SERIAL3        both serial variants (4)  25    0.06    0.12       0.32         0.46   1.61
  (3.21: window k33_l30, 0.59 in its pose part — an entry of the speed/bias rows, the same figure on both routes, outside either
   kernel's reach.)
  schur_mfma_kernel<9> and schur_kernel on the same upload: 6e-17 ... 9e-17 apart in the pose part (Dp = 66, 102).
  Riding and plain launches: the same bits.  No kernel fault found.  One host-side fault found and fixed: okvis_ba_create allowed
  schur_mfma_kernel<9> 61 568 bytes of dynamic LDS, make_plan asks 62 720 for pose parts of 66 - 78 rows (capi_launch.inc).
"""
import numpy as np
import pytest

from okvis_amd.window import TUNE_SCHUR_MFMA_LARGE, TUNE_SCHUR_SERIAL_BATCHES, TUNE_SCHUR_VALU

from . import schur_cases as cases
from . import schur_statement as stmt

pytestmark = pytest.mark.gpu

SEPARATE = dict(reserved0=4)          # keep the Schur launch where a small batch would fuse
RIDE = dict(reserved0=4, tuning_split_small_min=1)


@pytest.fixture(scope="module")
def ref(oracle):
    assert np.finfo(np.longdouble).eps < 2e-19, "the isolating statement needs an extended long double"
    r = cases.Referee(oracle)
    r.oracle = oracle
    for a in cases.ARRAYS:
        print(f"SCHURREF e_ref {a} whole {r.e_ref[a][0]:.3e} pose_part {r.e_ref[a][1]:.3e}")
    print(f"SCHURREF e_ref REDUCED_S landmark_only {r.e_ref_landmark_only:.3e}")
    return r


def _batch(ws, opt):
    from okvis_amd import solver
    return solver.WindowBatch(ws, options=opt)


def first_reduction(ref, name, mode, label, expect, **options):
    """Upload the case under the mode and options, assert the route, linearise (LM_V, LM_B, PAIR_W, pairs), run one iteration
    (REDUCED_S, REDUCED_RHS, STEP) and check every window as the module docstring says.  Returns the arrays per window."""
    ws = ref.case(name)
    b = _batch(ws, ref.options(name, mode, debug_arrays=1, **options))
    route = b.launch_route()
    assert route["fused"] == 0 and {k: route[k] for k in expect} == expect, (label, name, mode, route, expect)
    b.begin()
    b.finish()
    lin = [{a: b.array(a, i) for a in ("LM_V", "LM_B", "PAIR_W")} for i in range(len(ws))]
    pairs = [b.pairs(i) for i in range(len(ws))]
    b.begin()
    b.iterate(1)
    b.synchronize()
    got = [{a: b.array(a, i) for a in cases.ARRAYS + ("STEP",)} for i in range(len(ws))]
    b.close()
    failures = []
    for i, s in enumerate(ref.of(name, mode)):
        assert np.array_equal(pairs[i][0], s.pairs[0]) and np.array_equal(pairs[i][1], s.pairs[1]), (label, name, i)
        g = got[i]
        g["REDUCED_S"] = g["REDUCED_S"].reshape(s.D, s.D)
        alone = dict(zip(cases.ARRAYS, s.statement(lin[i], np.longdouble, pose_part=s.ref)))
        for a in cases.ARRAYS:
            assert np.isfinite(g[a]).all(), (label, name, i, a)
            for pose_only, part in ((False, "whole"), (True, "pose_part")):
                e = s.deviation(a, g[a], pose_only)                      # (asserts the exact zeros)
                e_alone = s.deviation(a, g[a], pose_only, ref=alone[a])
                e_ref = ref.e_ref[a][int(pose_only)]
                print(f"SCHURREF {label} {name} {mode} w{i} {a} {part} e_kernel {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref:.2f} "
                      f"alone {e_alone:.3e} ratio {e_alone / e_ref:.2f}")
                for what, v in (("referee", e), ("alone", e_alone)):
                    if not v <= ref.bound(a, pose_only):
                        ev, k = stmt.worst_entry(g[a], s.ref[a] if what == "referee" else np.asarray(alone[a], np.float64), s.a[a])
                        failures.append((label, name, mode, i, a, part, what, v, ref.bound(a, pose_only), "worst entry of the whole array",
                                         divmod(k, s.D) if a == "REDUCED_S" else k, ev))
        S = g["REDUCED_S"]
        e = s.deviation_landmark_only(S, alone["REDUCED_S"])
        print(f"SCHURREF {label} {name} {mode} w{i} REDUCED_S landmark_only e_kernel {e:.3e} e_ref {ref.e_ref_landmark_only:.3e} "
              f"ratio {e / ref.e_ref_landmark_only:.2f}")
        if not e <= cases.BOUND_FACTOR * ref.e_ref_landmark_only:
            d = np.where(s.landmark_only, np.abs(S - np.asarray(alone["REDUCED_S"], np.float64)) / np.where(s.landmark_only, s.a["REDUCED_S"], 1.0), 0.0)
            failures.append((label, name, mode, i, "REDUCED_S landmark-only", e, cases.BOUND_FACTOR * ref.e_ref_landmark_only,
                             "worst entry", divmod(int(np.argmax(d)), s.D), "entries beyond the bound", int((d > cases.BOUND_FACTOR * ref.e_ref_landmark_only).sum())))
        if not np.array_equal(S[:s.Dp, :s.Dp], S[:s.Dp, :s.Dp].T):
            failures.append((label, name, mode, i, "the pose part of S is not symmetric to the bit", float(np.abs(S - S.T)[:s.Dp, :s.Dp].max())))
        if not np.all(np.abs(S - S.T) <= ref.bound("REDUCED_S") * s.a["REDUCED_S"]):
            failures.append((label, name, mode, i, "S is not symmetric"))
        e_step = float(np.abs(g["STEP"] - s.ref["STEP"]).max() / np.abs(s.ref["STEP"]).max())
        print(f"SCHURREF {label} {name} {mode} w{i} STEP e_kernel {e_step:.3e} e_oracle {s.e_step:.3e} ratio {e_step / s.e_step:.2f}")
        if not e_step <= cases.BOUND_FACTOR * s.e_step:
            failures.append((label, name, mode, i, "STEP", e_step, cases.BOUND_FACTOR * s.e_step))
    assert not failures, failures
    return got


def _x(schur, rides=0, free=None):
    e = dict(schur_kernel=schur, small_rides=rides)
    if free is not None:
        e["decision_free_schur"] = free
    return e


# label: (cases, modes, options, expected route)
ROUTES = {
    # schur_kernel: (a) free extrinsics, (b) forced where the matrix core would run, (c) pose parts beyond 63 rows by default
    "VALU_ext": (("ext_shared", "ext_perframe"), ("dogleg", "lm"), SEPARATE, _x(1)),
    "VALU_forced": (cases.SMALL, ("dogleg", "lm"), dict(SEPARATE, tuning_flags=TUNE_SCHUR_VALU), _x(1, free=0)),
    "VALU_forced_large": (("k11_l30", "k17_l30"), ("dogleg",), dict(tuning_flags=TUNE_SCHUR_VALU), _x(1, free=0)),
    "VALU_large": (cases.LARGE, ("dogleg", "lm"), {}, _x(1)),
    # schur_mfma_kernel<3>: the ring loop, decision-free (GN, DOGLEG) and deciding (LM)
    "MFMA3": (cases.SMALL, ("gn", "dogleg"), SEPARATE, _x(2, free=1)),
    "MFMA3_lm": (cases.SMALL, ("lm",), SEPARATE, _x(2, free=0)),
    # schur_mfma_kernel<9>
    "MFMA9": (cases.LARGE, ("dogleg", "lm"), dict(tuning_flags=TUNE_SCHUR_MFMA_LARGE), _x(3)),
    # schur_ride_kernel<3>
    "RIDE3": (cases.SMALL, ("gn", "dogleg"), RIDE, _x(2, rides=1, free=1)),
    # schur_mfma_kernel<3, true>, schur_ride_kernel<3, true>
    "SERIAL3": (cases.SMALL, ("dogleg", "lm"), dict(SEPARATE, tuning_flags=TUNE_SCHUR_SERIAL_BATCHES), _x(4)),
    "SERIAL3_ride": (cases.SMALL, ("dogleg",), dict(RIDE, tuning_flags=TUNE_SCHUR_SERIAL_BATCHES), _x(4, rides=1, free=1)),
}
PARAMS = [(label, name, mode) for label, (names, modes, _, _) in ROUTES.items() for name in names for mode in modes
          if cases.MODES[mode][1] in cases.CASES[name][1]]


@pytest.mark.parametrize("label,name,mode", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_route(ref, label, name, mode):
    _, _, options, expect = ROUTES[label]
    first_reduction(ref, name, mode, label, expect, **options)


@pytest.mark.parametrize("name", ["k11_l30", "k17_l30"])
def test_matrix_core_and_fma_kernels_on_the_same_large_window(ref, name):
    """schur_mfma_kernel<9> against schur_kernel forced on the identical upload: both within the bound of the referee (asserted by
    first_reduction), and no further from each other than two results within the bound can be"""
    m = first_reduction(ref, name, "dogleg", "pair_MFMA9", _x(3), tuning_flags=TUNE_SCHUR_MFMA_LARGE)
    v = first_reduction(ref, name, "dogleg", "pair_VALU", _x(1, free=0), tuning_flags=TUNE_SCHUR_VALU)
    s = ref.of(name, "dogleg")[0]
    for a in cases.ARRAYS:
        e = s.deviation(a, m[0][a], True, ref=v[0][a])
        print(f"SCHURREF pair MFMA9/VALU {name} {a} pose_part {e:.3e}")
        assert e <= 2 * ref.bound(a, True)


@pytest.mark.parametrize("name", ["k3_l5", "k10_l67_wide", "ragged"])
@pytest.mark.parametrize("serial", [0, 1])
def test_riding_factors_do_not_change_the_reduction(ref, name, serial):
    """schur_ride_kernel<3> and schur_mfma_kernel<3> run the same body: the same bits"""
    flags = TUNE_SCHUR_SERIAL_BATCHES if serial else 0
    k = 4 if serial else 2
    r = first_reduction(ref, name, "dogleg", "pair_ride", _x(k, rides=1), **dict(RIDE, tuning_flags=flags))
    p = first_reduction(ref, name, "dogleg", "pair_plain", _x(k, rides=0), **dict(SEPARATE, tuning_flags=flags))
    for i in range(len(r)):
        for a in cases.ARRAYS:
            assert np.array_equal(r[i][a], p[i][a]), (name, i, a, float(np.abs(r[i][a] - p[i][a]).max()))


@pytest.mark.parametrize("label,name,options,expect", [
    ("MFMA9", "k11_l30", dict(tuning_flags=TUNE_SCHUR_MFMA_LARGE), _x(3)),
    ("VALU_forced", "k10_l30", dict(SEPARATE, tuning_flags=TUNE_SCHUR_VALU), _x(1))])
def test_marginalisation_through_the_route(ref, label, name, options, expect):
    """okvis_ba_marginalize eliminates the landmarks through the same launch (marg mode: no damping, the preconditioned
    pseudo-inverse of V) — with one landmark of rank two (a single observation), at the tolerances of test_gpu_marginalization.py"""
    from .test_gpu_marginalization import check, flags
    w = ref.case(name)[0]
    first = np.flatnonzero(np.asarray(w.obs_lm) == 0)
    keep = np.setdiff1d(np.arange(w.n_obs), first[1:])
    for k in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_uv", "obs_sqrtw"):
        setattr(w, k, np.asarray(getattr(w, k))[keep])
    pm, sm = flags(w, [0], [0])
    b = _batch([w], ref.options(name, "dogleg", **options))
    route = b.launch_route()
    assert route["fused"] == 0 and {k: route[k] for k in expect} == expect, (label, route)
    g = b.marginalize(0, pm, sm)
    b.close()
    r = ref.oracle.OracleWindow(w).marginalize(pm, sm)
    assert np.all(np.isfinite(g["H"]))
    check(g, r)
