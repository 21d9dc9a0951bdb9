"""The fp64 linearisation referee's yardstick and inputs checked on the CPU, no GPU needed (tests/lin64_cases.py,
tests/fp32_statement.py):

  * the e_ref table (printed): the deviation of three correct fp64 evaluations from the long-double oracle per array, entrywise and
    max-scaled, over every window of the cases;
  * condition 1: every entrywise e_ref stays below 1e3 x 2^-53.  The plain scale (sum |J|^T |J|, s (|z - c| + |f d|)) FAILS it:
    1.67e-13 for OBS_RESIDUAL (a point that projects next to the principal point: |f d| is small, its error is not), 1.62e-13
    for PAIR_W, 1.09e-13 for LM_B — Jacobian entries and the projected point are themselves cancelling sums.  So the scale is
    built from the operands' magnitudes, the way the Schur statement does (tests/fp32_statement.py, `scales`), and holds it;
  * condition 2: the four Jacobian mutations and the three sum mutations (last observation of a landmark left out, rho' for
    sqrt(rho'), LM_HQ robustified) exceed the entrywise bound 4 x e_ref tenfold on every window they apply to;
  * the argument for the entrywise scale: on the outlier window the left-out observation stays below the old 1e-9 x max |A|
    tolerance on all five arrays;
  * the long-double statement agrees with the long-double oracle to the rounding of the oracle's double output;
  * the new windows have the properties they are named after: the fused boundary of fp64 (Dp on both sides), the outliers'
    rho' and weights, the group edges (from the index lists), the depth margin.

Measured here (x86-64, numpy long double = x87 extended; numpy's products use the FMA of the CPU they run on, so the last digits
and phase A's figure move from one machine to the next — 1.5e-14 ... 2.1e-14):
  e_ref            OBS_RESIDUAL   LM_V        LM_B        LM_HQ       PAIR_W      phase A
  entrywise        1.88e-15       9.26e-14    7.27e-16    2.07e-15    1.00e-13    2.08e-14
  max-scaled       8.12e-15       9.43e-14    5.35e-14    7.24e-16    1.01e-13
  (LM_V, PAIR_W: the Cauchy weight 1 / (1 + |r|^2 / b^2) of a residual that is a difference of pixel coordinates of some hundred
   pixels; both scales see it alike.)
  mutations, deviation / entrywise bound, the smallest over the windows each applies to: see the printed lines
  (`-s`); the left-out observation of the outlier window: max-scaled 5e-15 ... 2e-10 on the five arrays (old tolerance 1e-9),
  entrywise 2e8 x the bound.
"""
import numpy as np
import pytest

from okvis_amd import solver

from . import fp32_statement as stmt
from . import lin64_cases as cases


@pytest.fixture(scope="module")
def referee(oracle):
    r = cases.Referee(oracle)
    for line in r.table():
        print(line)
    return r


def test_e_ref_table_and_entrywise_ceiling(referee):
    for name in cases.CASES:
        for i, e in enumerate(referee.e_case[name]):
            print(f"{name:26s} w{i} entrywise " + " ".join(f"{a} {e[a]['entry']:.2e}" for a in stmt.ARRAYS) + " | max " +
                  " ".join(f"{e[a]['max']:.2e}" for a in stmt.ARRAYS) +
                  f" | phase A lm {referee.e_phase_a_case[name, i, 'lm']:.2e} dl {referee.e_phase_a_case[name, i, 'dl']:.2e}")
    for line in referee.table():
        print(line)
    for a in stmt.ARRAYS:
        # not below a quarter of one rounding either: the three evaluations really are fp64
        assert 2.0 ** -55 < referee.e_ref[a]["entry"] < cases.ENTRYWISE_CEILING, (a, referee.e_ref[a])
        assert 2.0 ** -55 < referee.e_ref[a]["max"] < cases.ENTRYWISE_CEILING, (a, referee.e_ref[a])
    assert 2.0 ** -55 < referee.e_ref_phase_a < cases.ENTRYWISE_CEILING, referee.e_ref_phase_a


def test_input_condition_on_every_window(referee):
    for name in cases.CASES:
        referee.check_input_condition(name)
        for w in referee.windows[name]:
            assert w.n_obs <= 900, (name, w.n_obs)
    for name in cases.NEW_CASES:
        for w in referee.windows[name]:
            K = int((np.asarray(w.sb_fixed).size))
            assert 3 <= K <= 14 and 20 <= w.n_lm <= 60, (name, K, w.n_lm)


def test_long_double_statement_is_the_long_double_oracle(referee):
    """keep_dtype: the statement in numpy.longdouble, rounded once to double, against the oracle built with real = long double"""
    for name in ("route_small", "route_ext_shared", "model_equidistant", "model_radtan8", "outliers"):
        for i, w in enumerate(referee.windows[name]):
            s = stmt.window_arrays(w, np.longdouble, keep_dtype=True)
            for a in stmt.ARRAYS:
                assert s[a].dtype == np.longdouble
                e = stmt.deviation_entrywise(np.asarray(s[a], np.float64), referee.ref[name][i][a], referee.scale[name][i][a])
                print(f"{name} w{i} {a} long double statement - long double oracle, entrywise {e:.3e}")
                assert e <= 2.0 ** -52, (name, i, a, e)


def test_fused_boundary_of_fp64(referee):
    """Dp = 60 | 66 around 61 (fixed extrinsics) and 90 | 96 around 93 (free), D within the LDS solve on both sides: the stage decides"""
    for name, Dp, ext, fused in (("boundary64_10_fixed", 60, False, 1), ("boundary64_11_fixed", 66, False, 0),
                                 ("boundary64_13_shared", 90, True, 1), ("boundary64_14_shared", 96, True, 0)):
        w = referee.windows[name][0]
        c = solver.check_window(w, cases.options())
        assert c["Dp"] == Dp and c["D"] <= cases.MAX_D_LDS and Dp <= cases.TILE_DIM, (name, c)
        assert (2 * cases.SCHUR_LM_BATCH * 3 * Dp <= cases.STAGE_DOUBLES[ext]) == bool(fused), name
        r = cases.expected_route([w], cases.options())
        assert r == dict(fused=fused, piece_path=0 if ext else 1, split_small=0), (name, r)
    # the two numbers the layout names
    assert cases.STAGE_DOUBLES[False] // 96 == 61 and cases.STAGE_DOUBLES[True] // 96 == 93


def test_group_edges_from_the_index_lists(referee):
    cases.check_group_edges(referee.windows)


def test_outlier_window_has_its_outliers(referee):
    w = referee.windows["outliers"][0]
    s = referee.stmt64["outliers"][0]
    r = s["OBS_RESIDUAL"].reshape(-1, 2)
    n = np.linalg.norm(r, axis=1) / float(w.cauchy_b)
    rho1 = 1.0 / (1.0 + n * n)
    print("outliers: |r| / cauchy_b", n[w.outlier_obs], "rho'", rho1[w.outlier_obs])
    assert np.all((n[w.outlier_obs] >= 19.0) & (n[w.outlier_obs] <= 51.0)) and np.all(rho1[w.outlier_obs] <= 2.8e-3)
    typical = np.median(np.asarray(w.obs_sqrtw))
    assert np.all(np.asarray(w.obs_sqrtw)[w.light_obs] <= 0.011 * typical)
    assert s["valid"].all()
    far = np.flatnonzero(np.asarray(w.obs_lm) == w.far_lm)
    assert np.all(s["depth"][far] > 0.9 * cases.FAR_DEPTH) and far[-1] in w.outlier_obs and far[-1] in w.light_obs
    assert w.far_lm == stmt.drop_landmark(w)


# which windows a mutation applies to (the Jacobian mutations as in tests/test_fp32_statement_host.py; the sum mutations: every
# window with a Cauchy loss and the routes', and the outlier window)
SUM_CASES = ("route_small", "route_two", "route_ext_shared", "route_ext_perframe", "piece_odd_counts", "outliers", "group_obs_256",
             "group_pieces_128")
MUTATION_CASES = {"radtan_j00": ("route_small", "model_radtan"), "equi_dpoly": ("model_equidistant",),
                  "je_sign": ("route_ext_shared", "route_ext_perframe"), "jp_trans": ("route_small",),
                  "drop_last_obs": SUM_CASES, "rho_prime": SUM_CASES, "hq_robust": SUM_CASES}


@pytest.mark.parametrize("mutation", stmt.MUTATIONS + stmt.SUM_MUTATIONS)
def test_referee_notices_a_wrong_term_entrywise(referee, mutation):
    """On EVERY window the mutation applies to, some array deviates from the referee by 10 x (4 x e_ref) in the entrywise scale (and
    the four Jacobian mutations in the max scale too)."""
    assert set(MUTATION_CASES) == set(stmt.MUTATIONS + stmt.SUM_MUTATIONS)
    for name in MUTATION_CASES[mutation]:
        for i, w in enumerate(referee.windows[name]):
            assert float(w.cauchy_b) > 0
            m = stmt.window_arrays(w, np.float64, mutate=mutation)
            best = {k: 0.0 for k in cases.SCALES}
            for a in stmt.ARRAYS:
                scale = referee.scale[name][i][a]
                on = scale > 0
                e = {"entry": float((np.abs(m[a] - referee.ref[name][i][a])[on] / scale[on]).max()), "max": stmt.deviation(m[a], referee.ref[name][i][a])}
                for k in cases.SCALES:
                    ratio = e[k] / referee.bound(a, k)
                    print(f"{mutation:14s} {name:20s} w{i} {a:13s} {k:5s} deviation / bound = {ratio:9.3g}")
                    best[k] = max(best[k], ratio)
            assert best["entry"] >= cases.MUTATION_MARGIN, (mutation, name, i, best)
            if mutation in stmt.MUTATIONS:
                assert best["max"] >= cases.MUTATION_MARGIN, (mutation, name, i, best)


def test_old_tolerance_hides_a_left_out_observation_on_the_outlier_window(referee):
    """The argument for the entrywise scale: the far landmark's last observation — a gross outlier of a hundredth of the weight —
    left out of the sums stays below 1e-9 x max |A| on all five arrays (the check tests/test_gpu_parity.py had), against the fp64
    oracle as that test compares, and exceeds the entrywise bound by orders of magnitude."""
    w = referee.windows["outliers"][0]
    m = stmt.window_arrays(w, np.float64, mutate="drop_last_obs")
    worst_entry = 0.0
    for a in stmt.ARRAYS:
        old = stmt.deviation(m[a], referee.o64["outliers"][0][a])
        scale = referee.scale["outliers"][0][a]
        on = scale > 0
        entry = float((np.abs(m[a] - referee.ref["outliers"][0][a])[on] / scale[on]).max()) / referee.bound(a, "entry")
        print(f"drop_last_obs outliers {a:13s} max-scaled deviation {old:.3e} (old tolerance 1e-9)  entrywise deviation / bound {entry:.3g}")
        assert old < cases.OLD_TOLERANCE, (a, old)
        worst_entry = max(worst_entry, entry)
    assert worst_entry >= 1.0e3 * cases.MUTATION_MARGIN, worst_entry
