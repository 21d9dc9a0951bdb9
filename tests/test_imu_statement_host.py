"""The CPU half of the IMU referee (tests/imu_cases.py, tests/imu_statement.py; the GPU half: tests/test_gpu_imu_referee.py).

  * the two long-double evaluations — the oracle's sources built with real = long double and the numpy statement written from
    ImuError.cpp — agree better than the fp64 oracle agrees with either: the referee is not one restatement's opinion;
  * the oracle equals the compiled reference on every edge stream of the cases, at the tolerances of
    tests/test_oracle_vs_ref.py::test_imu_fixtures_are_reference_outputs (skipped where oracle/_ref cannot be had);
  * the referee would notice: seven deliberately wrong variants of the statement each leave the bound of the named case by more
    than MUTATION_MARGIN (measured: 2e9 x the bound and more; `inf`: an entry nothing sums into is not zero, or the covariance is
    no longer positive definite)."""
import numpy as np
import pytest

from . import imu_cases as cases
from . import imu_statement as stmt
from . import ref_lib as R


@pytest.fixture(scope="module")
def ref(oracle):
    assert np.finfo(np.longdouble).eps < 2e-19, "the referee needs an extended long double"
    return cases.Referee(oracle)


def test_record_layout_and_case_list(ref):
    assert set(cases.SINGLE) | {"ragged"} == set(cases.CASES)
    assert [len(w.imu_t0) for w in ref.windows["ragged"]] == [2, 4]
    steps = {name: [fac.n_steps for fs in ref.factors[name] for fac in fs] for name in cases.CASES}
    for name in cases.SINGLE:
        assert steps[name] == [cases.shape(name)[1]] * 2, (name, steps[name])
    assert steps["ragged"] == [20, 45, 33, 7, 64, 90]
    assert steps["long"][0] > 400 and all(w.imu_s_count.max() <= 500 for ws in ref.windows.values() for w in ws)
    # the shapes are what their names say
    w = ref.windows["lead300"][0]
    b, c = int(w.imu_s_begin[0]), int(w.imu_s_count[0])
    assert (np.asarray(w.imu_s_t)[b:b + c] <= w.imu_t0[0]).sum() == 301
    w = ref.windows["tail"][0]
    assert (np.asarray(w.imu_s_t)[:int(w.imu_s_count[0])] > w.imu_t1[0]).sum() == 21
    w = ref.windows["dup_run"][0]
    t = np.asarray(w.imu_s_t)[:int(w.imu_s_count[0])]
    assert np.bincount(np.unique(t, return_inverse=True)[1]).max() == 10
    w = ref.windows["dup"][0]
    t = np.asarray(w.imu_s_t)[:int(w.imu_s_count[0])]
    assert sorted(np.flatnonzero(np.diff(t) == 0).tolist()) == [11, 34]     # samples 10 and 32 behind one leading sample, twice
    w = ref.windows["inside_one"][0]
    t = np.asarray(w.imu_s_t)[:int(w.imu_s_count[0])]
    assert np.searchsorted(t, w.imu_t0[0]) == np.searchsorted(t, w.imu_t1[0]) and w.imu_t0[0] not in t and w.imu_t1[0] not in t
    w = ref.windows["sat"][0]
    p = w.imu_params
    assert (np.abs(w.imu_s_gyr).max(1) > p.g_max).sum() == 2 and (np.abs(w.imu_s_acc).max(1) > p.a_max).sum() == 2   # one per factor


def test_every_factor_is_finite_and_no_residual_is_near_zero(ref):
    for name, i, f, fac in ref.all():
        for q in cases.QUANTITIES:
            assert np.all(np.isfinite(np.asarray(fac.ref[q], np.float64))), (name, i, f, q)
        assert fac.redo_count == 1
        assert np.abs(fac.r).min() > 1e-3 and np.abs(fac.r).max() > 1.0, (name, i, f, fac.r)


def test_the_two_long_double_evaluations_agree_better_than_fp64_with_either(ref):
    """per factor and quantity.  Both sides hand out doubles, so one rounding (2^-52 in the quantity's scale) is the least two
    different correct evaluations can be told apart by: where the fp64 oracle has the referee's very bits (sqrt_info of
    inside_one) nothing can be closer."""
    worst = 0.0
    for name, i, f, fac in ref.all():
        ld = fac.statement(np.longdouble)
        for q in cases.QUANTITIES:
            x = np.asarray(ld[q], np.float64)
            d_ld = cases.deviation(x, fac.ref[q], fac.a[q])
            d_oracle, d_stmt = fac.e_oracle[q], cases.deviation(fac.o64[q], x, fac.a[q])
            assert d_ld <= max(min(d_oracle, d_stmt), cases.EPS), (name, i, f, q, d_ld, d_oracle, d_stmt)
            worst = max(worst, d_ld)
    print(f"IMUREF the long-double statement and oracle: at most {worst:.2e} apart (the information matrix; conditioning 1e9)")


def test_e_ref_figures(ref):
    """(printed for profiles/imu_referee_notes.md; e_ref is measured when the tests run, never committed as a limit)"""
    for q in cases.QUANTITIES:
        e = [(fac.e_ref[q], f"{name} w{i} f{f}") for name, i, f, fac in ref.all()]
        print(f"IMUREF e_ref {q}: {min(e)[0]:.2e} ... {max(e)[0]:.2e} ({max(e)[1]})")
        assert np.isfinite(max(e)[0])
    for name, i, f, fac in ref.all():
        print(f"IMUREF e_ref {name} w{i} f{f} n {fac.n_steps} " + " ".join(f"{q} {fac.e_ref[q]:.1e}" for q in cases.QUANTITIES))


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built and the reference tree absent")
def test_oracle_equals_the_compiled_reference_on_the_edge_streams(ref, oracle):
    """the tolerances of test_oracle_vs_ref.py::test_imu_fixtures_are_reference_outputs; the bias-correction path as
    test_imu_bias_correction_and_propagation has it, on every stream too"""
    from .test_oracle_vs_ref import TOL, rel
    rng = np.random.default_rng(17)
    for name, i, f, fac in ref.all():
        r, Js, si, cnt = R.imu_evaluate_fresh(*fac.inputs)
        ro, Jso, sio, cnto = oracle.imu_evaluate_fresh(*fac.inputs)
        assert cnt == cnto == 1, (name, i, f, cnt, cnto)
        assert rel(ro, r) <= TOL, (name, i, f, rel(ro, r))
        for k in range(4):
            assert rel(Jso[k], Js[k]) <= TOL, (name, i, f, k, rel(Jso[k], Js[k]))
        assert rel(sio, si) <= 1e-10, (name, i, f, rel(sio, si))
        assert rel(sio.T @ sio, si.T @ si) <= TOL, (name, i, f)
        # ... and orc_imu_evaluate_record is the same evaluation
        rr, Jsr, rec, steps, cntr = oracle.imu_evaluate_record(*fac.inputs)
        assert np.array_equal(rr, ro) and all(np.array_equal(a, b) for a, b in zip(Jsr, Jso)) and cntr == cnto
        assert np.array_equal(rec[slice(*cases.RECORD["sqrt_info"])].reshape(15, 15), sio)
        # the first-order bias correction around a reference bias inside the threshold
        t, g, a, prm, t0, t1, pose0, sb0, pose1, sb1 = fac.inputs
        d = rng.normal(size=3)
        d *= min(0.5e-4 / ((t1 - t0) * 1e-9), 1e-3) / np.linalg.norm(d)      # |db_g| Dt <= 0.5e-4: no re-preintegration
        sb_ref = sb0 + np.concatenate([rng.normal(size=3) * 0.01, d, rng.normal(size=3) * 1e-3])
        r, Js, cnt = R.imu_evaluate_at_ref(t, g, a, prm, t0, t1, sb_ref, pose0, sb0, pose1, sb1)
        ro, Jso, cnto = oracle.imu_evaluate_at_ref(t, g, a, prm, t0, t1, sb_ref, pose0, sb0, pose1, sb1)
        assert cnt == cnto == 0, (name, i, f, cnt, cnto)
        assert rel(ro, r) <= TOL, (name, i, f, rel(ro, r))
        for k in range(4):
            assert rel(Jso[k], Js[k]) <= TOL, (name, i, f, k)


# wrong variant: the case (window 0, factor 0 unless said) it must be caught on
CAUGHT_ON = {
    "no_t0_interpolation": ("unaligned_33", 0, 0),
    "drop_step_32": ("aligned_33", 0, 0),
    "no_saturation": ("sat", 0, 0),
    "propagation_dalpha": ("unaligned_33", 0, 0),
    "integrate_non_advancing": ("lead300", 0, 0),
    "transposed_F_block": ("inside_one", 0, 0),
    "wrong_permutation": ("ragged", 1, 2),
}


@pytest.mark.parametrize("mutation", stmt.MUTATIONS)
def test_a_wrong_factor_leaves_the_bound(ref, mutation):
    assert set(CAUGHT_ON) == set(stmt.MUTATIONS)
    name, i, f = CAUGHT_ON[mutation]
    fac = ref.factors[name][i][f]
    q = fac.statement(np.float64, mutation)
    ratio = {k: cases.deviation(q[k], fac.ref[k], fac.a[k]) / fac.bound(k) for k in cases.QUANTITIES}
    k = max(ratio, key=ratio.get)
    print(f"IMUREF wrong variant {mutation} on {name} w{i} f{f}: {ratio[k]:.2e} x the bound in {k}")
    assert ratio[k] >= cases.MUTATION_MARGIN, (mutation, name, ratio)
    # the unmutated statement is inside every bound (it is one of the two evaluations e_ref is made of)
    q = fac.statement(np.float64)
    for k in cases.QUANTITIES:
        assert cases.deviation(q[k], fac.ref[k], fac.a[k]) <= fac.bound(k), (name, k)
    # and the wrong variants that act on the device's special paths are not caught where those paths are not taken
    if mutation == "drop_step_32":
        fac = ref.factors["aligned_32"][0][0]
        q = fac.statement(np.float64, mutation)
        assert all(cases.deviation(q[k], fac.ref[k], fac.a[k]) <= fac.bound(k) for k in cases.QUANTITIES)
