"""The float32 referee's own statement (tests/fp32_statement.py) checked on the CPU, no GPU needed:

  * at float64 it IS the oracle: per observation (oracle_lib.reprojection) and for the five arrays of a whole window
    (OracleWindow.array), 1e-12 relative, all four distortion models, extrinsics fixed / shared / per frame, and every window of
    the GPU referee (tests/fp32_cases.py);
  * at float32 nothing is silently promoted;
  * sensitivity of the referee's inputs: each of four deliberately wrong Jacobian terms moves at least one array by 10 x the
    bound the kernels are held to (4 x e_stmt, tests/test_gpu_fp32_linearize.py) — a condition on the windows and cameras of
    tests/fp32_cases.py, not on any kernel;
  * the windows respect the input condition (no depth within 1e-4 of the 0.2 m validity threshold, float32 and float64 take
    the same branches) and really contain the edges they are named after.
"""
import numpy as np
import pytest

from okvis_amd import synthetic
from okvis_amd.window import DIST_EQUIDISTANT, DIST_NONE, DIST_RADTAN, DIST_RADTAN8

from . import fp32_cases as cases
from . import fp32_statement as stmt

MODELS = [DIST_NONE, DIST_RADTAN, DIST_EQUIDISTANT, DIST_RADTAN8]
TOL64 = 1.0e-12


@pytest.fixture(scope="module")
def referee(oracle):
    return cases.Referee(oracle)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ext", ["fixed", "shared", "perframe"])
def test_float64_statement_is_the_oracle_per_observation(oracle, model, ext):
    w = cases.referee_camera(synthetic.small_window(seed=71 + model, K=3, L=12, estimate_extrinsics=ext, cam_model=model))
    assert w.n_obs > 40
    for o in range(w.n_obs):
        args = (w.pose[w.obs_pose[o]], w.lm[w.obs_lm[o]], w.pose[w.obs_ext[o]], w.cam_intr[w.obs_cam[o]], model, w.obs_uv[o])
        sw = float(w.obs_sqrtw[o])
        r, Jp, Jl, Je, _, valid = oracle.reprojection(*args, sqrt_info=sw * np.eye(2))
        s = stmt.observation(args[0], args[2], args[1], args[3], model, args[5], sw, np.float64)
        assert s["valid"] == valid and s["defined"]
        for a, b in ((s["r"], r), (s["Jp"], Jp), (s["Jl"], Jl), (s["Je"], Je)):
            assert _rel(a, b) <= TOL64, (o, a, b)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ext", ["fixed", "shared", "perframe"])
def test_float64_statement_is_the_oracle_for_a_window(oracle, model, ext):
    w = cases.referee_camera(synthetic.small_window(seed=81 + model, K=3, L=20, estimate_extrinsics=ext, cam_model=model))
    o = oracle.OracleWindow(w)
    o.linearize()
    s = stmt.window_arrays(w, np.float64)
    assert np.array_equal(s["pairs"][0], o.pairs()[0]) and np.array_equal(s["pairs"][1], o.pairs()[1])
    for name in stmt.ARRAYS:
        assert np.abs(o.array(name)).max() > 0
        assert stmt.deviation(s[name], o.array(name)) <= TOL64, name


def test_float64_statement_is_the_oracle_on_every_referee_window(referee):
    for name in cases.CASES:
        for s64, arrays, prs in zip(referee.stmt64[name], referee.oracle_arrays[name], referee.oracle_pairs[name]):
            assert np.array_equal(s64["pairs"][0], prs[0]) and np.array_equal(s64["pairs"][1], prs[1]), name
            for a in stmt.ARRAYS:
                assert stmt.deviation(s64[a], arrays[a]) <= TOL64, (name, a)
                assert np.array_equal(s64[a] == 0.0, arrays[a] == 0.0), (name, a)     # the same exact zeros


@pytest.mark.parametrize("model", MODELS)
def test_float32_statement_is_float32_throughout(model):
    w = cases.referee_camera(synthetic.small_window(seed=91, K=3, L=8, estimate_extrinsics="shared", cam_model=model))
    for o in range(0, w.n_obs, 5):
        s = stmt.observation(w.pose[w.obs_pose[o]], w.pose[w.obs_ext[o]], w.lm[w.obs_lm[o]], w.cam_intr[w.obs_cam[o]], model,
                             w.obs_uv[o], float(w.obs_sqrtw[o]), np.float32)
        assert s["valid"]
        for k in ("r", "Jp", "Jl", "Je"):
            assert s[k].dtype == np.float32 and np.abs(s[k]).max() > 0
    k = np.array([-0.2, 0.1, 3e-3, 2e-3, 0.01, 0.002, -0.001, 0.0005], np.float32)
    d0, d1, J = stmt.distort(model, k, np.float32(0.3), np.float32(-0.2), np.float32)
    assert type(d0) is np.float32 and type(d1) is np.float32 and J.dtype == np.float32


def test_input_condition_and_edges_of_the_referee_windows(referee):
    for name in cases.CASES:
        referee.check_input_condition(name)
    s = referee.stmt64
    assert not s["edge_radtan8_undefined"][0]["defined"].all()                  # rho > 9 somewhere
    assert s["edge_radtan8_undefined"][0]["defined"].sum() > 50
    close = s["edge_too_close"][0]
    assert (close["defined"] & ~close["valid"]).any()                           # residual kept, Jacobians zeroed
    assert (np.asarray(referee.windows["edge_negative_w"][0].lm)[:, 3] < 0).any()
    w = referee.windows["edge_unobserved"][0]
    assert 5 not in np.asarray(w.obs_lm) and np.all(referee.oracle_arrays["edge_unobserved"][0]["LM_V"].reshape(-1, 6)[5] == 0)
    # the on-axis point: |u| below the equidistant model's 1e-8 switch in float64
    w = referee.windows["edge_equidistant_on_axis"][0]
    o = np.flatnonzero(np.asarray(w.obs_lm) == 3)[0]
    ob = stmt.observation(w.pose[w.obs_pose[o]], w.pose[w.obs_ext[o]], w.lm[3], w.cam_intr[w.obs_cam[o]], DIST_EQUIDISTANT, w.obs_uv[o], 1.0)
    Jl_axis = np.abs(ob["Jl"]).max()
    assert ob["valid"] and Jl_axis > 0
    for name in cases.CASES:       # every window is within the sizes the tests are meant to stay quick at
        for w in referee.windows[name]:
            assert w.n_obs <= 900, (name, w.n_obs)


# which windows a mutation is looked for in: it must show on at least one array of at least one of them
MUTATION_CASES = {"radtan_j00": ("route_small", "model_radtan"), "equi_dpoly": ("model_equidistant",),
                  "je_sign": ("route_ext_shared", "route_ext_perframe"), "jp_trans": ("route_small",)}


@pytest.mark.parametrize("mutation", stmt.MUTATIONS)
def test_referee_inputs_notice_a_wrong_term(referee, mutation):
    """Each mutation of the float32 statement deviates from the oracle by at least 10 x (4 x e_stmt(A)) on some array A."""
    assert set(MUTATION_CASES) == set(stmt.MUTATIONS)
    best = 0.0
    for name in MUTATION_CASES[mutation]:
        for w, arrays in zip(referee.windows[name], referee.oracle_arrays[name]):
            m = stmt.window_arrays(w, np.float32, mutate=mutation)
            for a in stmt.ARRAYS:
                bound = cases.BOUND_FACTOR * referee.e_stmt[a]
                ratio = stmt.deviation(m[a], arrays[a]) / bound
                print(f"{mutation:12s} {name:20s} {a:13s} deviation / bound = {ratio:9.1f}")
                best = max(best, ratio)
    assert best >= 10.0, (mutation, best, referee.e_stmt)


def test_e_stmt_is_float32_rounding(referee):
    """The yardstick itself is float32 rounding and nothing else: not below a quarter of one rounding (2^-24 = 6e-8: the statement
    would not be evaluating in float32), and not beyond 1e-3 — the residual is a difference of pixel coordinates of some hundred
    pixels, each known to 2^-24 relative, i.e. to some 1e-5 pixels, and the Cauchy weight 1 / (1 + |r|^2) hands that on to V, b
    and W as a relative error of 1e-5 .. 1e-4; the arrays without it (the residual against its own maximum, H_l) stay at a few
    1e-6 / 1e-7.  What keeps the yardstick USEFUL is test_referee_inputs_notice_a_wrong_term, not this ceiling."""
    for a in stmt.ARRAYS:
        print(f"e_stmt({a}) = {referee.e_stmt[a]:.3e}")
        assert 2.0 ** -26 < referee.e_stmt[a] < 1.0e-3, (a, referee.e_stmt[a])
    for name in cases.CASES:
        for i, e in enumerate(referee.e_case[name]):
            print(f"{name:26s} window {i}: " + "  ".join(f"{a} {e[a]:.2e}" for a in stmt.ARRAYS))
