"""BASELINE configs[4]: fp32 Jacobian/Hessian build with fp64 reduced-camera solve (okvis_ba_options.fp32_linearize).
A tolerance study, not a bit-parity claim: the mixed path must stay within 1e-5 relative of the fp64 oracle on
the final cost (SURVEY.md §8d expected 1e-5..1e-4 from naive fp32; the fp64 differencing of the two
translations brings it to ~3e-7, see profiles/r01_mixed_precision.json) and converge in about as many
iterations."""
import numpy as np
import pytest

from okvis_amd import synthetic
from okvis_amd.window import default_options

pytestmark = pytest.mark.gpu


def _run(w, fp32, iters):
    from okvis_amd import solver
    opt = default_options()
    opt.fp32_linearize = fp32
    b = solver.WindowBatch([w], options=opt)
    s = b.optimize(iters)[0]
    st = b.get_state(0)
    b.close()
    return s, st


@pytest.mark.parametrize("ext,model", [("fixed", 1), ("shared", 2), ("perframe", 1)])
def test_small_windows(oracle, ext, model):
    w = synthetic.small_window(seed=51, K=4, L=60, estimate_extrinsics=ext, cam_model=model)
    so = oracle.OracleWindow(w).optimize(12)
    s, _ = _run(w, 1, 12)
    assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-5 * so["initial_cost"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-5 * so["final_cost"]
    assert abs(s["iterations"] - so["iterations"]) <= 2


def test_config_A(oracle):
    w = synthetic.config_A()
    s64, st64 = _run(w, 0, 10)
    s32, st32 = _run(w, 1, 10)
    assert abs(s32["final_cost"] - s64["final_cost"]) <= 1e-5 * s64["final_cost"]
    assert s32["iterations"] == s64["iterations"]
    assert np.abs(st32[0][:, :3] - st64[0][:, :3]).max() < 1e-4     # positions [m]
    assert np.abs(st32[1] - st64[1]).max() < 1e-3                   # speed / biases


def test_switching_precision_rebuilds_the_graph(oracle):
    from okvis_amd import solver
    w = synthetic.small_window(seed=52, K=4, L=40)
    opt = default_options()
    b = solver.WindowBatch([w], options=opt)
    fused = [b.launch_route()["fused"]]             # Dp = 24: the upload lays the batch out for fused mode, in ITS precision
    a = b.optimize(5)[0]["final_cost"]
    b.set_state(0, w.pose, w.sb, w.lm)
    opt.fp32_linearize = 1
    b.set_options(opt)
    fused.append(b.launch_route()["fused"])         # the reduction's stage was sized for fp64: separate Schur launch
    c = b.optimize(5)[0]["final_cost"]
    b.set_state(0, w.pose, w.sb, w.lm)
    opt.fp32_linearize = 0
    b.set_options(opt)
    fused.append(b.launch_route()["fused"])         # back in the layout's own precision
    d = b.optimize(5)[0]["final_cost"]
    b.close()
    # ... and the other way round: uploaded for fp32, switched to fp64
    opt.fp32_linearize = 1
    b = solver.WindowBatch([w], options=opt)
    fused.append(b.launch_route()["fused"])
    opt.fp32_linearize = 0
    b.set_options(opt)
    fused.append(b.launch_route()["fused"])
    b.close()
    assert fused == [1, 0, 1, 1, 0]
    assert a == d                                   # back on the fp64 kernels: bit-identical rerun
    assert a != c and abs(a - c) <= 1e-5 * a        # the fp32 kernels really ran in between
