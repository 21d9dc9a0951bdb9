"""The pipelined landmark loop of the matrix-core Schur kernel (ba_schur2.hpp: stages of four landmarks over a ring of three tile
sets) against the serial batch loop it replaces (okvis_ba_tuning::flags & OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES, the referee).

A stage of four landmarks is 12 contraction indices = three whole groups of v_mfma_f64_16x16x4_f64, so both loops feed the matrix
core the same groups in the same order into the same accumulators: the damped reduced system, its right-hand side and the states
after ten iterations are compared as NUMBERS (numpy.array_equal: a signed zero is not a difference — the serial loop adds the
exact zeros of a ragged last batch, the ring loop does not).  The separate Schur launch is forced where a small batch would fuse
(options.reserved0 bit 2), and the route word OKVIS_BA_ROUTE_SCHUR_KERNEL is asserted in both legs (2: ring, 4: serial)."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import TUNE_SCHUR_SERIAL_BATCHES, default_options

pytestmark = pytest.mark.gpu

# (keyframes, landmarks, visibility): the bench window; sparse stages (the zeroing path); a last stage of 1 or 2 landmarks, a last
# chunk shorter than the ring, a pose part of 18 rows; one short chunk
SHAPES = [(10, 400, 1.0), (10, 400, 0.35), (6, 300, 0.3), (10, 397, 1.0), (7, 90, 0.8), (3, 50, 1.0), (10, 40, 1.0)]
FAR = dict(pose_noise=(0.4, np.deg2rad(6.0)), landmark_noise=0.8)   # far starts: rejected trials under DOGLEG


def _opts(mode, serial, separate=True, **kw):
    o = default_options()
    o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    if separate:
        o.reserved0 = 4                  # no fused linearise + reduce launch: the Schur launch of its own
    if mode == "gn":
        o.gauss_newton = 1
    elif mode == "lm":
        o.strategy = 1                   # OKVIS_BA_STRATEGY_LM: the Schur launch takes the decision (nodec = 0)
    o.tuning.flags = TUNE_SCHUR_SERIAL_BATCHES if serial else 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _route(b, mode, serial):
    r = b.launch_route()
    assert r["fused"] == 0 and r["schur_kernel"] == (4 if serial else 2), r
    assert r["decision_free_schur"] == (0 if mode == "lm" else 1), r
    return r


def _leg(ws, mode, serial, separate=True, **kw):
    """the reduced system of the first iteration, then the states and summaries after optimize(10)"""
    out = {}
    b = solver.WindowBatch(ws, options=_opts(mode, serial, separate, debug_arrays=1, **kw))
    out["route"] = _route(b, mode, serial)
    b.begin()
    b.iterate(1)
    b.synchronize()
    for i in range(len(ws)):
        out[f"S{i}"], out[f"rhs{i}"] = b.array("REDUCED_S", i), b.array("REDUCED_RHS", i)
    b.finish()
    b.close()
    b = solver.WindowBatch(ws, options=_opts(mode, serial, separate, **kw))
    _route(b, mode, serial)
    sm = b.optimize(10)
    out["cost"] = np.array([[x["initial_cost"], x["final_cost"]] for x in sm])
    out["steps"] = np.array([[x["iterations"], x["successful_steps"], x["termination"]] for x in sm])
    for i in range(len(ws)):
        out[f"pose{i}"], out[f"sb{i}"], out[f"lm{i}"] = (np.array(a) for a in b.get_state(i))
    b.close()
    return out


def _same(ring, serial, what):
    for k in ring:
        if k == "route":
            continue
        assert ring[k].shape == serial[k].shape and np.array_equal(ring[k], serial[k]), \
            (what, k, float(np.abs(ring[k] - serial[k]).max()))
        assert np.isfinite(ring[k]).all(), (what, k)


@pytest.mark.parametrize("mode", ["gn", "dogleg", "lm"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d_L%d_v%g" % s)
def test_ring_loop_equals_serial_loop(shape, mode):
    K, L, vis = shape
    ws = [synthetic.make_window(K, L, vis, 20240923)]
    ring, serial = _leg(ws, mode, False), _leg(ws, mode, True)
    assert ring["route"]["small_rides"] == 0, ring["route"]          # one window: schur_mfma_kernel<3>
    assert np.abs(ring["S0"]).max() > 0 and ring["steps"][0, 0] == 10, ring["steps"]
    _same(ring, serial, (shape, mode))


def test_ring_loop_equals_serial_loop_after_rejected_trials():
    """DOGLEG from far starts: a rejected trial makes the next launch reduce the other linearisation buffer again"""
    ws = [synthetic.make_window(K, L, vis, sd, **FAR) for (K, L, vis), sd in zip(SHAPES[1:], (42, 43, 44, 45, 46, 47))] + \
         [synthetic.small_window(seed=sd, K=5, L=60, **FAR) for sd in (42, 43, 44)]
    ring, serial = _leg(ws, "dogleg", False), _leg(ws, "dogleg", True)
    assert (ring["steps"][:, 1] < ring["steps"][:, 0]).any(), ("no rejected trial in the far-start windows", ring["steps"])
    _same(ring, serial, "rejected")


def test_ring_loop_equals_serial_loop_headline_batch():
    """the batch bench.py times: 64 bench windows through their default route — three sub-batches, graph replay, the IMU / prior
    factors riding in the Schur launch (schur_ride_kernel<3>)"""
    ws = [synthetic.make_window(10, 400, 1.0, 20240923 + i) for i in range(64)]
    ring = _leg(ws, "gn", False, separate=False, use_graph=1)
    serial = _leg(ws, "gn", True, separate=False, use_graph=1)
    for r in (ring["route"], serial["route"]):
        assert r["windows"] == 64 and r["small_rides"] == 1 and r["sub_batches"] == 3 and r["max_chunks"] == 9, r
    _same(ring, serial, "headline")


def test_ring_loop_equals_serial_loop_in_marginalisation():
    """okvis_ba_marginalize eliminates the landmarks through the same Schur launch (marg_mode: no damping, pseudo-inverse of V)"""
    for K, L, vis, seed in ((5, 40, 0.7, 41), (10, 397, 1.0, 20240923), (6, 300, 0.3, 20240923)):
        w = synthetic.make_window(K, L, vis, seed)
        pm, sm = np.zeros(w.n_pose, np.uint8), np.zeros(w.n_sb, np.uint8)
        pm[0] = sm[0] = 1
        out = []
        for serial in (False, True):
            o = default_options()
            o.reserved0 = 4              # (one window would fuse: the elimination through the Schur launch)
            o.tuning.flags = TUNE_SCHUR_SERIAL_BATCHES if serial else 0
            b = solver.WindowBatch([w], options=o)
            r = b.launch_route()
            assert r["fused"] == 0 and r["schur_kernel"] == (4 if serial else 2), r
            out.append(b.marginalize(0, pm, sm))
            b.close()
        g, r = out
        assert g["dim"] == r["dim"] and g["rank"] == r["rank"]
        for k in ("H", "b0", "J", "e0"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(r[k])), (K, L, vis, k)
            assert np.isfinite(np.asarray(g[k])).all() and np.abs(np.asarray(g[k])).max() > 0, (K, L, vis, k)
