"""The prologue of the ring Schur kernels on the decision-free launch (ba_schur2.hpp, SCH2_FREE): the landmark blocks, their Jacobi
scales, the first stages and the chunk's J^T J / J^T r list values leave in ONE trip, and work-item i forms (V_i + lambda D_i^2)^-1
and V_i^-1 b in front of the workgroup's first barrier.  The serial batch loop (OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES) keeps the old
order — scales loaded inside the V^-1 block, a barrier of its own behind it — and is the referee.

The inverse and the damping are spelled out with fma in the order the compiler gives the plain expressions in the other
instantiations, and absent list slots add the same exact zeros, so everything is compared with numpy.array_equal: the reduced
system and right-hand side after the first iteration, the states and summaries after optimize(10).  Every leg asserts its route
(okvis_ba_launch_route): `own` = a Schur launch of its own (schur_mfma_kernel<3>), `ride` = the route of bench.py's headline with the
IMU / prior factors riding (schur_ride_kernel<3>).  The shapes sit at the edges of the new code: a chunk of ONE landmark, chunks of
15, 7, 5 and 2 landmarks (no multiple of the stage's four), a window smaller than one chunk, a window of several chunks with a
ragged last one and missing (landmark, block) pairs.  The chunk sizes are asserted on the host (solver.index_lists)."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import TUNE_SCHUR_SERIAL_BATCHES, default_options

pytestmark = pytest.mark.gpu

FAR = dict(pose_noise=(0.4, np.deg2rad(6.0)), landmark_noise=0.8)   # far starts: rejected trials under DOGLEG
MODES = {"dogleg": {}, "dogleg_unscaled": dict(jacobi_scaling=0), "gn": dict(gauss_newton=1), "lm": dict(strategy=1)}
# a chunk is whole groups, up to the 16 landmarks of a small batch: groups of four fill it (a lone last landmark is a chunk of its
# own), groups of three stop at 15
GROUP4, GROUP3 = dict(tuning_group_lm=4), dict(tuning_group_lm=3)


def _windows(**kw):
    return [synthetic.small_window(seed=3, K=4, L=17, **kw),      # GROUP4: chunks of 16 and 1 landmarks
            synthetic.small_window(seed=4, K=3, L=7, **kw),       # one chunk of 7: smaller than a chunk, a last stage of three
            synthetic.make_window(6, 50, 0.6, 11, **kw)]          # 16, 16, 16, 2 / 15, 15, 15, 5: ragged last chunk, missing pairs


def _opts(mode, serial, route, **kw):
    o = default_options()
    o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    if route == "own":
        o.reserved0 = 4                      # no fused linearise + reduce launch: the Schur launch of its own
    else:
        o.tuning.split_small_min = 1         # the IMU / prior factors in a launch of their own, as from 40 windows on ...
        o.tuning.fused_max_windows = -1      # ... and no fused launch: they ride in the Schur launch
    o.tuning.flags = TUNE_SCHUR_SERIAL_BATCHES if serial else 0
    for k, v in {**MODES[mode], **kw}.items():
        if k.startswith("tuning_"):
            setattr(o.tuning, k[7:], v)
        else:
            setattr(o, k, v)
    return o


def _route(b, mode, serial, route, decision_free=None):
    r = b.launch_route()
    free = (mode != "lm") if decision_free is None else decision_free
    assert r["fused"] == 0 and r["schur_kernel"] == (4 if serial else 2), r
    assert r["decision_free_schur"] == int(free), r
    assert r["small_rides"] == int(route == "ride" and free), r
    return r


def _leg(ws, mode, serial, route, decision_free=None, **kw):
    """the reduced system of the first iteration, then the states and summaries after optimize(10)"""
    out = {}
    b = solver.WindowBatch(ws, options=_opts(mode, serial, route, debug_arrays=1, **kw))
    out["route"] = _route(b, mode, serial, route, decision_free)
    b.begin()
    b.iterate(1)
    b.synchronize()
    for i in range(len(ws)):
        out[f"S{i}"], out[f"rhs{i}"] = b.array("REDUCED_S", i), b.array("REDUCED_RHS", i)
    b.finish()
    b.close()
    b = solver.WindowBatch(ws, options=_opts(mode, serial, route, **kw))
    _route(b, mode, serial, route, decision_free)
    sm = b.optimize(10)
    out["cost"] = np.array([[x["initial_cost"], x["final_cost"]] for x in sm])
    out["steps"] = np.array([[x["iterations"], x["successful_steps"], x["termination"]] for x in sm])
    for i in range(len(ws)):
        out[f"pose{i}"], out[f"sb{i}"], out[f"lm{i}"] = (np.array(a) for a in b.get_state(i))
    assert b.helper_timeouts() == 0
    b.close()
    return out


def _same(ring, serial, what):
    for k in ring:
        if k == "route":
            continue
        assert ring[k].shape == serial[k].shape and np.array_equal(ring[k], serial[k]), \
            (what, k, float(np.abs(ring[k] - serial[k]).max()))
        assert np.isfinite(ring[k]).all(), (what, k)


def _chunk_sizes(ws, opts):
    out = []
    for w in ws:
        r = np.asarray(solver.index_lists(w, opts, len(ws))["chunk_recs"])
        out.append((r[:, 1] - r[:, 0]).tolist())
    return out


def _both(ws, mode, route, what, **kw):
    ring, serial = _leg(ws, mode, False, route, **kw), _leg(ws, mode, True, route, **kw)
    assert all(np.abs(ring[f"S{i}"]).max() > 0 for i in range(len(ws))), what
    _same(ring, serial, what)
    return ring


@pytest.mark.parametrize("route", ["own", "ride"])
@pytest.mark.parametrize("mode", list(MODES))
def test_prologue_at_the_chunk_edges(mode, route):
    """DOGLEG with and without Jacobi scaling, Gauss-Newton (decision-free: the new prologue) and LM (the deciding launch, untouched)"""
    ws = _windows()
    assert _chunk_sizes(ws, _opts(mode, False, route, **GROUP4)) == [[16, 1], [7], [16, 16, 16, 2]]
    ring = _both(ws, mode, route, (mode, route), **GROUP4)
    assert (ring["steps"][:, 0] == 10).all(), ring["steps"]


def test_prologue_with_chunks_of_fifteen():
    """groups of three: chunks of 15 landmarks (a last stage of three), a last chunk of five (a last stage of one)"""
    ws = _windows()
    assert _chunk_sizes(ws, _opts("dogleg", False, "ride", **GROUP3)) == [[15, 2], [7], [15, 15, 15, 5]]
    _both(ws, "dogleg", "ride", "chunks of fifteen", **GROUP3)


def test_chunks_by_schur_lm_per_block_keep_the_deciding_launch():
    """options.schur_lm_per_block shapes the chunks (six landmarks, last chunks of five, one and two) but asks for the deciding launch:
    the route is asserted, and that launch still agrees with the serial loop"""
    ws = _windows()
    kw = dict(schur_lm_per_block=6, **GROUP3)
    assert _chunk_sizes(ws, _opts("dogleg", False, "own", **kw)) == [[6, 6, 5], [6, 1], [6] * 8 + [2]]
    ring, serial = (_leg(ws, "dogleg", s, "own", decision_free=False, **kw) for s in (False, True))
    _same(ring, serial, "schur_lm_per_block")


@pytest.mark.parametrize("route", ["own", "ride"])
def test_prologue_after_rejected_trials(route):
    """DOGLEG from far starts: after a rejected trial the launch reduces the accepted buffer again, with the damping of the
    control words as the rejection left them"""
    ws = _windows(**FAR) + [synthetic.small_window(seed=sd, K=5, L=60, **FAR) for sd in (42, 43)]
    ring = _both(ws, "dogleg", route, ("rejected", route), **GROUP4)
    assert (ring["steps"][:, 1] < ring["steps"][:, 0]).any(), ("no rejected trial in the far-start windows", ring["steps"])


def test_marginalisation_keeps_its_path():
    """okvis_ba_marginalize eliminates the landmarks through the Schur launch without damping and without scales (marg_mode): the
    pseudo-inverse stays where it was, in the instantiation without the new prologue"""
    ws = _windows()
    out = {}
    for serial in (False, True):
        b = solver.WindowBatch(ws, options=_opts("dogleg", serial, "ride", **GROUP4))
        _route(b, "dogleg", serial, "ride")
        out[serial] = []
        for i, w in enumerate(ws):
            pm, sm = np.zeros(w.n_pose, np.uint8), np.zeros(w.n_sb, np.uint8)
            pm[0] = sm[0] = 1
            out[serial].append(b.marginalize(i, pm, sm))
        b.close()
    for g, r in zip(out[False], out[True]):
        assert g["dim"] == r["dim"] and g["rank"] == r["rank"]
        for k in ("H", "b0", "J", "e0"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(r[k])), k
            assert np.isfinite(np.asarray(g[k])).all() and np.abs(np.asarray(g[k])).max() > 0, k
