"""The chunk launch records of the ring loop of the matrix-core Schur kernel (ba_schur2.hpp; build_chunk_records) on the GPU.

A ring workgroup takes its chunk descriptor and the heads of its J^T J / J^T r lists from ONE array of the batch, addressed by the
kernel arguments and the workgroup's indices; the serial loop (OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES) keeps reading chunk_desc /
chunk_diag_begin / chunk_diag_out through the window record and is the referee.  No arithmetic differs, so everything is compared
with numpy.array_equal: the reduced system and right-hand side of the first iteration, the states and summaries after optimize(10),
the IMU reference biases and re-preintegration counts — on the route bench.py's headline takes (factors riding in the Schur launch,
forced at small sizes by tuning.split_small_min = 1 and tuning.fused_max_windows = -1), with OKVIS_BA_TUNE_NO_SMALL_RIDE as a third
leg.  The shapes are the ones at which the record's address or contents can go wrong: windows of different chunk and IMU term
counts in one batch (stride, slots behind a window's last chunk), sub-batches that start at a non-zero window, ragged chunks and
missing pairs, lists longer than a record's head, rejected trials, a finished window, a patched window, marginalisation."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import TUNE_NO_SMALL_RIDE, TUNE_SCHUR_SERIAL_BATCHES, default_options
from tests.patch_helpers import patch_between, sliding_pair

pytestmark = pytest.mark.gpu

FAR = dict(pose_noise=(0.4, np.deg2rad(6.0)), landmark_noise=0.8)   # far starts: rejected trials under DOGLEG
LEGS = {"ring": 0, "serial": TUNE_SCHUR_SERIAL_BATCHES, "no_ride": TUNE_NO_SMALL_RIDE}


def _opts(mode, flags, tol0=True, **kw):
    o = default_options()
    if tol0:
        o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    o.gauss_newton = 1 if mode == "gn" else 0
    o.tuning.split_small_min = 1         # the IMU / prior factors in a launch of their own, as from 40 windows on
    o.tuning.fused_max_windows = -1      # no fused linearise + reduce launch: the Schur launch
    o.tuning.flags = flags
    for k, v in kw.items():
        if k.startswith("tuning_"):
            setattr(o.tuning, k[7:], v)
        else:
            setattr(o, k, v)
    return o


def _route(b, leg):
    r = b.launch_route()
    assert r["fused"] == 0 and r["decision_free_schur"] == 1 and r["split_small"] == 1, r
    assert r["schur_kernel"] == (4 if leg == "serial" else 2) and r["small_rides"] == (0 if leg == "no_ride" else 1), (leg, r)
    return r


def _leg(ws, mode, leg, n=10, **kw):
    out = {}
    b = solver.WindowBatch(ws, options=_opts(mode, LEGS[leg], debug_arrays=1, **kw))
    out["route"] = _route(b, leg)
    b.begin()
    b.iterate(1)
    b.synchronize()
    for i in range(len(ws)):
        out[f"S{i}"], out[f"rhs{i}"] = b.array("REDUCED_S", i), b.array("REDUCED_RHS", i)
    b.finish()
    b.close()
    b = solver.WindowBatch(ws, options=_opts(mode, LEGS[leg], **kw))
    _route(b, leg)
    sm = b.optimize(n)
    out["cost"] = np.array([[x["initial_cost"], x["final_cost"]] for x in sm])
    out["steps"] = np.array([[x["iterations"], x["successful_steps"], x["termination"]] for x in sm])
    for i in range(len(ws)):
        out[f"pose{i}"], out[f"sb{i}"], out[f"lm{i}"] = (np.array(a) for a in b.get_state(i))
        out[f"sb_ref{i}"], out[f"redo{i}"] = np.array(b.array("IMU_SB_REF", i)), np.array(b.array("IMU_REDO_COUNT", i))
    assert b.helper_timeouts() == 0
    b.close()
    return out


def _same(a, b, what):
    for k in a:
        if k == "route":
            continue
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
        assert np.isfinite(a[k]).all(), (what, k)


def _three_legs(ws, mode, what, **kw):
    legs = {leg: _leg(ws, mode, leg, **kw) for leg in LEGS}
    _same(legs["ring"], legs["serial"], (what, "ring vs serial"))
    _same(legs["ring"], legs["no_ride"], (what, "riding vs single factor launch"))
    assert all(np.abs(legs["ring"][f"S{i}"]).max() > 0 for i in range(len(ws)))
    return legs["ring"]


def _mixed(**kw):
    # 33 / 10 / 4 chunks of up to 16 landmarks, 10 / 6 / 5 pose blocks, 9 / 5 / 4 IMU terms; visibility 0.5: missing pairs, ragged chunks
    return [synthetic.make_window(10, 400, 1.0, 20240923, **kw), synthetic.make_window(6, 150, 0.5, 11, **kw),
            synthetic.small_window(seed=12, K=5, L=60, **kw)]


@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_mixed_chunk_and_term_counts_in_one_batch(mode):
    ws = _mixed()
    assert len({w.n_imu for w in ws}) == 3
    ring = _three_legs(ws, mode, "mixed")
    assert ring["route"]["max_chunks"] == 33 and (ring["steps"][:, 0] == 10).all(), (ring["route"], ring["steps"])


def test_sub_batches_that_start_at_a_non_zero_window():
    """two streams over five windows: the second sub-batch's launches start at window 2 of the record array; a ragged last chunk
    (397 landmarks: a last stage of one landmark)"""
    ws = _mixed() + [synthetic.make_window(10, 397, 1.0, 20240924), synthetic.make_window(7, 90, 0.8, 13)]
    ring = _three_legs(ws, "gn", "w0", n_streams=2)
    assert ring["route"]["sub_batches"] == 2, ring["route"]


def test_lists_longer_than_the_head_of_a_record():
    """groups of two landmarks: eight groups per chunk of 16, so a pose block's list has up to eight partials, six of them in the record"""
    ws = [synthetic.make_window(7, 90, 0.8, 5), synthetic.make_window(6, 150, 0.5, 11)]
    for w in ws:   # (on the host: the shape really has such a list)
        L = solver.index_lists(w, _opts("gn", 0, tuning_group_lm=2), len(ws))
        assert L["chunk_recs"][:, 33::8].max() > 6, L["chunk_recs"][:, 33::8].max()
    _three_legs(ws, "dogleg", "long lists", tuning_group_lm=2)


def test_rejected_trials_from_far_starts():
    """DOGLEG from far starts: rejected trials reduce the other linearisation buffer again, terms re-preintegrate and take back"""
    ws = _mixed(**FAR)[1:] + [synthetic.small_window(seed=sd, K=5, L=60, **FAR) for sd in (42, 43, 44)]
    ring = _three_legs(ws, "dogleg", "far")
    assert (ring["steps"][:, 1] < ring["steps"][:, 0]).any(), ("no rejected trial in the far-start windows", ring["steps"])
    assert max(ring[f"redo{i}"].max() for i in range(len(ws))) >= 2, "no term re-preintegrated"


def test_a_finished_window_in_the_batch():
    """default tolerances: the near-start window converges and leaves its launches early while the far-start one goes on"""
    ws = [synthetic.small_window(seed=12, K=5, L=60), synthetic.make_window(6, 150, 0.5, 11, **FAR)]
    ring = _three_legs(ws, "dogleg", "finished", n=14, tol0=False)
    assert ring["steps"][:, 0].min() < ring["steps"][:, 0].max(), ring["steps"]


def test_a_patched_window_equals_a_fresh_upload():
    """okvis_ba_patch_window builds the records again with the batch: the patched solver and a fresh upload of its containers agree"""
    A, B = sliding_pair(seed=50, K=5, L=60)
    A2, _ = sliding_pair(seed=51, K=6, L=90)
    runs = {}
    for leg in ("ring", "serial"):
        b = solver.WindowBatch([A.window(), A2.window()], options=_opts("dogleg", LEGS[leg]), patchable=True)
        _route(b, leg)
        b.optimize(3)
        b.patch(0, patch_between(A, B))
        _route(b, leg)
        views = [b.patched_view(0), b.patched_view(1)]
        fresh = solver.WindowBatch(views, options=_opts("dogleg", LEGS[leg]))
        sp, sf = b.optimize(5), fresh.optimize(5)
        assert sp == sf and sp[0]["iterations"] == 5
        runs[leg] = [np.array(a) for i in range(2) for a in b.get_state(i)]
        for x, y in zip(runs[leg], [np.array(a) for i in range(2) for a in fresh.get_state(i)]):
            assert np.array_equal(x, y)
        b.close(); fresh.close()
    for x, y in zip(runs["ring"], runs["serial"]):
        assert np.array_equal(x, y)


def test_marginalisation_through_the_records():
    """okvis_ba_marginalize eliminates the landmarks through the same Schur launch, one window of the batch at a time"""
    ws = _mixed()
    out = {}
    for leg in ("ring", "serial"):
        b = solver.WindowBatch(ws, options=_opts("dogleg", LEGS[leg]))
        _route(b, leg)
        out[leg] = []
        for i, w in enumerate(ws):
            pm, sm = np.zeros(w.n_pose, np.uint8), np.zeros(w.n_sb, np.uint8)
            pm[0] = sm[0] = 1
            out[leg].append(b.marginalize(i, pm, sm))
        b.close()
    for g, r in zip(out["ring"], out["serial"]):
        assert g["dim"] == r["dim"] and g["rank"] == r["rank"]
        for k in ("H", "b0", "J", "e0"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(r[k])), k
            assert np.isfinite(np.asarray(g[k])).all() and np.abs(np.asarray(g[k])).max() > 0, k
