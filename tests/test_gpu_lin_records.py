"""The group launch records of linearize2_rec_kernel (ba_linearize2.hpp; build_group_records) on the GPU.

A workgroup of the record instantiations takes its Group record, the control words and the window record in one trip whose
addresses follow from kernel arguments and blockIdx, then requests every operand in straight-line code;
OKVIS_BA_TUNE_LIN_NO_RECORDS keeps linearize2_kernel, which reads the same things through the window record where it needs
them, and is the referee.  No arithmetic differs, so everything is compared with numpy.array_equal: the linearisation arrays of
the first iteration (debug_arrays = 1: residuals, V / b / H_l per landmark, W per pair, the trial landmarks, the reduced system
and right-hand side that the group partials sum into, gradient, damping, step, and the control record that the group scalars sum
into), then costs, book-keeping, states, IMU reference biases and re-preintegration counts after optimize(10) — on the route
bench.py's headline takes, forced at small sizes by tuning.split_small_min = 1 and tuning.fused_max_windows = -1.  The shapes are
the ones at which the record's address or contents can go wrong: windows of different group counts in one batch (stride, zero
slots behind a window's last group), sub-batches that start at a non-zero window, a ragged last group, Gauss-Newton and DOGLEG from
far starts (rejected trials: the not-pending exit; explicit dogleg steps), a finished window next to a running one,
okvis_ba_begin's init launch (every leg starts with it), a patched window, fp64 and fp32_linearize.  The record array itself is
read back from the device (GROUP_RECS) after an upload and after a patch: stride, contents, zero tail slots.
No group of these windows has more than LIN_TASK_CACHE = 64 tasks (a task is a pose block the group observes; the windows have
at most 12): the uncached task path is not reached here, test_the_task_lists_fit_the_cache says so on the host lists."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import TUNE_LIN_NO_RECORDS, default_options
from tests.patch_helpers import patch_between, sliding_pair

pytestmark = pytest.mark.gpu

FAR = dict(pose_noise=(0.4, np.deg2rad(6.0)), landmark_noise=0.8)   # far starts: rejected trials under DOGLEG
LEGS = {"records": 0, "window_record": TUNE_LIN_NO_RECORDS}
FIRST = ("OBS_RESIDUAL", "LM_V", "LM_B", "LM_HQ", "PAIR_W", "LM", "REDUCED_S", "REDUCED_RHS", "STEP", "GRADIENT", "DAMPING", "CTRL")


def _opts(mode, flags, tol0=True, **kw):
    o = default_options()
    if tol0:
        o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    o.gauss_newton = 1 if mode == "gn" else 0
    o.tuning.split_small_min = 1         # the IMU / prior factors in a launch of their own, as from 40 windows on
    o.tuning.fused_max_windows = -1      # no fused linearise + reduce launch
    o.tuning.flags = flags
    for k, v in kw.items():
        if k.startswith("tuning_"):
            setattr(o.tuning, k[7:], v)
        else:
            setattr(o, k, v)
    return o


def _route(b, leg):
    r = b.launch_route()
    assert r["fused"] == 0 and r["piece_path"] == 1 and r["split_small"] == 1 and r["decision_free_schur"] == 1, r
    assert r["lin_records"] == (1 if leg == "records" else 0), (leg, r)
    return r


def _leg(ws, mode, leg, n=10, **kw):
    out = {}
    b = solver.WindowBatch(ws, options=_opts(mode, LEGS[leg], debug_arrays=1, **kw))
    out["route"] = _route(b, leg)
    b.begin()          # (the init launch)
    b.iterate(1)
    b.synchronize()
    for i in range(len(ws)):
        for a in FIRST:
            out[f"{a}{i}"] = np.array(b.array(a, i))
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


def _both_legs(ws, mode, what, **kw):
    legs = {leg: _leg(ws, mode, leg, **kw) for leg in LEGS}
    _same(legs["records"], legs["window_record"], what)
    assert all(np.abs(legs["records"][f"PAIR_W{i}"]).max() > 0 and np.abs(legs["records"][f"REDUCED_S{i}"]).max() > 0 for i in range(len(ws)))
    return legs["records"]


def _mixed(**kw):
    # 34 / 10 / 4 groups of up to 16 landmarks, 12 / 8 / 7 pose blocks; visibility 0.5: missing pairs
    return [synthetic.make_window(10, 400, 1.0, 20240923, **kw), synthetic.make_window(6, 150, 0.5, 11, **kw),
            synthetic.small_window(seed=12, K=5, L=60, **kw)]


def test_the_task_lists_fit_the_cache():
    """(host lists) group counts differ between the windows of _mixed, and no group has more than LIN_TASK_CACHE tasks"""
    counts = []
    for w in _mixed() + [synthetic.make_window(10, 397, 1.0, 20240924), synthetic.make_window(7, 90, 0.8, 13)]:
        L = solver.index_lists(w, _opts("gn", 0), 5)
        assert L["group_recs"][:, 19].max() <= 64, L["group_recs"][:, 19].max()
        counts.append(len(L["groups"]))
    assert len(set(counts[:3])) == 3, counts


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_mixed_group_counts_in_one_batch(mode, fp32):
    rec = _both_legs(_mixed(), mode, ("mixed", mode, fp32), fp32_linearize=fp32)
    assert (rec["steps"][:, 0] == 10).all(), rec["steps"]


def test_sub_batches_that_start_at_a_non_zero_window():
    """two streams over five windows: the second sub-batch's launches start at window 2 of the record array and of the control
    records; a ragged last group (397 landmarks)"""
    ws = _mixed() + [synthetic.make_window(10, 397, 1.0, 20240924), synthetic.make_window(7, 90, 0.8, 13)]
    rec = _both_legs(ws, "gn", "w0", n_streams=2)
    assert rec["route"]["sub_batches"] == 2, rec["route"]


@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_far_starts(mode):
    """DOGLEG from far starts: rejected trials (the launch after them leaves at once: nothing pending), explicit dogleg steps"""
    ws = _mixed(**FAR)[1:] + [synthetic.small_window(seed=sd, K=5, L=60, **FAR) for sd in (42, 43, 44)]
    rec = _both_legs(ws, mode, ("far", mode))
    if mode == "dogleg":
        assert (rec["steps"][:, 1] < rec["steps"][:, 0]).any(), ("no rejected trial in the far-start windows", rec["steps"])
        # ... and an explicit dogleg step (Ctrl::tr_kind == 1, entry 16 of CTRL) was the pending trial of some launch
        b = solver.WindowBatch(ws, options=_opts(mode, 0))
        _route(b, "records")
        b.begin()
        kinds = []
        for _ in range(10):
            b.iterate(1)
            b.synchronize()
            kinds.append([int(b.array("CTRL", i)[16]) for i in range(len(ws))])
        b.finish()
        b.close()
        assert (np.array(kinds) == 1).any(), kinds


def test_a_finished_window_in_the_batch():
    """default tolerances: the near-start window converges and leaves its launches early while the far-start one goes on"""
    ws = [synthetic.small_window(seed=12, K=5, L=60), synthetic.make_window(6, 150, 0.5, 11, **FAR)]
    rec = _both_legs(ws, "dogleg", "finished", n=14, tol0=False)
    assert rec["steps"][:, 0].min() < rec["steps"][:, 0].max(), rec["steps"]


def test_a_patched_window_equals_a_fresh_upload():
    """okvis_ba_patch_window builds the records again with the batch: the patched solver and a fresh upload of its containers agree"""
    A, B = sliding_pair(seed=50, K=5, L=60)
    A2, _ = sliding_pair(seed=51, K=6, L=90)
    runs = {}
    for leg in LEGS:
        b = solver.WindowBatch([A.window(), A2.window()], options=_opts("dogleg", LEGS[leg]), patchable=True)
        _route(b, leg)
        b.optimize(3)
        b.patch(0, patch_between(A, B))
        _route(b, leg)
        views = [b.patched_view(0), b.patched_view(1)]
        fresh = solver.WindowBatch(views, options=_opts("dogleg", LEGS[leg]))
        sp, sf = b.optimize(5), fresh.optimize(5)
        assert sp == sf and sp[0]["iterations"] == 5
        assert b.helper_timeouts() == 0 and fresh.helper_timeouts() == 0
        runs[leg] = [np.array(a) for i in range(2) for a in b.get_state(i)]
        for x, y in zip(runs[leg], [np.array(a) for i in range(2) for a in fresh.get_state(i)]):
            assert np.array_equal(x, y)
        b.close(); fresh.close()
    for x, y in zip(runs["records"], runs["window_record"]):
        assert np.array_equal(x, y)


def _check_device_records(b, ws, opts, what):
    """the record array as the DEVICE holds it (GROUP_RECS: [0] the stride, then every slot of the window) against the group
    arrays of the same windows' index builds: the stride is the batch's largest group count, a window's records equal its groups
    field for field (+ counts, valid word), and every slot behind its last group is zero"""
    lists = [solver.index_lists(w, opts, len(ws)) for w in ws]
    n_groups = [len(L["groups"]) for L in lists]
    for i, L in enumerate(lists):
        a = b.array("GROUP_RECS", i)
        assert a[0] == max(n_groups), (what, i, a[0], n_groups)
        recs = a[1:].astype(np.int64).reshape(max(n_groups), REC_INTS)
        assert np.array_equal(a[1:], recs.reshape(-1)), (what, i)   # (whole numbers)
        g = L["groups"].astype(np.int64)
        want = np.zeros_like(recs)
        want[:len(g), :16] = g
        want[:len(g), 16:20] = g[:, 1:8:2] - g[:, 0:8:2]
        want[:len(g), 20] = 1
        assert np.array_equal(recs, want), (what, i, np.argwhere(recs != want)[:4])
        assert len(g) == max(n_groups) or not recs[len(g):].any()
    return n_groups


REC_INTS = 32


def test_the_uploaded_records_after_upload_and_after_a_patch():
    """what the launch reads, read back from the device: mixed group counts in one batch (stride, tail slots), both legs (the
    records are built whichever kernel the plan selects), then a patched window (landmarks left and arrived: other lists)"""
    ws = _mixed()
    for leg in LEGS:
        b = solver.WindowBatch(ws, options=_opts("dogleg", LEGS[leg]))
        n = _check_device_records(b, ws, _opts("dogleg", LEGS[leg]), ("upload", leg))
        assert n == [34, 10, 4], n
        b.close()
    A, B = sliding_pair(seed=50, K=5, L=60)
    A2, _ = sliding_pair(seed=51, K=6, L=90)
    o = _opts("dogleg", 0)
    b = solver.WindowBatch([A.window(), A2.window()], options=o, patchable=True)
    before = _check_device_records(b, [A.window(), A2.window()], o, "before the patch")
    b.optimize(2)
    b.patch(0, patch_between(A, B))
    views = [b.patched_view(0), b.patched_view(1)]
    after = _check_device_records(b, views, o, "after the patch")
    assert views[0].n_lm != A.window().n_lm and len(before) == len(after) == 2, (before, after)   # (the patch changed the window's lists)
    b.close()


def test_a_batch_without_records_keeps_the_window_record_kernel():
    """free extrinsics: the batch is not on the piece path, gets no records, and nothing selects a record instantiation"""
    ws = [synthetic.make_window(4, 40, 1.0, 1, estimate_extrinsics="shared"), synthetic.small_window(seed=12, K=5, L=60)]
    b = solver.WindowBatch(ws, options=_opts("dogleg", 0))
    r = b.launch_route()
    assert r["piece_path"] == 0 and r["lin_records"] == 0, r
    assert b.array("GROUP_RECS", 0).tolist() == [0.0]
    sm = b.optimize(3)
    assert all(np.isfinite(x["final_cost"]) for x in sm)
    b.close()
    # a fused batch keeps linearize2_kernel too
    b = solver.WindowBatch(_mixed()[1:], options=default_options())
    r = b.launch_route()
    assert r["fused"] == 1 and r["lin_records"] == 0, r
    b.close()
