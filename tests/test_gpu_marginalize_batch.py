"""okvis_ba_marginalize_batch: a range of windows of one solver marginalised in one call.  The contract is bit-identity — on one and
the same uploaded solver the batched call returns, for every window, the bits okvis_ba_marginalize returns for that window (H, b0, J,
e0, dim, rank, sweeps, the block lists).  The single call is the range of one window of the same implementation (marg_begin,
capi_marginalize.inc), so np.array_equal here compares a launch over a range with launches of one window each: the helper workgroups
or none, a workgroup of a shared dense launch or a launch of its own, the place in the call's scratch block.  What anchors the numbers
themselves is independent of that: the oracle's MarginalizationError at the tolerances of tests/test_gpu_marginalization.py in every
case, and profiles/marg_digest_parent.json (tools/marg_digest.py: the bits of the commit that still had two implementations).  Shapes
are that file's: the smallest at which each branch of the dense tail is taken."""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import synthetic
from okvis_amd.window import SummaryC, Window, default_options, marg_marshal_batch, marg_unpack
from tests.test_gpu_marginalization import check, flags

pytestmark = pytest.mark.gpu

KEYS = ("dim", "rank", "sweeps", "block_type", "block_idx", "block_off", "H", "b0", "J", "e0")
ERR_ARG, ERR_STATE = -1, -2


def same_bits(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def observation_free(w):
    """the second-stage window of test_with_previous_prior_two_stage: the blocks of w, no landmark and no observation"""
    return Window(pose=w.pose, pose_fixed=w.pose_fixed, sb=w.sb, sb_fixed=w.sb_fixed, lm=np.zeros((0, 4)),
                  cam_intr=w.cam_intr, cam_model=w.cam_model, obs_lm=np.zeros(0, np.int32), obs_pose=np.zeros(0, np.int32),
                  obs_ext=np.zeros(0, np.int32), obs_cam=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)),
                  obs_sqrtw=np.zeros(0), imu_params=w.imu_params)


def rank_deficient_landmark(seed):
    """the window of test_rank_deficient_landmark: landmark 0 keeps one observation"""
    w = synthetic.small_window(seed=seed, K=3, L=12, visibility=1.0)
    first = np.flatnonzero(np.asarray(w.obs_lm) == 0)
    keep = np.setdiff1d(np.arange(w.n_obs), first[1:])
    for k in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_uv", "obs_sqrtw"):
        setattr(w, k, np.asarray(getattr(w, k))[keep])
    return w


def mixed_six(oracle, shift=0):
    """The six windows (seeds + shift where a window is generated) and their jobs (pose_marg, sb_marg, prior)."""
    ws, jobs = [], []
    w = synthetic.small_window(seed=41 + shift, K=5, L=40)                # a pose and two speed/bias blocks eliminated
    ws.append(w); jobs.append(flags(w, [0], [0, 1]) + (None,))
    w = synthetic.small_window(seed=42 + shift, K=4, L=30)                # landmarks only
    ws.append(w); jobs.append(flags(w) + (None,))
    w = synthetic.small_window(seed=43 + shift, K=4, L=30)                # a speed/bias block
    ws.append(w); jobs.append(flags(w, [], [0]) + (None,))
    r1 = oracle.OracleWindow(w).marginalize(*flags(w, [], [0]))           # ... whose result is the previous prior of the next one
    w2 = observation_free(w)
    ws.append(w2); jobs.append(flags(w2, [0], []) + (dict(block_type=r1["block_type"], block_idx=r1["block_idx"], H=r1["H"], b0=r1["b0"]),))
    w = synthetic.small_window(seed=51 + shift, K=5, L=40)                # no first-pose prior: the pivoted-Cholesky path
    w.pprior_pose = np.zeros(0, np.int32); w.pprior_meas = np.zeros((0, 7)); w.pprior_sqrtinfo = np.zeros((0, 36))
    ws.append(w); jobs.append(flags(w, [0], [0]) + (None,))
    w = rank_deficient_landmark(44 + shift)
    ws.append(w); jobs.append(flags(w, [0], [0]) + (None,))
    return ws, jobs


def with_marg_prior():
    """a window that carries a marg_* prior of its own: okvis_ba_marginalize refuses it (the previous prior comes in through the spec)"""
    w = synthetic.small_window(seed=47, K=3, L=20)
    rng = np.random.default_rng(47)
    w.marg_block_type, w.marg_block_idx, w.marg_block_off = (np.array(a, np.int32) for a in ([0, 1], [0, 0], [0, 6]))
    w.marg_J = np.triu(rng.standard_normal((15, 15))) * 3.0
    w.marg_e0 = rng.standard_normal(15) * 0.01
    w.marg_lin = np.array([np.r_[w.pose[0], 0, 0], w.sb[0]])
    return w


class Shared:
    pass


@pytest.fixture(scope="module")
def six(oracle):
    """One solver for the cases below: the mixed six as windows 0 .. 5 and, behind them, a window with a marg_* prior (window 6, for
    the error case).  The batched call comes first, then the single calls on the same solver; the oracle's results once."""
    from okvis_amd import solver
    S = Shared()
    S.ws, S.jobs = mixed_six(oracle)
    S.all = S.ws + [with_marg_prior()]
    S.b = solver.WindowBatch(S.all, options=default_options())
    S.route = S.b.launch_route()
    S.batch = S.b.marginalize_batch(0, S.jobs)
    S.single = [S.b.marginalize(i, *S.jobs[i]) for i in range(6)]
    S.oracle = [oracle.OracleWindow(w).marginalize(*j) for w, j in zip(S.ws, S.jobs)]
    yield S
    S.b.close()


def test_mixed_six_against_single_calls_and_the_oracle(six):
    assert len(six.batch) == 6
    for i in range(6):
        same_bits(six.batch[i], six.single[i], i)
        check(six.batch[i], six.oracle[i], 1e-9)
    assert six.batch[4]["sweeps"][1] == 0 and six.batch[4]["rank"] < six.batch[4]["dim"]     # the pivoted-Cholesky path
    assert six.batch[1]["dim"] == six.ws[1].reduced_dim()                                     # landmarks only: every block kept


def test_sub_range_and_one_window(six):
    b = six.b
    outside = (0, 1, 5, 6)
    before = [b.get_state(i) for i in outside]
    part = b.marginalize_batch(2, six.jobs[2:5])
    assert len(part) == 3
    for k in range(3):
        same_bits(part[k], six.single[2 + k], 2 + k)
    after = [b.get_state(i) for i in outside]
    for u, v in zip(before, after):
        for x, y in zip(u, v):
            assert np.array_equal(x, y)
    for i in (0, 3, 5):
        one = b.marginalize_batch(i, [six.jobs[i]])
        assert len(one) == 1
        same_bits(one[0], six.single[i], i)


@pytest.mark.parametrize("n_windows, separate, rides", [(9, False, False), (40, False, False), (40, True, True), (49, False, True)])
def test_plans(oracle, n_windows, separate, rides):
    """Solvers whose whole-batch extent has no helper workgroups (more than 8 windows): the batched call sums the Schur chunk
    partials inside the solving workgroup, the single calls have their helpers — the same order of additions, the same bits.  From 40
    windows on the IMU / prior factors have a launch of their own, and where the batch has a Schur launch their evaluation rides in
    it.  Under the default options 40 of these windows do not select that route: up to 48 windows a batch of windows this small is
    fused (the linearise launch reduces its groups, there is no Schur launch to ride in) whatever the windows are — the pose part
    would have to exceed the 63 rows the riding kernel takes.  So the riding route is visited twice besides: by the same 40 windows
    with the separate Schur launch kept (options.reserved0 bit 2, the switch of tests/test_gpu_separate_launch.py), and by 49
    windows under the default options, the route of every larger batch."""
    from okvis_amd import solver
    ws, jobs = [], []
    for c in range((n_windows + 5) // 6):
        w6, j6 = mixed_six(oracle, shift=100 * c)
        ws += w6; jobs += j6
    ws, jobs = ws[:n_windows], jobs[:n_windows]
    o = default_options()
    if separate:
        o.reserved0 = 4
    b = solver.WindowBatch(ws, options=o)
    route = b.launch_route()
    print("route", n_windows, separate, route)
    assert route["windows"] == n_windows > 8, route       # (SOLVE_HELPED_MAX_WINDOWS: the range's launches have no helpers)
    assert route["split_small"] == (1 if n_windows >= 40 else 0), route
    assert route["small_rides"] == (1 if rides else 0) and route["fused"] == (0 if rides else 1), route
    batch = b.marginalize_batch(0, jobs)
    for i in range(n_windows):
        same_bits(batch[i], b.marginalize(i, *jobs[i]), i)
    for i in (0, 1, n_windows - 1):
        check(batch[i], oracle.OracleWindow(ws[i]).marginalize(*jobs[i]), 1e-9)
    b.close()


def test_mixed_routes(oracle, six):
    """A window off the LDS route between two on it: D = 120 <= 174 but 105 kept rows > 96, the tiled tail (ba_marg_tiles.hpp),
    served inside the same call by the single call's code."""
    from okvis_amd import solver
    w = synthetic.small_window(seed=61, K=8, L=30)
    assert w.reduced_dim() == 120
    ws = [six.ws[0], w, six.ws[4]]
    jobs = [six.jobs[0], flags(w, [0], [0]) + (None,), six.jobs[4]]
    b = solver.WindowBatch(ws, options=default_options())
    batch = b.marginalize_batch(0, jobs)
    assert batch[1]["dim"] == 105
    for i in range(3):
        same_bits(batch[i], b.marginalize(i, *jobs[i]), i)
    check(batch[0], six.oracle[0], 1e-8)
    check(batch[1], oracle.OracleWindow(w).marginalize(*jobs[1]), 1e-8)
    check(batch[2], six.oracle[4], 1e-8)
    b.close()


def _gauge_deficient_tiled(oracle):
    """test_mixed_routes' window without its first-pose prior: 105 kept rows, singular along the gauge directions — the tiled route
    finds no proof of full rank and the single workgroup takes over (marg_tiles_fallback)"""
    w = synthetic.small_window(seed=61, K=8, L=30)
    w.pprior_pose = np.zeros(0, np.int32); w.pprior_meas = np.zeros((0, 7)); w.pprior_sqrtinfo = np.zeros((0, 36))
    return w, flags(w, [0], [0]) + (None,)


def _hbm_workspace(oracle):
    """test_window_beyond_the_lds_solve_path: D = 300, the system assembled in HBM, the large instantiation"""
    w = synthetic.make_window(20, 30, 1.0, 2, frame_dt=0.1)
    return w, flags(w, [0, 1], [0, 1]) + (None,)


def _prior_of_291_rows(oracle):
    """the second stage of test_previous_prior_of_more_than_192_rows: the large instantiation with a previous prior"""
    w = synthetic.make_window(20, 30, 1.0, 3, frame_dt=0.1)
    r1 = oracle.OracleWindow(w).marginalize(*flags(w, [], [0]))
    assert r1["dim"] == 291
    w2 = observation_free(w)
    return w2, flags(w2, [0], []) + (dict(block_type=r1["block_type"], block_idx=r1["block_idx"], H=r1["H"], b0=r1["b0"]),)


@pytest.mark.parametrize("case", [_gauge_deficient_tiled, _hbm_workspace, _prior_of_291_rows])
def test_off_the_lds_route_one_window_or_in_a_range(oracle, six, case):
    """A window off the LDS route between two on it: the single call, the batched call of that one window and the batched call of
    all three return the same bits, and they are the oracle's numbers."""
    from okvis_amd import solver
    w, job = case(oracle)
    ws, jobs = [six.ws[0], w, six.ws[4]], [six.jobs[0], job, six.jobs[4]]
    b = solver.WindowBatch(ws, options=default_options())
    single = b.marginalize(1, *job)
    one = b.marginalize_batch(1, [job])
    three = b.marginalize_batch(0, jobs)
    b.close()
    assert len(one) == 1 and len(three) == 3
    same_bits(one[0], single, "batch of one")
    same_bits(three[1], single, "inside a batch of three")
    check(single, oracle.OracleWindow(w).marginalize(*job), 1e-8)
    if case is _gauge_deficient_tiled:   # the tiled route ends only with a proof of full rank: the fall-back ran
        assert single["rank"] < single["dim"] and single["dim"] > 96, (single["rank"], single["dim"])


def test_two_halves(six):
    b = six.b
    L, h = b._L, b._h
    shapes = [(w.n_pose, w.n_sb) for w in six.ws]
    specs, results, outs, keep = marg_marshal_batch(shapes, six.jobs)
    assert L.okvis_ba_marginalize_batch_begin(h, 0, 6, specs, results) == 0
    # the kept blocks are known when _begin returns
    for i in range(6):
        assert results[i].dim == six.single[i]["dim"] and results[i].nblocks == len(six.single[i]["block_type"])
        assert np.array_equal(outs[i]["block_off"][:results[i].nblocks], six.single[i]["block_off"])
    # between the halves the solver takes no edits and hands out no results
    dp = C.POINTER(C.c_double)
    pose = np.zeros((six.ws[0].n_pose, 7))
    sm = (SummaryC * len(b))()
    seen = dict(optimize=L.okvis_ba_optimize(h, 1, sm), get_state=L.okvis_ba_get_state(h, 0, pose.ctypes.data_as(dp), None, None))
    s1, r1, o1, k1 = marg_marshal_batch(shapes[:1], six.jobs[:1])
    seen["marginalize"] = L.okvis_ba_marginalize(h, 0, s1, r1)
    seen["marginalize_begin"] = L.okvis_ba_marginalize_begin(h, 0, s1, r1)
    seen["marginalize_end"] = L.okvis_ba_marginalize_end(h, r1)
    seen["batch_begin"] = L.okvis_ba_marginalize_batch_begin(h, 0, 6, specs, results)
    assert all(v == ERR_STATE for v in seen.values()), seen
    # an _end with too little room in one result changes nothing: it can be repeated with room
    cap = results[3].capacity_dim
    results[3].capacity_dim = 1
    assert L.okvis_ba_marginalize_batch_end(h, results) == ERR_ARG
    results[3].capacity_dim = cap
    assert L.okvis_ba_marginalize_batch_end(h, results) == 0
    for i in range(6):
        same_bits(marg_unpack(results[i], outs[i]), six.batch[i], i)
    assert L.okvis_ba_marginalize_batch_end(h, results) == ERR_STATE      # nothing is pending any more
    # a pending single call refuses the batch entries the same way
    assert L.okvis_ba_marginalize_begin(h, 0, s1, r1) == 0
    assert L.okvis_ba_marginalize_batch_begin(h, 0, 6, specs, results) == ERR_STATE
    assert L.okvis_ba_marginalize_batch_end(h, results) == ERR_STATE
    assert L.okvis_ba_marginalize_end(h, r1) == 0
    same_bits(marg_unpack(r1[0], o1[0]), six.single[0], 0)
    del keep, k1


def _untouched(results, outs):
    for i, out in enumerate(outs):
        r = results[i]
        assert (r.dim, r.nblocks, r.rank, r.sweeps[0], r.sweeps[1]) == (0, 0, 0, 0, 0), i
        assert all(not np.any(a) for a in out.values()), i


def test_errors(six):
    b = six.b
    L, h = b._L, b._h
    shapes = [(w.n_pose, w.n_sb) for w in six.all]

    def call(w0, n, jobs, w_shapes, null=None, spoil=None):
        specs, results, outs, keep = marg_marshal_batch(w_shapes, jobs)
        if spoil:
            spoil(specs)
        rc = L.okvis_ba_marginalize_batch(h, w0, n, None if null == "specs" else specs, None if null == "results" else results)
        _untouched(results, outs)
        del keep
        return rc

    def afterwards():
        out = b.marginalize_batch(0, six.jobs)
        for i in range(6):
            same_bits(out[i], six.batch[i], i)

    def bad_offset(specs):
        specs[2].prior_block_off[1] += 1
    prior_job = six.jobs[3]
    jobs_bad = six.jobs[:2] + [prior_job] + six.jobs[3:]      # window 2 has window 3's blocks: the same prior fits it
    marg_job = flags(six.all[6]) + (None,)
    cases = [("n = 0", lambda: call(0, 0, six.jobs, shapes[:6])),
             ("range past the batch", lambda: call(2, 6, six.jobs, shapes[:6])),
             ("negative start", lambda: call(-1, 6, six.jobs, shapes[:6])),
             ("NULL specs", lambda: call(0, 6, six.jobs, shapes[:6], null="specs")),
             ("NULL results", lambda: call(0, 6, six.jobs, shapes[:6], null="results")),
             ("bad prior offset in specs[2] only", lambda: call(0, 6, jobs_bad, shapes[:6], spoil=bad_offset)),
             ("a window with a marg_* prior in the range", lambda: call(4, 3, six.jobs[4:6] + [marg_job], shapes[4:7]))]
    for what, f in cases:
        assert f() == ERR_ARG, what
        afterwards()
    # (the spoiled prior is a good one otherwise: without the edit the same call goes through)
    specs, results, outs, keep = marg_marshal_batch(shapes[:6], jobs_bad)
    assert L.okvis_ba_marginalize_batch(h, 0, 6, specs, results) == 0
    del keep
    specs, results, outs, keep = marg_marshal_batch(shapes[:6], six.jobs)
    assert L.okvis_ba_marginalize_batch(None, 0, 6, specs, results) == -1
    assert L.okvis_ba_marginalize_batch_begin(None, 0, 6, specs, results) == -1
    assert L.okvis_ba_marginalize_batch_end(None, results) == -1
    _untouched(results, outs)
    del keep
    afterwards()


def test_optimize_afterwards(six):
    """okvis_ba_marginalize_batch leaves the solver usable (the device's option record was never touched): optimize(3) behind it
    is a fresh solver's optimize(3) on the same windows."""
    from okvis_amd import solver
    b = solver.WindowBatch(six.all, options=default_options())
    out = b.marginalize_batch(0, six.jobs)
    for i in range(6):
        same_bits(out[i], six.batch[i], i)
    got = b.optimize(3)
    fresh = solver.WindowBatch(six.all, options=default_options())
    ref = fresh.optimize(3)
    for i in range(len(six.all)):
        assert (got[i]["iterations"], got[i]["successful_steps"]) == (ref[i]["iterations"], ref[i]["successful_steps"]), i
        assert got[i]["final_cost"] == ref[i]["final_cost"], (i, got[i]["final_cost"], ref[i]["final_cost"])
        for x, y in zip(b.get_state(i), fresh.get_state(i)):
            assert np.array_equal(x, y), i
    b.close()
    fresh.close()
