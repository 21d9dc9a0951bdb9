"""The status of the solver's C-ABI entries (include/okvis_amd_ba.h), cell by cell: a null solver, a solver without an upload, an
uploaded idle solver, between okvis_ba_begin and okvis_ba_finish, between the halves of a marginalisation, a window index one
outside either end, and each required output pointer null.  Through the library itself, not the raising wrappers.

Every expected status is a literal read from the source (okvis_amd/csrc/ba_capi.hip and its parts), including the cells that do
not agree with their neighbours: okvis_ba_array_size, okvis_ba_download and okvis_ba_algorithmic_bytes answer ERR_ARG where the
others answer ERR_STATE for a solver without an upload; okvis_ba_reduced_dim, okvis_ba_pair_count and okvis_ba_pairs look at
neither the upload nor a pending marginalisation; null arguments come before the state in some entries and behind it in others.
No cell can fault the device: each returns before its first HIP call or is a valid call on a valid solver.  What
test_gpu_marginalize_batch.py::test_two_halves pins between the halves (optimize, get_state, the marginalisation entries) is not
repeated here; profiles/ba_entries_notes.md lists the cells that were left out.
"""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib, synthetic
from okvis_amd.window import Patch, SummaryC, WindowC, default_options, marg_marshal_batch
from tests.test_gpu_marginalization import flags

pytestmark = pytest.mark.gpu

OK, ARG, STATE = 0, -1, -2
POSE = 0          # OKVIS_BA_ARR_POSE
dp = C.POINTER(C.c_double)


class Ctx:
    """One patchable one-window solver and the arguments of every cell."""

    def __init__(self):
        self.L = _lib.lib()
        self.w = synthetic.small_window(seed=1, K=4, L=40)
        self.wc, self.keep_w = self.w.as_c()
        self.arr = (WindowC * 1)(self.wc)
        self.opt = default_options()
        self.sm = (SummaryC * 1)()
        self.d = np.zeros(8192)
        self.dptr = self.d.ctypes.data_as(dp)
        self.i32a, self.i32b = (C.c_int32 * 8192)(), (C.c_int32 * 8192)()
        self.i64 = C.c_int64()
        self.f4 = (C.c_float * 8)()
        self.route = (C.c_int32 * 64)()
        self.view = WindowC()
        self.patch, self.keep_p = Patch(set_lm_idx=np.array([0], np.int32), set_lm=np.asarray(self.w.lm, np.float64).reshape(-1, 4)[:1]).as_c()
        self.specs, self.results, self.outs, self.keep_m = marg_marshal_batch([(self.w.n_pose, self.w.n_sb)], [flags(self.w, [0], [0]) + (None,)])
        self.n_pose_doubles = 7 * self.w.n_pose

    def table(self, h, w=0):
        """entry -> a call with valid arguments on solver h and window w"""
        L, c = self.L, self
        return {
            "set_options": lambda: L.okvis_ba_set_options(h, C.byref(c.opt)),
            "upload": lambda: L.okvis_ba_upload(h, 1, c.arr),
            "patch_window": lambda: L.okvis_ba_patch_window(h, w, C.byref(c.patch)),
            "patched_view": lambda: L.okvis_ba_patched_view(h, w, C.byref(c.view)),
            "set_marg_prior_values": lambda: L.okvis_ba_set_marg_prior_values(h, w, c.dptr, c.dptr),
            "set_state": lambda: L.okvis_ba_set_state(h, w, None, None, None),
            "get_state": lambda: L.okvis_ba_get_state(h, w, None, None, None),
            "optimize": lambda: L.okvis_ba_optimize(h, 1, c.sm),
            "optimize_timed": lambda: L.okvis_ba_optimize_timed(h, 1, 1, -1.0, c.sm),
            "begin": lambda: L.okvis_ba_begin(h),
            "iterate": lambda: L.okvis_ba_iterate(h, 1),
            "finish": lambda: L.okvis_ba_finish(h, None),
            "evaluate_cost": lambda: L.okvis_ba_evaluate_cost(h, c.dptr),
            "fetch_results": lambda: L.okvis_ba_fetch_results(h, w, c.dptr, None, None, None, None),
            "fetch_imu_caches": lambda: L.okvis_ba_fetch_imu_caches(h, w, c.dptr),
            "array_size": lambda: L.okvis_ba_array_size(h, w, POSE, C.byref(c.i64)),
            "download": lambda: L.okvis_ba_download(h, w, POSE, c.dptr, c.n_pose_doubles),
            "reduced_dim": lambda: L.okvis_ba_reduced_dim(h, w, c.i32a),
            "pair_count": lambda: L.okvis_ba_pair_count(h, w, c.i32a),
            "pairs": lambda: L.okvis_ba_pairs(h, w, c.i32a, c.i32b),
            "profile_iterations": lambda: L.okvis_ba_profile_iterations(h, 1, c.f4),
            "profile_launches": lambda: L.okvis_ba_profile_launches(h, 1, c.f4),
            "algorithmic_bytes": lambda: L.okvis_ba_algorithmic_bytes(h, None, None, None, None),
            "synchronize": lambda: L.okvis_ba_synchronize(h),
            "helper_timeouts": lambda: L.okvis_ba_helper_timeouts(h, C.byref(c.i64)),
            "launch_route": lambda: L.okvis_ba_launch_route(h, c.route),
            "pause_count": lambda: L.okvis_ba_pause_count(h, C.byref(c.i64)),
            "marginalize": lambda: L.okvis_ba_marginalize(h, w, c.specs, c.results),
            "marginalize_begin": lambda: L.okvis_ba_marginalize_begin(h, w, c.specs, c.results),
            "marginalize_end": lambda: L.okvis_ba_marginalize_end(h, c.results),
            "marginalize_batch": lambda: L.okvis_ba_marginalize_batch(h, w, 1, c.specs, c.results),
            "marginalize_batch_begin": lambda: L.okvis_ba_marginalize_batch_begin(h, w, 1, c.specs, c.results),
            "marginalize_batch_end": lambda: L.okvis_ba_marginalize_batch_end(h, c.results),
        }


def run(cells, expected, prepare=None):
    seen = {}
    for name, want in expected.items():
        if prepare:
            prepare()
        seen[name] = cells[name]()
    assert seen == expected


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.h = C.c_void_p()
    assert c.L.okvis_ba_create(C.byref(c.h), 0) == OK
    assert c.L.okvis_ba_set_patchable(c.h, 1) == OK
    yield c
    assert c.L.okvis_ba_destroy(c.h) == OK


def test_null_solver(ctx):
    L = ctx.L
    assert L.okvis_ba_destroy(None) == OK
    assert L.okvis_ba_set_patchable(None, 1) == ARG
    assert L.okvis_ba_last_iterate_ms(None, ctx.f4) == ARG
    assert L.okvis_ba_state_covariance(None, 0, 1, None, None) == ARG
    assert L.okvis_ba_landmark_covariance(None, 0, 1, None, None) == ARG
    assert L.okvis_ba_predicted_measurement(None, 0, 1, None, None) == ARG
    assert L.okvis_ba_last_covariance_ms(None, ctx.f4, ctx.f4) == ARG
    assert L.okvis_ba_last_landmark_covariance_ms(None, ctx.f4, ctx.f4, ctx.f4) == ARG
    assert L.okvis_ba_last_predicted_measurement_ms(None, ctx.f4, ctx.f4, ctx.f4) == ARG
    cells = ctx.table(None)
    run(cells, {name: ARG for name in cells})


def test_created_without_an_upload(ctx):
    # (first in the module after the null solver: the fixture's solver has had no upload yet)
    run(ctx.table(ctx.h), dict(
        set_options=OK, patch_window=STATE, patched_view=STATE, set_marg_prior_values=STATE, set_state=STATE, get_state=STATE,
        optimize=STATE, optimize_timed=STATE, begin=STATE, iterate=STATE, finish=STATE, evaluate_cost=STATE, fetch_results=STATE,
        fetch_imu_caches=STATE, array_size=ARG, download=ARG, reduced_dim=ARG, pair_count=ARG, pairs=ARG, profile_iterations=STATE,
        profile_launches=STATE, algorithmic_bytes=ARG, synchronize=OK, helper_timeouts=STATE, launch_route=STATE, pause_count=STATE,
        marginalize=STATE, marginalize_begin=STATE, marginalize_end=STATE, marginalize_batch=STATE, marginalize_batch_begin=STATE,
        marginalize_batch_end=STATE))
    L, h = ctx.L, ctx.h
    # where a null argument meets the missing upload: the argument first, but for okvis_ba_fetch_imu_caches
    assert L.okvis_ba_fetch_imu_caches(h, 0, None) == STATE
    assert L.okvis_ba_patch_window(h, 0, None) == ARG
    assert L.okvis_ba_set_marg_prior_values(h, 0, None, ctx.dptr) == ARG
    assert L.okvis_ba_helper_timeouts(h, None) == ARG
    assert L.okvis_ba_upload(h, 1, ctx.arr) == OK   # (the tests below start from here)


def test_uploaded_and_idle(ctx):
    run(ctx.table(ctx.h), dict(
        set_options=OK, upload=OK, patched_view=OK, set_marg_prior_values=ARG,   # (the window has no prior: ERR_ARG before any HIP call)
        set_state=OK, get_state=OK, iterate=STATE, finish=STATE, profile_iterations=STATE, profile_launches=STATE, optimize=OK,
        optimize_timed=OK, evaluate_cost=OK, fetch_results=OK, fetch_imu_caches=OK, array_size=OK, download=OK, reduced_dim=OK,
        pair_count=OK, pairs=OK, algorithmic_bytes=OK, synchronize=OK, helper_timeouts=OK, launch_route=OK, pause_count=OK,
        patch_window=OK, marginalize_end=STATE, marginalize_batch_end=STATE, marginalize=OK, marginalize_batch=OK))
    L, h = ctx.L, ctx.h
    assert L.okvis_ba_last_iterate_ms(h, ctx.f4) == OK   # (behind the optimize above: both events have been recorded)
    assert L.okvis_ba_iterate(h, -1) == ARG              # the count before the state
    assert L.okvis_ba_profile_iterations(h, 0, ctx.f4) == ARG
    assert L.okvis_ba_optimize_timed(h, -1, 0, -1.0, ctx.sm) == ARG
    assert L.okvis_ba_array_size(h, 0, 1000, C.byref(ctx.i64)) == ARG
    assert L.okvis_ba_download(h, 0, POSE, ctx.dptr, ctx.n_pose_doubles + 1) == ARG


def test_window_index_outside(ctx):
    for w in (-1, 1):
        run(ctx.table(ctx.h, w), dict(
            patch_window=ARG, patched_view=ARG, set_marg_prior_values=ARG, set_state=ARG, get_state=ARG, fetch_results=ARG,
            fetch_imu_caches=ARG, array_size=ARG, download=ARG, reduced_dim=ARG, pair_count=ARG, pairs=ARG, marginalize=ARG,
            marginalize_begin=ARG, marginalize_batch=ARG, marginalize_batch_begin=ARG))


def test_null_output_pointers(ctx):
    L, h, c = ctx.L, ctx.h, ctx
    seen = dict(
        set_options=L.okvis_ba_set_options(h, None), upload_windows=L.okvis_ba_upload(h, 1, None), upload_count=L.okvis_ba_upload(h, 0, c.arr),
        patch_window=L.okvis_ba_patch_window(h, 0, None), patched_view=L.okvis_ba_patched_view(h, 0, None),
        marg_prior_J=L.okvis_ba_set_marg_prior_values(h, 0, None, c.dptr), marg_prior_e0=L.okvis_ba_set_marg_prior_values(h, 0, c.dptr, None),
        evaluate_cost=L.okvis_ba_evaluate_cost(h, None), fetch_imu_caches=L.okvis_ba_fetch_imu_caches(h, 0, None),
        fetch_imu_caches_outside=L.okvis_ba_fetch_imu_caches(h, 1, None),
        array_size=L.okvis_ba_array_size(h, 0, POSE, None), download=L.okvis_ba_download(h, 0, POSE, None, c.n_pose_doubles),
        reduced_dim=L.okvis_ba_reduced_dim(h, 0, None), pair_count=L.okvis_ba_pair_count(h, 0, None),
        pairs_lm=L.okvis_ba_pairs(h, 0, None, c.i32b), pairs_block=L.okvis_ba_pairs(h, 0, c.i32a, None),
        last_iterate_ms=L.okvis_ba_last_iterate_ms(h, None), profile_iterations=L.okvis_ba_profile_iterations(h, 1, None),
        profile_launches=L.okvis_ba_profile_launches(h, 1, None), helper_timeouts=L.okvis_ba_helper_timeouts(h, None),
        launch_route=L.okvis_ba_launch_route(h, None), pause_count=L.okvis_ba_pause_count(h, None),
        marginalize_spec=L.okvis_ba_marginalize(h, 0, None, c.results), marginalize_result=L.okvis_ba_marginalize(h, 0, c.specs, None),
        marginalize_end=L.okvis_ba_marginalize_end(h, None), marginalize_batch_end=L.okvis_ba_marginalize_batch_end(h, None))
    assert seen == {k: ARG for k in seen}
    # (pointers that may be null: the arrays of set_state / get_state / fetch_results, okvis_ba_finish's summaries,
    #  okvis_ba_algorithmic_bytes' four - test_uploaded_and_idle passes them as null)


def test_between_begin_and_finish(ctx):
    L, h = ctx.L, ctx.h
    # every cell starts from a fresh okvis_ba_begin: some entries end the begin ... finish they meet
    run(ctx.table(h), dict(
        set_options=OK, patched_view=OK, set_marg_prior_values=ARG, get_state=OK, fetch_results=OK, fetch_imu_caches=OK, array_size=OK,
        download=OK, reduced_dim=OK, pair_count=OK, pairs=OK, algorithmic_bytes=OK, synchronize=OK, helper_timeouts=OK, launch_route=OK,
        pause_count=OK, iterate=OK, profile_iterations=OK, profile_launches=OK, begin=OK, set_state=OK, evaluate_cost=OK, optimize=OK,
        finish=OK), prepare=lambda: L.okvis_ba_begin(h))
    assert L.okvis_ba_finish(h, None) == STATE   # (the finish above ended it)
    assert L.okvis_ba_begin(h) == OK
    assert L.okvis_ba_set_state(h, 0, None, None, None) == OK
    assert L.okvis_ba_iterate(h, 1) == STATE     # okvis_ba_set_state ends a begin ... finish
    assert L.okvis_ba_begin(h) == OK
    assert L.okvis_ba_iterate(h, 0) == OK
    assert L.okvis_ba_finish(h, ctx.sm) == OK


def test_between_the_halves_of_a_marginalisation(ctx):
    L, h, c = ctx.L, ctx.h, ctx
    assert L.okvis_ba_marginalize_begin(h, 0, c.specs, c.results) == OK
    run(ctx.table(h), dict(
        set_options=OK, patch_window=STATE, patched_view=STATE, set_marg_prior_values=STATE, set_state=STATE, optimize_timed=STATE,
        begin=STATE, iterate=STATE, finish=STATE, evaluate_cost=STATE, fetch_results=STATE, fetch_imu_caches=STATE, array_size=OK,
        download=STATE, reduced_dim=OK, pair_count=OK, pairs=OK, profile_iterations=STATE, profile_launches=STATE, algorithmic_bytes=OK,
        synchronize=OK, helper_timeouts=OK, launch_route=OK, pause_count=OK))
    # null arguments against the pending call: the pending call first where the entry asks for it first
    assert L.okvis_ba_patch_window(h, 0, None) == STATE
    assert L.okvis_ba_download(h, 0, POSE, None, c.n_pose_doubles) == STATE
    assert L.okvis_ba_fetch_imu_caches(h, 0, None) == STATE
    assert L.okvis_ba_set_state(h, -1, None, None, None) == STATE
    assert L.okvis_ba_set_marg_prior_values(h, 0, None, c.dptr) == ARG
    assert L.okvis_ba_set_marg_prior_values(h, -1, c.dptr, c.dptr) == STATE
    assert L.okvis_ba_iterate(h, -1) == STATE
    assert L.okvis_ba_upload(h, 1, c.arr) == STATE   # (last: a refused upload drops the containers of a patchable solver)
    assert L.okvis_ba_marginalize_end(h, c.results) == OK
    assert L.okvis_ba_patched_view(h, 0, C.byref(c.view)) == STATE   # ... which a new upload brings back
    assert L.okvis_ba_upload(h, 1, c.arr) == OK
    assert L.okvis_ba_patched_view(h, 0, C.byref(c.view)) == OK
