"""What the solver's host-view flags protect (HostView, okvis_amd/csrc/capi_solver.inc).

The invariant of a window w: okvis_ba_fetch_results(w) equals, byte for byte, okvis_ba_get_state(w) and the okvis_ba_download of
POSE, SB, LM, LM_QUALITY and IMU_SB_REF, and on a patchable solver okvis_ba_patched_view(w) holds the same pose, speed/bias and
landmarks.  A stale res_staged, acc_fresh or mirror_fresh breaks it without any error: one of the readers hands out the values of
an earlier call.  The invariant is asserted on every window after each step of a sequence that goes through every transition, on
a one-window solver (where okvis_ba_finish stages the results) and on a three-window batch of different shapes (where it does not).

The step "finish" found a defect: okvis_ba_patched_view between okvis_ba_begin and okvis_ba_finish left mirror_fresh set, and the
view behind okvis_ba_finish held the values of the middle of the call.  okvis_ba_iterate, the profiling hooks and okvis_ba_finish
clear the flag now (HostView::iterations_enqueued, finish_done).
"""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib, solver, synthetic
from okvis_amd.window import Patch
from tests import cov_cases as cc
from tests.test_gpu_marginalization import flags

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def invariant(b, what):
    """asserts the invariant on every window; returns the fetched results"""
    out = []
    for w in range(len(b)):
        r = b.fetch_results(w)
        pose, sb, lm = b.get_state(w)
        assert bits(r["pose"]) == bits(pose) and bits(r["sb"]) == bits(sb) and bits(r["lm"]) == bits(lm), (what, w, "get_state")
        for name, key in (("POSE", "pose"), ("SB", "sb"), ("LM", "lm"), ("LM_QUALITY", "quality"), ("IMU_SB_REF", "imu_sb_ref")):
            assert bits(b.array(name, w)) == bits(r[key]), (what, w, name)
        v = b.patched_view(w)
        assert bits(v.pose) == bits(pose) and bits(v.sb) == bits(sb) and bits(v.lm) == bits(lm), (what, w, "patched_view")
        assert bits(b.fetch_results(w)["pose"]) == bits(pose), (what, w, "second fetch")
        out.append(r)
    return out


def same_results(a, b, what):
    for w, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert bits(x[k]) == bits(y[k]), (what, w, k)


def sequence(b, w_cov, w_prior, w_marg):
    """every transition of the host view, the invariant behind each; w_cov: the window of the okvis_ba_state_covariance step,
    w_prior: a window with a marg_* prior (or None), w_marg: a window okvis_ba_marginalize takes (one without such a prior, or None)"""
    invariant(b, "upload")
    b.optimize(3)
    staged = invariant(b, "optimize: the staged-results shortcut")
    # values set by the caller: the fetch returns them, not the staging
    w = len(b) - 1
    pose, sb, lm = (a.copy() for a in b.get_state(w))
    pose[:, :3] += 0.01
    sb += 0.001
    lm[:, :3] += 0.02
    b.set_state(w, pose, sb, lm)
    r = invariant(b, "set_state")
    assert bits(r[w]["pose"]) == bits(pose) and bits(r[w]["sb"]) == bits(sb) and bits(r[w]["lm"]) == bits(lm), "set_state: the values set"
    assert bits(r[w]["pose"]) != bits(staged[w]["pose"])
    b.begin()
    b.iterate(2)
    moved = invariant(b, "begin + iterate without finish: the accepted-buffer index is read back")
    assert bits(moved[w]["pose"]) != bits(pose), "two iterations from perturbed values move the poses"
    b.finish()
    invariant(b, "finish")
    b.evaluate_cost()
    invariant(b, "evaluate_cost")
    b.optimize_timed(3, 1, 0.0)
    before = invariant(b, "optimize_timed with a zero time limit")
    if w_cov is not None:
        b.state_covariance(w0=w_cov, n=1)
        same_results(before, invariant(b, "state_covariance"), "state_covariance leaves every value as it was")
    if w_marg is not None:
        win = b.windows[w_marg]
        b.marginalize(w_marg, *flags(win, [0], [0]))
        invariant(b, "marginalize")
    if w_prior is not None:
        v = b.patched_view(w_prior)
        J, e0 = np.ascontiguousarray(np.asarray(v.marg_J, np.float64) * 1.5), np.ascontiguousarray(np.asarray(v.marg_e0, np.float64) + 0.125)
        _lib.check(b._L.okvis_ba_set_marg_prior_values(b._h, w_prior, J.ctypes.data_as(dp), e0.ctypes.data_as(dp)), "set_marg_prior_values")
        invariant(b, "set_marg_prior_values")
        v = b.patched_view(w_prior)
        assert bits(v.marg_J) == bits(J) and bits(v.marg_e0) == bits(e0), "the view holds the prior values that were set"
    # a value-only patch
    new_lm = np.asarray(b.get_state(0)[2][:1]) + 0.03
    b.patch(0, Patch(set_lm_idx=np.array([0], np.int32), set_lm=new_lm))
    r = invariant(b, "value-only patch")
    assert bits(r[0]["lm"][:1]) == bits(new_lm)
    # a patch that is rejected changes nothing
    with pytest.raises(_lib.BackendError):
        b.patch(0, Patch(set_lm_idx=np.array([b.windows[0].n_lm + 5], np.int32), set_lm=new_lm))
    same_results(r, invariant(b, "rejected patch"), "rejected patch")
    b.optimize(2)
    invariant(b, "optimize after the patches")


# cov_cases A is synthetic.small_window(seed=1, K=4, L=40); E is the same window with a dense marg_* prior (which okvis_ba_marginalize
# refuses and okvis_ba_set_marg_prior_values needs)
CASES = dict(A=(lambda: [cc.window("A")], 0, None, 0), E=(lambda: [cc.window("E")], 0, 0, None),
             three=(lambda: [cc.window("A"), cc.window("E"), synthetic.small_window(seed=2, K=3, L=25)], 0, 1, 0))


@pytest.mark.parametrize("case", list(CASES))
def test_readers_agree_after_every_step(case):
    windows, w_cov, w_prior, w_marg = CASES[case]
    b = solver.WindowBatch(windows(), patchable=True)
    try:
        sequence(b, w_cov, w_prior, w_marg)
    finally:
        b.close()
