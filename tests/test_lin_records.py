"""The group launch records of linearize2_rec_kernel (build_group_records, capi_index_build.inc) against the group arrays they are
copied from: every record equals the Group record of the same index build field for field, carries the group's four counts and
the valid word, and is zero everywhere else.  Host only (okvis_ba_check_window_lists, a batch of one window).  okvis_ba_upload and
okvis_ba_patch_window need a device, so the records of an uploaded batch of several windows — the stride, the zero slots behind a
window's last group, the records after a patch — are read back from the device and held against the group arrays in
tests/test_gpu_lin_records.py (test_the_uploaded_records_after_upload_and_after_a_patch), next to the instantiation a batch
without records selects."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import default_options, set_options

REC_INTS, COUNTS, VALID, GROUP_INTS = 32, 16, 20, 16

# the windows of tests/test_launch_records.py: the bench window, missing pairs, a ragged last group, a small window, groups of two
# landmarks (many groups, many tasks per pose block)
CASES = {
    "bench_64": (lambda: synthetic.make_window(10, 400, 1.0, 20240923), 64, {}),
    "bench_1": (lambda: synthetic.make_window(10, 400, 1.0, 20240923), 1, {}),
    "sparse": (lambda: synthetic.make_window(6, 150, 0.5, 7), 3, {}),
    "ragged": (lambda: synthetic.make_window(10, 397, 1.0, 20240923), 64, {}),
    "small": (lambda: synthetic.small_window(seed=3, K=5, L=60), 3, {}),
    "groups_of_two": (lambda: synthetic.make_window(7, 90, 0.8, 5), 1, dict(tuning_group_lm=2, tuning_fused_max_windows=-1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_equal_the_group_arrays_field_for_field(name):
    make, n_windows, kw = CASES[name]
    w = make()
    L = solver.index_lists(w, set_options(default_options(), **kw), n_windows)
    recs, groups = L["group_recs"], L["groups"]
    assert L["piece_path"] == 1
    # (a batch of one window: the stride is its own group count, no slot behind the last group)
    assert recs.shape == (len(groups), REC_INTS) and groups.shape[1] == GROUP_INTS and len(groups) >= 1
    for g in range(len(groups)):
        want = np.zeros(REC_INTS, np.int32)
        want[:GROUP_INTS] = groups[g]
        lm0, lm1, ob0, ob1, pr0, pr1, tk0, tk1 = groups[g][:8]
        want[COUNTS:COUNTS + 4] = lm1 - lm0, ob1 - ob0, pr1 - pr0, tk1 - tk0
        want[VALID] = 1
        assert np.array_equal(recs[g], want), (name, g)
    n = recs[:, COUNTS:COUNTS + 4]
    assert (n[:, 0] > 0).all() and n[:, 0].sum() == w.n_lm and n[:, 1].sum() == w.n_obs
    assert n[:, 0].max() <= 64 and n[:, 1].max() <= 256 and n[:, 2].max() <= 128
    if name == "ragged":
        assert n[-1, 0] != n[0, 0]
    if name == "groups_of_two":
        assert len(groups) >= 45 and n[:, 0].max() == 2


def test_no_records_off_the_piece_path():
    """free extrinsics: the staged kernel (linearize_kernel) reads W.groups, and so does every instantiation of such a batch"""
    ext = synthetic.make_window(4, 40, 1.0, 1, estimate_extrinsics="shared")
    L = solver.index_lists(ext, default_options(), 1)
    assert L["piece_path"] == 0 and L["group_recs"].size == 0 and len(L["groups"]) > 0
