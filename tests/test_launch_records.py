"""The chunk launch records of the matrix-core Schur kernel's ring loop (build_chunk_records, capi_index_build.inc) against the
lists they are gathered from: every field of every record equals chunk_desc / chunk_diag_begin / chunk_diag_out of the same index
build, everything else in a record is zero.  Host only (okvis_ba_check_window_lists)."""
import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import default_options, set_options

REC_INTS, REC_LISTS, REC_LL, DESC_INTS = 128, 32, 6, 20

# (window, batch size the chunks are sized for, options): the bench window at 48 / 16 landmarks per chunk; missing pairs; a last chunk
# that is no multiple of 4; a pose part of 24 rows; groups of two landmarks = lists of 8 and 24 partials per pose block (a small batch
# fuses by default, and then a chunk is one group: tuning.fused_max_windows = -1 keeps the Schur launch and its chunks of 16)
CASES = {
    "bench_64": (lambda: synthetic.make_window(10, 400, 1.0, 20240923), 64, {}),
    "bench_1": (lambda: synthetic.make_window(10, 400, 1.0, 20240923), 1, {}),
    "sparse": (lambda: synthetic.make_window(6, 150, 0.5, 7), 3, {}),
    "ragged": (lambda: synthetic.make_window(10, 397, 1.0, 20240923), 64, {}),
    "small": (lambda: synthetic.small_window(seed=3, K=5, L=60), 3, {}),
    "long_lists_16": (lambda: synthetic.make_window(7, 90, 0.8, 5), 1, dict(tuning_group_lm=2, tuning_fused_max_windows=-1)),
    "long_lists_48": (lambda: synthetic.make_window(10, 400, 1.0, 20240923), 64, dict(tuning_group_lm=2)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_equal_the_lists_they_are_gathered_from(name):
    make, n_windows, kw = CASES[name]
    w = make()
    L = solver.index_lists(w, set_options(default_options(), **kw), n_windows)
    recs, desc, begin, out = L["chunk_recs"], L["chunk_desc"].reshape(-1, DESC_INTS), L["chunk_diag_begin"], L["chunk_diag_out"]
    n_chunk = len(L["chunks"])
    nb = (len(begin) - 1) // n_chunk
    assert recs.shape == (n_chunk, REC_INTS) and n_chunk > 1 and 1 <= nb <= (REC_INTS - REC_LISTS) // 8
    longest = 0
    for c in range(n_chunk):
        want = np.zeros(REC_INTS, np.int32)
        want[:DESC_INTS] = desc[c]
        for b in range(nb):
            q0, q1 = begin[c * nb + b], begin[c * nb + b + 1]
            head = out[q0:min(q1, q0 + REC_LL)]
            want[REC_LISTS + 8 * b:REC_LISTS + 8 * b + 2] = q0, q1 - q0
            want[REC_LISTS + 8 * b + 2:REC_LISTS + 8 * b + 2 + len(head)] = head
            longest = max(longest, q1 - q0)
        assert np.array_equal(recs[c], want), (name, c)
    nl = desc[:, 1] - desc[:, 0]
    assert (nl > 0).all() and nl.sum() == w.n_lm
    if name.startswith("long_lists"):
        assert longest > REC_LL, longest                 # the kernel walks the rest of such a list in chunk_diag_out
    else:
        assert longest <= REC_LL, longest
    if name == "ragged":
        assert (nl % 4 != 0).any()
    if name == "sparse":
        pairs = np.diff(desc[:, 2:19], axis=1)
        assert (pairs[:, 0] < 4 * nb).any()              # a stage of four landmarks with a missing (landmark, block) pair


def test_no_records_where_the_ring_loop_does_not_serve():
    """free extrinsics (pose x extrinsics cross blocks: schur_kernel) and pose parts beyond 63 rows (the serial loop's tiles)"""
    ext = synthetic.make_window(4, 40, 1.0, 1, estimate_extrinsics="shared")
    wide = synthetic.make_window(12, 60, 1.0, 1)
    for w in (ext, wide):
        L = solver.index_lists(w, default_options(), 1)
        assert L["chunk_recs"].size == 0 and len(L["chunks"]) > 0
