"""GPU: descriptor matching on the device.  okvis_fe_hamming_candidates against numpy (np.unpackbits of the XOR, order included),
okvis_fe_match_descriptors against the cases recorded from the reference's own DenseMatcher (tests/golden/dense_matcher.npz) and
against its sequential restatement (tests/matcher_statement.py) on larger inputs.  Everything is an integer or an integer held
in a float: all comparisons are exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matcher_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_matcher.npz")


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


def image(rng, base, n):
    """n descriptors as wide as `base`: base descriptors with a few flipped bits (half of them from a few popular ones), exact
    duplicates of earlier keypoints, and some that look like nothing else"""
    width = base.shape[1]
    out = np.zeros((n, width), np.uint8)
    for k in range(n):
        u = rng.random()
        if u < 0.08:
            out[k] = rng.integers(0, 256, width)
        elif u < 0.2 and k > 0:
            out[k] = out[rng.integers(0, k)]
        else:
            d = base[rng.integers(0, 8) if rng.random() < 0.5 else rng.integers(0, len(base))].copy()
            for _ in range(rng.integers(0, 5)):
                d[rng.integers(0, width)] ^= np.uint8(1 << rng.integers(0, 8))
            out[k] = d
    return out


def scene(seed, n_a, n_b, width=48, skipped=0.0, n_base=40):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_base, width)).astype(np.uint8)
    a, b = image(rng, base, n_a), image(rng, base, n_b)
    if skipped:
        return a, b, rng.random(n_a) < skipped, rng.random(n_b) < skipped
    return a, b, None, None


def golden_cases():
    g = np.load(GOLDEN)
    return [{k[len(f"c{i}_"):]: g[k] for k in g.files if k.startswith(f"c{i}_")} for i in range(int(g["n_cases"]))]


# ---------------------------------------------------------------- candidates

SIZES = [(0, 5), (5, 0), (0, 0), (1, 1), (63, 65), (64, 64), (65, 63), (1, 300), (300, 1), (400, 400)]


@pytest.mark.parametrize("width", [16, 32, 48, 64])
@pytest.mark.parametrize("skips", [False, True])
def test_candidates_equal_numpy(fe, width, skips):
    for k, (n_a, n_b) in enumerate(SIZES):
        a, b, sa, sb = scene(100 * width + k, n_a, n_b, width, 0.25 if skips else 0.0)
        for threshold in (width * 8 * 0.12, 4.5, 1.0, 1e9):   # a usual one, few pairs, exact duplicates only, every pair
            want_p, want_d = S.candidates(a, b, threshold, sa, sb)
            pairs, dist = fe.hamming_candidates(a, b, threshold, sa, sb)
            assert pairs.shape == want_p.shape, (n_a, n_b, threshold)
            assert (pairs == want_p).all() and (dist == want_d).all(), (n_a, n_b, threshold)
        if n_a * n_b >= 63 * 65:
            assert len(S.candidates(a, b, width * 8 * 0.12, sa, sb)[0]) > 0


@pytest.mark.parametrize("width,skips", [(48, True), (64, False)])
def test_candidates_large(fe, width, skips):
    a, b, sa, sb = scene(7, 3000, 2500, width, 0.1 if skips else 0.0, n_base=600)
    want_p, want_d = S.candidates(a, b, width * 8 * 0.1, sa, sb)
    pairs, dist = fe.hamming_candidates(a, b, width * 8 * 0.1, sa, sb)
    assert len(want_p) > 3000
    assert pairs.shape == want_p.shape and (pairs == want_p).all() and (dist == want_d).all()


def test_candidates_capacity_smaller_than_total(fe):
    a, b, sa, sb = scene(11, 400, 400, 48, 0.1)
    want_p, want_d = S.candidates(a, b, 60.0, sa, sb)
    total = len(want_p)
    assert total > 1000
    sa8, sb8 = np.ascontiguousarray(sa, np.uint8), np.ascontiguousarray(sb, np.uint8)
    for capacity in (0, 1, 63, 64, 65, 777, total - 1, total, total + 5):
        pairs = np.full((max(capacity, 1) + 1, 2), -7, np.int32)
        dist = np.full(max(capacity, 1) + 1, -7.0, np.float32)
        n = C.c_int32(-1)
        fe._call("hamming_candidates", 48, len(a), a.ctypes.data, sa8.ctypes.data, len(b), b.ctypes.data,
                 sb8.ctypes.data, 60.0, capacity, pairs.ctypes.data, dist.ctypes.data, C.byref(n))
        assert n.value == total
        k = min(capacity, total)
        assert (pairs[:k] == want_p[:k]).all() and (dist[:k] == want_d[:k]).all()
        assert (pairs[k:] == -7).all() and (dist[k:] == -7.0).all()      # nothing behind the prefix is touched
    # dist may be NULL
    pairs, n = np.zeros((total, 2), np.int32), C.c_int32(0)
    fe._call("hamming_candidates", 48, len(a), a.ctypes.data, sa8.ctypes.data, len(b), b.ctypes.data,
             sb8.ctypes.data, 60.0, total, pairs.ctypes.data, None, C.byref(n))
    assert n.value == total and (pairs == want_p).all()


def test_candidates_are_repeatable():
    a, b, sa, sb = scene(13, 700, 900, 48, 0.1)
    runs = []
    for _ in range(2):
        f = F.Frontend()
        runs.append(f.hamming_candidates(a, b, 55.0, sa, sb))
        runs.append(f.hamming_candidates(a, b, 55.0, sa, sb))
        f.close()
    for p, d in runs[1:]:
        assert (p == runs[0][0]).all() and (d == runs[0][1]).all()


# ---------------------------------------------------------------- the matcher

def expect(job, threshold, num_best, use_ratio, ratio):
    a, b = job[0], job[1]
    sa, sb = (job[2], job[3]) if len(job) > 2 else (None, None)
    pair_a, pair_dist, calls = S.match(a, b, threshold, num_best, use_ratio, ratio, sa, sb)
    return pair_a, pair_dist, S.accepted_mask(calls, len(b))


def same(got, want):
    return all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def test_match_equals_every_recorded_reference_case(fe):
    for i, c in enumerate(golden_cases()):
        (pair_a, pair_dist, accepted), = fe.match_descriptors([(c["desc_a"], c["desc_b"], c["skip_a"], c["skip_b"])], float(c["threshold"]),
                                                              int(c["num_best"]), bool(c["use_ratio"]), float(c["ratio_threshold"]))
        assert (pair_a == c["pair_a"]).all(), i
        assert (pair_dist == c["pair_dist"]).all(), i
        # the setBestMatch calls, in the order of the reference's final loop (ascending b)
        bs = np.nonzero(accepted)[0]
        assert np.stack([pair_a[bs], bs], 1).tolist() == c["calls_ab"].tolist(), i
        assert pair_dist[bs].astype(np.float64).tolist() == c["calls_dist"].tolist(), i


def test_recorded_cases_that_share_their_settings_in_one_batch(fe):
    cases = golden_cases()
    for settings in {(float(c["threshold"]), int(c["num_best"]), bool(c["use_ratio"]), float(c["ratio_threshold"])) for c in cases}:
        # every case under these settings, its own expectation only where the settings are its own
        out = fe.match_descriptors([(c["desc_a"], c["desc_b"], c["skip_a"], c["skip_b"]) for c in cases], *settings)
        for c, (pair_a, pair_dist, accepted) in zip(cases, out):
            if (float(c["threshold"]), int(c["num_best"]), bool(c["use_ratio"]), float(c["ratio_threshold"])) == settings:
                assert (pair_a == c["pair_a"]).all() and (pair_dist == c["pair_dist"]).all()
                assert np.nonzero(accepted)[0].tolist() == c["calls_ab"][:, 1].tolist()


@pytest.mark.parametrize("num_best", range(1, 9))
@pytest.mark.parametrize("use_ratio", [False, True])
def test_match_equals_statement(fe, num_best, use_ratio):
    if use_ratio and num_best < 2:
        with pytest.raises(_lib.BackendError):   # the rule reads list entry 1
            fe.match_descriptors([scene(1, 8, 8)[:2]], 60.0, num_best, True, 1.2)
        return
    n_a, n_b = 1000 + 37 * num_best, 1300 - 41 * num_best
    job = scene(300 + num_best + 10 * use_ratio, n_a, n_b, 48, 0.1 if num_best % 2 else 0.0)
    threshold, ratio = (60.0, 1.25) if num_best % 3 else (35.5, 1.0)
    want = expect(job, threshold, num_best, use_ratio, ratio)
    got, = fe.match_descriptors([job], threshold, num_best, use_ratio, ratio)
    assert same(got, want)
    assert (want[0] >= 0).sum() > 40 and want[2].sum() > 40          # the case is not an empty one


@pytest.mark.parametrize("width", [16, 32, 64])
def test_match_other_descriptor_lengths(fe, width):
    job = scene(40 + width, 330, 290, width, 0.1)
    for use_ratio in (False, True):
        want = expect(job, width * 8 * 0.15, 4, use_ratio, 1.3)
        got, = fe.match_descriptors([job], width * 8 * 0.15, 4, use_ratio, 1.3)
        assert same(got, want)


def test_batch_of_mixed_sizes_equals_each_job_alone(fe):
    shapes = [(400, 400), (1, 1), (0, 7), (63, 65), (5, 0), (64, 64), (257, 513), (65, 63), (3, 700), (700, 3), (0, 0), (400, 380)]
    jobs = [scene(500 + k, n_a, n_b, 48, 0.15 if k % 2 else 0.0) for k, (n_a, n_b) in enumerate(shapes)]
    for num_best, use_ratio in ((4, False), (3, True)):
        batch = fe.match_descriptors(jobs, 60.0, num_best, use_ratio, 1.2)
        assert len(batch) == len(jobs)
        for job, got in zip(jobs, batch):
            alone, = fe.match_descriptors([job], 60.0, num_best, use_ratio, 1.2)
            assert same(got, alone)
            assert same(got, expect(job, 60.0, num_best, use_ratio, 1.2))
    assert fe.match_descriptors([], 60.0) == []


def test_second_call_after_the_staging_block_grew():
    f = F.Frontend()                      # a context of its own: its staging block starts empty
    small = scene(21, 90, 80)             # fits the first block
    large = [scene(22 + k, 900, 1100, 64) for k in range(3)]
    first, = f.match_descriptors([small], 60.0, 4, True, 1.2)
    cand_first = f.hamming_candidates(small[0], small[1], 60.0)
    big = f.match_descriptors(large, 80.0, 4)
    again, = f.match_descriptors([small], 60.0, 4, True, 1.2)
    cand_again = f.hamming_candidates(small[0], small[1], 60.0)
    big_again = f.match_descriptors(large, 80.0, 4)
    f.close()
    assert same(first, again) and same(first, expect(small, 60.0, 4, True, 1.2))
    assert same(cand_first, cand_again)
    for x, y in zip(big, big_again):
        assert same(x, y)
    assert same(big[0], expect(large[0], 80.0, 4, False, 0.0))
