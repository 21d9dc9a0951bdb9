"""CPU: the descriptor matcher's boundary (okvis_fe_hamming_candidates, okvis_fe_match_descriptors) and its referee.  The statement
(tests/matcher_statement.py) reproduces every case recorded from the reference's own DenseMatcher (tests/golden/dense_matcher.npz)
exactly; both entries are exported; a NULL context and every argument outside the documented limits is OKVIS_BA_ERR_ARG before
the device is touched (there is none here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matcher_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_matcher.npz")


def golden_cases():
    g = np.load(GOLDEN)
    return [{k[len(f"c{i}_"):]: g[k] for k in g.files if k.startswith(f"c{i}_")} for i in range(int(g["n_cases"]))]


def test_fixture_is_what_the_issue_asks_for():
    cases = golden_cases()
    assert len(cases) >= 6
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
                                          for f in ("factors.npz", "marginalization.npz", "windows.npz"))
    for c in cases:
        assert c["desc_a"].shape[1] == c["desc_b"].shape[1] == 48 and c["desc_a"].dtype == np.uint8
        assert len(c["desc_a"]) <= 300 and len(c["desc_b"]) <= 300
    assert {int(c["use_ratio"]) for c in cases} == {0, 1}


@pytest.mark.parametrize("i", range(6))
def test_statement_reproduces_the_recorded_reference_run(i):
    c = golden_cases()[i]
    ev = {}
    pair_a, pair_dist, calls = S.match(c["desc_a"], c["desc_b"], c["threshold"], int(c["num_best"]), bool(c["use_ratio"]),
                                       c["ratio_threshold"], c["skip_a"], c["skip_b"], events=ev)
    assert (pair_a == c["pair_a"]).all()
    assert (pair_dist == c["pair_dist"]).all()
    assert [(a, b) for a, b, _ in calls] == [tuple(r) for r in c["calls_ab"].tolist()]
    assert [d for _, _, d in calls] == c["calls_dist"].tolist()
    # the tie rules were under test when this case was recorded
    assert ev["rows_with_equal_kept"] >= 1 and ev["equal_to_last_turned_away"] >= 1 and ev["max_chain_depth"] >= 2


def test_statement_candidates_are_the_double_loop():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (9, 16)).astype(np.uint8), rng.integers(0, 256, (7, 16)).astype(np.uint8)
    b[3] = a[2]
    sa, sb = np.zeros(9, bool), np.zeros(7, bool)
    sa[4] = sb[0] = True
    want = []
    for i in range(9):
        for j in range(7):
            d = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a[i], b[j]))
            if not sa[i] and not sb[j] and float(d) < 62.5:
                want.append((i, j, d))
    pairs, dist = S.candidates(a, b, 62.5, sa, sb)
    assert [tuple(p) for p in pairs.tolist()] == [(i, j) for i, j, _ in want] and dist.tolist() == [float(d) for _, _, d in want]
    assert (2, 3, 0) in want


def test_library_exports_both_entries():
    L = _lib.lib()
    for s in ("okvis_fe_hamming_candidates", "okvis_fe_match_descriptors"):
        assert s in F.SYMBOLS
        getattr(L, s)


def _lib_declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _job(n_a=4, n_b=4, width=48):
    keep = [np.zeros((max(n_a, 1), width), np.uint8), np.zeros((max(n_b, 1), width), np.uint8), np.zeros(max(n_b, 1), np.int32),
            np.zeros(max(n_b, 1), np.float32), np.zeros(max(n_b, 1), np.uint8)]
    j = F.MatchJobC()
    j.n_a, j.n_b = n_a, n_b
    j.desc_a, j.desc_b = keep[0].ctypes.data, keep[1].ctypes.data
    j.pair_a, j.pair_dist, j.accepted = keep[2].ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data
    return j, keep


def test_null_context_is_an_argument_error():
    L = _lib_declared()
    d = np.zeros((4, 48), np.uint8)
    pairs, n = np.zeros((8, 2), np.int32), C.c_int32(7)
    assert L.okvis_fe_hamming_candidates(None, 48, 4, d.ctypes.data, None, 4, d.ctypes.data, None, 10.0, 8, pairs.ctypes.data, None,
                                         C.byref(n)) == ERR_ARG
    j, keep = _job()
    assert L.okvis_fe_match_descriptors(None, 1, C.byref(j), 48, 10.0, 4, 0, 0.0) == ERR_ARG
    assert L.okvis_fe_match_descriptors(None, 0, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG


# Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros.
@pytest.fixture
def fake_ctx():
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


@pytest.mark.parametrize("desc_bytes,n_a,n_b", [(0, 4, 4), (8, 4, 4), (24, 4, 4), (47, 4, 4), (80, 4, 4), (-48, 4, 4), (48, -1, 4),
                                                (48, 4, -1), (48, 65537, 4), (48, 4, 65537)])
def test_candidates_bad_arguments(fake_ctx, desc_bytes, n_a, n_b):
    L = _lib_declared()
    d = np.zeros((4, 64), np.uint8)
    pairs, n = np.zeros((8, 2), np.int32), C.c_int32(0)
    assert L.okvis_fe_hamming_candidates(fake_ctx[0], desc_bytes, n_a, d.ctypes.data, None, n_b, d.ctypes.data, None, 10.0, 8,
                                         pairs.ctypes.data, None, C.byref(n)) == ERR_ARG


@pytest.mark.parametrize("desc_bytes,n_a,n_b,num_best,use_ratio", [(0, 4, 4, 4, 0), (8, 4, 4, 4, 0), (40, 4, 4, 4, 0), (128, 4, 4, 4, 0),
                                                                   (48, -1, 4, 4, 0), (48, 4, -1, 4, 0), (48, 65537, 4, 4, 0),
                                                                   (48, 4, 65537, 4, 0), (48, 4, 4, 0, 0), (48, 4, 4, 9, 0),
                                                                   (48, 4, 4, -1, 0), (48, 4, 4, 1, 1)])
def test_match_bad_arguments(fake_ctx, desc_bytes, n_a, n_b, num_best, use_ratio):
    L = _lib_declared()
    j, keep = _job(4, 4, 64)
    j.n_a, j.n_b = n_a, n_b
    assert L.okvis_fe_match_descriptors(fake_ctx[0], 1, C.byref(j), desc_bytes, 10.0, num_best, use_ratio, 1.2) == ERR_ARG


def test_match_negative_job_count(fake_ctx):
    L = _lib_declared()
    assert L.okvis_fe_match_descriptors(fake_ctx[0], -1, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG
    assert L.okvis_fe_match_descriptors(fake_ctx[0], 1, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG
