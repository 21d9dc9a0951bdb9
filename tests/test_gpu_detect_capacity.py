"""GPU: the selection core of both detect entries at the capacity of its slots.  The count families of tests/detect_cases.py stop
at 1025 candidates, two of a lane's eight slots; here detect_cases.dot_grid gives 8191, 8192 and 8193 candidates (a 639 x 639
image each) against cand_capacity 8192, so every lane of the selection workgroup holds eight, the last lane seven, or the job
overflows by one.  With min_dist 0 the 2048 strongest are taken and one more would have been (FULL); with min_dist 10 the grid's
neighbours (7 apart) suppress each other and the rounds run until nothing is left in play.

Each case goes through okvis_fe_detect_keypoints and, with octaves 0, through okvis_fe_detect_keypoints_scaled: both equal the
statement (tests/detect_statement.py) byte for byte, the score image included, both equal each other, and rows past n_keypoints
keep the pattern they were filled with.  Nothing here has a tolerance."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_cases as DC  # noqa: E402
import detect_scale_cases as SC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("threshold", "min_dist", "max_keypoints", "cand_capacity", "kp_size")
ROWS = ("kp", "response", "pixel")
# (n, min_dist) -> (candidates, keypoints, flags) of the statement; None: what the statement gives is not written down here
EXPECTED = {(8191, 0): (8191, 2048, F.DETECT_FULL), (8192, 0): (8192, 2048, F.DETECT_FULL), (8192, 10): (8192, 1801, 0),
            (8193, 0): (8193, 0, F.DETECT_OVERFLOW), (8193, 10): (8193, 0, F.DETECT_OVERFLOW), (8191, 10): None}


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def case(n, min_dist):
    image, _ = DC.dot_grid(n)
    assert image.shape == (639, 639)
    job = DC.job(image, 1, min_dist, F.DETECT_MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES)
    return job, DC.state(job)


def call(fe, entry, table, out):
    for a in out.values():
        if a is not None:
            a.view(np.uint8)[...] = 0x5A
    fe._call(entry, 1, table)
    return dict(out, record=np.array([table[0].n_keypoints, table[0].n_candidates, table[0].flags]))


@pytest.mark.parametrize("n,min_dist", sorted(EXPECTED))
def test_the_selection_at_the_capacity_of_its_slots(fe, n, min_dist):
    job, want = case(n, min_dist)
    assert F.DETECT_MAX_CANDIDATES == 8192 and F.DETECT_MAX_KEYPOINTS == 2048
    if EXPECTED[n, min_dist] is not None:
        assert (want["n_candidates"], len(want["kp"]), want["flags"]) == EXPECTED[n, min_dist]
    table, keep, (out,) = F.detect_job_table([job["image"]], *[[job[k]] for k in FIELDS], want_score=True)
    one = call(fe, "detect_keypoints", table, out)
    scaled = SC.as_scaled(job)
    table, keep, (out,) = F.detect_scale_job_table([scaled["image"]], *[[scaled[k]] for k in SC.FIELDS], want_score=True)
    two = call(fe, "detect_keypoints_scaled", table, out)
    rows = len(want["kp"])
    for name, got in (("detect_keypoints", one), ("detect_keypoints_scaled", two)):
        assert list(got["record"]) == [rows, want["n_candidates"], want["flags"]], (name, list(got["record"]))
        for k in ROWS:
            assert got[k][:rows].tobytes() == want[k].tobytes(), (name, k)
            assert (got[k][rows:].view(np.uint8) == 0x5A).all(), (name, k)                 # rows past n_keypoints are left alone
        assert got["score"].reshape(want["score"].shape).tobytes() == want["score"].tobytes(), name
    assert all(one[k].tobytes() == two[k].tobytes() for k in ROWS + ("score", "record"))
    assert table[0].n_layers == 1 and list(table[0].n_layer_candidates) == [want["n_candidates"], 0, 0, 0, 0]
    assert not two["layer"][:rows].any() and (two["layer"][rows:].view(np.uint8) == 0x5A).all()
