"""GPU: okvis_fe_detect_keypoints against its statement (tests/detect_statement.py) on the seeded cases of tests/detect_cases.py.
Nothing here has a tolerance: images are 8-bit, scores are integers, a sub-pixel offset is one IEEE division and one addition.

  - kp, response, pixel, n_keypoints, n_candidates, flags and the whole score image equal the statement's bytes on every case;
  - the mixed batch of 130 jobs equals its jobs run one per call, and two runs of the batch are equal (the candidate list's order
    in memory, which differs from run to run, reaches no output);
  - leaving out each optional output changes none of the others: without the score image the rest is unchanged (the production
    path is the tested path);
  - a call after a larger call of another entry on the same context equals a fresh context;
  - whole-pixel shifts of the image shift the keypoints by exactly that;
  - on a scene of rectangles every corner has a keypoint within a pixel and every keypoint lies within a pixel of a corner.

The statement of every case is computed once per process (detect_cases.stated) and shared with tests/test_detect_host.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_cases as DC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("threshold", "min_dist", "max_keypoints", "cand_capacity", "kp_size")


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


def run(fe, jobs, want_score=True):
    return fe.detect_keypoints([j["image"] for j in jobs], *[[j[k] for j in jobs] for k in FIELDS], want_score=want_score)


def raw(fe, jobs, leave_out=(), want_score=True):
    """the entry through the table: the record's three results and every output array per job, filled from a byte pattern before
    the call; those in leave_out passed as NULL"""
    table, keep, out = F.detect_job_table([j["image"] for j in jobs], *[[j[k] for j in jobs] for k in FIELDS], want_score=want_score,
                                          leave_out=leave_out)
    for o in out:
        for a in o.values():
            if a is not None:
                a.view(np.uint8)[...] = 0x5A
    fe._call("detect_keypoints", len(jobs), table)
    return [dict(o, record=np.array([table[j].n_keypoints, table[j].n_candidates, table[j].flags])) for j, o in enumerate(out)]


def same(x, y, skip=()):
    return len(x) == len(y) and all(a[k].tobytes() == b[k].tobytes() for a, b in zip(x, y) for k in a if k not in skip and a[k] is not None)


@pytest.mark.parametrize("name", DC.NAMES)
def test_every_output_equals_the_statement(fe, name):
    jobs, want = DC.cases(name), DC.stated(name)
    got = run(fe, jobs)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        DC.check(g, w, (name, j))


def test_the_mixed_batch_equals_its_jobs_one_per_call_and_itself(fe):
    jobs = DC.cases("mixed")
    batch = raw(fe, jobs)
    again = raw(fe, jobs)
    assert same(batch, again)
    for j, job in enumerate(jobs):
        assert same(raw(fe, [job]), batch[j:j + 1]), j


def test_rows_past_n_keypoints_are_left_alone(fe):
    for o in raw(fe, DC.cases("selection") + DC.cases("capacity")):
        n = o["record"][0]
        assert all((o[k][n:].view(np.uint8) == 0x5A).all() for k in ("kp", "response", "pixel"))


def test_leaving_out_optional_outputs_changes_none_of_the_rest(fe):
    jobs = DC.cases("ties") + DC.cases("selection") + DC.cases("capacity") + DC.cases("mixed")[:20]
    full = raw(fe, jobs)
    for name in ("response", "pixel", "score"):
        part = raw(fe, jobs, leave_out=(name,))
        assert all(o[name] is None for o in part) and same(part, full, skip=(name,)), name
    assert same(raw(fe, jobs, leave_out=("response", "pixel", "score")), full, skip=("response", "pixel", "score"))
    assert same(raw(fe, jobs, want_score=False), full, skip=("score",))           # the production path


def test_a_call_after_a_larger_call_of_another_entry_equals_a_fresh_context(fe):
    jobs = DC.cases("edges") + DC.cases("selection") + DC.cases("mixed")[:10]
    fresh = F.Frontend()
    want = raw(fresh, jobs)
    fresh.close()
    used = F.Frontend()
    rng = np.random.default_rng(5)
    used.bearing_vectors(F.camera([450, 450, 376, 240, -0.28, 0.07, 1e-4, 1e-5], 1), rng.uniform(0, 400, (300000, 3)))   # 3.6 MB staged
    first = raw(used, jobs)
    run(used, DC.cases("counts"))                                                  # and a larger call of its own
    second = raw(used, jobs)
    used.close()
    assert same(first, want) and same(second, want)


def test_whole_pixel_shifts_shift_the_keypoints_by_exactly_that(fe):
    got = run(fe, [DC.translated(dx, dy) for dx, dy in DC.SHIFTS])
    assert len(got[0]["kp"]) >= 10
    for (dx, dy), g in zip(DC.SHIFTS[1:], got[1:]):
        DC.check_shifted(g, got[0], dx, dy)


def test_rectangle_corners_are_found_and_nothing_else(fe):
    scenes = [DC.scene(seed, noise) for seed in DC.SCENE_SEEDS for noise in (False, True)]
    got = run(fe, [j for j, _ in scenes], want_score=False)
    for (j, corners), g in zip(scenes, got):
        assert g["flags"] == 0 and len(g["kp"]) >= len(corners) == 20
        assert DC.scene_holds(DC.pixels(g), corners)
        assert (np.abs(g["kp"][:, :2] - g["pixel"]) <= 0.5).all() and (g["kp"][:, 2] == np.float32(j["kp_size"])).all()


def test_the_longest_sides_the_header_allows(fe):
    """8192 x 5 and 5 x 8192 (one row and one column of scores): the keys' halves at their largest, 128 and 512 tiles in a line"""
    jobs = [DC.job(DC.uniform(70, F.DETECT_MAX_DIM, 5), 1, 9, F.DETECT_MAX_KEYPOINTS), DC.job(DC.uniform(71, 5, F.DETECT_MAX_DIM), 1, 9, F.DETECT_MAX_KEYPOINTS)]
    for j, (g, job) in enumerate(zip(run(fe, jobs), jobs)):
        want = DC.state(job)
        assert want["n_candidates"] > 500 and want["pixel"].max() > F.DETECT_MAX_DIM - 20
        DC.check(g, want, ("longest", j))
