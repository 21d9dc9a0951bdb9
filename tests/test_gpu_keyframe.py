"""GPU: okvis_fe_keyframe_decision against its statement in exact arithmetic (tests/keyframe_statement.py) on the seeded cases of
tests/keyframe_cases.py.  Nothing here has a tolerance: keypoints are float, every quantity has an exact rational value.

  - hull index lists, sizes, n_matched, n_inside, flags and decision equal the statement's;
  - area_all, area_matched, overlap and ratio equal the statement's doubles bit for bit, NaN and inf included (bytes are compared);
  - the mixed batch equals the same jobs run one per call, byte for byte;
  - leaving out optional outputs changes none of the rest;
  - a call staged after a larger call of another entry on the same context equals the call on a fresh context.

The statement of every case is computed once per process (keyframe_cases.stated) and shared with tests/test_keyframe_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_cases as KC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


@pytest.mark.parametrize("name", KC.NAMES)
def test_every_output_equals_the_statement(fe, name):
    jobs, want = KC.cases(name), KC.stated(name)
    got = fe.keyframe_decision(jobs, want_hulls=True)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        KC.check(g, w, (name, j))


def raw(fe, jobs, leave_out=()):
    """the entry through the tables: every output array by name, filled from a byte pattern; those in leave_out passed as NULL"""
    kp, matched, images, table, counts = F.keyframe_job_table(jobs)
    out = F.keyframe_outputs(len(jobs), len(counts), sum(counts), True)
    for a in out.values():
        a.view(np.uint8)[...] = 0x5A
    fe._call("keyframe_decision", len(matched), kp.ctypes.data, matched.ctypes.data, len(counts), images, len(jobs), table,
             *[None if k in leave_out else out[k].ctypes.data for k in F.KF_OUTPUTS])
    return out


def same(x, y):
    return x.keys() == y.keys() and all(x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes() for k in x)


def test_the_mixed_batch_equals_its_jobs_one_per_call(fe):
    jobs = KC.cases("mixed")
    batch = fe.keyframe_decision(jobs, want_hulls=True)
    kinds = ("n_matched", "hull_all_size", "hull_matched_size", "area_all", "area_matched", "n_inside", "flags")
    for j, job in enumerate(jobs):
        one = fe.keyframe_decision([job], want_hulls=True)[0]
        b = batch[j]
        assert one["decision"] == b["decision"] and KC.bits(one["overlap"]) == KC.bits(b["overlap"]) and KC.bits(one["ratio"]) == KC.bits(b["ratio"]), j
        for c, (x, y) in enumerate(zip(one["images"], b["images"])):
            assert all(KC.bits(x[k]) == KC.bits(y[k]) for k in kinds), (j, c)
            assert x["hull_all"].tobytes() == y["hull_all"].tobytes() and x["hull_matched"].tobytes() == y["hull_matched"].tobytes(), (j, c)


def test_leaving_out_optional_outputs_changes_none_of_the_rest(fe):
    jobs = KC.cases("degenerate") + KC.cases("on_edges") + KC.cases("convex")[:2] + KC.cases("mixed")[:20]
    full = raw(fe, jobs)
    for name in F.KF_OUTPUTS:
        part = raw(fe, jobs, leave_out=(name,))
        assert (part[name].view(np.uint8) == 0x5A).all(), name
        for k in F.KF_OUTPUTS:
            if k != name:
                assert part[k].tobytes() == full[k].tobytes(), (name, k)
    # without the referees' lists the hulls are the kernel's working memory only: the same results come back
    part = raw(fe, jobs, leave_out=("hull_all", "hull_matched"))
    assert all(part[k].tobytes() == full[k].tobytes() for k in F.KF_OUTPUTS[:10])
    none = raw(fe, jobs, leave_out=F.KF_OUTPUTS)
    assert all((a.view(np.uint8) == 0x5A).all() for a in none.values())


def test_a_call_after_a_larger_call_of_another_entry_equals_a_fresh_context(fe):
    jobs = KC.cases("adversarial") + KC.cases("regular")[:4] + KC.cases("skips")
    fresh = F.Frontend()
    want = raw(fresh, jobs)
    fresh.close()
    used = F.Frontend()
    rng = np.random.default_rng(5)
    used.bearing_vectors(F.camera([450, 450, 376, 240, -0.28, 0.07, 1e-4, 1e-5], 1), rng.uniform(0, 400, (300000, 3)))   # 3.6 MB staged
    first = raw(used, jobs)
    used.keyframe_decision(KC.cases("limit"))                                                          # and a larger call of its own
    second = raw(used, jobs)
    used.close()
    assert same(first, want) and same(second, want)
