"""GPU: okvis_fe_detect_keypoints_scaled and okvis_fe_detect_scaled_and_describe against their statement
(tests/detect_scale_statement.py) on the seeded cases of tests/detect_scale_cases.py.  Nothing here has a tolerance: images are
8-bit, scores are integers, scale and position are a handful of IEEE operations.

  - with octaves = 0 every family of tests/detect_cases.py gives, through the new entry, the one-layer entry's bytes;
  - kp, response, pixel, layer, scale, the counts, flags, every layer's score image and every layer's pixels equal the statement's
    on every family;
  - the mixed batch of 130 jobs equals its jobs run one per call, and two runs of the batch are equal (the order of the candidate
    and survivor lists in memory, which differs from run to run, reaches no output);
  - rows past n_keypoints are left alone; leaving out each optional output changes none of the others;
  - a call after a larger call of another entry on the same context equals a fresh context;
  - okvis_fe_detect_scaled_and_describe equals the two calls in sequence byte for byte, OVERFLOW jobs included.

The statement of every case is computed once per process (detect_scale_cases.stated) and shared with
tests/test_detect_scale_host.py."""
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
OLD_FIELDS = ("threshold", "min_dist", "max_keypoints", "cand_capacity", "kp_size")
REFEREE = ("scale", "score", "pyramid")


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


def args(jobs):
    return [[j["image"] for j in jobs]] + [[j[k] for j in jobs] for k in SC.FIELDS]


def run(fe, jobs, referee=True):
    return fe.detect_keypoints_scaled(*args(jobs), want_score=referee, want_pyramid=referee, want_scale=referee)


def table_of(jobs, leave_out=(), referee=True):
    table, keep, out = F.detect_scale_job_table(*args(jobs), want_score=referee, want_pyramid=referee, want_scale=referee, leave_out=leave_out)
    for o in out:
        for a in o.values():
            if a is not None:
                a.view(np.uint8)[...] = 0x5A
    return table, keep, out


def record(table, j):
    t = table[j]
    return np.array([t.n_keypoints, t.n_candidates, t.flags, t.n_layers] + list(t.n_layer_candidates))


def raw(fe, jobs, leave_out=(), referee=True):
    """the entry through the table: the record's results and every output array per job, filled from a byte pattern before the
    call; those in leave_out passed as NULL"""
    table, keep, out = table_of(jobs, leave_out, referee)
    fe._call("detect_keypoints_scaled", len(jobs), table)
    return [dict(o, record=record(table, j)) for j, o in enumerate(out)]


def same(x, y, skip=()):
    return len(x) == len(y) and all(a[k].tobytes() == b[k].tobytes() for a, b in zip(x, y) for k in a if k not in skip and a[k] is not None)


@pytest.mark.parametrize("name", DC.NAMES)
def test_octaves_0_gives_the_one_layer_entrys_bytes(fe, name):
    jobs = DC.cases(name)
    old_table, keep, old = F.detect_job_table([j["image"] for j in jobs], *[[j[k] for j in jobs] for k in OLD_FIELDS], want_score=True)
    for o in old:
        for a in o.values():
            a.view(np.uint8)[...] = 0x5A
    fe._call("detect_keypoints", len(jobs), old_table)
    new = raw(fe, [SC.as_scaled(j) for j in jobs])
    assert len(new) == len(old) > 0
    for j, (n, o) in enumerate(zip(new, old)):
        assert list(n["record"][:3]) == [old_table[j].n_keypoints, old_table[j].n_candidates, old_table[j].flags], (name, j)
        assert n["record"][3] == 1 and not n["record"][5:].any()
        assert n["record"][4] == old_table[j].n_candidates                     # one layer: every candidate survives
        for k in ("kp", "response", "pixel"):
            assert n[k].tobytes() == o[k].tobytes(), (name, j, k)                  # the untouched rows included
        assert n["score"].tobytes() == o["score"].tobytes(), (name, j)
        rows = n["record"][0]
        assert not n["layer"][:rows].any() and (n["scale"][:rows] == 1.0).all()


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_output_equals_the_statement(fe, name):
    jobs, want = SC.cases(name), SC.stated(name)
    got = run(fe, jobs)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        SC.check(g, w, (name, j))


def test_the_mixed_batch_equals_its_jobs_one_per_call_and_itself(fe):
    jobs = SC.cases("mixed")
    batch = raw(fe, jobs)
    again = raw(fe, jobs)
    assert same(batch, again)
    for j, job in enumerate(jobs):
        assert same(raw(fe, [job]), batch[j:j + 1]), j


def test_rows_past_n_keypoints_are_left_alone(fe):
    got = raw(fe, SC.cases("capacity") + SC.cases("edges"))
    assert any(o["record"][2] & F.DETECT_OVERFLOW for o in got) and any(o["record"][2] & F.DETECT_FULL for o in got)
    for o in got:
        n = o["record"][0]
        assert all((o[k][n:].view(np.uint8) == 0x5A).all() for k in ("kp", "response", "pixel", "layer", "scale"))


def test_leaving_out_optional_outputs_changes_none_of_the_rest(fe):
    jobs = SC.cases("ties") + SC.cases("edges") + SC.cases("capacity") + SC.cases("mixed")[:20]
    full = raw(fe, jobs)
    optional = ("response", "pixel", "layer", "scale", "score", "pyramid")
    for name in optional:
        part = raw(fe, jobs, leave_out=(name,))
        assert all(o[name] is None for o in part) and same(part, full, skip=(name,)), name
    assert same(raw(fe, jobs, leave_out=optional), full, skip=optional)
    assert same(raw(fe, jobs, referee=False), full, skip=REFEREE)                 # the production path


def test_a_call_after_a_larger_call_of_another_entry_equals_a_fresh_context(fe):
    jobs = SC.cases("edges") + SC.cases("pitch") + SC.cases("mixed")[:10]
    fresh = F.Frontend()
    want = raw(fresh, jobs)
    fresh.close()
    used = F.Frontend()
    rng = np.random.default_rng(5)
    used.bearing_vectors(F.camera([450, 450, 376, 240, -0.28, 0.07, 1e-4, 1e-5], 1), rng.uniform(0, 400, (300000, 3)))   # 3.6 MB staged
    first = raw(used, jobs)
    run(used, SC.cases("counts"))                                                  # and a larger call of its own
    second = raw(used, jobs)
    used.close()
    assert same(first, want) and same(second, want)


def test_keypoints_of_coarser_layers_carry_a_larger_size(fe):
    """what the consumers read: sigma = 0.8 size / 12 in the gate and the triangulator, 64 / size^2 in the backend"""
    j = SC.cases("waves")[4]
    g = run(fe, [j], referee=True)[0]
    size, layer = g["kp"][:, 2].astype(np.float64), g["layer"]
    assert set(int(l) for l in layer) == {0, 1, 2, 3, 4}
    assert ((size >= 0.75 * j["kp_size"] * 2.0 ** layer) & (size <= 1.5 * j["kp_size"] * 2.0 ** layer)).all()
    assert (size[layer == 0] >= j["kp_size"]).all() and (np.abs(g["kp"][:, 0] - ((g["pixel"][:, 0] + 0.5) * 2.0 ** layer - 0.5)) <= 0.5 * 2.0 ** layer + 1e-3).all()


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_detect_scaled_and_describe_equals_the_two_calls_in_sequence(fe):
    jobs = SC.cases("capacity") + SC.cases("edges") + SC.cases("mixed")[:40] + SC.cases("waves")[3:]
    rng = np.random.default_rng(11)
    rot = [rng.integers(0, F.DESCRIBE_ROTATIONS, j["max_keypoints"]).astype(np.int32) for j in jobs]
    cam = F.camera([450, 450, 190, 50, -0.28, 0.07, 1e-4, 1e-5], 1, 384, 96)
    use_cam = [k % 3 == 0 for k in range(len(jobs))]
    cams = [cam if u else None for u in use_cam]
    rots = [None if u else r for u, r in zip(use_cam, rot)]
    dirs = np.tile(np.array([0.1, 0.9, -0.2]), (len(jobs), 1))
    images = [j["image"] for j in jobs]
    # in sequence: detect, then describe what was selected
    det = raw(fe, jobs)
    kps = [d["kp"][:d["record"][0]] for d in det]
    seq_rot = [None if u else r[:len(k)] for u, r, k in zip(use_cam, rot, kps)]
    seq = fe.describe_keypoints(images, kps, cams, dirs, seq_rot, want=("rot", "angle", "angle64"))
    # in one call
    table, keep, out = table_of(jobs)
    rows = [j["max_keypoints"] for j in jobs]
    dtab, keep2, out2 = F.describe_job_table(images, [np.zeros((r, 3), np.float32) for r in rows], cams, dirs, rots, want=("rot", "angle", "angle64"))
    for o in out2:
        for a in o.values():
            if a is not None:
                a.view(np.uint8)[...] = 0x5A
    fe._call("detect_scaled_and_describe", len(jobs), table, dtab)
    chained = [dict(o, record=record(table, j)) for j, o in enumerate(out)]
    assert same(chained, det)
    assert any(d["record"][2] & F.DETECT_OVERFLOW for d in det) and sum(len(k) for k in kps) > 500 and sum(s["n_valid"] for s in seq) > 200
    for j, (s, o) in enumerate(zip(seq, out2)):
        n = len(kps[j])
        assert dtab[j].n_valid == s["n_valid"], j
        for k in F.DESCRIBE_OUTPUTS:
            if k in s:
                assert o[k][:n].tobytes() == s[k].tobytes(), (j, k)
            if o[k] is not None:
                assert (o[k][n:].view(np.uint8) == 0x5A).all(), (j, k)                # rows past n_keypoints are left alone


def test_the_python_chain_gives_what_its_parts_give(fe):
    jobs = SC.cases("waves")[2:4]
    rot = [np.zeros(j["max_keypoints"], np.int32) for j in jobs]
    got = fe.detect_scaled_and_describe(*args(jobs)[:3], rot=rot, min_dist=[j["min_dist"] for j in jobs], max_keypoints=[j["max_keypoints"] for j in jobs],
                                        cand_capacity=[j["cand_capacity"] for j in jobs], kp_size=[j["kp_size"] for j in jobs], want_scale=True,
                                        want_score=True, want_pyramid=True, want=("rot",))
    for j, (g, w) in enumerate(zip(got, SC.stated("waves")[2:4])):
        SC.check(dict(g, flags=g["detect_flags"]), w, ("chain", j))
        assert g["desc"].shape == (len(w["kp"]), F.DESCRIBE_BYTES) and g["n_valid"] == int((g["flags"] & F.DESCRIBE_VALID).sum()) > 0
