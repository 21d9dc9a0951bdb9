"""CPU: the boundary of okvis_fe_bearing_vectors / okvis_fe_sac_consensus and their referee.  Both entries are declared in the
header, listed in SYMBOLS and exported; a NULL context and every argument outside the documented limits is OKVIS_BA_ERR_ARG before
the device is touched (there is none here).  The statement (tests/sac_statement.py, long double) reproduces the run recorded from
the reference's own adapters and sample-consensus problems (tests/golden/sac_consensus.npz): bearing vectors, sigma angles and
scores within the distances written down in tests/sac_cases.py (which are measured here again), counts, best and inliers exactly.
The fixture puts the first-best rule, empty and full inlier sets under test, and keeps every score away from the threshold; the
seeded random problems of the GPU test leave at most 0.5 % of a job's cells too close to the threshold to call."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_cases as SC  # noqa: E402
import sac_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
NEW = ("okvis_fe_bearing_vectors", "okvis_fe_sac_consensus")


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    L = _lib.lib()
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header)
        assert s in F.SYMBOLS
        getattr(L, s)
    for name, value in (("ABSOLUTE", F.SAC_ABSOLUTE), ("ROTATION_ONLY", F.SAC_ROTATION_ONLY), ("RELATIVE", F.SAC_RELATIVE)):
        assert re.search(rf"#define\s+OKVIS_FE_SAC_{name}\s+{value}\b", header)
    assert (S.ABSOLUTE, S.ROTATION_ONLY, S.RELATIVE) == (F.SAC_ABSOLUTE, F.SAC_ROTATION_ONLY, F.SAC_RELATIVE)
    assert re.search(r"triangulate2.*?NOT\s+(\*\s+)?pinned", header, re.S)      # the triangulate2 caveat


def _declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _small_job(kind, n=4, k=3, n_cams=2):
    rng = np.random.default_rng(1)
    return SC.random_job(rng, kind, n, k) if kind != S.ABSOLUTE else dict(SC.random_job(rng, kind, n, k), **_cams(n, n_cams))


def _cams(n, n_cams):
    return {"cam_index": np.zeros(n, np.int32), "cam_offsets": np.zeros((n_cams, 3)), "cam_rotations": np.tile(np.eye(3), (n_cams, 1, 1))}


@pytest.fixture
def fake_ctx():
    """Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros."""
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _call(ctx, job, edit=None):
    table, keep, out = F.sac_job_table([job])
    if edit:
        edit(table[0])
    return _declared().okvis_fe_sac_consensus(ctx, 1, table)


@pytest.mark.parametrize("kind", [S.ABSOLUTE, S.ROTATION_ONLY, S.RELATIVE])
def test_null_context_is_an_argument_error(kind):
    assert _call(None, _small_job(kind)) == ERR_ARG
    L = _declared()
    assert L.okvis_fe_sac_consensus(None, 0, None) == ERR_ARG
    cam = F.camera([450, 450, 376, 240], 0)
    kp = np.zeros((4, 3), np.float32)
    assert L.okvis_fe_bearing_vectors(None, C.byref(cam), 4, kp.ctypes.data, None, None, None) == ERR_ARG


def test_bearing_vectors_bad_arguments(fake_ctx):
    L = _declared()
    cam = F.camera([450, 450, 376, 240], 1)
    kp = np.zeros((4, 3), np.float32)
    assert L.okvis_fe_bearing_vectors(fake_ctx[0], None, 4, kp.ctypes.data, None, None, None) == ERR_ARG
    assert L.okvis_fe_bearing_vectors(fake_ctx[0], C.byref(cam), -1, kp.ctypes.data, None, None, None) == ERR_ARG
    assert L.okvis_fe_bearing_vectors(fake_ctx[0], C.byref(cam), 4, None, None, None, None) == ERR_ARG
    for model in (-1, 4):
        bad = F.camera([450, 450, 376, 240], model)
        assert L.okvis_fe_bearing_vectors(fake_ctx[0], C.byref(bad), 4, kp.ctypes.data, None, None, None) == ERR_ARG
    assert L.okvis_fe_bearing_vectors(fake_ctx[0], C.byref(cam), 0, None, None, None, None) == 0      # n = 0 is valid, and touches nothing


def test_negative_job_count_and_missing_table(fake_ctx):
    L = _declared()
    assert L.okvis_fe_sac_consensus(fake_ctx[0], -1, None) == ERR_ARG
    assert L.okvis_fe_sac_consensus(fake_ctx[0], 1, None) == ERR_ARG


@pytest.mark.parametrize("kind", [-1, 3, 7])
def test_bad_kind(fake_ctx, kind):
    def edit(t):
        t.kind = kind
    assert _call(fake_ctx[0], _small_job(S.RELATIVE), edit) == ERR_ARG


@pytest.mark.parametrize("kind", [S.ABSOLUTE, S.ROTATION_ONLY, S.RELATIVE])
@pytest.mark.parametrize("n_models", [0, -1, 1025])
def test_bad_number_of_hypotheses(fake_ctx, kind, n_models):
    def edit(t):
        t.n_models = n_models
    assert _call(fake_ctx[0], _small_job(kind), edit) == ERR_ARG


@pytest.mark.parametrize("n", [-1, 65537])
def test_bad_number_of_correspondences(fake_ctx, n):
    def edit(t):
        t.n = n
    assert _call(fake_ctx[0], _small_job(S.ROTATION_ONLY), edit) == ERR_ARG


@pytest.mark.parametrize("n_cams", [0, -1, 9])
def test_bad_number_of_cameras(fake_ctx, n_cams):
    def edit(t):
        t.n_cams = n_cams
    assert _call(fake_ctx[0], _small_job(S.ABSOLUTE), edit) == ERR_ARG


@pytest.mark.parametrize("kind,field", [(S.ABSOLUTE, f) for f in ("models", "points", "bearing", "sigma", "cam_index", "cam_offsets", "cam_rotations")] +
                         [(k, f) for k in (S.ROTATION_ONLY, S.RELATIVE) for f in ("models", "bearing1", "bearing2", "sigma1", "sigma2")])
def test_null_input_with_correspondences(fake_ctx, kind, field):
    def edit(t):
        setattr(t, field, None)
    assert _call(fake_ctx[0], _small_job(kind), edit) == ERR_ARG


@pytest.mark.parametrize("entry,value", [(0, -1), (3, 2), (2, 8), (1, 1 << 30), (0, -(1 << 31))])
def test_camera_index_out_of_range_is_an_argument_error_not_a_fault(fake_ctx, entry, value):
    job = _small_job(S.ABSOLUTE, n=4, n_cams=2)
    job["cam_index"] = job["cam_index"].copy()
    job["cam_index"][entry] = value
    assert _call(fake_ctx[0], job) == ERR_ARG


# ---- the statement against the recorded reference run ---------------------------------------------------------------------------------
def test_fixture_has_the_cases_the_issue_asks_for():
    g = SC.golden()
    assert os.path.getsize(SC.GOLDEN) < 1 << 20
    n = int(g["n_cases"])
    assert {int(g[f"c{i}_model"]) for i in range(n)} == {S.DIST_RADTAN, S.DIST_EQUI, S.DIST_RADTAN8}
    for i in range(n):
        T = g[f"c{i}_T_SC"]
        assert np.abs(T[0] - T[1]).max() > 1e-3 and np.abs(T[0, 3:6] - T[1, 3:6]).max() > 1e-3       # two cameras, rotations included
        assert set(g[f"c{i}_abs_cam_index"].tolist()) == {0, 1}
        sizes = np.concatenate([g[f"c{i}_kp_{w}"][:, 2] for w in ("a0", "a1", "b0", "b1")])
        assert sizes.max() > 2 * sizes.min()
        assert len(np.unique(np.round(g[f"c{i}_abs_sigma"] / g[f"c{i}_abs_sigma"].min(), 6))) > 10
        for name in SC.PROBLEMS:
            assert int(g[f"c{i}_{name}_pinned"]) == (0 if name.startswith("rel") else 1)
            assert g[f"c{i}_{name}_scores"].shape[0] == 50
    assert max(g[f"c{i}_abs_scores"].shape[1] for i in range(n)) >= 200


def test_fixture_conditions():
    seen = {k: {"tie": False, "none": False, "all": False} for k in SC.KINDS.values()}
    for i, name, job in SC.golden_jobs():
        counts, n = job["ref_counts"], job["ref_scores"].shape[1]
        top = counts == counts.max()
        s = seen[job["kind"]]
        # a tie for the largest count that the first-best rule decides: the best one is not hypothesis 0, and a later one equals it
        s["tie"] |= bool(top.sum() >= 2 and counts.max() > 0 and int(job["ref_best"]) > 0)
        s["none"] |= bool((counts == 0).any())
        s["all"] |= bool((counts == n).any())
        assert int(job["ref_best"]) == int(np.argmax(counts))
        # no recorded score within the comparison band of the threshold: every inlier decision is unambiguous
        assert not S.near_threshold(job["ref_scores"], job["threshold"], SC.GPU_SCORE[job["kind"]]).any(), (i, name)
    assert all(all(v.values()) for v in seen.values()), seen


def test_hypotheses_go_from_near_exact_to_far_off():
    """per kind: a hypothesis under which the typical correspondence is an inlier, and one under which it is far from one (the
    rotation-only problem has the former only where the frames are next to each other)"""
    lo, hi = {k: np.inf for k in SC.KINDS.values()}, {k: 0.0 for k in SC.KINDS.values()}
    for i, name, job in SC.golden_jobs():
        med = np.median(job["ref_scores"], axis=1)
        lo[job["kind"]], hi[job["kind"]] = min(lo[job["kind"]], med.min()), max(hi[job["kind"]], med.max())
        assert med.max() > 1e3, (i, name)
    assert all(v < 9.0 for v in lo.values()), lo


@pytest.mark.parametrize("i", range(5))
def test_statement_reproduces_the_recorded_bearing_vectors(i):
    g = SC.golden()
    model, intr = int(g[f"c{i}_model"]), g[f"c{i}_intr"]
    stated = {w: S.bearing_vectors(intr, model, g[f"c{i}_kp_{w}"]) for w in ("a0", "a1", "b0", "b1")}
    worst_b = worst_s = 0.0
    a = SC.golden_job(g, i, "abs")
    for c in range(2):
        m = a["cam_index"] == c
        b, s, ok, _ = stated[f"b{c}"]
        k = a["kp_index"][m]
        assert ok[k].all()
        worst_b = max(worst_b, float(np.abs(a["bearing"][m] - b[k]).max()))
        worst_s = max(worst_s, float(np.abs(a["sigma"][m] / s[k] - 1).max()))
        r = SC.golden_job(g, i, f"rot{c}")
        for w, idx, bk, sk in ((f"a{c}", "idx_a", "bearing1", "sigma1"), (f"b{c}", "idx_b", "bearing2", "sigma2")):
            b, s, ok, _ = stated[w]
            worst_b = max(worst_b, float(np.abs(r[bk] - b[r[idx]]).max()))
            worst_s = max(worst_s, float(np.abs(r[sk] / s[r[idx]] - 1).max()))
    print(f"case {i}: bearing {worst_b:.3e} (bound {SC.REF_BEARING:.3e}), sigma {worst_s:.3e} (bound {SC.REF_SIGMA:.3e})")
    assert worst_b <= SC.REF_BEARING * 1.0005 and worst_s <= SC.REF_SIGMA * 1.0005       # (the constants are printed to 4 digits)


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("name", SC.PROBLEMS)
def test_statement_reproduces_the_recorded_scores_and_consensus(i, name):
    job = SC.golden_job(SC.golden(), i, name)
    want = S.scores(job)
    dist = float(S.distance(job["ref_scores"], want).max())
    print(f"case {i} {name}: reference vs statement {dist:.3e} (bound {SC.REF_SCORE[job['kind']]:.3e})")
    assert dist <= SC.REF_SCORE[job["kind"]] * 1.0005
    counts, best, inliers = S.consensus(want, job["threshold"])
    assert (counts == job["ref_counts"]).all() and best == int(job["ref_best"])
    assert inliers.tolist() == job["ref_inliers"].tolist()
    # and from the recorded scores themselves, by the `<` rule
    counts, best, inliers = S.consensus(job["ref_scores"], job["threshold"])
    assert (counts == job["ref_counts"]).all() and best == int(job["ref_best"]) and inliers.tolist() == job["ref_inliers"].tolist()


def test_the_written_tolerances_are_the_measured_ones():
    """the largest of the distances the two tests above print is the constant in sac_cases.py, to its 4 digits: neither looser nor
    a figure from somewhere else"""
    worst = {k: 0.0 for k in SC.KINDS.values()}
    for i, name, job in SC.golden_jobs():
        worst[job["kind"]] = max(worst[job["kind"]], float(S.distance(job["ref_scores"], S.scores(job)).max()))
    for k, v in worst.items():
        assert abs(v / SC.REF_SCORE[k] - 1) < 5e-4, (k, v)
        assert SC.GPU_SCORE[k] == 10.0 * SC.REF_SCORE[k]


# ---- the random problems of the GPU test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SC.RANDOM_SEEDS)
def test_random_problems_stay_within_the_exclusion_cap(seed):
    jobs, stated = SC.random_jobs(seed), SC.stated(seed)
    assert len(jobs) == 64 and {j["kind"] for j in jobs} == set(SC.KINDS.values())
    ns = [len(j["sigma"] if j["kind"] == S.ABSOLUTE else j["sigma1"]) for j in jobs]
    ks = [len(j["models"]) for j in jobs]
    assert 0 in ns and 1 in ns and max(ns) >= 5000 and any(n % 64 for n in ns) and min(ks) == 1 and max(ks) == 1024
    excluded = 0
    for job, st in zip(jobs, stated):
        cells = st["near"].size
        assert st["near"].sum() <= SC.MAX_EXCLUDED * cells
        excluded += int(st["near"].sum())
        assert np.isfinite(st["scores"].astype(np.float64)).all()
    print(f"seed {seed}: {excluded} of {sum(st['near'].size for st in stated)} cells within the band of the threshold")
