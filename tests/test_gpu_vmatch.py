"""GPU: whole verified matching steps in one call (okvis_fe_match_verified).

  A  against the reference: numpy Hamming distances, the reference's own triangulator / projection / gate (oracle/_ref) for the
     verification, the sequential statement (tests/vmatch_statement.py) over that distance matrix.  pair_a, pair_dist, accepted and
     proj_status are equal exactly; uv and U within the tolerances tests/test_gpu_frontend.py holds those quantities to.
  B  against the product's own pieces: the same statement over hamming_candidates + gate_3d2d / stereo_triangulate of the existing
     entries, equal exactly; chi2 / gate_flags / hp_a / cov / tri_flags of the accepted pairs are bit-equal to the existing entries
     called on those pairs, and zero elsewhere.
  C  the verification decisions of the existing entries and of the reference agree on every candidate of every scene used here.
  D  a batch of all shapes with mixed kinds and skip masks equals each job alone.
  E  calls on one context and on a fresh one are identical, also after the staging block grew.
  F  the unverified matcher on the same descriptors is unchanged.

Scenes: tests/vmatch_scene.py.  The shapes cover the wave edge at 64, the four rows of a workgroup and the tile edge at 256."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matcher_statement as S0  # noqa: E402
import ref_lib as R  # noqa: E402
import vmatch_scene as SC  # noqa: E402
import vmatch_statement as VS  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402
from okvis_amd.window import DIST_EQUIDISTANT, DIST_RADTAN  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not available")

SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (257, 513), (400, 400)]
KINDS = [F.MATCH_3D2D, F.MATCH_2D2D]
MODELS = [DIST_RADTAN, DIST_EQUIDISTANT]
SETTINGS = [(1, False), (4, False), (8, False), (4, True), (8, True)]   # (num_best, use_ratio)
RATIO = 1.2
THRESHOLD = SC.THRESHOLD


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def scene(model, k, skipped=0.0):
    n_a, n_b = SHAPES[k]
    return SC.scene(model, 1000 + 10 * k + model, n_a, n_b, skipped)


def job(kind, s):
    cam = F.camera(s["intr"], s["model"])
    j = {"kind": kind, "desc_a": s["desc_a"], "desc_b": s["desc_b"], "kp_a": s["kp_a"], "kp_b": s["kp_b"], "cam_a": cam, "cam_b": cam,
         "skip_a": s["skip_a"], "skip_b": s["skip_b"]}
    if kind == F.MATCH_3D2D:
        j.update(hp_W=s["hp_W"], T_CbW=s["T_CbW"], P3=s["P3"])
    else:
        j.update(T_AB=s["T_AB"], UOplus=s["UOplus"])
    return j


def verification(api, kind, s, pairs):
    """the pieces one by one through `api` (the product's existing entries or the reference build): for every candidate pair whether
    verifyMatch holds, the number behind the decision (chi2 of the gate; for a triangulation its flags), and the projections"""
    cam = F.camera(s["intr"], s["model"])
    if kind == F.MATCH_2D2D:
        _, _, flags = api.stereo_triangulate(cam, cam, s["T_AB"], s["UOplus"], s["kp_a"], s["kp_b"], pairs, SC.pair_sigmas(s, pairs),
                                             want_uncertainty=False)
        return flags & F.TRI_VALID != 0, flags.astype(np.float64), None
    uv, U, st = api.project_landmarks(cam, s["T_CbW"], s["P3"], s["hp_W"])
    ok, chi2 = np.zeros(len(pairs), bool), np.zeros(len(pairs))
    play = st[pairs[:, 0]] == F.PROJ_SUCCESSFUL          # (rows with skip_a set carry no candidates)
    if play.any():
        chi2[play], flags = api.gate_3d2d(uv, U, s["kp_b"], pairs[play])
        ok[play] = flags & F.GATE_VERIFIED != 0
    return ok, chi2, (uv, U, st)


def distances(s, pairs, ok):
    n_a, n_b = len(s["desc_a"]), len(s["desc_b"])
    ham = S0.hamming_matrix(s["desc_a"], s["desc_b"]) if n_a and n_b else np.zeros((n_a, n_b), np.int32)
    verified = np.zeros((n_a, n_b), bool)
    verified[pairs[:, 0], pairs[:, 1]] = ok
    return VS.distance_matrix(ham, THRESHOLD, verified), VS.distance_matrix(ham, THRESHOLD)


@functools.lru_cache(maxsize=None)
def by_reference(kind, model, k, skipped=0.0):
    s = scene(model, k, skipped)
    pairs, _ = S0.candidates(s["desc_a"], s["desc_b"], THRESHOLD, s["skip_a"], s["skip_b"])
    ok, num, proj = verification(F.Frontend(api=(R.lib(), "ref_fe_")), kind, s, pairs)
    return pairs, ok, num, proj, distances(s, pairs, ok)


PRODUCT = {}


def by_product(fe, kind, model, k, skipped=0.0):
    key = (kind, model, k, skipped)
    if key not in PRODUCT:
        s = scene(model, k, skipped)
        pairs, _ = fe.hamming_candidates(s["desc_a"], s["desc_b"], THRESHOLD, s["skip_a"], s["skip_b"])
        ok, num, proj = verification(fe, kind, s, pairs)
        PRODUCT[key] = pairs, ok, num, proj, distances(s, pairs, ok)
    return PRODUCT[key]


def expect(dist, s, num_best, use_ratio):
    pair_a, pair_dist, calls, _ = VS.match(dist, THRESHOLD, num_best, use_ratio, RATIO, s["skip_a"], s["skip_b"])
    return pair_a, pair_dist, VS.accepted_mask(calls, dist.shape[1])


def same_matches(got, want):
    return all(got[name].shape == w.shape and (got[name] == w).all() for name, w in zip(("pair_a", "pair_dist", "accepted"), want))


def identical(x, y):
    return x.keys() == y.keys() and all(x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes() for k in x)


# ---------------------------------------------------------------- A: the reference

@needs_ref
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_equals_the_statement_over_the_reference_verification(fe, kind, model):
    verified_pairs = 0
    for k in range(len(SHAPES)):
        s = scene(model, k)
        pairs, ok, _, proj, (dist, plain) = by_reference(kind, model, k)
        verified_pairs += int(ok.sum())
        if SHAPES[k] in ((257, 513), (400, 400)):     # the referee alone: the scene exercises what it is for
            st = VS.scene_statistics(dist, plain, THRESHOLD, SC.NUM_BEST)
            print(SHAPES[k], "candidates", len(pairs), "verified", int(ok.sum()), st)
            assert st["two_or_more"] >= 0.25 and st["tie"] >= 0.05 and st["lost_first"] >= 0.05 and st["changed"] >= 0.5, st
        for num_best, use_ratio in SETTINGS:
            got, = fe.match_verified([job(kind, s)], THRESHOLD, num_best, use_ratio, RATIO)
            assert same_matches(got, expect(dist, s, num_best, use_ratio)), (SHAPES[k], num_best, use_ratio)
            if kind == F.MATCH_3D2D:
                uv, U, st = proj
                assert np.array_equal(got["proj_status"], st)
                good = st == F.PROJ_SUCCESSFUL
                if good.any():      # the bounds of test_projection_and_gating_3d2d
                    assert np.abs(got["uv"][good] - uv[good]).max() <= 1e-9
                    assert (np.abs(got["U"][good] - U[good]) / np.abs(U[good]).max(axis=(1, 2))[:, None, None]).max() <= 1e-10
    assert verified_pairs > 1500


# ---------------------------------------------------------------- B: the product's own pieces

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_b_equals_the_statement_over_the_existing_entries(fe, kind, model):
    accepted_pairs = 0
    for k in range(len(SHAPES)):
        s = scene(model, k)
        cam = F.camera(s["intr"], model)
        n_a, n_b = SHAPES[k]
        _, _, _, proj, (dist, _) = by_product(fe, kind, model, k)
        for num_best, use_ratio in SETTINGS:
            got, = fe.match_verified([job(kind, s)], THRESHOLD, num_best, use_ratio, RATIO)
            assert same_matches(got, expect(dist, s, num_best, use_ratio)), (SHAPES[k], num_best, use_ratio)
            bs = np.flatnonzero(got["accepted"])
            acc = np.stack([got["pair_a"][bs], bs], 1).astype(np.int32)
            accepted_pairs += len(acc)
            if kind == F.MATCH_3D2D:
                uv, U, st = proj
                assert np.array_equal(got["proj_status"], st)
                assert got["uv"].tobytes() == uv.tobytes() and got["U"].tobytes() == U.tobytes()
                chi2, flags = np.zeros(n_b), np.zeros(n_b, np.uint8)
                if len(acc):
                    chi2[bs], flags[bs] = fe.gate_3d2d(uv, U, s["kp_b"], acc)
                    assert (flags[bs] & F.GATE_VERIFIED != 0).all()
                assert got["chi2"].tobytes() == chi2.tobytes() and np.array_equal(got["gate_flags"], flags)
            else:
                hp, cov, flags = np.zeros((n_b, 4)), np.zeros((n_b, 3, 3)), np.zeros(n_b, np.uint8)
                if len(acc):
                    hp[bs], cov[bs], flags[bs] = fe.stereo_triangulate(cam, cam, s["T_AB"], s["UOplus"], s["kp_a"], s["kp_b"], acc,
                                                                       SC.pair_sigmas(s, acc), want_uncertainty=True)
                    assert (flags[bs] & F.TRI_VALID != 0).all()
                assert got["hp_a"].tobytes() == hp.tobytes() and got["cov"].tobytes() == cov.tobytes()
                assert np.array_equal(got["tri_flags"], flags)
    assert accepted_pairs > 2000


# ---------------------------------------------------------------- C: the decisions of the two sides

@needs_ref
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_c_existing_entries_and_reference_decide_alike_on_every_candidate(fe, kind, model):
    total = 0
    for skipped in (0.0, 0.15):
        for k in range(len(SHAPES)):
            pairs_r, ok_r, num_r, _, _ = by_reference(kind, model, k, skipped)
            pairs_p, ok_p, num_p, _, _ = by_product(fe, kind, model, k, skipped)
            assert np.array_equal(pairs_p, pairs_r)
            total += len(pairs_r)
            bad = np.flatnonzero(ok_p != ok_r)
            what = "chi2" if kind == F.MATCH_3D2D else "TRI_* flags"
            assert bad.size == 0, [(SHAPES[k], tuple(pairs_r[i]), f"{what}: product {num_p[i]!r}, reference {num_r[i]!r}") for i in bad[:10]]
    assert total > 20000


# ---------------------------------------------------------------- D: batching

def test_d_batch_of_all_shapes_and_mixed_kinds_equals_each_job_alone(fe):
    jobs, want = [], []
    for k in range(len(SHAPES)):
        kind, model, skipped = KINDS[k % 2], MODELS[(k // 2) % 2], 0.15 if k % 2 else 0.0
        jobs.append(job(kind, scene(model, k, skipped)))
        want.append(by_product(fe, kind, model, k, skipped)[4][0])
    assert any(j["skip_a"] is not None and j["skip_a"].any() and j["skip_b"].any() for j in jobs)
    for num_best, use_ratio in ((4, False), (3, True)):
        batch = fe.match_verified(jobs, THRESHOLD, num_best, use_ratio, RATIO)
        assert len(batch) == len(jobs)
        for j, dist, got in zip(jobs, want, batch):
            alone, = fe.match_verified([j], THRESHOLD, num_best, use_ratio, RATIO)
            assert identical(got, alone)
            assert same_matches(got, expect(dist, j, num_best, use_ratio))
            if j["skip_a"] is not None and j["kind"] == F.MATCH_3D2D:     # rows out of play are not projected
                assert (got["proj_status"][j["skip_a"]] == 0).all() and (got["uv"][j["skip_a"]] == 0).all()
    assert fe.match_verified([], THRESHOLD) == []


# ---------------------------------------------------------------- E: context reuse

def test_e_two_calls_on_one_context_and_one_on_a_fresh_context_are_identical(fe):
    jobs = [job(KINDS[k % 2], scene(DIST_RADTAN, k)) for k in (3, 6, 7, 6)]
    f = F.Frontend()
    first = f.match_verified(jobs, THRESHOLD, 4, True, RATIO)
    second = f.match_verified(jobs, THRESHOLD, 4, True, RATIO)
    f.close()
    fresh = fe.match_verified(jobs, THRESHOLD, 4, True, RATIO)
    assert sum(int(r["accepted"].sum()) for r in first) > 300
    for x, y, z in zip(first, second, fresh):
        assert identical(x, y) and identical(x, z)


def test_e_second_call_after_the_staging_block_grew():
    f = F.Frontend()                      # a context of its own: its staging block starts empty
    small = [job(F.MATCH_2D2D, scene(DIST_EQUIDISTANT, 3)), job(F.MATCH_3D2D, scene(DIST_EQUIDISTANT, 4))]   # fit the first block
    large = [job(KINDS[k % 2], scene(DIST_EQUIDISTANT, 6 + k % 2)) for k in range(6)]
    first = f.match_verified(small, THRESHOLD, 4, True, RATIO)
    big = f.match_verified(large, THRESHOLD, 4)
    again = f.match_verified(small, THRESHOLD, 4, True, RATIO)
    big_again = f.match_verified(large, THRESHOLD, 4)
    f.close()
    for x, y in zip(first + big, again + big_again):
        assert identical(x, y)
    assert sum(int(r["accepted"].sum()) for r in first) > 20 and sum(int(r["accepted"].sum()) for r in big) > 1000


# ---------------------------------------------------------------- F: the existing matcher

def test_f_descriptor_matcher_is_unchanged(fe):
    for k in (3, 6, 7):
        s = scene(DIST_RADTAN, k, 0.15)
        for num_best, use_ratio in ((4, False), (4, True)):
            pair_a, pair_dist, calls = S0.match(s["desc_a"], s["desc_b"], THRESHOLD, num_best, use_ratio, RATIO, s["skip_a"], s["skip_b"])
            (ga, gd, gacc), = fe.match_descriptors([(s["desc_a"], s["desc_b"], s["skip_a"], s["skip_b"])], THRESHOLD, num_best, use_ratio,
                                                   RATIO)
            assert (ga == pair_a).all() and (gd == pair_dist).all() and (gacc == S0.accepted_mask(calls, len(s["desc_b"]))).all()
