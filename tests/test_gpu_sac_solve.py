"""GPU: okvis_fe_sac_solve against its statement (tests/sac_solve_statement.py) on the seeded cases of tests/sac_solve_cases.py.

  - two-point: jobs of 1, 63, 64, 65 and 130 samples (the lane packing's edges) with n = 2 and n = 400: the nine doubles equal the
    float64 numpy statement bit for bit; i == j, parallel and exactly antiparallel bearings: invalid, all NaN;
  - five-point: n = 8 with one sample, n = 400 with 1, 50 and 130 samples, and the sample with the most real roots among 20 000:
    d = max(|R - R_st|_F, |t - t_st|) <= 4 max(e64, e_in) per sample, n_roots and valid equal the statement's (samples with
    separation < 1e-3 or margin < 1e-6 stay out of this comparison, at most 2 % of a case); a repeated index: invalid;
  - every reported essential matrix, excluded samples included: unit norm, |f1^T E f2| and |2 E E^T E - tr(E E^T) E| within 4x
    what the numpy evaluation's own roots leave on the same sample; every valid hypothesis a pose to ORTHO_TOL;
  - a pure-rotation scene and a scene with all points on one plane through both centres: OKVIS_BA_OK, every hypothesis invalid
    and NaN or valid and finite, two calls identical bytes;
  - chaining: a mixed batch of 130 jobs, fused call = solve-only call + okvis_fe_sac_consensus on its models, bit for bit;
    invalid hypotheses have count 0;
  - end to end, one scene per kind: 300 exact inliers + 15 % gross outliers, 50 samples: exactly the true inlier set;
  - leaving any output pointer NULL changes none of the others.

The statement of every case is computed once per process (sac_solve_cases.stated) and shared between the tests."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_solve_cases as SC  # noqa: E402
import sac_solve_statement as S  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


# ---- two points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 400])
def test_two_point_bit_for_bit_at_the_packing_edges(fe, n):
    rng = np.random.default_rng(n)
    R, t, b1, b2 = SC.scene(rng, n)
    c = {"bearing1": b1, "bearing2": b2, "sigma1": None, "sigma2": None}
    sizes = [1, 63, 64, 65, 130]
    qs = [np.stack([rng.permutation(n)[:2] for _ in range(k)]).astype(np.int32) for k in sizes]
    got = fe.sac_solve([SC.rotation_job(c, q, consensus=False) for q in qs])
    for q, g in zip(qs, got):
        assert g["models"].shape == (len(q), 3, 3) and g["valid"].all()
        for m, (i, j) in enumerate(q):
            want, ok = S.two_point(c["bearing1"], c["bearing2"], i, j)
            assert ok and g["models"][m].tobytes() == want.tobytes(), (len(q), m)


def test_two_point_degenerate_samples_are_invalid(fe):
    c = SC.case(SC.MAIN_SEED, 400, 1)
    b1, b2 = c["bearing1"].copy(), c["bearing2"].copy()
    b1[1], b2[1] = b1[0], b2[0]                    # parallel
    b1[2], b2[2] = -b1[0], -b2[0]                  # exactly antiparallel
    b1[4] = b1[3]                                  # parallel in frame 1 only
    q = np.array([[5, 5], [0, 1], [0, 2], [3, 4], [6, 7]], np.int32)
    g = fe.sac_solve([dict(SC.rotation_job(c, q), bearing1=b1, bearing2=b2)])[0]
    assert g["valid"].tolist() == [False, False, False, False, True]
    assert np.isnan(g["models"][:4]).all() and np.isfinite(g["models"][4]).all()
    assert (g["counts"][:4] == 0).all() and g["best"] == 4


# ---- five points ----------------------------------------------------------------------------------------------------------------------
def _solve5(fe, c, q5):
    g = fe.sac_solve([SC.relative_job(c, q5, consensus=False)], want_essentials=True)[0]
    return g["valid"], g["n_roots"], g["models"], g["essentials"]


@pytest.mark.parametrize("seed,n,k", [(SC.SMALL_SEED, 8, 1), (SC.MAIN_SEED, 400, 1), (SC.MAIN_SEED, 400, 50), (SC.MAIN_SEED, 400, 130)])
def test_five_point_within_the_bound(fe, seed, n, k):
    c, st = SC.case(seed, n, k), SC.stated(seed, n)[:k]
    SC.check_five_point(c, c["samples5"], st, *_solve5(fe, c, c["samples5"]), f"device seed {seed} n {n} samples {k}")


def test_five_point_most_roots_and_repeated_index(fe):
    c, q, k = SC.most_roots()
    assert k >= 8
    st = SC.state(c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], q[None], 1)
    rep = q.copy()
    rep[6] = rep[2]
    valid, roots, T, Es = _solve5(fe, c, np.stack([q, rep]))
    print(f"most real roots among 20000 samples: {k}; the statement finds {st[0]['n_roots']}, the device {roots[0]}")
    SC.check_five_point(c, q[None], st, valid[:1], roots[:1], T[:1], Es[:1], "device most roots")
    assert st[0]["excluded"] or roots[0] == st[0]["n_roots"] >= 8
    assert not valid[1] and np.isnan(T[1]).all() and roots[1] == 0 and np.isnan(Es[1]).all()


@pytest.mark.parametrize("make", [SC.pure_rotation_case, SC.planar_case])
def test_degenerate_scenes_are_flagged_consistently(fe, make):
    c = make()
    jobs = [SC.relative_job(c), SC.rotation_job(c)]
    a, b = fe.sac_solve(jobs, want_scores=True, want_essentials=True), fe.sac_solve(jobs, want_scores=True, want_essentials=True)
    for g in a:
        for m in range(len(g["models"])):
            assert np.isfinite(g["models"][m]).all() if g["valid"][m] else np.isnan(g["models"][m]).all()
        assert (g["counts"][~g["valid"]] == 0).all()
    for g, h in zip(a, b):
        assert g.keys() == h.keys()
        for key in g:
            assert np.asarray(g[key]).tobytes() == np.asarray(h[key]).tobytes(), key


# ---- chaining -------------------------------------------------------------------------------------------------------------------------
def _mixed_batch():
    rng = np.random.default_rng(77)
    jobs = []
    for j in range(130):
        n, k = int(rng.integers(8, 150)), int(rng.integers(1, 12))
        R, t, b1, b2 = SC.scene(rng, n)
        kind = 1 + j % 2
        q = SC.samples(rng, n, k, 8 if kind == 2 else 2)
        if j % 7 == 0:
            q[0, 1] = q[0, 0]                      # an invalid hypothesis
        jobs.append({"kind": kind, "bearing1": b1, "bearing2": b2, "sigma1": rng.uniform(0.5e-6, 2e-6, n), "sigma2": rng.uniform(0.5e-6, 2e-6, n),
                     "samples": q, "threshold": 9.0})
    return jobs


def test_fused_call_equals_solve_then_consensus(fe):
    jobs = _mixed_batch()
    fused = fe.sac_solve(jobs, want_scores=True)
    alone = fe.sac_solve([dict(j, consensus=False) for j in jobs])
    cons = fe.sac_consensus([dict(j, models=a["models"]) for j, a in zip(jobs, alone)], want_scores=True)
    n_invalid = 0
    for j, (f, a, c) in enumerate(zip(fused, alone, cons)):
        assert f["models"].tobytes() == a["models"].tobytes() and (f["valid"] == a["valid"]).all(), j
        for key in ("counts", "inliers", "scores"):
            assert np.asarray(f[key]).tobytes() == np.asarray(c[key]).tobytes(), (j, key)
        assert f["best"] == c["best"] and f["n_inliers"] == c["n_inliers"], j
        assert (f["counts"][~f["valid"]] == 0).all() and np.isnan(f["scores"][~f["valid"]]).all()
        n_invalid += int((~f["valid"]).sum())
    assert n_invalid >= 19


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [F.SAC_ROTATION_ONLY, F.SAC_RELATIVE])
def test_end_to_end_inlier_set_is_the_true_one(fe, kind):
    job, truth = SC.end_to_end(kind)
    g = fe.sac_solve([job])[0]
    assert g["n_inliers"] == 300 and np.array_equal(g["inliers"], truth)
    assert g["valid"][g["best"]] and g["counts"][g["best"]] == 300


# ---- optional outputs -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ["models", "valid", "n_roots", "essentials", "counts", "best", "n_inliers", "inliers", "scores"]


def _raw(fe, jobs, leave_out=()):
    table, keep, out = F.sac_solve_job_table(jobs, want_scores=True, want_essentials=True)
    for t in table:
        for name in leave_out:
            setattr(t, name, None)
    fe._call("sac_solve", len(jobs), table)
    res = []
    for o in out:
        r = dict(o)
        r["best"], r["n_inliers"] = r["scalars"][:1], r["scalars"][1:]
        del r["scalars"]
        res.append(r)
    return res


@pytest.mark.parametrize("leave_out", [(k,) for k in OUTPUTS] + [("counts", "best", "n_inliers", "inliers", "scores"), ("models", "valid", "n_roots", "essentials")])
def test_leaving_an_output_out_changes_none_of_the_others(fe, leave_out):
    c = SC.case(SC.MAIN_SEED, 400, 5)
    jobs = [SC.relative_job(c), SC.rotation_job(c)]
    full, part = _raw(fe, jobs), _raw(fe, jobs, leave_out)
    for f, p in zip(full, part):
        for key in f:
            if key in leave_out:
                assert not p[key].any()            # untouched: still the zeros it was created with
            elif key == "inliers":
                k = int(f["n_inliers"][0])
                assert "n_inliers" in leave_out or np.array_equal(f[key][:k], p[key][:k])
            else:
                assert f[key].tobytes() == p[key].tobytes(), key
