"""GPU: okvis_fe_sac_solve_absolute against its statement (tests/sac_abs_statement.py) on the seeded cases of tests/sac_abs_cases.py.

  - within the bound: n = 4 with one sample, n = 400 with 1, 50 and 130 samples, the far scene (points at 50-100 m):
    d = max(|R - R_st|_F, |t - t_st|) <= 4 max(e64, e_in) per sample, n_roots and valid equal the statement's (samples with
    separation < 1e-3 or margin < 1e-6 stay out of this comparison, at most 2 % of a case); every reported candidate, excluded
    samples included, a proper rotation to ORTHO_TOL that maps the three points onto their rays; NaN exactly where invalid;
  - packing: a wave holds GP3_PER_WAVE = 4 samples, so jobs of 3, 4 and 5 samples, alone and two in one call, equal the host
    side of the core (tests/sac_abs_probe.cpp, built plain) bit for bit;
  - cameras: n_cams = 1 (central), 2, and 8 with indices 0 and 7 in use; with two cameras samples with all three from one camera
    and samples with two from one and one from the other;
  - the sample with the most candidates among 20 000;
  - degenerate samples: a repeated index and collinear world points are invalid, NaN, count 0; two world points on one ray are
    not degenerate under the definition (tests/test_sac_abs_host.py) and are held to the statement; all equal the probe bit for bit;
  - chaining: fused call = solve-only call + okvis_fe_sac_consensus on its models, bit for bit; a mixed batch equals each job alone;
  - leaving any output pointer NULL changes none of the others;
  - end to end: 300 exact inliers + 15 % gross outliers over two cameras, 50 samples, threshold 9: exactly the true inlier set.

The statement of every case is computed once per process (sac_abs_cases.stated) and shared between the tests."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_abs_cases as AC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
PER_WAVE = 4          # fe_sac_gp3p.hpp: GP3_PER_WAVE


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sac_abs_probe")
    return AC.build_probe(d, sanitize=False), d


def _solve(fe, c, q):
    g = fe.sac_solve_absolute([AC.job(c, q, consensus=False)], want_candidates=True)[0]
    return g["valid"], g["n_roots"], g["models"], g["candidates"]


def _same_bits(got, want):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("seed,n,k,far", [(AC.SMALL_SEED, 4, 1, False), (AC.MAIN_SEED, 400, 1, False), (AC.MAIN_SEED, 400, 50, False),
                                          (AC.MAIN_SEED, 400, 130, False), (AC.FAR_SEED, 400, 50, True)])
def test_within_the_bound(fe, seed, n, k, far):
    c, st = AC.case(seed, n, k, 2, far), AC.stated(seed, n, 2, far)[:k]
    AC.check(c, c["samples"], st, *_solve(fe, c, c["samples"]), f"device seed {seed} n {n} samples {k} far {far}")


def test_packing_edges_equal_the_host_core_bit_for_bit(fe, probe):
    c = AC.case(AC.MAIN_SEED, 400, 130)
    qs = [c["samples"][:PER_WAVE - 1], c["samples"][10:10 + PER_WAVE], c["samples"][20:20 + PER_WAVE + 1]]
    want = [AC.run_probe(*probe, c, q, tag=f"k{len(q)}") for q in qs]
    for q, w in zip(qs, want):
        assert _same_bits(_solve(fe, c, q), w), len(q)
    for pair in ((0, 2), (2, 1)):
        got = fe.sac_solve_absolute([AC.job(c, qs[i], consensus=False) for i in pair], want_candidates=True)
        for i, g in zip(pair, got):
            assert _same_bits((g["valid"], g["n_roots"], g["models"], g["candidates"]), want[i]), pair


@pytest.mark.parametrize("n_cams,used", [(1, None), (2, None), (8, (0, 7))])
def test_cameras(fe, n_cams, used):
    seed = AC.MAIN_SEED + 10 + n_cams
    c, st = AC.case(seed, 400, 20, n_cams, False, used), AC.stated(seed, 400, n_cams, False, used, 20)
    assert set(c["cam_index"]) == set(used or range(n_cams))
    kinds = {len(set(c["cam_index"][q[:3]])) for q in c["samples"]}
    assert kinds == ({1} if n_cams == 1 else {1, 2})          # all three from one camera; two from one and one from another
    AC.check(c, c["samples"], st, *_solve(fe, c, c["samples"]), f"device {n_cams} cameras")


def test_most_candidates(fe):
    c, q, k, k_real = AC.most_roots()
    st = AC.state(c, q[None], 1)
    valid, roots, T, cands = _solve(fe, c, q[None])
    print(f"most candidates among 20000 samples: {k} (most real solutions: {k_real}); the statement finds {st[0]['n_roots']} of "
          f"{st[0]['n_real']} real, the device {roots[0]}")
    assert k >= 4 and k_real == 8
    AC.check(c, q[None], st, valid, roots, T, cands, "device most candidates")
    assert st[0]["excluded"] or roots[0] == st[0]["n_roots"] == k


def test_degenerate_samples(fe, probe):
    c, q = AC.degenerate_case()
    g = fe.sac_solve_absolute([AC.job(c, q)], want_candidates=True)[0]
    got = (g["valid"], g["n_roots"], g["models"], g["candidates"])
    assert g["valid"].tolist()[:4] == [True, False, False, False]
    assert np.isnan(g["models"][1:4]).all() and (g["n_roots"][1:4] == 0).all() and np.isnan(g["candidates"][1:4]).all()
    assert (g["counts"][1:4] == 0).all() and g["best"] in (0, 4)
    st = AC.state(c, q[[0, 4]], 2)
    AC.check(c, q[[0, 4]], st, *[x[[0, 4]] for x in got], "device degenerate")
    assert _same_bits(got, AC.run_probe(*probe, c, q))


def _mixed_batch():
    rng = np.random.default_rng(78)
    jobs = []
    for j in range(40):
        n, k, n_cams = int(rng.integers(4, 150)), int(rng.integers(1, 12)), int(rng.integers(1, 9))
        c = AC.scene(rng, n, n_cams)
        q = AC.samples(rng, n, k)
        if j % 5 == 0:
            q[0, 1] = q[0, 0]                      # an invalid hypothesis
        jobs.append(dict(AC.job(dict(c, sigma=rng.uniform(0.5e-6, 2e-6, n)), q), threshold=9.0))
    return jobs


def test_fused_call_equals_solve_then_consensus_and_each_job_alone(fe):
    jobs = _mixed_batch()
    fused = fe.sac_solve_absolute(jobs, want_scores=True, want_candidates=True)
    alone = fe.sac_solve_absolute([dict(j, consensus=False) for j in jobs])
    cons = fe.sac_consensus([dict(j, kind=F.SAC_ABSOLUTE, models=a["models"]) for j, a in zip(jobs, alone)], want_scores=True)
    n_invalid = 0
    for j, (f, a, c) in enumerate(zip(fused, alone, cons)):
        assert f["models"].tobytes() == a["models"].tobytes() and (f["valid"] == a["valid"]).all(), j
        for key in ("counts", "inliers", "scores"):
            assert np.asarray(f[key]).tobytes() == np.asarray(c[key]).tobytes(), (j, key)
        assert f["best"] == c["best"] and f["n_inliers"] == c["n_inliers"], j
        assert (f["counts"][~f["valid"]] == 0).all() and np.isnan(f["scores"][~f["valid"]]).all()
        n_invalid += int((~f["valid"]).sum())
    assert n_invalid >= 8
    for j in (0, 7, 39):
        one = fe.sac_solve_absolute([jobs[j]], want_scores=True, want_candidates=True)[0]
        assert one.keys() == fused[j].keys()
        for key in one:
            assert np.asarray(one[key]).tobytes() == np.asarray(fused[j][key]).tobytes(), (j, key)


def test_end_to_end_inlier_set_is_the_true_one(fe):
    job, truth = AC.end_to_end()
    g = fe.sac_solve_absolute([job])[0]
    assert g["n_inliers"] == 300 and np.array_equal(g["inliers"], truth)
    assert g["valid"][g["best"]] and g["counts"][g["best"]] == 300


OUTPUTS = ["models", "valid", "n_roots", "candidates", "counts", "best", "n_inliers", "inliers", "scores"]


def _raw(fe, jobs, leave_out=()):
    table, keep, out = F.sac_absolute_job_table(jobs, want_scores=True, want_candidates=True)
    for t in table:
        for name in leave_out:
            setattr(t, name, None)
    fe._call("sac_solve_absolute", len(jobs), table)
    res = []
    for o in out:
        r = dict(o)
        r["best"], r["n_inliers"] = r["scalars"][:1], r["scalars"][1:]
        del r["scalars"]
        res.append(r)
    return res


@pytest.mark.parametrize("leave_out", [(k,) for k in OUTPUTS] + [("counts", "best", "n_inliers", "inliers", "scores"), ("models", "valid", "n_roots", "candidates")])
def test_leaving_an_output_out_changes_none_of_the_others(fe, leave_out):
    c = AC.case(AC.MAIN_SEED, 400, 5)
    jobs = [AC.job(c), AC.job(AC.case(AC.SMALL_SEED, 4, 1))]
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
