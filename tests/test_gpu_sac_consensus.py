"""GPU: okvis_fe_bearing_vectors and okvis_fe_sac_consensus against the run recorded from the reference's own RANSAC adapters and
sample-consensus problems (tests/golden/sac_consensus.npz) and, on inputs larger than the golden file can hold, against the long
double statement (tests/sac_statement.py).

Tolerances (tests/sac_cases.py; distance = |a - b| / max(|b|, 1e-3) for scores, per component for the unit bearing vectors, relative
for the sigma angles).  Measured on the golden cases, reference (double) against statement (long double), and what the GPU gets,
10 times that:
                      reference vs statement     GPU
    absolute score          6.023e-12          6.023e-11
    rotation-only score     5.490e-13          5.490e-12
    relative-pose score     3.549e-08          3.549e-07     (one golden case has 4 mm of translation: the midpoint is ill-conditioned)
    bearing vector          2.748e-16          2.748e-15
    sigma angle             4.939e-16          4.939e-15
tests/test_sac_consensus_host.py measures the left column again and checks that no recorded score lies within the right column of
the threshold, so on the golden cases counts, best and inliers are compared exactly, every cell included.  On the random problems
the cells whose statement score lies within the right column of the threshold (the host test caps them at 0.5 % of a job's cells;
the seed in use has none) stay out of the exact comparison, and best is compared only where the two largest counts differ by more
than the number of such cells in their rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_cases as SC  # noqa: E402
import sac_statement as S  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    f = F.Frontend()
    yield f
    f.close()


def _n(job):
    return len(job["sigma"] if job["kind"] == S.ABSOLUTE else job["sigma1"])


def _check_bearings(fe, intr, model, kp, label):
    cam = F.camera(intr, model)
    b, s, ok = fe.bearing_vectors(cam, kp)
    want_b, want_s, want_ok, _ = S.bearing_vectors(intr, model, kp)
    db = float(np.abs(b - want_b).max()) if len(kp) else 0.0
    ds = float(np.abs(s / want_s - 1).max()) if len(kp) else 0.0
    print(f"{label}: bearing {db:.3e} (bound {SC.GPU_BEARING:.3e}), sigma {ds:.3e} (bound {SC.GPU_SIGMA:.3e}), ok {int(ok.sum())} of {len(ok)}")
    assert db <= SC.GPU_BEARING and ds <= SC.GPU_SIGMA
    assert (ok == want_ok).all()
    return b, s


@pytest.mark.parametrize("i", range(5))
def test_bearing_vectors_against_the_recorded_adapters(fe, i):
    g = SC.golden()
    model, intr = int(g[f"c{i}_model"]), g[f"c{i}_intr"]
    got = {w: _check_bearings(fe, intr, model, g[f"c{i}_kp_{w}"], f"case {i} {w}") for w in ("a0", "a1", "b0", "b1")}
    # ... and what the adapters themselves held, by keypoint
    a = SC.golden_job(g, i, "abs")
    for c in range(2):
        m = a["cam_index"] == c
        b, s = got[f"b{c}"]
        assert np.abs(b[a["kp_index"][m]] - a["bearing"][m]).max() <= SC.GPU_BEARING
        assert np.abs(s[a["kp_index"][m]] / a["sigma"][m] - 1).max() <= SC.GPU_SIGMA
        r = SC.golden_job(g, i, f"rot{c}")
        for w, idx, bk, sk in ((f"a{c}", "idx_a", "bearing1", "sigma1"), (f"b{c}", "idx_b", "bearing2", "sigma2")):
            b, s = got[w]
            assert np.abs(b[r[idx]] - r[bk]).max() <= SC.GPU_BEARING
            assert np.abs(s[r[idx]] / r[sk] - 1).max() <= SC.GPU_SIGMA


@pytest.mark.parametrize("model", [S.DIST_NONE, S.DIST_RADTAN, S.DIST_EQUI, S.DIST_RADTAN8])
def test_bearing_vectors_all_models_against_the_statement(fe, model):
    rng = np.random.default_rng(40 + model)
    intr = {S.DIST_NONE: [455.0, 452.0, 370.0, 245.0], S.DIST_RADTAN: [458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05],
            S.DIST_EQUI: [350.0, 360.0, 378.0, 238.0, -0.021, 0.014, 0.0006, 0.0003],
            S.DIST_RADTAN8: [420.0, 418.0, 370.0, 243.0, -0.25, 0.06, 0.0002, -0.0001, 0.004, 0.03, -0.01, 0.002]}[model]
    for n in (0, 1, 257, 5000):
        kp = np.stack([rng.uniform(5, 747, n), rng.uniform(5, 475, n), rng.uniform(4, 30, n)], axis=1).astype(np.float32)
        _check_bearings(fe, intr, model, kp, f"model {model} n {n}")
    cam = F.camera(intr, model)
    kp = np.array([[100.5, 200.25, 9.0]], np.float32)
    fe._call("bearing_vectors", C.byref(cam), 1, kp.ctypes.data, None, None, None)      # every output may be NULL


@pytest.mark.parametrize("i", range(5))
def test_scores_and_consensus_against_the_recorded_reference(fe, i):
    g = SC.golden()
    jobs = [SC.golden_job(g, i, name) for name in SC.PROBLEMS]
    res = fe.sac_consensus(jobs, want_scores=True)          # the frame's problems in one call
    for name, job, r in zip(SC.PROBLEMS, jobs, res):
        d_ref = float(S.distance(r["scores"], job["ref_scores"]).max())
        d_st = float(S.distance(r["scores"], S.scores(job)).max())
        same = bool((r["scores"] == job["ref_scores"]).all())
        print(f"case {i} {name}: GPU vs reference {d_ref:.3e}{' (bit for bit)' if same else ''}, vs statement {d_st:.3e} "
              f"(bound {SC.GPU_SCORE[job['kind']]:.3e})")
        assert d_ref <= SC.GPU_SCORE[job["kind"]] and d_st <= SC.GPU_SCORE[job["kind"]]
        # nothing excluded: every cell's decision, the first-best rule, the inlier list
        assert (r["counts"] == job["ref_counts"]).all()
        assert r["best"] == int(job["ref_best"])
        assert r["n_inliers"] == len(job["ref_inliers"]) and r["inliers"].tolist() == job["ref_inliers"].tolist()


@pytest.fixture(scope="module")
def random_run(fe):
    seed = SC.RANDOM_SEEDS[0]
    jobs = SC.random_jobs(seed)
    return jobs, SC.stated(seed), fe.sac_consensus(jobs, want_scores=True)      # 64 jobs of mixed kinds, one call


def test_random_problems_scores_against_the_statement(random_run):
    jobs, stated, res = random_run
    worst = {k: 0.0 for k in SC.KINDS.values()}
    for job, st, r in zip(jobs, stated, res):
        assert r["scores"].shape == st["scores"].shape
        if st["scores"].size:
            worst[job["kind"]] = max(worst[job["kind"]], float(S.distance(r["scores"], st["scores"]).max()))
    print({k: f"{v:.3e} (bound {SC.GPU_SCORE[k]:.3e})" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= SC.GPU_SCORE[k]


def test_random_problems_consensus_against_the_statement(random_run):
    jobs, stated, res = random_run
    compared_best = 0
    for j, (job, st, r) in enumerate(zip(jobs, stated, res)):
        n, thr = _n(job), job["threshold"]
        assert st["near"].sum() <= SC.MAX_EXCLUDED * max(1, st["near"].size)
        on_device = r["scores"] < thr                      # the decisions the device took, cell by cell
        sure = ~st["near"]
        assert (on_device[sure] == (st["scores"] < thr)[sure]).all(), j
        # the counts are the device's own integer sums of those decisions; best and the inliers follow from them
        assert (r["counts"] == on_device.sum(axis=1)).all(), j
        assert r["best"] == int(np.argmax(r["counts"])) and r["n_inliers"] == int(r["counts"][r["best"]])
        assert r["inliers"].tolist() == np.nonzero(on_device[r["best"]])[0].tolist() if n else r["n_inliers"] == 0
        # against the statement's counts, up to the excluded cells of each row
        lo = ((st["scores"] < thr) & sure).sum(axis=1)
        assert ((r["counts"] >= lo) & (r["counts"] <= lo + st["near"].sum(axis=1))).all(), j
        counts, best, inliers = S.consensus(st["scores"], thr)
        order = np.sort(counts)[::-1]
        second = order[1] if len(order) > 1 else -1
        runner_up = int(np.argmax(np.where(np.arange(len(counts)) == best, -1, counts))) if len(counts) > 1 else best
        if order[0] - second > st["near"][best].sum() + st["near"][runner_up].sum():
            compared_best += 1
            assert r["best"] == best, j
            if not st["near"][best].any():
                assert r["inliers"].tolist() == inliers.tolist(), j
        elif not st["near"].any():                           # a tie the first-best rule decides, and no cell in doubt
            assert r["best"] == best and r["inliers"].tolist() == inliers.tolist(), j
    assert compared_best >= len(jobs) // 4


def test_scores_are_an_extra_not_an_influence(fe, random_run):
    jobs, _, with_scores = random_run
    without = fe.sac_consensus(jobs, want_scores=False)
    for a, b in zip(with_scores, without):
        assert "scores" not in b
        assert (a["counts"] == b["counts"]).all() and a["best"] == b["best"] and a["n_inliers"] == b["n_inliers"]
        assert a["inliers"].tolist() == b["inliers"].tolist()


def test_scratch_grows_between_calls():
    """a small call, a call many times its size, the small one again, all through one context: the same results as from contexts
    of their own"""
    g = SC.golden()
    small = [SC.golden_job(g, 0, name) for name in SC.PROBLEMS]
    rng = np.random.default_rng(77)
    big = [SC.random_job(rng, k, 8000 + 37 * k, 200) for k in (S.ABSOLUTE, S.ROTATION_ONLY, S.RELATIVE)]
    one = F.Frontend()
    runs = [one.sac_consensus(small), one.sac_consensus(big, want_scores=True), one.sac_consensus(small, want_scores=True),
            one.sac_consensus(big)]
    one.close()
    fresh = []
    for jobs, ws in ((small, False), (big, True), (small, True), (big, False)):
        f = F.Frontend()
        fresh.append(f.sac_consensus(jobs, want_scores=ws))
        f.close()
    for got, want in zip(runs, fresh):
        for a, b in zip(got, want):
            assert (a["counts"] == b["counts"]).all() and a["best"] == b["best"] and a["inliers"].tolist() == b["inliers"].tolist()
            if "scores" in a:
                assert (a["scores"] == b["scores"]).all()
    for job, r in zip(small, runs[0]):
        assert (r["counts"] == job["ref_counts"]).all() and r["inliers"].tolist() == job["ref_inliers"].tolist()
    for job, r in zip(big, runs[1]):                           # the large jobs are right, not merely repeatable
        assert 0 < r["n_inliers"] <= _n(job) and (r["counts"] == (r["scores"] < job["threshold"]).sum(axis=1)).all()
        m = r["best"]
        want = S.scores(dict(job, models=np.asarray(job["models"])[m:m + 1]))[0]
        assert float(S.distance(r["scores"][m], want).max()) <= SC.GPU_SCORE[job["kind"]]


def test_empty_calls(fe):
    assert fe.sac_consensus([]) == []
    rng = np.random.default_rng(3)
    res = fe.sac_consensus([SC.random_job(rng, k, 0, 4) for k in (S.ABSOLUTE, S.ROTATION_ONLY, S.RELATIVE)], want_scores=True)
    for r in res:
        assert r["counts"].tolist() == [0, 0, 0, 0] and r["best"] == 0 and r["n_inliers"] == 0 and len(r["inliers"]) == 0
        assert r["scores"].shape == (4, 0)


def test_largest_problem_the_interface_allows(fe):
    rng = np.random.default_rng(5)
    job = SC.random_job(rng, S.RELATIVE, 65536, 1024)
    r = fe.sac_consensus([job])[0]
    rows = [0, 511, 1023, r["best"]]
    want = S.scores(dict(job, models=np.asarray(job["models"])[rows]))
    near = S.near_threshold(want, 9.0, SC.GPU_SCORE[S.RELATIVE])
    lo = ((want < 9.0) & ~near).sum(axis=1)
    assert ((r["counts"][rows] >= lo) & (r["counts"][rows] <= lo + near.sum(axis=1))).all()
    assert r["n_inliers"] == r["counts"][r["best"]] == len(r["inliers"]) and (np.diff(r["inliers"]) > 0).all()
    if not near[3].any():
        assert r["inliers"].tolist() == np.nonzero(want[3] < 9.0)[0].tolist()
