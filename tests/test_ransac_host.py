"""CPU: the boundary of okvis_fe_ransac, the statement of its sampler and loop, and the host side of both.

  - the entry is declared in the header, listed in SYMBOLS and exported, the ABI is still 7, and the struct as ctypes sees it is
    the struct of the header; every documented argument error is OKVIS_BA_ERR_ARG before the context is read (the "context" is a
    block of zeros: there is no device here) and nothing is written; n below the sample size is not an error;
  - the numpy Philox4x32-10 (tests/ransac_statement.py) reproduces the known-answer vectors;
  - the BA_HD sampler and loop (okvis_amd/csrc/fe_sac_loop.hpp) run on the CPU through tests/ransac_probe.cpp, a stand-alone program
    built with -fsanitize=address,undefined (runtime linked statically; nothing is preloaded) and run as a child process, and equal
    the statement exactly: every sample of every shape, every constructed loop case, the decision function on both sides of its
    edge;
  - the float64 statement of whole runs (stated samples, numpy hypotheses and scores, the loop rule) returns exactly the true
    inliers of the end-to-end scenes under the seeds the GPU test uses;
  - ransac_2d2d_outcome on both sides of each of its comparisons."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC  # noqa: E402
import ransac_statement as R  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def hexes(block):
    return " ".join(f"{int(x):08x}" for x in block)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert re.search(r"\bint\s+okvis_fe_ransac\s*\(okvis_fe_context\* ctx, int32_t n_jobs, const okvis_fe_ransac_job\* jobs\)", header)
    assert "okvis_fe_ransac" in F.SYMBOLS
    getattr(_lib.lib(), "okvis_fe_ransac")
    assert _lib.lib().okvis_ba_abi_version() == 7          # an addition only
    for name, value in (("CONVERGED", F.RANSAC_STOP_CONVERGED), ("MAX_ITERATIONS", F.RANSAC_STOP_MAX_ITERATIONS),
                        ("EXHAUSTED", F.RANSAC_STOP_EXHAUSTED), ("SKIPS", F.RANSAC_STOP_SKIPS), ("NO_SAMPLE", F.RANSAC_STOP_NO_SAMPLE)):
        assert re.search(rf"#define\s+OKVIS_FE_RANSAC_STOP_{name}\s+{value}\b", header)
        assert getattr(R, "STOP_" + name) == value
    assert F.SAC_SAMPLE_SIZE == R.SAMPLE_SIZE == {0: 4, 1: 2, 2: 8}
    flat = " ".join(header.replace("*", " ").split())
    assert "the sampler and the loop are stated here and are NOT pinned to OpenGV" in flat
    assert "the loop may run max_iterations + 1 iterations" in flat
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "okvis_fe_ransac" in text, doc
        assert "Out of scope: the sampler and the `Ransac` loop" not in text, doc
    assert "What is not here: the sampler, the loop" not in header


def test_struct_equals_the_ctypes_view():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    body = re.search(r"typedef struct okvis_fe_ransac_job \{(.*?)\} okvis_fe_ransac_job;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [n for d in decls for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", d.split(None, 1)[1])]
    assert names == [f[0] for f in F.RansacJobC._fields_], names
    kinds = {"int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}
    at = 0
    for d in decls:          # field by field: the type of every declaration
        words = d.replace("*", " * ").split()
        pointer, base = "*" in words, [w for w in words if w in kinds or w == "uint8_t"][0]
        for _ in re.findall(r"(\w+)\s*(?:,|$)", d.split(None, 1)[1]):
            assert F.RansacJobC._fields_[at][1] is (C.c_void_p if pointer else kinds[base]), d
            at += 1
    assert C.sizeof(F.RansacJobC) == 6 * 4 + 2 * 8 + 8 + 21 * 8          # no padding


@pytest.fixture
def fake_ctx():
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _job(kind, n=12, **kw):
    return RC.ransac_job(kind, RC.random_fields(kind, n, 5), n_slots=8, **kw)


def _call(ctx, job, edit=None, expect_written=False):
    table, keep, out = F.ransac_job_table([job], want_referee=True)
    for o in out:
        for a in o.values():
            a.fill(77)
    if edit:
        edit(table[0])
    rc = _declared().okvis_fe_ransac(ctx, 1, table)
    if not expect_written:
        assert all((a == 77).all() for o in out for a in o.values())          # nothing written
    return rc, out[0]


def test_null_context_and_table(fake_ctx):
    L = _declared()
    assert _call(None, _job(1))[0] == ERR_ARG
    assert L.okvis_fe_ransac(None, 0, None) == ERR_ARG
    assert L.okvis_fe_ransac(fake_ctx[0], -1, None) == ERR_ARG
    assert L.okvis_fe_ransac(fake_ctx[0], 1, None) == ERR_ARG
    assert L.okvis_fe_ransac(fake_ctx[0], 0, None) == 0          # n_jobs = 0 is valid and touches nothing


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("field,value", [("kind", -1), ("kind", 3), ("n", -1), ("n", 65537), ("n_slots", 0), ("n_slots", -1), ("n_slots", 1025),
                                         ("max_iterations", 0), ("max_iterations", -5), ("probability", 0.0), ("probability", 1.0),
                                         ("probability", -0.1), ("probability", 1.5), ("probability", float("nan"))])
def test_value_out_of_range(fake_ctx, kind, field, value):
    def edit(t):
        setattr(t, field, value)
    assert _call(fake_ctx[0], _job(kind), edit)[0] == ERR_ARG


@pytest.mark.parametrize("kind,field", [(0, f) for f in ("points", "bearing", "sigma", "cam_index", "cam_offsets", "cam_rotations")] +
                         [(k, f) for k in (1, 2) for f in ("bearing1", "bearing2", "sigma1", "sigma2")])
def test_null_input(fake_ctx, kind, field):
    def edit(t):
        setattr(t, field, None)
    assert _call(fake_ctx[0], _job(kind), edit)[0] == ERR_ARG


@pytest.mark.parametrize("n_cams", [0, -1, 9, 1])
def test_cameras_out_of_range(fake_ctx, n_cams):
    def edit(t):
        t.n_cams = n_cams          # 1: the scene's cam_index holds a 1
    job = _job(0)
    assert 1 in job["cam_index"]
    assert _call(fake_ctx[0], job, edit)[0] == ERR_ARG


@pytest.mark.parametrize("entry,value", [(0, -1), (5, 2), (-1, 1 << 30)])
def test_cam_index_out_of_range(fake_ctx, entry, value):
    job = _job(0)
    job["cam_index"] = job["cam_index"].copy()
    job["cam_index"][entry] = value
    assert _call(fake_ctx[0], job)[0] == ERR_ARG


def test_an_error_in_a_later_job_leaves_the_earlier_ones_unwritten(fake_ctx):
    table, keep, out = F.ransac_job_table([_job(1, n=1), _job(2)], want_referee=True)          # the first: n below the sample size
    for o in out:
        for a in o.values():
            a.fill(77)
    table[1].n_slots = 0
    assert _declared().okvis_fe_ransac(fake_ctx[0], 2, table) == ERR_ARG
    assert all((a == 77).all() for o in out for a in o.values())


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("short", [1, None])          # n = s - 1, and n = 0 with every input NULL
def test_n_below_the_sample_size_is_not_an_error(fake_ctx, kind, short):
    s = R.SAMPLE_SIZE[kind]
    n = s - 1 if short else 0

    def edit(t):
        if not short:
            for f in ("points", "bearing", "sigma", "cam_index", "bearing1", "bearing2", "sigma1", "sigma2"):
                setattr(t, f, None)
    rc, o = _call(fake_ctx[0], _job(kind, n), edit, expect_written=True)          # nothing is launched: no device is needed
    assert rc == 0
    assert o["scalars"].tolist() == [-1, 0, 0, 0, F.RANSAC_STOP_NO_SAMPLE]
    assert np.isnan(o["model"]).all() and (o["inliers"] == 77).all()
    assert all((o[k] == 77).all() for k in ("samples", "valid", "counts", "models"))          # referee outputs: not written


# ---- the generator and the sampler ----------------------------------------------------------------------------------------------------
def test_numpy_philox_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        assert hexes(R.philox(ctr, key)) == want
    got = R.philox(np.array([k[0] for k in KAT], np.uint64), np.array([k[1] for k in KAT], np.uint64))          # vectorised
    assert [hexes(b) for b in got] == [k[2] for k in KAT]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ransac_probe")
    return RC.build_probe(d), d


def test_probe_philox_reproduces_the_known_answers(probe):
    blocks, _, _, _ = RC.run_probe(*probe, philox=[(k[0], k[1]) for k in KAT], tag="kat")
    assert [hexes(b) for b in blocks] == [k[2] for k in KAT]


@pytest.mark.parametrize("kind", RC.KINDS)
def test_sampler_statement_equals_the_probe(probe, kind):
    s = R.SAMPLE_SIZE[kind]
    shapes = [(seed, n, n_slots, s) for seed in RC.SEEDS for n in RC.sample_sizes(s) for n_slots in RC.SLOTS]
    _, tables, _, _ = RC.run_probe(*probe, sample=shapes, tag=f"sample{kind}")
    for (seed, n, n_slots, _), got in zip(shapes, tables):
        want = R.samples(seed, n_slots, n, s)
        assert np.array_equal(got, want), (seed, n, n_slots)
        assert (want >= 0).all() and (want < n).all()
        srt = np.sort(want, axis=1)
        assert (srt[:, 1:] > srt[:, :-1]).all()          # distinct
        if n == s:
            assert (srt == np.arange(s)).all()          # a permutation of 0..s-1
    assert R.sample(RC.SEEDS[2], 1023, 300, s) == R.samples(RC.SEEDS[2], 1024, 300, s)[1023].tolist()          # the two forms of the statement
    # the draw depends on (seed, slot, n, s) only: a longer table begins with the shorter one
    assert np.array_equal(R.samples(7, 65, 300, s)[:64], R.samples(7, 64, 300, s))


def test_sampler_is_roughly_uniform():
    """not a proof: every index of n = 10 is drawn about equally often over 1024 slots, in every position"""
    q = R.samples(12345, 1024, 10, 4)
    for k in range(4):
        hist = np.bincount(q[:, k], minlength=10)
        assert hist.min() > 60 and hist.max() < 150, hist          # mean 102.4, sigma 9.6: within 4.5 sigma


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
def test_loop_statement_equals_the_probe_on_the_constructed_cases(probe):
    cases = RC.loop_cases()
    _, _, results, _ = RC.run_probe(*probe, loop=cases, tag="loop")
    seen = set()
    for c, got in zip(cases, results):
        want = R.loop(c["counts"], c["valid"], c["n"], c["s"], c["max_iterations"], c["p"])
        assert got == want, (c["name"], got, want)
        for k, v in c["expect"].items():
            assert want[k] == v, (c["name"], k, want)          # the case reaches the edge it was built for
        seen.add(want["stop"])
    assert seen == {R.STOP_CONVERGED, R.STOP_MAX_ITERATIONS, R.STOP_EXHAUSTED, R.STOP_SKIPS}


@pytest.mark.parametrize("s", [2, 4, 8])
def test_decision_function_equals_the_probe_over_the_sweep(probe, s):
    n, p = 300, 0.99
    sweep = RC.done_sweep(s, n, p)
    _, _, _, got = RC.run_probe(*probe, done=[(it, c, n, s, p) for it, c in sweep], tag=f"done{s}")
    want = np.array([R.done(it, c, n, s, p) for it, c in sweep])
    assert np.array_equal(got, want)
    grid = want.reshape(-1, n + 1)
    assert not grid[:, 0].any() and grid[:, n].all()          # count 0 never, count n always
    assert (np.diff(grid.astype(int), axis=1) >= 0).all()          # monotone in the count: one edge per iteration
    edges = grid.argmax(axis=1)
    assert len(set(edges)) > 10          # the sweep crosses the edge at many counts
    log_form = np.array([R.done_log(it, c, n, s, p) for it, c in sweep])
    print(f"s = {s}: {int((log_form != want).sum())} of {len(sweep)} (it, c) pairs differ between the stated form and the log form")
    for other_p in (0.5, 0.999999):
        q = [(it, c, n, s, other_p) for it, c in sweep[::37]]
        assert np.array_equal(RC.run_probe(*probe, done=q, tag=f"done{s}p")[3], np.array([R.done(*a) for a in q]))


# ---- whole runs in float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
def test_float64_run_returns_exactly_the_true_inliers(kind):
    job, truth = RC.end_to_end(kind)
    assert len(truth) == 300 and RC.job_n(job) == 345 and job["n_slots"] == RC.SLOTS_E2E
    res = RC.run_float64(job)
    print(f"kind {kind}: {res['iterations']} iterations, {res['skipped']} skipped, best {res['best']}, stop {res['stop']}")
    assert res["stop"] == R.STOP_CONVERGED and res["n_inliers"] == 300
    assert np.array_equal(res["inliers"], truth)


def test_multi_chunk_scenes_reach_what_they_were_chosen_for():
    """the scenes of the GPU test that run past 64 slots, on the float64 statement: each stops, and finds its best, where its
    description says"""
    for name, job, expect in RC.multi_chunk_cases():
        res = RC.run_float64(job)
        assert {k: res[k] for k in expect} == expect, (name, res)
        assert res["iterations"] + res["skipped"] > 64, name          # the run ends past the first step of 64 slots


# ---- the outcome of runRansac2d2d -----------------------------------------------------------------------------------------------------
def test_outcome_helper_on_both_sides_of_each_comparison():
    o = F.ransac_2d2d_outcome
    # rotation_only_ratio > rel_pose_ratio
    assert o(100, 51, 50)["rotation_only"] and o(100, 51, 50)["inliers_from"] == "rotation_only"
    assert not o(100, 50, 50)["rotation_only"] and o(100, 50, 50)["inliers_from"] == "rel_pose"          # equal: not larger
    assert not o(100, 49, 50)["rotation_only"]
    # ... || rotation_only_ratio > 0.8, the float against the double literal: float(4) / float(5) is above the double 0.8 although
    # 4 / 5 is not above 0.8 as a fraction; 0.75 is exact in both
    assert float(np.float32(4) / np.float32(5)) > 0.8
    r = o(100, 80, 90)
    assert r["rotation_only"] and r["rotation_only_success"] and r["inliers_from"] == "rotation_only" and not r["rel_pose_success"]
    r = o(100, 75, 90)
    assert not r["rotation_only"] and r["rel_pose_success"] and r["inliers_from"] == "rel_pose"
    assert o(100, 81, 90)["rotation_only"]
    # a pair of ratios that differ as floats: 2^24 + 1 is not a float, so the integers' order would put 16777217 / n above
    # 16777216 / n while the floats are equal; within the entry's n <= 65536 the float order is the integers'
    assert np.float32(16777217) == np.float32(16777216)
    assert not o(40000000, 16777217, 16777216)["rotation_only"]
    assert o(65536, 30001, 30000)["rotation_only"] and o(65536, 30001, 30000)["rotation_only_ratio"] > o(65536, 30001, 30000)["rel_pose_ratio"]
    # > 10 on either branch
    assert o(100, 11, 5)["rotation_only_success"] and not o(100, 10, 5)["rotation_only_success"]
    assert o(100, 10, 5)["rotation_only"] and o(100, 10, 5)["inliers_from"] is None          # chosen, but a failure
    assert o(100, 5, 11)["rel_pose_success"] and not o(100, 5, 10)["rel_pose_success"] and o(100, 5, 10)["inliers_from"] is None
    r = o(345, 300, 120)
    assert r["rotation_only_ratio"].dtype == np.float32 and r["rotation_only_ratio"] == np.float32(300) / np.float32(345)
