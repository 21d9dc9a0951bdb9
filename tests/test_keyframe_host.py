"""CPU: the boundary of okvis_fe_keyframe_decision, its predicate and its statement (cases: tests/keyframe_cases.py).

  - the entry is declared in the header, listed in SYMBOLS and exported, and the header says that hull, area and inside test are
    NOT pinned to OpenCV;
  - every documented argument error is OKVIS_BA_ERR_ARG on a zeroed fake context, before the device is touched (there is none here);
  - kf_orient_sign of okvis_amd/csrc/fe_keyframe.hpp, compiled for the host (tests/keyframe_probe.cpp), equals the exact sign on
    10^5 triples of the adversarial family and 10^5 random ones, through its filter and through the exact path alone, and the plain
    double expression does not (otherwise the family would prove nothing);
  - the header's plain loop (the same comparator the kernel reduces with) gives the statement's hulls, counts and bits on every case;
  - the statement's double area lies within (2h + 1) 2^-53 sum(|x_i y_i+1| + |x_i+1 y_i|) of its exact area on every case.  The
    bound is derived, not measured: the products are exact; each of the h differences is rounded once (relative 2^-53 of at most
    |x_i y_i+1| + |x_i+1 y_i|); each of the h running sums is rounded once, and a running sum never exceeds the sum of the terms'
    magnitudes times (1 + 2^-53)^h, which the "+ 1" absorbs for h <= 8192; the halving is exact;
  - the cases are what the issue asks for: both orders of the NaN camera differ, the triangle case has ratio +inf and decision 0,
    at most 1 in 20 regular seeds is dropped for lying within 1e-6 of a threshold."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import keyframe_cases as KC  # noqa: E402
import keyframe_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
ENTRY = "okvis_fe_keyframe_decision"


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(okvis_fe_context\* ctx", header)
    assert ENTRY in F.SYMBOLS
    getattr(_lib.lib(), ENTRY)
    assert re.search(r"convexHull.*?NOT\s+(\*\s+)?pinned\s+to\s+OpenCV", header, re.S)
    assert "Frontend.cpp:295-369" in header
    for name, value in (("FEW_POINTS", F.KF_FEW_POINTS), ("FEW_MATCHES", F.KF_FEW_MATCHES)):
        assert re.search(rf"#define\s+OKVIS_FE_KF_{name}\s+{value}u\b", header)
    assert (S.FEW_POINTS, S.FEW_MATCHES) == (F.KF_FEW_POINTS, F.KF_FEW_MATCHES)
    assert C.sizeof(F.KfImageC) == 8 and C.sizeof(F.KfJobC) == 24


@pytest.fixture
def fake_ctx():
    """Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros."""
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _job(n=5, n_cams=2):
    rng = np.random.default_rng(n)
    return {"images": [KC.im(rng.integers(0, 100, (n, 2)), "all") for _ in range(n_cams)]}


def _call(ctx, job_list, edit=None, **override):
    """the entry through ctypes; edit(images, table) changes the tables, override replaces arguments by name"""
    L = _lib.lib()
    F.declare(L)
    jobs = job_list
    kp, matched, images, table, counts = F.keyframe_job_table(jobs)
    if edit:
        edit(images, table)
    out = F.keyframe_outputs(len(jobs), len(counts), sum(counts), True)
    a = {"n_kp": len(matched), "kp": kp.ctypes.data, "matched": matched.ctypes.data, "n_images": len(counts), "images": images,
         "n_jobs": len(jobs), "jobs": table}
    if "kp_array" in override:
        a["kp"] = override.pop("kp_array").ctypes.data
    a.update(override)
    before = {k: v.copy() for k, v in out.items()}
    rc = L.okvis_fe_keyframe_decision(ctx, a["n_kp"], a["kp"], a["matched"], a["n_images"], a["images"], a["n_jobs"], a["jobs"],
                                      *[out[k].ctypes.data for k in F.KF_OUTPUTS])
    assert all(out[k].tobytes() == before[k].tobytes() for k in out)       # nothing is written on the way to an error (or to n = 0)
    return rc


def test_null_context_is_an_argument_error():
    assert _call(None, [_job()]) == ERR_ARG
    assert _call(None, []) == ERR_ARG


def test_no_jobs_and_no_images_is_valid_and_touches_nothing(fake_ctx):
    assert _call(fake_ctx[0], []) == 0
    assert _call(fake_ctx[0], [], kp=None, matched=None, images=None, jobs=None) == 0


@pytest.mark.parametrize("name", ["n_kp", "n_images", "n_jobs"])
def test_negative_counts(fake_ctx, name):
    assert _call(fake_ctx[0], [_job()], **{name: -1}) == ERR_ARG


@pytest.mark.parametrize("name", ["kp", "matched", "images", "jobs"])
def test_null_required_pointer(fake_ctx, name):
    assert _call(fake_ctx[0], [_job()], **{name: None}) == ERR_ARG


@pytest.mark.parametrize("n_cams", [0, -1, 9])
def test_bad_number_of_cameras(fake_ctx, n_cams):
    def edit(images, table):
        table[0].n_cams = n_cams
    assert _call(fake_ctx[0], [_job()], edit) == ERR_ARG


@pytest.mark.parametrize("im_begin", [-1, 1, 2, 1 << 30])
def test_image_range_outside_the_pool(fake_ctx, im_begin):
    def edit(images, table):
        table[0].im_begin = im_begin
    assert _call(fake_ctx[0], [_job()], edit) == ERR_ARG


def test_negative_num_frames(fake_ctx):
    def edit(images, table):
        table[0].num_frames = -1
    assert _call(fake_ctx[0], [_job()], edit) == ERR_ARG


@pytest.mark.parametrize("begin,count", [(-1, 5), (6, 5), (0, 11), (0, -1), (1 << 30, 1 << 30), (0, 8193)])
def test_keypoint_range_outside_the_pool_or_the_limit(fake_ctx, begin, count):
    def edit(images, table):
        images[1].kp_begin, images[1].kp_count = begin, count
    assert _call(fake_ctx[0], [_job()], edit) == ERR_ARG


def test_more_than_the_limit_of_keypoints_in_a_pool_that_holds_them(fake_ctx):
    job = {"images": [KC.im(np.zeros((8193, 2)), "all")]}
    assert _call(fake_ctx[0], [job]) == ERR_ARG


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("col", [0, 1])
def test_non_finite_coordinate(fake_ctx, value, col):
    job = _job()
    kp, *_ = F.keyframe_job_table([job])
    kp = kp.copy()
    kp[7, col] = value
    assert _call(fake_ctx[0], [job], kp_array=kp) == ERR_ARG


# ---- the predicate ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("probe") / "libkeyframe_probe.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "keyframe_probe.cpp"),
                           "-o", so])
    return C.CDLL(so)


def _probe_signs(probe, a, b, c):
    a, b, c = (np.ascontiguousarray(v, np.float32) for v in (a, b, c))
    n = len(a)
    sign, naive, exact = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    probe.probe_orient(n, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                       sign.ctypes.data_as(C.c_void_p), naive.ctypes.data_as(C.c_void_p))
    probe.probe_orient_exact(n, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                             exact.ctypes.data_as(C.c_void_p))
    return sign, naive, exact


def test_orient_sign_is_exact_on_the_adversarial_family_and_the_plain_expression_is_not(probe):
    a, b, c = KC.family()
    want, numpy_naive = KC.family_signs()
    sign, naive, exact = _probe_signs(probe, a, b, c)
    assert len(a) >= 100000
    wrong = int((naive != want).sum())
    print(f"family: the plain double expression is wrong on {wrong} of {len(a)} triples; exact signs -1/0/+1: "
          f"{[int((want == s).sum()) for s in (-1, 0, 1)]}")
    assert (sign == want).all() and (exact == want).all()
    assert wrong >= 1 and (naive == numpy_naive).all()
    assert len(KC.wrong_triples()) >= 2 and {s for *_, s in KC.wrong_triples()} >= {-1, 1}


def test_orient_sign_is_exact_on_random_floats_of_every_exponent(probe):
    a, b, c = KC.random_triples()
    want = KC.exact_signs(a, b, c)
    sign, naive, exact = _probe_signs(probe, a, b, c)
    assert len(a) >= 100000 and np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()
    print(f"random: exact signs -1/0/+1: {[int((want == s).sum()) for s in (-1, 0, 1)]}; the plain expression is wrong on "
          f"{int((naive != want).sum())}")
    assert (want == 0).sum() >= 100 and (want == 1).sum() >= 1000 and (want == -1).sum() >= 1000
    assert (sign == want).all() and (exact == want).all()
    # antisymmetry, which the wave's butterfly relies on: both lanes of a pair must name the same winner
    swapped, _, _ = _probe_signs(probe, a, c, b)
    assert (swapped == -want).all()


def test_orient_sign_at_the_ends_of_the_float_range(probe):
    big, tiny = np.float32(3.4028235e38), np.float32(1e-45)
    a = np.array([[big, big], [-big, -big], [tiny, tiny], [0, 0], [big, -big], [tiny, 0]], np.float32)
    b = np.array([[-big, -big], [big, big], [-tiny, -tiny], [tiny, tiny], [-big, big], [0, tiny]], np.float32)
    c = np.array([[big, -big], [tiny, -tiny], [tiny, -tiny], [2 * tiny, 2 * tiny], [tiny, tiny], [big, big]], np.float32)
    want = KC.exact_signs(a, b, c)
    sign, _, exact = _probe_signs(probe, a, b, c)
    assert (sign == want).all() and (exact == want).all() and set(want) == {-1, 0, 1}


# ---- the header's plain loop against the statement --------------------------------------------------------------------------------------
def _probe_jobs(probe, jobs):
    kp, matched, images, table, counts = F.keyframe_job_table(jobs)
    n_im = len(counts)
    begin = np.array([images[i].kp_begin for i in range(n_im)], np.int32)
    count = np.array(counts, np.int32)
    rec = np.zeros((max(n_im, 1), 8))
    ha, hm = np.zeros(max(len(matched), 1), np.int32), np.zeros(max(len(matched), 1), np.int32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    probe.probe_kf_images(n_im, vp(begin), vp(count), vp(kp), vp(matched), vp(rec), vp(ha), vp(hm))
    probe.probe_kf_fold.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    res = []
    for j in range(len(jobs)):
        t, ims = table[j], []
        for i in range(t.im_begin, t.im_begin + t.n_cams):
            r = rec[i]
            ims.append({"area_all": r[0], "area_matched": r[1], "n_matched": int(r[2]), "hull_all_size": int(r[3]), "hull_matched_size": int(r[4]),
                        "n_inside": int(r[5]), "flags": int(r[6]), "hull_all": ha[begin[i]:begin[i] + int(r[3])], "hull_matched": hm[begin[i]:begin[i] + int(r[4])]})
            assert (ha[begin[i] + int(r[3]):begin[i] + count[i]] == -1).all() and (hm[begin[i] + int(r[4]):begin[i] + count[i]] == -1).all()
        o, ra = np.zeros(1), np.zeros(1)
        d = probe.probe_kf_fold(t.n_cams, rec[t.im_begin:].ctypes.data, t.num_frames, t.initialized, t.overlap_threshold, t.ratio_threshold,
                                o.ctypes.data, ra.ctypes.data)
        res.append({"decision": bool(d), "overlap": o[0], "ratio": ra[0], "images": ims})
    return res


@pytest.mark.parametrize("name", KC.NAMES)
def test_the_plain_loop_of_the_header_gives_the_statement(probe, name):
    got, want = _probe_jobs(probe, KC.cases(name)), KC.stated(name)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        KC.check(g, w, (name, j))


# ---- the statement and the cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.NAMES)
def test_double_area_lies_within_the_derived_bound_of_the_exact_area(name):
    worst = Fraction(0)
    for j, st in enumerate(KC.stated(name)):
        for c, r in enumerate(st["images"]):
            for which, hull in (("all", r["hull_all"]), ("matched", r["hull_matched"])):
                h = len(hull)
                bound = (2 * h + 1) * Fraction(1, 2 ** 53) * r["mag_" + which]
                err = abs(Fraction(float(r["area_" + which])) - r["exact_" + which])
                assert err <= bound, (name, j, c, which, float(err), float(bound))
                if bound:
                    worst = max(worst, err / bound)
    print(f"{name}: the largest error is {float(worst):.3f} of its bound")


def test_the_cases_are_the_ones_asked_for():
    sk = KC.stated("skips")
    assert [i["flags"] for i in sk[0]["images"]] == [S.FEW_POINTS, S.FEW_POINTS, S.FEW_MATCHES] and sk[0]["decision"]
    tri = sk[1]
    assert tri["images"][0]["n_inside"] == 0 and np.isposinf(tri["ratio"]) and tri["overlap"] == 1.0 and not tri["decision"]
    dg = KC.stated("degenerate")
    assert not np.isnan(dg[0]["overlap"]) and not dg[0]["decision"]       # NaN in camera 0: camera 1 replaces it
    assert np.isnan(dg[1]["overlap"]) and dg[1]["decision"]               # NaN in camera 1: it stays
    assert dg[0]["images"][0]["hull_all"] == dg[0]["images"][0]["hull_matched"] == [1, 2]       # the extremes, lowest (y, x) first
    assert len(dg[3]["images"][0]["hull_matched"]) == 2 and dg[3]["images"][0]["n_inside"] == 0 and len(dg[3]["images"][0]["hull_all"]) > 2
    assert dg[4]["images"][0]["hull_matched"] == [0] and dg[5]["images"][0]["hull_all"] == [0]
    assert dg[6]["images"][0]["hull_all"] == [1, 2, 0, 5] and dg[6]["images"][0]["hull_matched"] == [3, 2, 0, 5]      # lowest index
    oe = KC.stated("on_edges")[0]["images"]
    assert oe[0]["hull_matched"] == [1, 2, 0, 3] and oe[0]["n_inside"] == 5 and oe[1]["n_inside"] == 1
    adv = KC.stated("adversarial")
    assert {len(s["images"][0]["hull_matched"]) for s in adv} == {3, 4} and {s["images"][1]["n_inside"] for s in adv} == {0, 1}
    for s, n in zip(KC.stated("convex"), (64, 65, 512)):
        assert len(s["images"][0]["hull_all"]) == len(s["images"][0]["hull_matched"]) == n and s["images"][0]["n_inside"] == 0
    assert len(KC.cases("limit")[0]["images"][0][0]) == F.KF_MAX_KEYPOINTS


def test_regular_scenes_keep_away_from_the_thresholds():
    jobs, stated, generated = KC.regular_kept()
    print(f"regular: {len(jobs)} of {generated} seeds kept; decisions {[int(s['decision']) for s in stated]}")
    assert generated - len(jobs) <= generated // 20
    assert {s["decision"] for s in stated} == {True, False}
    for j in jobs:
        assert len(j["images"]) == 2 and all(len(kp) == 400 and 40 <= m.sum() <= 240 for kp, m in j["images"])      # 10 to 60 % matched
        assert all((kp[:, :2] * 16 == np.round(kp[:, :2] * 16)).all() for kp, _ in j["images"])


def test_mixed_batch_has_what_it_should():
    jobs, st = KC.cases("mixed"), KC.stated("mixed")
    assert len(jobs) == 130 and {len(j["images"]) for j in jobs} == set(range(1, 9))
    assert any(len(kp) == 0 for j in jobs for kp, _ in j["images"])
    assert any(j["num_frames"] < 2 for j in jobs) and any(not j["initialized"] for j in jobs)
    assert {s["decision"] for s in st} == {True, False}
    flags = {i["flags"] for s in st for i in s["images"]}
    assert flags == {0, S.FEW_POINTS, S.FEW_MATCHES}
