"""CPU: the boundary of okvis_fe_detect_keypoints, its statement and its host code (cases: tests/detect_cases.py).

  - the entry is declared in the header, listed in SYMBOLS and exported; the header says that the detector is NOT pinned to BRISK
    and that the selection rule is not BRISK's; the ABI is 7; the constants of okvis_amd/frontend.py are the header's and the
    kernels';
  - every documented argument error is OKVIS_BA_ERR_ARG on a zeroed fake context, before the device is touched (there is none
    here) and with nothing written;
  - properties of the statement that need no second implementation: transposition, inversion, translation;
  - detect_image_serial of okvis_amd/csrc/fe_detect.hpp (the per-pixel and per-candidate functions the kernels use), built into
    tests/detect_probe.cpp with -fsanitize=address,undefined and run as a process of its own, equals the statement byte for byte
    on every case."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_cases as DC  # noqa: E402
import detect_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
ENTRY = "okvis_fe_detect_keypoints"


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(okvis_fe_context\* ctx", header)
    assert ENTRY in F.SYMBOLS
    getattr(_lib.lib(), ENTRY)
    assert re.search(r"detector\s+is\s+stated\s+here\s+and\s+is\s+NOT\s+pinned\s+to\s+BRISK", header)
    assert re.search(r"this\s+rule\s+is\s+NOT\s+BRISK's", header)
    assert "Frontend.cpp:92-114" in header
    for name, value in (("OVERFLOW", F.DETECT_OVERFLOW), ("FULL", F.DETECT_FULL)):
        assert re.search(rf"#define\s+OKVIS_FE_DETECT_{name}\s+{value}u\b", header)
    for name, value in (("MAX_DIM", F.DETECT_MAX_DIM), ("MAX_KEYPOINTS", F.DETECT_MAX_KEYPOINTS), ("MAX_CANDIDATES", F.DETECT_MAX_CANDIDATES)):
        assert re.search(rf"#define\s+OKVIS_FE_DETECT_{name}\s+{value}\b", header)
    assert F.DETECT_MAX_DIM >= 4096 and F.DETECT_MAX_KEYPOINTS >= 1024
    assert (S.OVERFLOW, S.FULL) == (F.DETECT_OVERFLOW, F.DETECT_FULL)
    assert C.sizeof(F.DetectJobC) == 88


def test_the_constants_of_the_wrapper_are_the_kernels():
    src = open(os.path.join(ROOT, "okvis_amd", "csrc", "fe_detect.hpp")).read()
    value = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", src).group(1))
    assert (value("DET_TILE_X"), value("DET_TILE_Y")) == (F.DETECT_TILE_X, F.DETECT_TILE_Y)
    assert value("DET_SEL_THREADS") == F.DETECT_SELECT_THREADS and value("DET_SEL_THREADS") * value("DET_SEL_PER_LANE") == F.DETECT_MAX_CANDIDATES
    assert (value("DET_MAX_DIM"), value("DET_MAX_KEYPOINTS")) == (F.DETECT_MAX_DIM, F.DETECT_MAX_KEYPOINTS)


def test_abi_is_7():
    header = open(os.path.join(ROOT, "include", "okvis_amd_ba.h")).read()
    assert re.search(r"#define\s+OKVIS_BA_ABI_VERSION\s+7\b", header)
    L = _lib.lib()
    L.okvis_ba_abi_version.restype = C.c_int
    assert L.okvis_ba_abi_version() == 7


@pytest.fixture
def fake_ctx():
    """Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros."""
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _call(ctx, n_images=2, edit=None, n_jobs=None, null_table=False):
    L = _lib.lib()
    F.declare(L)
    images = [DC.uniform(k, 20 + k, 12 + k) for k in range(n_images)]
    table, keep, out = F.detect_job_table(images, 1, 5, 30, 100, 12.0, want_score=True)
    for j in range(n_images):
        table[j].n_keypoints = table[j].n_candidates = table[j].flags = -77
    if edit:
        edit(table)
    for o in out:
        for a in o.values():
            a.view(np.uint8)[...] = 0x5A
    rc = L.okvis_fe_detect_keypoints(ctx, len(images) if n_jobs is None else n_jobs, None if null_table else table)
    assert all((a.view(np.uint8) == 0x5A).all() for o in out for a in o.values())          # nothing is written
    assert all(table[j].n_keypoints == table[j].n_candidates == table[j].flags == -77 for j in range(n_images))
    return rc


def test_null_context_is_an_argument_error():
    assert _call(None) == ERR_ARG
    assert _call(None, 0) == ERR_ARG


def test_no_jobs_is_valid_and_touches_nothing(fake_ctx):
    assert _call(fake_ctx[0], 0) == 0
    assert _call(fake_ctx[0], 0, null_table=True) == 0
    assert _call(fake_ctx[0], 2, n_jobs=0) == 0


def test_negative_count_and_null_table(fake_ctx):
    assert _call(fake_ctx[0], n_jobs=-1) == ERR_ARG
    assert _call(fake_ctx[0], null_table=True) == ERR_ARG


BAD = {"image": [None], "kp": [None], "width": [4, 0, -1, F.DETECT_MAX_DIM + 1], "height": [4, 0, -1, F.DETECT_MAX_DIM + 1],
       "pitch": [20, 0, -1], "threshold": [0, -1, -2 ** 62], "min_dist": [-1, -2 ** 31], "max_keypoints": [0, -1, F.DETECT_MAX_KEYPOINTS + 1],
       "cand_capacity": [0, -1, F.DETECT_MAX_CANDIDATES + 1]}


@pytest.mark.parametrize("field,value", [(f, v) for f, vs in BAD.items() for v in vs])
def test_argument_outside_its_documented_limits(fake_ctx, field, value):
    def edit(table):
        setattr(table[1], field, value)           # job 1 is 21 x 13 with pitch 21
    assert _call(fake_ctx[0], edit=edit) == ERR_ARG


def test_the_table_builder_lays_a_job_out_as_the_header_does():
    """the limits themselves pass the wrapper; the entry is exercised at them on the device (tests/test_gpu_detect.py)"""
    im = DC.with_pitch(np.zeros((5, 7), np.uint8), 13, 1)
    table, keep, out = F.detect_job_table([im], 2 ** 40, 0, F.DETECT_MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES, 7.5)
    t = table[0]
    assert (t.width, t.height, t.pitch, t.image) == (7, 5, 20, im.ctypes.data) and t.threshold == 2 ** 40 and t.kp_size == 7.5
    assert out[0]["kp"].shape == (F.DETECT_MAX_KEYPOINTS, 3) and t.kp == out[0]["kp"].ctypes.data and not t.score


def test_the_wrapper_refuses_what_is_not_an_image():
    for bad in (np.zeros((5, 5), np.int32), np.zeros((5, 5, 1), np.uint8), np.zeros((5, 10), np.uint8)[:, ::2], np.zeros((10, 5), np.uint8)[::-1]):
        with pytest.raises(ValueError):
            F.detect_job_table([bad], 1)


# ---- the statement ----------------------------------------------------------------------------------------------------------------
IMAGES = [DC.uniform(1, 33, 21), DC.uniform(2, 8, 40), DC.patch_image(DC.BEST_PATCH, 40, 30), DC.dot_grid(20)[0]]


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_score_commutes_with_transposition_and_ignores_inversion(k):
    im = IMAGES[k]
    sc = S.score(im)
    assert sc.any()
    assert np.array_equal(S.score(np.ascontiguousarray(im.T)), sc.T)
    assert np.array_equal(S.score(255 - im), sc)


def test_whole_pixel_shifts_shift_candidates_and_keypoints_and_nothing_else():
    base = DC.state(DC.translated(0, 0))
    assert len(base["kp"]) >= 10 and base["n_candidates"] > len(base["kp"])
    for dx, dy in DC.SHIFTS[1:]:
        DC.check_shifted(DC.state(DC.translated(dx, dy)), base, dx, dy)


def test_the_scene_condition_holds_for_the_statement():
    for seed in DC.SCENE_SEEDS:
        for noise in (False, True):
            j, corners = DC.scene(seed, noise)
            st = DC.state(j)
            assert len(corners) == 20 and st["flags"] == 0 and DC.scene_holds(DC.pixels(st), corners), (seed, noise)


def test_the_cases_are_the_ones_asked_for():
    for name in DC.NAMES:
        assert len(DC.cases(name)) == len(DC.stated(name)) > 0
    assert len(DC.cases("mixed")) == 130
    assert {j["image"].strides[0] - j["image"].shape[1] for j in DC.cases("pitch")} == {0, 1, 13}
    assert {63, 64, 65, DC.WAVE - 1, DC.WAVE, DC.WAVE + 1, DC.GROUP - 1, DC.GROUP, DC.GROUP + 1} <= {s["n_candidates"] for s in DC.stated("counts")}
    assert {(j["image"].shape[1], j["image"].shape[0]) for j in DC.cases("shapes")} == set(DC.SHAPES)


# ---- the header's host code against the statement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("detect_probe")
    return DC.build_probe(d), d


@pytest.mark.parametrize("name", DC.NAMES)
def test_the_serial_driver_of_the_header_gives_the_statement(probe, name):
    got, want = DC.run_probe(*probe, DC.cases(name), tag=name), DC.stated(name)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        DC.check(g, w, (name, j))


def test_the_serial_driver_on_the_scenes_and_the_shifts(probe):
    jobs = [DC.scene(seed, noise)[0] for seed in DC.SCENE_SEEDS for noise in (False, True)] + [DC.translated(dx, dy) for dx, dy in DC.SHIFTS]
    for j, (g, job) in enumerate(zip(DC.run_probe(*probe, jobs, tag="scenes"), jobs)):
        DC.check(g, DC.state(job), ("scenes", j))
