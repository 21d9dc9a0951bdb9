"""CPU: the boundary of okvis_fe_detect_keypoints_scaled and okvis_fe_detect_scaled_and_describe, their statement and their host
code (cases: tests/detect_scale_cases.py).

  - the entries are declared in the header, listed in SYMBOLS and exported; the header says that the scale space is NOT pinned to
    BRISK and names what it leaves out; the ABI is 7; okvis_fe_detect_job keeps its 88 bytes; the constants of
    okvis_amd/frontend.py are the header's and the kernels';
  - every documented argument error is OKVIS_BA_ERR_ARG on a zeroed fake context, before the device is touched (there is none
    here) and with nothing written, octaves outside 0..4 among them;
  - properties of the statement that need no second implementation: transposition commutes with it; an image whose pixels are
    replicated 2^k times has, on layer l + k, the scores of layer l of the image itself.  (Inversion does not commute above
    layer 0: the +2 rounding of the pyramid is not symmetric.);
  - detect_scaled_image_serial of okvis_amd/csrc/fe_detect_scale.hpp (the per-candidate functions the kernels use), built into
    tests/detect_scale_probe.cpp with -fsanitize=address,undefined and run as a process of its own, equals the statement byte for
    byte on every case; the same program holds the per-candidate functions to hand-made scores."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_cases as DC  # noqa: E402
import detect_scale_cases as SC  # noqa: E402
import detect_scale_statement as SS  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
ENTRIES = ("okvis_fe_detect_keypoints_scaled", "okvis_fe_detect_scaled_and_describe")


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    for entry in ENTRIES:
        assert re.search(r"\bint\s+" + entry + r"\s*\(okvis_fe_context\* ctx,\s*int32_t n_jobs,\s*okvis_fe_detect_scale_job\*", header)
        assert entry in F.SYMBOLS
        getattr(_lib.lib(), entry)
    assert re.search(r"scale\s+space\s+is\s+stated\s+here\s+from\s+its\s+definition\s+and\s+is\s+NOT\s+pinned\s+to\s+BRISK", header)
    assert re.search(r"no\s+intra-octaves,\s+a\s+raw\s+Harris\s+comparison\s+across\s+layers,\s+a\s+linear\s+scale\s+interpolation", header)
    assert re.search(rf"#define\s+OKVIS_FE_DETECT_MAX_OCTAVES\s+{F.DETECT_MAX_OCTAVES}\b", header)
    assert F.DETECT_MAX_OCTAVES == 4 == SS.MAX_OCTAVES and F.DETECT_MAX_LAYERS == 5
    assert C.sizeof(F.DetectJobC) == 88 and C.sizeof(F.DetectScaleJobC) == 144
    old = [f[0] for f in F.DetectJobC._fields_[:9]]
    assert [f[0] for f in F.DetectScaleJobC._fields_[:9]] == old and all(getattr(F.DetectJobC, n).offset == getattr(F.DetectScaleJobC, n).offset for n in old)


def test_the_constants_of_the_wrapper_are_the_kernels():
    src = open(os.path.join(ROOT, "okvis_amd", "csrc", "fe_detect_scale.hpp")).read()
    assert int(re.search(r"\bDET_MAX_OCTAVES\s*=\s*(\d+)", src).group(1)) == F.DETECT_MAX_OCTAVES
    assert '#include "fe_detect.hpp"' in src


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


def _call(ctx, entry, n_images=2, edit=None, n_jobs=None, null_table=False, null_desc=False):
    L = _lib.lib()
    F.declare(L)
    images = [DC.uniform(k, 20 + k, 12 + k) for k in range(n_images)]
    table, keep, out = F.detect_scale_job_table(images, 1, 2, 5, 30, 100, 12.0, want_score=True, want_pyramid=True, want_scale=True)
    desc, keep2, out2 = F.describe_job_table(images, [np.zeros((30, 3), np.float32)] * n_images, rot=[np.zeros(30, np.int32)] * n_images)
    for j in range(n_images):
        table[j].n_keypoints = table[j].n_candidates = table[j].flags = table[j].n_layers = desc[j].n_valid = -77
        table[j].n_layer_candidates[:] = [-77] * 5
    if edit:
        edit(table, desc)
    arrays = [a for o in out + out2 for a in o.values() if a is not None]
    for a in arrays:
        a.view(np.uint8)[...] = 0x5A
    n = len(images) if n_jobs is None else n_jobs
    if entry == ENTRIES[0]:
        rc = L.okvis_fe_detect_keypoints_scaled(ctx, n, None if null_table else table)
    else:
        rc = L.okvis_fe_detect_scaled_and_describe(ctx, n, None if null_table else table, None if null_desc else desc)
    assert all((a.view(np.uint8) == 0x5A).all() for a in arrays)          # nothing is written
    for j in range(n_images):
        assert table[j].n_keypoints == table[j].n_candidates == table[j].flags == table[j].n_layers == desc[j].n_valid == -77
        assert list(table[j].n_layer_candidates) == [-77] * 5
    return rc


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_context_no_jobs_negative_count_and_null_tables(fake_ctx, entry):
    assert _call(None, entry) == ERR_ARG and _call(None, entry, 0) == ERR_ARG
    assert _call(fake_ctx[0], entry, 0) == 0 and _call(fake_ctx[0], entry, 0, null_table=True, null_desc=True) == 0
    assert _call(fake_ctx[0], entry, 2, n_jobs=0) == 0
    assert _call(fake_ctx[0], entry, n_jobs=-1) == ERR_ARG and _call(fake_ctx[0], entry, null_table=True) == ERR_ARG
    if entry == ENTRIES[1]:
        assert _call(fake_ctx[0], entry, null_desc=True) == ERR_ARG


BAD = {"image": [None], "kp": [None], "width": [4, 0, -1, F.DETECT_MAX_DIM + 1], "height": [4, 0, -1, F.DETECT_MAX_DIM + 1],
       "pitch": [20, 0, -1], "threshold": [0, -1, -2 ** 62], "min_dist": [-1, -2 ** 31], "max_keypoints": [0, -1, F.DETECT_MAX_KEYPOINTS + 1],
       "cand_capacity": [0, -1, F.DETECT_MAX_CANDIDATES + 1], "octaves": [-1, F.DETECT_MAX_OCTAVES + 1, 2 ** 31 - 1, -2 ** 31]}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("field,value", [(f, v) for f, vs in BAD.items() for v in vs])
def test_argument_outside_its_documented_limits(fake_ctx, entry, field, value):
    def edit(table, desc):
        setattr(table[1], field, value)           # job 1 is 21 x 13 with pitch 21
    assert _call(fake_ctx[0], entry, edit=edit) == ERR_ARG


@pytest.mark.parametrize("field", ["desc", "flags"])
def test_the_chain_checks_the_describe_jobs_too(fake_ctx, field):
    def edit(table, desc):
        setattr(desc[1], field, None)
    assert _call(fake_ctx[0], ENTRIES[1], edit=edit) == ERR_ARG

    def bad_rot(table, desc):
        C.cast(C.c_void_p(desc[0].rot_in), C.POINTER(C.c_int32))[29] = F.DESCRIBE_ROTATIONS
    assert _call(fake_ctx[0], ENTRIES[1], edit=bad_rot) == ERR_ARG


def test_the_table_builder_lays_a_job_out_as_the_header_does():
    im = DC.with_pitch(np.zeros((11, 23), np.uint8), 13, 1)
    table, keep, out = F.detect_scale_job_table([im], 2 ** 40, 4, 0, F.DETECT_MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES, 7.5, want_score=True, want_pyramid=True)
    t = table[0]
    assert (t.width, t.height, t.pitch, t.image, t.octaves) == (23, 11, 36, im.ctypes.data, 4) and t.threshold == 2 ** 40 and t.kp_size == 7.5
    assert out[0]["kp"].shape == (F.DETECT_MAX_KEYPOINTS, 3) and t.kp == out[0]["kp"].ctypes.data and not t.scale
    assert F.detect_layers(23, 11, 4) == [(23, 11), (11, 5)] and out[0]["score"].shape == (23 * 11 + 11 * 5,) and out[0]["pyramid"].shape == (55,)
    assert F.detect_layers(10, 10, 4) == [(10, 10), (5, 5)] and len(F.detect_layers(9, 9, 4)) == len(F.detect_layers(20, 9, 4)) == 1
    assert len(F.detect_layers(8192, 80, 4)) == 5 and F.detect_layers(8192, 80, 4)[-1] == (512, 5) and len(F.detect_layers(8192, 80, 1)) == 2


# ---- the statement ----------------------------------------------------------------------------------------------------------------
IMAGES = [SC.blurred(1, 67, 45, 4), SC.blurred(3, 97, 64, 6), SC.blurred(4, 80, 80, 3)]
OUTPUTS = ("kp", "response", "pixel", "layer", "scale")


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_the_statement_commutes_with_transposition(k):
    """the row-major tie-break is the one thing that does not: the images have no two survivors with one score on one layer"""
    im = IMAGES[k]
    a = SS.detect(im, 1, 4, 6, 300, 8192, 12.0)
    b = SS.detect(np.ascontiguousarray(im.T), 1, 4, 6, 300, 8192, 12.0)
    assert a["n_layers"] >= 3 and len(a["kp"]) > 10 and len(set(a["layer"])) >= 2
    assert len({(c["S"], c["layer"]) for c in a["survivors"]}) == len(a["survivors"])
    assert all(np.array_equal(x.T, y) for x, y in zip(a["score"], b["score"])) and all(np.array_equal(x.T, y) for x, y in zip(a["pyramid"], b["pyramid"]))
    assert np.array_equal(a["n_layer_candidates"], b["n_layer_candidates"]) and a["n_candidates"] == b["n_candidates"] and a["flags"] == b["flags"]
    assert a["pixel"][:, ::-1].tobytes() == np.ascontiguousarray(b["pixel"]).tobytes() and a["kp"][:, [1, 0, 2]].tobytes() == b["kp"].tobytes()
    assert all(a[n].tobytes() == b[n].tobytes() for n in ("response", "layer", "scale"))


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_replicated_pixels_move_the_scores_up_by_whole_layers(k):
    """I replicated 2^k times per pixel (k = 2): the mean of four equal pixels is the pixel, so layer l + 2 is layer l of I"""
    im = IMAGES[k]
    big = np.repeat(np.repeat(im, 4, axis=0), 4, axis=1)
    small, large = SS.pyramid(im, 2), SS.pyramid(big, 4)
    assert len(small) == 3 and len(large) == 5
    for l in range(3):
        assert np.array_equal(large[l + 2], small[l]) and np.array_equal(SS.S.score(large[l + 2]), SS.S.score(small[l])) and SS.S.score(small[l]).any()


def test_octaves_0_is_the_one_layer_statement():
    for name in ("shapes", "ties", "selection", "capacity"):
        for j, want in zip(DC.cases(name), DC.stated(name)):
            got = SC.state(SC.as_scaled(j))
            DC.check(dict(got, score=got["score"][0]), want, (name,))
            assert got["n_layers"] == 1 and not got["layer"].any() and (got["scale"] == 1.0).all() and got["n_layer_candidates"][0] == want["n_candidates"]


def test_the_cases_are_the_ones_asked_for():
    for name in SC.NAMES:
        assert len(SC.cases(name)) == len(SC.stated(name)) > 0
    assert len(SC.cases("mixed")) == 130 and {j["octaves"] for j in SC.cases("mixed")} == {0, 1, 2, 3, 4}
    shapes = {(j["image"].shape[1], j["image"].shape[0]) for j in SC.cases("shapes")}
    assert shapes == set(SC.SMALL) | set(SC.TILE_EDGE) and all(j["octaves"] == 4 for j in SC.cases("shapes"))
    assert {(j["image"].shape[1], j["image"].shape[0]) for j in SC.cases("long")} == {(8192, 80), (8192, 5), (5, 8192)}
    assert [j["octaves"] for j in SC.cases("waves")] == [0, 1, 2, 3, 4] and SC.cases("waves")[0]["image"].shape == (96, 384)
    assert [s["n_candidates"] for s in SC.stated("counts")] == list(SC.COUNTS)
    assert {j["image"].strides[0] - j["image"].shape[1] for j in SC.cases("pitch")} == {0, 1, 13}


# ---- the header's host code against the statement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("detect_scale_probe")
    return SC.build_probe(d), d


def test_the_per_candidate_functions_on_hand_made_scores(probe):
    done = subprocess.run([probe[0], "--rules"], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_serial_driver_of_the_header_gives_the_statement(probe, name):
    got, want = SC.run_probe(*probe, SC.cases(name), tag=name), SC.stated(name)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        SC.check(g, w, (name, j))


def test_the_serial_driver_at_octaves_0_gives_the_one_layer_statement(probe):
    jobs = DC.cases("mixed") + DC.cases("edges") + DC.cases("counts")
    got = SC.run_probe(*probe, [SC.as_scaled(j) for j in jobs], tag="octaves0")
    for j, (g, w) in enumerate(zip(got, DC.stated("mixed") + DC.stated("edges") + DC.stated("counts"))):
        DC.check(dict(g, score=g["score"][0]), w, ("octaves0", j))
