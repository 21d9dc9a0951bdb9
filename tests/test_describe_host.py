"""CPU: the boundary of okvis_fe_describe_keypoints / okvis_fe_detect_and_describe, their statement and their host code (cases:
tests/describe_cases.py).

  - both entries are declared in the header, listed in SYMBOLS and exported; the job record's size and the flag values are the
    header's; the header says that the extractor is NOT pinned to BRISK and names Frame.hpp:128-156; the ABI is 7;
  - the library's tables (okvis_fe_describe_tables) equal the statement's own, built from mpmath: 383 pairs, the quarter-turn
    symmetry of cs, the reach of every rotated offset; the committed table file is what the generator writes;
  - every documented argument error is OKVIS_BA_ERR_ARG on a zeroed fake context, before the device is touched (there is none
    here) and with nothing written;
  - the quarter-turn identity on the statement alone, byte for byte for every keypoint; whole-pixel shifts;
  - describe_image_serial of okvis_amd/csrc/fe_describe.hpp (the functions the kernel uses), built into tests/describe_probe.cpp
    with -fsanitize=address,undefined and run as a process of its own, equals the statement byte for byte on every case;
  - the tail of the angle stage (dsc_angle_degrees) rounds once: within half an ulp of the long double value;
  - the seeded angle cases keep the float64 evaluation's share of keypoints near a bin boundary within the cap of 1 %."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import describe_cases as DC  # noqa: E402
import describe_statement as S  # noqa: E402
import detect_cases as DET  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
ENTRIES = ("okvis_fe_describe_keypoints", "okvis_fe_detect_and_describe")


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    for entry in ENTRIES + ("okvis_fe_describe_tables",):
        assert re.search(r"\bint\s+" + entry + r"\s*\(", header)
        assert entry in F.SYMBOLS
        getattr(_lib.lib(), entry)
    words = "stated here from the published BRISK construction and is NOT pinned to BRISK".split()
    assert re.search(r"[\s*]+".join(words), header)            # across the comment's line breaks
    assert "Frame.hpp:128-156" in header and "Frame.hpp:139-150" in header
    for name, value in (("VALID", F.DESCRIBE_VALID), ("ANGLE_UNDEFINED", F.DESCRIBE_ANGLE_UNDEFINED)):
        assert re.search(rf"#define\s+OKVIS_FE_DESCRIBE_{name}\s+{value}u\b", header)
    for name, value in (("BYTES", F.DESCRIBE_BYTES), ("ROTATIONS", F.DESCRIBE_ROTATIONS), ("PAIRS", F.DESCRIBE_PAIRS)):
        assert re.search(rf"#define\s+OKVIS_FE_DESCRIBE_{name}\s+{value}\b", header)
    assert (S.VALID, S.ANGLE_UNDEFINED, S.DESC_BYTES, S.N_ROT, S.N_PAIRS, S.MARGIN) == (
        F.DESCRIBE_VALID, F.DESCRIBE_ANGLE_UNDEFINED, F.DESCRIBE_BYTES, F.DESCRIBE_ROTATIONS, F.DESCRIBE_PAIRS, F.DESCRIBE_MARGIN)
    assert C.sizeof(F.DescribeJobC) == 120
    # the record as the header lays it out: pointers and doubles at multiples of 8
    offs = {n: getattr(F.DescribeJobC, n).offset for n, _ in F.DescribeJobC._fields_}
    assert (offs["image"], offs["width"], offs["n"], offs["kp"], offs["cam"], offs["direction"], offs["rot_in"], offs["n_valid"], offs["desc"],
            offs["angle64"]) == (0, 8, 20, 24, 32, 40, 64, 72, 80, 112)


def test_the_constants_of_the_wrapper_are_the_kernels_and_the_abi_is_7():
    src = open(os.path.join(ROOT, "okvis_amd", "csrc", "fe_describe.hpp")).read()
    value = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", src).group(1))
    assert (value("DSC_POINTS"), value("DSC_PAIRS"), value("DSC_BYTES"), value("DSC_ROTS"), value("DSC_MARGIN")) == (
        F.DESCRIBE_POINTS, F.DESCRIBE_PAIRS, F.DESCRIBE_BYTES, F.DESCRIBE_ROTATIONS, F.DESCRIBE_MARGIN)
    assert re.search(r"#define\s+OKVIS_BA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "okvis_amd_ba.h")).read())
    L = _lib.lib()
    L.okvis_ba_abi_version.restype = C.c_int
    assert L.okvis_ba_abi_version() == 7


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def test_the_librarys_tables_are_the_statements():
    got, want = F.describe_tables(), S.tables()
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert len(got["pairs"]) == 383 and (got["pairs"][:, 0] < got["pairs"][:, 1]).all()
    assert [tuple(p) for p in got["pairs"]] == sorted(tuple(p) for p in got["pairs"])
    cs = got["cs"]
    assert np.array_equal(np.roll(cs, -256, axis=0), np.stack([-cs[:, 1], cs[:, 0]], axis=1))          # cs[j + 256] = (-s_j, c_j)
    dx, dy = S.offsets(np.arange(S.N_ROT))
    reach = np.maximum(np.abs(dx), np.abs(dy)) + want["half"][want["ring"]][None, :]
    assert reach.max() == 177 <= S.MARGIN + 8
    assert np.bincount(got["ring"]).tolist() == list(S.N_RING) and got["half"].tolist() == [10, 16, 19, 27, 30]


def test_the_committed_table_file_is_what_the_generator_writes():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_describe_tables.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


# ---- argument errors ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake_ctx():
    """Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros."""
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


CAM = F.camera([450.0, 450.0, 376.0, 240.0, -0.28, 0.07, 1e-4, 1e-5], 1)


def _tables(n_images=2, with_rot=True, with_cam=False):
    images = [DET.uniform(k, 30 + k, 26 + k) for k in range(n_images)]
    kps = [np.array([[14.0, 13.0, 12.0], [15.5, 12.25, 12.0], [2.0, 2.0, 12.0]], np.float32) for _ in images]
    rot = [np.array([0, 1023, 512], np.int32) for _ in images] if with_rot else None
    table, keep, out = F.describe_job_table(images, kps, CAM if with_cam else None, [0.1, 0.9, 0.3] if with_cam else None, rot,
                                            want=("rot", "angle", "angle64"))
    return images, table, keep, out


def _call(ctx, edit=None, n_jobs=None, null_table=False, n_images=2, **kw):
    L = _lib.lib()
    F.declare(L)
    images, table, keep, out = _tables(n_images, **kw)
    for j in range(n_images):
        table[j].n_valid = -77
    if edit:
        edit(table, keep)
    for o in out:
        for a in o.values():
            a.view(np.uint8)[...] = 0x5A
    rc = L.okvis_fe_describe_keypoints(ctx, n_images if n_jobs is None else n_jobs, None if null_table else table)
    assert all((a.view(np.uint8) == 0x5A).all() for o in out for a in o.values())          # nothing is written
    assert all(table[j].n_valid == -77 for j in range(n_images))
    return rc


def test_null_context_negative_count_and_null_table(fake_ctx):
    assert _call(None) == ERR_ARG and _call(None, n_jobs=0) == ERR_ARG
    assert _call(fake_ctx[0], n_jobs=-1) == ERR_ARG and _call(fake_ctx[0], null_table=True) == ERR_ARG


def test_no_jobs_is_valid_and_touches_nothing(fake_ctx):
    assert _call(fake_ctx[0], n_jobs=0) == 0 and _call(fake_ctx[0], n_jobs=0, null_table=True) == 0


BAD = {"image": [None], "kp": [None], "desc": [None], "flags": [None], "n": [-1, -2 ** 31], "width": [4, 0, -1, F.DETECT_MAX_DIM + 1],
       "height": [4, 0, -1, F.DETECT_MAX_DIM + 1], "pitch": [30, 0, -1], "rot_in": [None]}


@pytest.mark.parametrize("field,value", [(f, v) for f, vs in BAD.items() for v in vs])
def test_argument_outside_its_documented_limits(fake_ctx, field, value):
    def edit(table, keep):
        setattr(table[1], field, value)           # job 1 is 31 x 27 with pitch 31; without rot_in it has no camera either
    assert _call(fake_ctx[0], edit=edit) == ERR_ARG


@pytest.mark.parametrize("value", [-1, 1024, 2 ** 31 - 1, -2 ** 31])
def test_a_rotation_index_outside_its_range(fake_ctx, value):
    def edit(table, keep):
        rot = np.array([5, 6, value], np.int32)
        keep.append(rot)
        table[1].rot_in = rot.ctypes.data
    assert _call(fake_ctx[0], edit=edit) == ERR_ARG


def test_a_camera_that_is_not_one(fake_ctx):
    def edit(table, keep):
        bad = F.camera([0.0, 450.0, 376.0, 240.0], 0)          # fu = 0
        keep.append(bad)
        table[0].cam = C.pointer(bad)
    assert _call(fake_ctx[0], edit=edit, with_rot=False, with_cam=True) == ERR_ARG


def test_the_chain_checks_both_tables(fake_ctx):
    L = _lib.lib()
    F.declare(L)
    images = [DET.uniform(k, 30 + k, 26 + k) for k in range(2)]
    for what in ("det", "desc", "rot", "null_det", "null_desc", "null_ctx"):
        det, keep, out = F.detect_job_table(images, 1, 5, 30, 100, 12.0)
        rot = [np.zeros(30, np.int32) for _ in images]
        table, keep2, out2 = F.describe_job_table(images, [np.zeros((30, 3), np.float32)] * 2, None, None, rot)
        if what == "det":
            det[1].threshold = 0
        elif what == "desc":
            table[1].desc = None
        elif what == "rot":
            rot[1][29] = 1024          # row 29 = max_keypoints - 1: the whole capacity is checked
        for o in out + out2:
            for a in o.values():
                if a is not None:
                    a.view(np.uint8)[...] = 0x5A
        rc = L.okvis_fe_detect_and_describe(None if what == "null_ctx" else fake_ctx[0], 2, None if what == "null_det" else det,
                                            None if what == "null_desc" else table)
        assert rc == ERR_ARG, what
        assert all((a.view(np.uint8) == 0x5A).all() for o in out + out2 for a in o.values() if a is not None)
    assert L.okvis_fe_detect_and_describe(fake_ctx[0], 0, None, None) == 0


def test_the_table_builder_lays_a_job_out_as_the_header_does():
    im = DET.with_pitch(np.zeros((25, 27), np.uint8), 13, 1)
    kp = np.array([[12.0, 12.0]], np.float32)
    table, keep, out = F.describe_job_table([im], [kp], CAM, [0.0, 1.0, 0.0], None, want=("angle64",))
    t = table[0]
    assert (t.width, t.height, t.pitch, t.image, t.n) == (27, 25, 40, im.ctypes.data, 1) and list(t.direction) == [0.0, 1.0, 0.0]
    assert t.cam.contents.model == 1 and not t.rot_in and not t.rot and not t.angle and t.angle64 == out[0]["angle64"].ctypes.data
    with pytest.raises(ValueError):
        F.describe_job_table([im], [kp], None, None, None)
    with pytest.raises(ValueError):
        F.describe_job_table([np.zeros((25, 27), np.int32)], [kp], None, None, [np.zeros(1, np.int32)])


# ---- the statement --------------------------------------------------------------------------------------------------------------
def test_the_quarter_turn_identity_on_the_statement():
    a, b = DC.quarter_turn()
    sa, sb = DC.state(a), DC.state(b)
    assert sa["n_valid"] == sb["n_valid"] == len(a["kp"]) == 40 and sa["desc"].any(axis=1).all()
    assert sa["desc"].tobytes() == sb["desc"].tobytes()
    assert np.array_equal(sa["V"], sb["V"])                    # every sample, not only their order


def test_whole_pixel_shifts_leave_the_descriptors_alone():
    base = DC.state(DC.shifted(0, 0))
    assert base["n_valid"] == 30 and base["desc"].any(axis=1).all()
    for dx, dy in DC.SHIFTS[1:]:
        assert DC.state(DC.shifted(dx, dy))["desc"].tobytes() == base["desc"].tobytes(), (dx, dy)


def test_descriptor_distances_behave():
    """neighbouring rotation indices and a quarter-pixel shift are close, unrelated points are far"""
    bits = lambda a, b: int(np.unpackbits(a ^ b).sum())
    d = DC.stated("rot")[0]["desc"]
    assert np.median([bits(d[i], d[(i + 1) % S.N_ROT]) for i in range(S.N_ROT)]) <= 4
    im = DC.cases("rot")[0]["image"]
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(13, 50, 60), rng.uniform(13, 50, 60)], axis=1)
    p = DC.state(DC.job(im, pts, 0))["desc"]
    q = DC.state(DC.job(im, pts + [0.25, 0.0], 0))["desc"]
    near, far = np.median([bits(a, b) for a, b in zip(p, q)]), np.median([bits(p[i], p[(i + 7) % 60]) for i in range(60)])
    assert near < 40 < 100 < far, (near, far)


def test_the_cases_are_the_ones_asked_for():
    for name in DC.NAMES:
        assert len(DC.cases(name)) == len(DC.stated(name)) > 0
    assert len(DC.cases("mixed")) == 130 and len(DC.cases("rot")[0]["kp"]) == 1024 and len(DC.cases("phase")[0]["kp"]) == 256
    assert {j["image"].shape for j in DC.cases("edge")} >= {(23, 23), (40, 23), (23, 40)}
    assert [len(j["kp"]) for j in DC.scene()] == [400, 400] and DC.scene()[0]["image"].shape == (480, 752)


# ---- the angle stage's cases ----------------------------------------------------------------------------------------------------
def test_the_angle_cases_are_the_ones_asked_for_and_stay_within_the_cap():
    cases, st = DC.angle_cases(), DC.stated_angles()
    assert {c["cam"]["model"] for c in cases} == {0, 1, 2, 3} and len(cases) == 20
    undefined = 0
    for c, s in zip(cases, st):
        live = s["defined"]
        undefined += int((~live).sum())
        assert np.isfinite(s["bound"][live]).all() and live.sum() >= 190, c["name"]
        # the float64 evaluation is itself held to what the device is: its own rot differs from the statement's only near a boundary
        rot_np = S.rot_of_angle(s["angle_np"].astype(np.float32))
        assert np.array_equal(rot_np[live & ~s["near_boundary"]], s["rot"][live & ~s["near_boundary"]]), c["name"]
        assert (live & s["near_boundary"]).sum() <= 0.01 * len(live), (c["name"], int(s["near_boundary"].sum()))
        if c["name"].endswith("/axis"):
            d = c["direction"]
            assert 0 < np.hypot(d[0], d[1]) / abs(d[2]) < 1e-6
        if c["name"].endswith("/along_ray"):
            assert s["bound"][0] > 1e3 * np.median(s["bound"][1:][live[1:]])       # eg ~ 0 at keypoint 0: the angle there means nothing
    assert undefined >= 4                                                         # backProject fails somewhere


# ---- the header's host code against the statement -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("describe_probe")
    return DC.build_probe(d), d


@pytest.mark.parametrize("name", DC.NAMES)
def test_the_serial_driver_of_the_header_gives_the_statement(probe, name):
    got, want = DC.run_probe(*probe, DC.cases(name), tag=name), DC.stated(name)
    assert len(got) == len(want) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        DC.check(g, w, (name, j))


def test_the_serial_driver_on_the_scene_the_shifts_and_the_turn(probe):
    jobs = DC.scene() + [DC.shifted(dx, dy) for dx, dy in DC.SHIFTS] + list(DC.quarter_turn())
    for j, (g, job) in enumerate(zip(DC.run_probe(*probe, jobs, tag="scene"), jobs)):
        DC.check(g, DC.state(job), ("scene", j))


def test_the_angles_tail_of_the_header_rounds_once(probe):
    """dsc_angle_degrees(y, x) is atan2(y, x) / M_PI * 180 rounded to the nearest double: within half an ulp of the long double
    value (whose own 2^-64 is the 0.001 on top), where the three operations in double reach 2 ulp; over all directions, twelve
    decades of magnitude, the table's angles and the middles between them, and the neighbourhood of +-180 and +-90 degrees"""
    rng = np.random.default_rng(1)
    n = 100000
    ang, r = rng.uniform(-np.pi, np.pi, n), 10.0 ** rng.uniform(-6, 6, n)
    k = np.arange(-64, 65) * np.pi / 64
    y = np.concatenate([r * np.sin(ang), np.sin(k), np.sin(k + np.pi / 128), [1e-14, -1e-14, 3.0, -3.0, 0.0, -0.0, 2.0, -2.0, 0.0]])
    x = np.concatenate([r * np.cos(ang), np.cos(k), np.cos(k + np.pi / 128), [-400.0, -400.0, 1e-13, -1e-13, -1.0, -1.0, 0.0, 0.0, 5.0]])
    got = DC.run_angle_probe(*probe, y, x)
    LD = S.T.LD
    want = np.arctan2(LD(y), LD(x)) / LD(np.float64(np.pi)) * LD(180)
    ulp = np.spacing(np.maximum(np.abs(np.asarray(want, np.float64)), np.finfo(np.float64).tiny))
    d = np.abs(np.asarray(LD(got) - want, np.float64)) / ulp
    plain = np.abs(np.asarray(LD(np.arctan2(y, x) / np.pi * 180.0) - want, np.float64)) / ulp
    assert d.max() <= 0.501 and plain.max() > 1.0, (d.max(), plain.max())
    assert got[-5:].tolist() == [180.0, -180.0, 90.0, -90.0, 0.0] and (np.abs(got) <= 180.0).all()

