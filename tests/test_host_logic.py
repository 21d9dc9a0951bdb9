"""CPU tests of the product's host side: the C-ABI library loads and exports every symbol the header
declares, fails loudly without a GPU, and the structure building (what replaces okvis::ceres::Map's
bookkeeping, reference okvis_ceres/src/Map.cpp:292-565) produces the documented ordering."""
import ctypes as C
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

from okvis_amd import _lib, solver, synthetic
from okvis_amd.window import OptionsC, WindowC, default_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    hdr = open(os.path.join(ROOT, "include", "okvis_amd_ba.h")).read()
    declared = set(re.findall(r"\b(okvis_ba_[a-z_]+)\s*\(", hdr))
    declared -= {"okvis_ba_array"}
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert set(_lib.SYMBOLS) == declared
    assert L.okvis_ba_abi_version() == 7


def test_struct_layout_matches_header():
    # sizes computed by the C compiler for the same header (guards the ctypes mirror)
    import subprocess, tempfile
    src = '#include <stdio.h>\n#include "okvis_amd_ba.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(okvis_ba_window),sizeof(okvis_ba_options),sizeof(okvis_ba_summary),sizeof(okvis_ba_limits),sizeof(okvis_ba_marg_spec),sizeof(okvis_ba_marg_result));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).split()
    from okvis_amd.window import LimitsC, MargResultC, MargSpecC, SummaryC
    assert [int(x) for x in out] == [C.sizeof(WindowC), C.sizeof(OptionsC), C.sizeof(SummaryC), C.sizeof(LimitsC),
                                     C.sizeof(MargSpecC), C.sizeof(MargResultC)]


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    h = C.c_void_p()
    assert L.okvis_ba_create(C.byref(h), 0) == -4          # OKVIS_BA_ERR_NO_DEVICE
    with pytest.raises(_lib.BackendError):
        solver.WindowBatch([synthetic.small_window()])


def test_default_options_match_python_mirror():
    o = OptionsC()
    _lib.lib().okvis_ba_default_options(C.byref(o))
    d = default_options()
    for n, _ in OptionsC._fields_:
        if n == "tuning":     # (a nested record: all zero = the library's defaults)
            assert bytes(o.tuning) == bytes(d.tuning) == bytes(C.sizeof(o.tuning))
            continue
        assert getattr(o, n) == getattr(d, n), n


@pytest.mark.parametrize("ext,expD", [("fixed", 4 * 15), ("shared", 4 * 15 + 12), ("perframe", 4 * 15 + 4 * 12)])
def test_structure_building_matches_oracle_ordering(oracle, ext, expD):
    w = synthetic.small_window(seed=5, K=4, L=40, estimate_extrinsics=ext)
    st = solver.check_window(w)
    o = oracle.OracleWindow(w)
    assert st["D"] == expD == o.D == w.reduced_dim()
    assert st["n_pair"] == o.n_pair
    assert st["n_group"] >= 1 and st["n_chunk"] >= 1


def test_config_A_structure():
    st = solver.check_window(synthetic.config_A())
    assert st["D"] == 150 and st["Dp"] == 60 and st["n_pair"] == 4000
    assert st["n_group"] == 34          # 12 landmarks x 20 observations per 256-lane group
    assert st["arena_bytes"] < 4 << 20


def test_upload_validation_errors():
    w = synthetic.small_window(seed=6)
    L = _lib.lib()

    def status(win):
        wc, keep = win.as_c()
        return L.okvis_ba_check_window(C.byref(wc), None, None)
    assert status(w) == 0
    import copy
    bad = copy.deepcopy(w); bad.obs_lm = bad.obs_lm[::-1].copy()          # unsorted
    assert status(bad) == -1
    bad = copy.deepcopy(w); bad.obs_pose = bad.obs_pose.copy(); bad.obs_pose[0] = 99   # out of range
    assert status(bad) == -1
    rep = copy.deepcopy(w)                                                 # a repeated (landmark, pose, cam) triple is legal:
    for n in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_uv", "obs_sqrtw"):   # two keypoints of one image matched to one landmark
        a = getattr(rep, n); setattr(rep, n, np.concatenate([a[:1], a]))
    assert status(rep) == 0
    bad = copy.deepcopy(w); bad.imu_s_count = bad.imu_s_count.copy(); bad.imu_s_count[0] = 5   # samples do not reach t1
    assert status(bad) == -1
    # the observation pass is one walk, landmark by landmark: the first offending observation decides, in list order
    first = int(np.flatnonzero(w.obs_lm == w.obs_lm[0]).size)              # observations of landmark 0
    assert first >= 2
    bad = copy.deepcopy(w); bad.obs_pose = bad.obs_pose.copy(); bad.obs_pose[[0, first - 1]] = bad.obs_pose[[first - 1, 0]]
    assert status(bad) == -1                                               # poses of one landmark out of order
    same = np.flatnonzero((w.obs_lm[1:] == w.obs_lm[:-1]) & (w.obs_pose[1:] == w.obs_pose[:-1]))
    if same.size:                                                          # cameras of one (landmark, pose) out of order
        bad = copy.deepcopy(w); bad.obs_cam = bad.obs_cam.copy(); i = int(same[0]); bad.obs_cam[[i, i + 1]] = bad.obs_cam[[i + 1, i]]
        assert status(bad) == -1
    bad = copy.deepcopy(w); bad.obs_lm = bad.obs_lm.copy(); bad.obs_lm[-1] = w.n_lm   # landmark out of range
    assert status(bad) == -1
    bad = copy.deepcopy(w); bad.obs_lm = bad.obs_lm.copy(); bad.obs_lm[-1] = -1
    assert status(bad) == -1
    bad = copy.deepcopy(w); bad.obs_cam = bad.obs_cam.copy(); bad.obs_cam[3] = len(w.cam_model)
    assert status(bad) == -1
    bad = copy.deepcopy(w); bad.obs_ext = bad.obs_ext.copy(); bad.obs_ext[-1] = bad.obs_pose[0]   # a block in both roles
    assert status(bad) == -3
    bad = copy.deepcopy(w); bad.obs_ext = bad.obs_ext.copy(); bad.obs_ext[2] = bad.obs_pose[2]   # pose = extrinsics
    assert status(bad) == -3
    # a role conflict early in the list is reported although a later observation is out of range (and the other way round)
    bad = copy.deepcopy(w); bad.obs_ext = bad.obs_ext.copy(); bad.obs_pose = bad.obs_pose.copy()
    bad.obs_ext[1] = bad.obs_pose[0]; bad.obs_pose[-1] = 99
    assert status(bad) == -3
    bad = copy.deepcopy(w); bad.obs_ext = bad.obs_ext.copy(); bad.obs_pose = bad.obs_pose.copy()
    bad.obs_pose[0] = 99; bad.obs_ext[-1] = w.obs_pose[-1]
    assert status(bad) == -1
    big = synthetic.make_window(3, 5, 1.0, 1)
    big.obs_lm = np.zeros(300, np.int32)                                   # > 256 observations of one landmark
    big.obs_pose = np.arange(300, dtype=np.int32) % 3
    assert status(big) in (-1, -3)
    # too large a reduced system for the LDS solver is reported, not silently mis-solved
    assert status(synthetic.make_window(20, 30, 1.0, 2, frame_dt=0.1)) == 0      # D = 300: HBM-resident solve path
    assert status(synthetic.make_window(64, 30, 0.5, 2, frame_dt=0.05)) == -3    # D = 960 > 900


def test_malformed_windows_are_refused_before_they_are_read():
    """The argument check the index build (okvis_ba_check_window / okvis_ba_upload) and the window container (okvis_ba_store_*) share
    (check_window_args, ba_store.hpp) runs before either reads anything through an index: every window below is
    OKVIS_BA_ERR_ARG (-1) from both.  The index build used to read pose_off / sb_off with the IMU terms' and the pose priors' block
    indices before it checked them, and took a null array with a non-zero count for an empty one."""
    import copy
    L = _lib.lib()

    def both(win, edit=None):
        wc, keep = win.as_c()
        if edit is not None:
            edit(wc)
        h = C.c_void_p()
        rs = L.okvis_ba_store_create(C.byref(wc), C.byref(h))
        if rs == 0:
            L.okvis_ba_store_destroy(h)
        return L.okvis_ba_check_window(C.byref(wc), None, None), rs

    w = synthetic.small_window(seed=6)
    rng = np.random.default_rng(6)
    w.rel_pose0, w.rel_pose1, w.rel_sqrtinfo = np.array([0], np.int32), np.array([1], np.int32), np.eye(6).reshape(1, 36)
    w.marg_J, w.marg_e0 = np.triu(rng.standard_normal((15, 15))), rng.standard_normal(15) * 0.1   # a prior over pose 0 and speed/bias 0
    w.marg_block_type, w.marg_block_idx, w.marg_block_off = (np.array(a, np.int32) for a in ([0, 1], [0, 0], [0, 6]))
    w.marg_lin = np.zeros((2, 9)); w.marg_lin[0, :7] = w.pose[0]; w.marg_lin[1] = w.sb[0]
    assert both(w) == (0, 0) and w.n_imu > 0 and len(w.pprior_pose) > 0 and len(w.sbprior_sb) > 0

    def with_entry(name, i, v):
        bad = copy.deepcopy(w)
        a = np.array(getattr(bad, name)); a[i] = v; setattr(bad, name, a)
        return bad
    # block indices out of range, above and below
    for name, n in (("imu_pose0", w.n_pose), ("imu_pose1", w.n_pose), ("imu_sb0", w.n_sb), ("imu_sb1", w.n_sb), ("pprior_pose", w.n_pose),
                    ("sbprior_sb", w.n_sb), ("rel_pose0", w.n_pose), ("rel_pose1", w.n_pose)):
        for v in (n, 50_000_000, -1, -3):
            assert both(with_entry(name, 0, v)) == (-1, -1), (name, v)
    for i, n in ((0, w.n_pose), (1, w.n_sb)):
        for v in (n, -1):
            assert both(with_entry("marg_block_idx", i, v)) == (-1, -1), (i, v)
    assert both(with_entry("marg_block_off", 1, 7)) == (-1, -1)      # the block's columns end behind marg_dim
    assert both(with_entry("marg_block_type", 1, 7)) == (-1, -1)     # neither OKVIS_BA_BLOCK_POSE nor _SPEEDBIAS
    # IMU samples outside the sample arrays (64-bit: begin + count does not wrap)
    assert both(with_entry("imu_s_begin", 0, 2**31 - 1)) == (-1, -1) and both(with_entry("imu_s_begin", 0, -1)) == (-1, -1)
    # a null array with a non-zero count
    for field in ("imu_pose0", "imu_sb1", "imu_t0", "imu_s_count", "imu_s_t", "imu_s_gyr", "imu_s_acc", "pprior_pose", "pprior_meas",
                  "pprior_sqrtinfo", "sbprior_sb", "sbprior_meas", "sbprior_sqrtinfo", "rel_pose0", "rel_pose1", "rel_sqrtinfo",
                  "marg_J", "marg_e0", "marg_lin", "marg_block_off"):
        assert both(w, lambda wc: setattr(wc, field, None)) == (-1, -1), field
    # negative counts
    for field in ("n_pprior", "n_sbprior", "n_relpose", "n_imu", "marg_dim"):
        assert both(w, lambda wc: setattr(wc, field, -1)) == (-1, -1), field
    # two defects: the argument check comes first (capi_index_build.inc), so a malformed argument decides although the observation
    # walk alone would report a block in both roles (-3, see test_upload_validation_errors)
    bad = with_entry("obs_ext", -1, w.obs_pose[0])
    assert both(bad)[0] == -3
    for name in ("imu_pose0", "pprior_pose"):
        worse = copy.deepcopy(bad)
        a = np.array(getattr(worse, name)); a[0] = w.n_pose; setattr(worse, name, a)
        assert both(worse) == (-1, -1)
    # ... and what only the index build requires comes behind it: fewer than two samples is its rule, not the container's
    assert both(with_entry("imu_s_count", 0, 1)) == (-1, 0)


def test_window_validate_rejects_bad_input():
    w = synthetic.small_window(seed=7)
    w.obs_lm = w.obs_lm.copy(); w.obs_lm[3] = 10**6
    with pytest.raises(ValueError):
        w.validate()


def test_header_is_plain_c_and_links_from_c(tmp_path):
    # the drop-in boundary is a C ABI: the header must compile as strict C99 and the library link from a C program
    import subprocess
    src = tmp_path / "t.c"
    src.write_text(
        '#include "okvis_amd_ba.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  okvis_ba_options o; okvis_ba_limits l; okvis_ba_solver* s = 0;\n"
        "  okvis_ba_default_options(&o); okvis_ba_get_limits(&l);\n"
        "  int rc = okvis_ba_create(&s, 0);\n"
        '  printf("%d %d %d %s\\n", okvis_ba_abi_version(), (int)l.max_reduced_dim, rc, okvis_ba_error_string(rc));\n'
        "  if (rc == 0) okvis_ba_destroy(s);\n"
        "  return 0;\n}\n")
    libdir = os.path.join(ROOT, "okvis_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lokvis_amd_ba", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)]).decode().split(None, 3)
    assert int(out[0]) == 7 and int(out[1]) == 900
    import torch
    if not torch.cuda.is_available():
        assert int(out[2]) == -4 and "no CPU path" in out[3]      # fails loudly without a GPU


def test_null_solver_is_an_argument_error_everywhere():
    """Entry points check their handle before touching the device (no GPU needed): OKVIS_BA_ERR_ARG = -1."""
    L = _lib.lib()
    assert L.okvis_ba_fetch_results(None, 0, None, None, None, None, None) == -1
    assert L.okvis_ba_get_state(None, 0, None, None, None) == -1
    assert L.okvis_ba_begin(None) == -1
    assert L.okvis_ba_iterate(None, 1) == -1
    assert L.okvis_ba_finish(None, None) == -1
    assert L.okvis_ba_marginalize(None, 0, None, None) == -1
    assert L.okvis_ba_marginalize_begin(None, 0, None, None) == -1 and L.okvis_ba_marginalize_end(None, None) == -1
    assert L.okvis_ba_fetch_imu_caches(None, 0, None) == -1
    import ctypes as C
    n = C.c_int64()
    assert L.okvis_ba_check_window_lists(None, None, 1, 0, None, 0, C.byref(n)) == -1


def test_okvis_adapter_compiles_against_the_interface():
    """okvis_estimator_adapter.hpp against stand-in declarations of the Eigen / OKVIS types it touches
    (tests/mock_okvis/, signatures of the reference's VioBackendInterface.hpp:67-336 etc.): well-formed, every pure
    virtual overridden with the exact signature (the class is instantiated), addObservation<> instantiates."""
    import shutil
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    root = pathlib.Path(__file__).resolve().parents[1]
    cmd = [gxx, "-std=c++17", "-Wall", "-Werror", "-c", "-o", os.devnull, "-I", str(root / "tests" / "mock_okvis"),
           "-I", str(root / "include"), "-I", str(root / "okvis_amd" / "csrc" / "host"),
           str(root / "tests" / "mock_okvis" / "adapter_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_record_gather_checks_its_arguments_and_times_out_without_an_id_file(tmp_path):
    """okvis_ba_gather_records before any device is touched: bad ranks are argument errors; a rank > 0 whose rank 0 never
    publishes the ncclUniqueId gives up after timeout_s with a state error instead of hanging"""
    import ctypes as C
    import time
    from okvis_amd.dist import WindowRecordC
    L = _lib.lib()
    L.okvis_ba_gather_records.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_char_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p]
    mine, out = (WindowRecordC * 2)(), (WindowRecordC * 4)()
    assert L.okvis_ba_gather_records(2, 2, 0, b"x", 0.1, mine, 2, out) == -1          # rank out of range
    assert L.okvis_ba_gather_records(0, 2, 0, None, 0.1, mine, 2, out) == -1          # two ranks need an id file
    assert L.okvis_ba_gather_records(0, 1, 0, None, 0.1, mine, 0, out) == 0           # nothing to gather
    t = time.time()
    assert L.okvis_ba_gather_records(1, 2, 0, os.fsencode(str(tmp_path / "never")), 0.2, mine, 2, out) == -2
    assert 0.15 < time.time() - t < 5.0


def test_record_gather_id_file_belongs_to_one_gather(tmp_path):
    """Two ranks without a device (this container): rank 0 replaces a stale id file left by an earlier job before it publishes
    its own, rank 1 picks the id up within its time-out, both then fail alike at the first device call (OKVIS_BA_ERR_NO_DEVICE,
    not a hang in ncclCommInitRank), and rank 0 leaves no file behind."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a host without a GPU: with one, two ranks on the same device cannot form a communicator")
    idf = tmp_path / "nccl_id"
    idf.write_bytes(b"\x55" * 128)   # a crashed job's left-over
    code = (
        "import ctypes as C, os, sys\n"
        "sys.path.insert(0, %r)\n"
        "from okvis_amd import _lib\n"
        "from okvis_amd.dist import WindowRecordC\n"
        "L = _lib.lib()\n"
        "L.okvis_ba_gather_records.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_char_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p]\n"
        "mine, out = (WindowRecordC * 1)(), (WindowRecordC * 2)()\n"
        "print(L.okvis_ba_gather_records(int(sys.argv[1]), 2, 0, os.fsencode(sys.argv[2]), 20.0, mine, 1, out))\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p0 = subprocess.Popen([sys.executable, "-c", code, "0", str(idf)], stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in p0.communicate(timeout=120)[0].strip().splitlines() if ln.strip().lstrip("-").isdigit()]
    # rank 0 fails for want of a device (in ncclGetUniqueId: OKVIS_BA_ERR_STATE, or at the first HIP call: _NO_DEVICE; without a
    # librccl.so: _UNSUPPORTED) — and the stale id is gone: a rank 1 started now times out instead of joining a dead communicator
    assert lines and int(lines[-1]) in (-2, -3, -4), lines
    assert not idf.exists()
