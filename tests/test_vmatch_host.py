"""CPU: the boundary of the verified matcher (okvis_fe_match_verified) and its referee.  With "every pair verifies" the statement over
a distance matrix (tests/vmatch_statement.py) is the descriptor matcher's statement (tests/matcher_statement.py) on every case
recorded from the reference's own DenseMatcher; the entry is exported; a NULL context and every argument outside the documented
limits is OKVIS_BA_ERR_ARG before the context is read or the device is touched (there is none here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matcher_statement as S0  # noqa: E402
import vmatch_statement as VS  # noqa: E402
from okvis_amd import _lib, frontend as F, synthetic  # noqa: E402
from okvis_amd.window import DIST_RADTAN  # noqa: E402

ERR_ARG = -1
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_matcher.npz")


def golden_cases():
    g = np.load(GOLDEN)
    return [{k[len(f"c{i}_"):]: g[k] for k in g.files if k.startswith(f"c{i}_")} for i in range(int(g["n_cases"]))]


@pytest.mark.parametrize("i", range(6))
def test_statement_with_every_pair_verified_is_the_descriptor_matcher(i):
    c = golden_cases()[i]
    args = (c["threshold"], int(c["num_best"]), bool(c["use_ratio"]), c["ratio_threshold"], c["skip_a"], c["skip_b"])
    want_a, want_d, want_calls = S0.match(c["desc_a"], c["desc_b"], *args)
    dist = VS.distance_matrix(S0.hamming_matrix(c["desc_a"], c["desc_b"]), c["threshold"])
    pair_a, pair_dist, calls, lists = VS.match(dist, *args)
    assert (pair_a == want_a).all() and (pair_dist == want_d).all() and calls == want_calls
    # ... and the recorded run itself
    assert (pair_a == c["pair_a"]).all() and (pair_dist == c["pair_dist"]).all()
    assert [(a, b) for a, b, _ in calls] == [tuple(r) for r in c["calls_ab"].tolist()]
    assert len(calls) > 0 and all(len(lst) == int(c["num_best"]) for lst in lists.values())


def test_statement_drops_unverified_pairs():
    ham = np.array([[3, 5, 70], [3, 4, 1]])
    verified = np.array([[0, 1, 1], [1, 1, 0]], bool)
    dist = VS.distance_matrix(ham, 60.0, verified)
    assert dist.tolist() == [[float(VS.FLT_MAX), 5.0, float(VS.FLT_MAX)], [3.0, 4.0, float(VS.FLT_MAX)]]
    pair_a, pair_dist, calls, lists = VS.match(dist, 60.0, 2)
    assert pair_a.tolist() == [1, 0, -1] and calls == [(1, 0, 3.0), (0, 1, 5.0)]
    assert lists[0] == [(1, 5.0), (-1, 60.0)] and lists[1] == [(0, 3.0), (1, 4.0)]


def test_library_exports_the_entry():
    assert "okvis_fe_match_verified" in F.SYMBOLS
    getattr(_lib.lib(), "okvis_fe_match_verified")
    hdr = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert f"#define OKVIS_FE_MATCH_3D2D {F.MATCH_3D2D}" in hdr and f"#define OKVIS_FE_MATCH_2D2D {F.MATCH_2D2D}" in hdr


def test_job_struct_has_the_size_the_c_compiler_gives_it(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "okvis_amd_frontend.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%d %d %d\\n", (int)sizeof(okvis_fe_vmatch_job), (int)offsetof(okvis_fe_vmatch_job, hp_W),\n'
                   "  (int)offsetof(okvis_fe_vmatch_job, tri_flags)); return 0; }\n")
    import subprocess
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t")])
    size, o_hp, o_tri = (int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split())
    assert (size, o_hp, o_tri) == (C.sizeof(F.VMatchJobC), F.VMatchJobC.hp_W.offset, F.VMatchJobC.tri_flags.offset)


def _lib_declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _job(kind, n_a=4, n_b=4, width=64):
    """a valid job of zeros; the arrays it points into"""
    cam = F.camera(synthetic.TEST_INTR_RADTAN, DIST_RADTAN)
    spec = {"kind": kind, "desc_a": np.zeros((n_a, width), np.uint8), "desc_b": np.zeros((n_b, width), np.uint8),
            "kp_a": np.ones((n_a, 3), np.float32), "kp_b": np.ones((n_b, 3), np.float32), "cam_a": cam, "cam_b": cam}
    if kind == F.MATCH_3D2D:
        spec.update(hp_W=np.ones((n_a, 4)), T_CbW=[0, 0, 0, 0, 0, 0, 1], P3=np.eye(3))
    else:
        spec.update(T_AB=[0.1, 0, 0, 0, 0, 0, 1], UOplus=np.eye(6))
    table, keep, out = F.vmatch_job_table([spec])
    return table, (keep, out)


def _call(L, ctx, table, n_jobs=1, desc_bytes=64, num_best=4, use_ratio=0):
    return L.okvis_fe_match_verified(ctx, n_jobs, table, desc_bytes, 10.0, num_best, use_ratio, 1.2)


KINDS = [F.MATCH_3D2D, F.MATCH_2D2D]


@pytest.mark.parametrize("kind", KINDS)
def test_null_context_is_an_argument_error(kind):
    L = _lib_declared()
    table, keep = _job(kind)
    assert _call(L, None, table) == ERR_ARG
    assert L.okvis_fe_match_verified(None, 0, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG


# Arguments are checked before the context is read or the device is touched: the "context" here is a block of zeros.
@pytest.fixture
def fake_ctx():
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("desc_bytes,n_a,n_b,num_best,use_ratio", [(0, 4, 4, 4, 0), (8, 4, 4, 4, 0), (40, 4, 4, 4, 0), (128, 4, 4, 4, 0),
                                                                   (48, -1, 4, 4, 0), (48, 4, -1, 4, 0), (48, 65537, 4, 4, 0),
                                                                   (48, 4, 65537, 4, 0), (48, 4, 4, 0, 0), (48, 4, 4, 9, 0),
                                                                   (48, 4, 4, -1, 0), (48, 4, 4, 1, 1)])
def test_bad_sizes_and_settings(fake_ctx, kind, desc_bytes, n_a, n_b, num_best, use_ratio):
    L = _lib_declared()
    table, keep = _job(kind)
    table[0].n_a, table[0].n_b = n_a, n_b
    assert _call(L, fake_ctx[0], table, 1, desc_bytes, num_best, use_ratio) == ERR_ARG


def test_bad_job_count_and_kind(fake_ctx):
    L = _lib_declared()
    assert L.okvis_fe_match_verified(fake_ctx[0], -1, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG
    assert L.okvis_fe_match_verified(fake_ctx[0], 1, None, 48, 10.0, 4, 0, 0.0) == ERR_ARG
    for kind in (0, 3, -1):
        table, keep = _job(F.MATCH_2D2D)
        table[0].kind = kind
        assert _call(L, fake_ctx[0], table) == ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["cam_a", "cam_b"])
@pytest.mark.parametrize("what", ["model", "fu", "fv", "width", "height"])
def test_bad_camera(fake_ctx, kind, which, what):
    L = _lib_declared()
    table, keep = _job(kind)
    cam = getattr(table[0], which)
    if what == "model":
        cam.model = 17
    elif what == "fu":
        cam.intr[0] = 0.0
    elif what == "fv":
        cam.intr[1] = -1.0
    else:
        setattr(cam, what, 0)
    assert _call(L, fake_ctx[0], table) == ERR_ARG


@pytest.mark.parametrize("kind,field", [(F.MATCH_3D2D, "kp_b"), (F.MATCH_2D2D, "kp_b"), (F.MATCH_2D2D, "kp_a"), (F.MATCH_3D2D, "hp_W"),
                                        (F.MATCH_3D2D, "desc_a"), (F.MATCH_2D2D, "desc_b"), (F.MATCH_3D2D, "pair_a"),
                                        (F.MATCH_2D2D, "pair_dist"), (F.MATCH_3D2D, "accepted")])
def test_null_required_pointer(fake_ctx, kind, field):
    L = _lib_declared()
    table, keep = _job(kind)
    setattr(table[0], field, None)
    assert _call(L, fake_ctx[0], table) == ERR_ARG


def test_uoplus_not_positive_definite(fake_ctx):
    L = _lib_declared()
    for bad in (-np.eye(6), np.zeros((6, 6)), np.diag([1.0, 1, 1, 1, 1, -1e-9])):
        table, keep = _job(F.MATCH_2D2D)
        table[0].UOplus[:] = list(bad.reshape(-1))
        assert _call(L, fake_ctx[0], table) == ERR_ARG
