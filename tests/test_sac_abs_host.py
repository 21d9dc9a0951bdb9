"""CPU: the boundary of okvis_fe_sac_solve_absolute, its referee, and the host side of its core.

  - the entry is declared in the header, listed in SYMBOLS and exported, the ABI is still 7, and the struct as ctypes sees it is
    the struct of the header; every argument outside the documented limits is OKVIS_BA_ERR_ARG before the context is read (the
    "context" is a block of zeros: there is no device here) and nothing is written;
  - the statement (tests/sac_abs_statement.py, mpmath) recovers the true pose on exact scenes, and the float64 numpy evaluation
    is measured against it;
  - at most 2 % of a case's samples are excluded (separation below 1e-3 or margin below 1e-6), on the statement alone;
  - the continuation used for the perturbed inputs (gp3p_near) equals the full statement on them;
  - the float64 statement of the whole rejection returns exactly the true inlier set on the end-to-end scene;
  - the BA_HD core (okvis_amd/csrc/fe_sac_gp3p.hpp) runs on the CPU through tests/sac_abs_probe.cpp, a stand-alone program built
    with -fsanitize=address,undefined (runtime linked statically; nothing is preloaded) and run as a child process, and is held to
    the device's bounds: within 4 max(e64, e_in), candidate counts and validity equal, every candidate a pose that maps the
    three points.

Two world points on one ray of one camera (the last sample of degenerate_case) are not degenerate under the definition: the
three quadrics still have finitely many solutions and the true pose is one of them.  The statement finds it, so such a sample is
held to the statement like any other, not to "invalid"."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_abs_cases as AC  # noqa: E402
import sac_abs_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1
CASES = [(AC.SMALL_SEED, 4, 1, False), (AC.MAIN_SEED, 400, 1, False), (AC.MAIN_SEED, 400, 50, False), (AC.MAIN_SEED, 400, 130, False),
         (AC.FAR_SEED, 400, 50, True)]


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert re.search(r"\bint\s+okvis_fe_sac_solve_absolute\s*\(", header)
    assert "okvis_fe_sac_solve_absolute" in F.SYMBOLS
    getattr(_lib.lib(), "okvis_fe_sac_solve_absolute")
    assert _lib.lib().okvis_ba_abi_version() == 7          # an addition only
    for name, value in (("SAMPLE_ABSOLUTE", F.SAC_SAMPLE_ABSOLUTE), ("MAX_ROOTS_ABSOLUTE", F.SAC_MAX_ROOTS_ABSOLUTE)):
        assert re.search(rf"#define\s+OKVIS_FE_SAC_{name}\s+{value}\b", header)
    assert (F.SAC_SAMPLE_ABSOLUTE, F.SAC_MAX_ROOTS_ABSOLUTE) == (4, 8)
    assert re.search(r"stated from its mathematical definition and is NOT pinned to OpenGV", " ".join(header.replace("*", " ").split()))
    for doc in ("README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "okvis_fe_sac_solve_absolute" in text, doc
        assert "keeps taking caller hypotheses" not in text and "on the host as before" not in text, doc
    assert "What is not here: the generalised P3P" not in header


def test_struct_equals_the_ctypes_view():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    body = re.search(r"typedef struct okvis_fe_sac_absolute_job \{(.*?)\} okvis_fe_sac_absolute_job;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "")]
    assert names == [f[0] for f in F.SacAbsoluteJobC._fields_], names
    assert C.sizeof(F.SacAbsoluteJobC) == 16 + 8 + 16 * 8          # four int32, the threshold, sixteen pointers: no padding


@pytest.fixture
def fake_ctx():
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _job(n=12, k=3):
    return AC.job(AC.case(5, n, k))


def _call(ctx, job, edit=None):
    table, keep, out = F.sac_absolute_job_table([job], want_scores=True, want_candidates=True)
    before = [{k: v.copy() for k, v in o.items()} for o in out]
    if edit:
        edit(table[0])
    rc = _declared().okvis_fe_sac_solve_absolute(ctx, 1, table)
    for o, b in zip(out, before):
        assert all((o[k] == b[k]).all() for k in o)          # nothing written
    return rc


def test_null_context_and_table(fake_ctx):
    L = _declared()
    assert _call(None, _job()) == ERR_ARG
    assert L.okvis_fe_sac_solve_absolute(None, 0, None) == ERR_ARG
    assert L.okvis_fe_sac_solve_absolute(fake_ctx[0], -1, None) == ERR_ARG
    assert L.okvis_fe_sac_solve_absolute(fake_ctx[0], 1, None) == ERR_ARG
    assert L.okvis_fe_sac_solve_absolute(fake_ctx[0], 0, None) == 0          # n_jobs = 0 is valid and touches nothing


@pytest.mark.parametrize("field,value", [("n_models", 0), ("n_models", -1), ("n_models", 1025), ("n", -1), ("n", 0), ("n", 65537),
                                         ("n_cams", 0), ("n_cams", -1), ("n_cams", 9), ("n_cams", 1)])
def test_count_out_of_range(fake_ctx, field, value):
    def edit(t):
        setattr(t, field, value)          # n = 0: no sample index is in range; n_cams = 1: the scene's cam_index holds a 1
    assert _call(fake_ctx[0], _job(), edit) == ERR_ARG


@pytest.mark.parametrize("field", ["points", "bearing", "cam_index", "cam_offsets", "cam_rotations", "samples", "sigma"])
def test_null_input(fake_ctx, field):
    def edit(t):
        setattr(t, field, None)
    assert _call(fake_ctx[0], _job(), edit) == ERR_ARG          # sigma: a consensus output is wanted


@pytest.mark.parametrize("entry,value", [(0, -1), (1, 12), (-1, 1 << 30), (2, -(1 << 31))])
def test_sample_index_out_of_range_is_an_argument_error_not_a_fault(fake_ctx, entry, value):
    job = _job()
    job["samples"] = job["samples"].copy()
    job["samples"].reshape(-1)[entry] = value
    assert _call(fake_ctx[0], job) == ERR_ARG


@pytest.mark.parametrize("entry,value", [(0, -1), (5, 2), (-1, 1 << 30)])
def test_cam_index_out_of_range(fake_ctx, entry, value):
    job = _job()
    job["cam_index"] = job["cam_index"].copy()
    job["cam_index"][entry] = value
    assert _call(fake_ctx[0], job) == ERR_ARG


# ---- the statement -------------------------------------------------------------------------------------------------------------------
def test_statement_recovers_the_true_pose_and_numpy_is_measured_against_it():
    for seed, far in ((AC.MAIN_SEED, False), (AC.FAR_SEED, True)):
        c, st = AC.case(seed, 400, 130, 2, far), AC.stated(seed, 400, 2, far)
        d_true = [S.pose_distance(s["R"], s["t"], c["R"], c["t"]) for s in st]
        e64, e_in = np.array([s["e64"] for s in st]), np.array([s["e_in"] for s in st])
        print(f"far {far}: statement to truth: largest {max(d_true):.3e}; numpy to statement: median {np.median(e64):.3e}, largest {e64.max():.3e}; "
              f"e_in: median {np.median(e_in):.3e}, largest {e_in.max():.3e}; candidates {np.bincount([s['n_roots'] for s in st]).tolist()}, "
              f"real solutions {np.bincount([s['n_real'] for s in st]).tolist()}")
        assert all(s["valid"] for s in st)
        # the inputs are the true ones rounded to double: the exact solution of the rounded problem is within its e_in-sized
        # neighbourhood of the truth (the perturbation there is one rounding per component, as in a draw)
        assert all(d <= 8 * max(s["e_in"], 1e-16) for d, s in zip(d_true, st))
        assert np.isfinite(e64).all() and np.median(e64) < 1e-11
        kinds = [len(set(c["cam_index"][q[:3]])) for q in c["samples"]]
        assert 1 in kinds and 2 in kinds          # central and non-central samples


@pytest.mark.parametrize("seed,n,k,far", CASES)
def test_exclusion_cap(seed, n, k, far):
    st = AC.stated(seed, n, 2, far)[:k]
    n_ex = sum(s["excluded"] for s in st)
    print(f"seed {seed} n {n} samples {k}: {n_ex} excluded; least separation {min(s['separation'] for s in st):.3e}, "
          f"least margin {min(s['margin'] for s in st):.3e}")
    assert n_ex <= S.MAX_EXCLUDED * k


def test_continuation_equals_the_full_statement_on_perturbed_inputs():
    c = AC.case(AC.MAIN_SEED, 400, 2)
    rng = np.random.default_rng(3)
    for q in c["samples"]:
        X, f, off, rot = AC.sample_inputs(c, q)
        base = S.gp3p(X, f, off, rot)
        g = f * (1.0 + rng.choice([-1.0, 1.0], f.shape) * 2.0 ** -53)
        Y = X * (1.0 + rng.choice([-1.0, 1.0], X.shape) * 2.0 ** -53)
        full = S.gp3p(Y, g, off, rot)
        R, t = S.gp3p_near(Y, g, off, rot, base)
        assert S.pose_distance(R, t, full["R"], full["t"]) == 0.0          # both rounded from 60 digits to double


def test_float64_statement_finds_exactly_the_true_inliers():
    job, truth = AC.end_to_end()
    assert len(truth) == 300 and len(job["points"]) == 345 and len(job["samples"]) == 50 and set(job["cam_index"]) == {0, 1}
    assert np.array_equal(AC.end_to_end_float64(), truth)


# ---- the core on the CPU, sanitised ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sac_abs_probe")
    return AC.build_probe(d), d


@pytest.mark.parametrize("seed,n,k,far", [CASES[0], CASES[3], CASES[4]])
def test_probe_within_the_bound(probe, seed, n, k, far):
    c, st = AC.case(seed, n, k, 2, far), AC.stated(seed, n, 2, far)[:k]
    AC.check(c, c["samples"], st, *AC.run_probe(*probe, c, c["samples"]), f"probe seed {seed} n {n} far {far}")


@pytest.mark.parametrize("n_cams,used", [(1, None), (8, (0, 7))])
def test_probe_cameras(probe, n_cams, used):
    c = AC.case(AC.MAIN_SEED + 10 + n_cams, 400, 20, n_cams, False, used)
    assert set(c["cam_index"]) == set(used or (0,))
    st = AC.stated(AC.MAIN_SEED + 10 + n_cams, 400, n_cams, False, used, 20)
    AC.check(c, c["samples"], st, *AC.run_probe(*probe, c, c["samples"]), f"probe {n_cams} cameras")


def test_probe_most_candidates(probe):
    c, q, k, k_real = AC.most_roots()
    st = AC.state(c, q[None], 1)
    valid, roots, T, cands = AC.run_probe(*probe, c, q[None])
    print(f"most candidates among 20000 samples: {k} (most real solutions: {k_real}); the statement finds {st[0]['n_roots']} of "
          f"{st[0]['n_real']} real, the probe {roots[0]}")
    assert k >= 4 and k_real == 8
    AC.check(c, q[None], st, valid, roots, T, cands, "probe most candidates")
    assert st[0]["excluded"] or roots[0] == st[0]["n_roots"] == k


def test_probe_degenerate_samples(probe):
    c, q = AC.degenerate_case()
    valid, roots, T, cands = AC.run_probe(*probe, c, q)
    assert valid.tolist()[:4] == [True, False, False, False]
    assert np.isnan(T[1:4]).all() and (roots[1:4] == 0).all() and np.isnan(cands[1:4]).all()
    st = AC.state(c, q[[0, 4]], 2)          # the plain sample, and two points on one ray: not degenerate under the definition
    assert st[1]["valid"]
    AC.check(c, q[[0, 4]], st, valid[[0, 4]], roots[[0, 4]], T[[0, 4]], cands[[0, 4]], "probe degenerate")
    again = AC.run_probe(*probe, c, q, tag="again")
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((valid, roots, T, cands), again))
