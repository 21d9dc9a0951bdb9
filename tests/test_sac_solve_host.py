"""CPU: the boundary of okvis_fe_sac_solve, its referee, and the host side of its core.

  - the entry is declared in the header, listed in SYMBOLS and exported; every argument outside the documented limits is
    OKVIS_BA_ERR_ARG before the context is read (the "context" is a block of zeros: there is no device here);
  - the statement (tests/sac_solve_statement.py, mpmath) recovers the true pose on exact scenes, and the float64 numpy evaluation
    is measured against it;
  - at most 2 % of a case's samples are excluded (separation below 1e-3 or margin below 1e-6), on the statement alone;
  - the continuation used for the perturbed bearings (five_point_near) equals the full statement on them;
  - the two-point statement returns a rotation with R f2 = f1 for the first sample index to 1e-15;
  - the float64 statement of the whole rejection returns exactly the true inlier set on the end-to-end scenes;
  - the BA_HD core (okvis_amd/csrc/fe_sac_solve.hpp) runs on the CPU through tests/sac_solve_probe.cpp, a stand-alone program
    built with -fsanitize=address,undefined (runtime linked statically; nothing is preloaded) and run as a child process, and is
    held to the device's bounds: two-point bit for bit, five-point within 4 max(e64, e_in), root counts and validity equal."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_solve_cases as SC  # noqa: E402
import sac_solve_statement as S  # noqa: E402
from okvis_amd import _lib, frontend as F  # noqa: E402

ERR_ARG = -1


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert re.search(r"\bint\s+okvis_fe_sac_solve\s*\(", header)
    assert "okvis_fe_sac_solve" in F.SYMBOLS
    getattr(_lib.lib(), "okvis_fe_sac_solve")
    for name, value in (("SAMPLE_ROTATION_ONLY", F.SAC_SAMPLE_ROTATION_ONLY), ("SAMPLE_RELATIVE", F.SAC_SAMPLE_RELATIVE),
                        ("MAX_ROOTS", F.SAC_MAX_ROOTS)):
        assert re.search(rf"#define\s+OKVIS_FE_SAC_{name}\s+{value}\b", header)
    assert re.search(r"both solvers are stated\s+(\*\s+)?from their published mathematical definitions and are NOT pinned to OpenGV", header)
    for doc in ("README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().split())
        assert "stated from their published mathematical definitions and are **not pinned to OpenGV**" in text, doc
    # the struct as ctypes sees it is the struct of the header: same fields in the same order
    body = re.search(r"typedef struct okvis_fe_sac_solve_job \{(.*?)\} okvis_fe_sac_solve_job;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "")]
    assert names == [f[0] for f in F.SacSolveJobC._fields_], names


@pytest.fixture
def fake_ctx():
    block = C.create_string_buffer(256)
    return C.cast(block, C.c_void_p), block


def _declared():
    L = _lib.lib()
    F.declare(L)
    return L


def _job(kind, n=12, k=3):
    c = SC.case(5, n, k)
    return SC.relative_job(c) if kind == F.SAC_RELATIVE else SC.rotation_job(c)


def _call(ctx, job, edit=None, **kw):
    table, keep, out = F.sac_solve_job_table([job], **kw)
    before = [{k: v.copy() for k, v in o.items()} for o in out]
    if edit:
        edit(table[0])
    rc = _declared().okvis_fe_sac_solve(ctx, 1, table)
    for o, b in zip(out, before):
        assert all((o[k] == b[k]).all() for k in o)          # nothing written
    return rc


KINDS = [F.SAC_ROTATION_ONLY, F.SAC_RELATIVE]


@pytest.mark.parametrize("kind", KINDS)
def test_null_context_and_table(fake_ctx, kind):
    L = _declared()
    assert _call(None, _job(kind)) == ERR_ARG
    assert L.okvis_fe_sac_solve(None, 0, None) == ERR_ARG
    assert L.okvis_fe_sac_solve(fake_ctx[0], -1, None) == ERR_ARG
    assert L.okvis_fe_sac_solve(fake_ctx[0], 1, None) == ERR_ARG
    assert L.okvis_fe_sac_solve(fake_ctx[0], 0, None) == 0          # n_jobs = 0 is valid and touches nothing


@pytest.mark.parametrize("kind", [-1, F.SAC_ABSOLUTE, 3, 7])
def test_bad_kind(fake_ctx, kind):
    def edit(t):
        t.kind = kind
    assert _call(fake_ctx[0], _job(F.SAC_RELATIVE), edit) == ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_models", [0, -1, 1025])
def test_bad_number_of_samples(fake_ctx, kind, n_models):
    def edit(t):
        t.n_models = n_models
    assert _call(fake_ctx[0], _job(kind), edit) == ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [-1, 0, 65537])
def test_bad_number_of_correspondences(fake_ctx, kind, n):
    def edit(t):
        t.n = n          # n = 0: no sample index is in range
    assert _call(fake_ctx[0], _job(kind), edit) == ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", ["bearing1", "bearing2", "samples", "sigma1", "sigma2"])
def test_null_input(fake_ctx, kind, field):
    def edit(t):
        setattr(t, field, None)
    assert _call(fake_ctx[0], _job(kind), edit) == ERR_ARG          # the sigmas: a consensus output is wanted


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry,value", [(0, -1), (1, 12), (-1, 1 << 30), (2, -(1 << 31))])
def test_sample_index_out_of_range_is_an_argument_error_not_a_fault(fake_ctx, kind, entry, value):
    job = _job(kind)
    job["samples"] = job["samples"].copy()
    job["samples"].reshape(-1)[entry] = value
    assert _call(fake_ctx[0], job) == ERR_ARG


# ---- the statement -------------------------------------------------------------------------------------------------------------------
def test_statement_recovers_the_true_pose_and_numpy_is_measured_against_it():
    c, st = SC.case(SC.MAIN_SEED, 400, 130), SC.stated(SC.MAIN_SEED, 400)
    t_true = c["t"] / np.linalg.norm(c["t"])
    d_true = [S.pose_distance(s["R"], s["t"], c["R"], t_true) for s in st]
    e64 = np.array([s["e64"] for s in st])
    e_in = np.array([s["e_in"] for s in st])
    print(f"statement to truth: largest {max(d_true):.3e}; numpy to statement: median {np.median(e64):.3e}, largest {e64.max():.3e}; "
          f"e_in: median {np.median(e_in):.3e}, largest {e_in.max():.3e}; roots {np.bincount([s['n_roots'] for s in st]).tolist()}")
    assert all(s["valid"] for s in st)
    # the bearings are the true ones rounded to double: the exact solution of the rounded problem is within its e_in-sized
    # neighbourhood of the truth (the perturbation there is one rounding per component, as in a draw)
    assert all(d <= 8 * max(s["e_in"], 1e-16) for d, s in zip(d_true, st))
    assert np.isfinite(e64).all() and np.median(e64) < 1e-11


@pytest.mark.parametrize("seed,n,k", [(SC.SMALL_SEED, 8, 1), (SC.MAIN_SEED, 400, 1), (SC.MAIN_SEED, 400, 50), (SC.MAIN_SEED, 400, 130)])
def test_exclusion_cap(seed, n, k):
    st = SC.stated(seed, n)[:k]
    n_ex = sum(s["excluded"] for s in st)
    print(f"seed {seed} n {n} samples {k}: {n_ex} excluded; least separation {min(s['separation'] for s in st):.3e}, "
          f"least margin {min(s['margin'] for s in st):.3e}")
    assert n_ex <= S.MAX_EXCLUDED * k


def test_continuation_equals_the_full_statement_on_perturbed_bearings():
    c = SC.case(SC.MAIN_SEED, 400, 2)
    rng = np.random.default_rng(3)
    for q in c["samples5"]:
        f1, f2 = c["bearing1"][q], c["bearing2"][q]
        base = S.five_point(f1, f2, c["sigma1"][q], c["sigma2"][q])
        g1 = f1 * (1.0 + rng.choice([-1.0, 1.0], f1.shape) * 2.0 ** -53)
        g2 = f2 * (1.0 + rng.choice([-1.0, 1.0], f2.shape) * 2.0 ** -53)
        full = S.five_point(g1, g2, c["sigma1"][q], c["sigma2"][q])
        R, t = S.five_point_near(g1, g2, base)
        assert S.pose_distance(R, t, full["R"], full["t"]) == 0.0          # both rounded from 60 digits to double


def test_two_point_statement_maps_the_first_bearing():
    c = SC.case(SC.MAIN_SEED, 400, 130)
    for i, j in c["samples2"]:
        R, ok = S.two_point(c["bearing1"], c["bearing2"], i, j)
        assert ok and np.abs(R @ c["bearing2"][i] - c["bearing1"][i]).max() <= 1e-15
    for i, j in ((3, 3),):
        R, ok = S.two_point(c["bearing1"], c["bearing2"], i, j)
        assert not ok and np.isnan(R).all()


@pytest.mark.parametrize("kind", KINDS)
def test_float64_statement_finds_exactly_the_true_inliers(kind):
    job, truth = SC.end_to_end(kind)
    assert len(truth) == 300 and len(job["bearing1"]) == 345 and len(job["samples"]) == 50
    assert np.array_equal(SC.end_to_end_float64(kind), truth)


# ---- the core on the CPU, sanitised ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sac_solve_probe")
    return SC.build_probe(d), d


def test_probe_two_point_bit_for_bit(probe):
    c = SC.case(SC.MAIN_SEED, 400, 130)
    b1, b2 = c["bearing1"].copy(), c["bearing2"].copy()
    b1[1], b2[1] = b1[0], b2[0]                    # parallel
    b1[2], b2[2] = -b1[0], -b2[0]                  # exactly antiparallel
    q2 = np.concatenate([c["samples2"], [[5, 5], [0, 1], [0, 2]]]).astype(np.int32)
    _, (valid, R) = SC.run_probe(*probe, b1, b2, None, None, np.zeros((0, 8), np.int32), q2)
    for m, (i, j) in enumerate(q2):
        want, ok = S.two_point(b1, b2, i, j)
        assert bool(valid[m]) == ok and R[m].tobytes() == want.tobytes(), m
    assert not valid[-3:].any() and np.isnan(R[-3:]).all() and valid[:-3].all()


@pytest.mark.parametrize("seed,n,k", [(SC.SMALL_SEED, 8, 1), (SC.MAIN_SEED, 400, 130)])
def test_probe_five_point_within_the_bound(probe, seed, n, k):
    c, st = SC.case(seed, n, k), SC.stated(seed, n)[:k]
    (valid, roots, T, Es), _ = SC.run_probe(*probe, c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], c["samples5"], c["samples2"])
    SC.check_five_point(c, c["samples5"], st, valid, roots, T, Es, f"probe seed {seed} n {n}")


def test_probe_most_roots_and_repeated_index(probe):
    c, q, k = SC.most_roots()
    assert k >= 8
    st = SC.state(c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], q[None], 1)
    rep = q.copy()
    rep[6] = rep[2]
    (valid, roots, T, Es), _ = SC.run_probe(*probe, c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], np.stack([q, rep]), np.zeros((0, 2), np.int32))
    print(f"most real roots among 20000 samples: {k}; the statement finds {st[0]['n_roots']}, the probe {roots[0]}")
    SC.check_five_point(c, q[None], st, valid[:1], roots[:1], T[:1], Es[:1], "probe most roots")
    assert st[0]["excluded"] or roots[0] == st[0]["n_roots"] >= 8
    assert not valid[1] and np.isnan(T[1]).all() and roots[1] == 0


@pytest.mark.parametrize("make", [SC.pure_rotation_case, SC.planar_case])
def test_probe_degenerate_scenes_are_flagged_consistently(probe, make):
    c = make()
    runs = [SC.run_probe(*probe, c["bearing1"], c["bearing2"], c["sigma1"], c["sigma2"], c["samples5"], c["samples2"], tag=f"d{r}") for r in range(2)]
    (valid, roots, T, Es), _ = runs[0]
    for m in range(len(T)):
        assert np.isfinite(T[m]).all() if valid[m] else np.isnan(T[m]).all()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0][0], runs[1][0]))
