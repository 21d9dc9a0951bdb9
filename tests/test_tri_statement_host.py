"""CPU: the referee of okvis_fe_stereo_triangulate, okvis_fe_project_landmarks and okvis_fe_gate_3d2d before it is pointed at the
kernels (tests/test_gpu_tri_referee.py): the statement (tests/tri_statement.py) against the recorded values of the reference build
(tests/golden/stereo_gate.npz), the conditions the cases (tests/tri_cases.py) must meet for the comparison to mean something, and the
sensitivity of the bounds to deliberately wrong statements.  None of it needs oracle/_ref or the reference tree."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_statement as SAC  # noqa: E402
import tri_cases as TC  # noqa: E402
import tri_statement as S  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

ALL = TC.names()
GOLDEN = [n for n in ALL if TC.in_golden(TC.cases()[n])]
MAX_LEFT_OUT = 0.02          # of the candidates of an ordinary case


def _judge(name, got, **kw):
    c = TC.cases()[name]
    return S.judge(c["entry"], TC.args(c), got, evals=TC.evaluated(name), exact_rows=c.get("exact"), **kw)


def test_the_undistort_loop_is_the_one_of_the_sac_statement():
    rng = np.random.default_rng(5)
    for model in (SAC.DIST_RADTAN, SAC.DIST_EQUI, SAC.DIST_RADTAN8):
        k = TC.INTR[model][4:]
        xd, yd = S.LD(1) * rng.uniform(-1.2, 1.2, 200), S.LD(1) * rng.uniform(-0.9, 0.9, 200)
        x, y, ok = S.undistort_steps(S.Ctx(), model, k, xd, yd, "", np.ones(200, bool))
        x0, y0, ok0, _ = SAC.undistort(model, k, xd, yd)
        assert (x == x0).all() and (y == y0).all() and (ok == ok0).all()


def test_the_golden_file_holds_the_cases_as_they_are_built_here():
    g = TC.golden()
    assert sorted({k.split("/")[0] for k in g.files}) == sorted(GOLDEN)
    for name in GOLDEN:
        for k, v in TC.arrays(TC.cases()[name]).items():
            assert np.array_equal(g[f"{name}/in/{k}"], v), (name, k)


@pytest.mark.parametrize("name", GOLDEN)
def test_reference_values_lie_within_the_twins_spread_of_the_statement(name):
    """the reference's own classes (recorded) against the statement: flags exact outside the bands, numbers within 4 x the spread of
    the two double precision twins"""
    v = _judge(name, TC.recorded(name), of_reference=True)
    print(name, {k: f"{v['figure'][k]:.2e} / {v['e_ref'][k]:.2e}" for k in v["figure"]}, "left out", v["left_out"], "of", v["n"])
    assert not v["failures"], v["failures"]


@pytest.mark.parametrize("name", ALL)
def test_conditions_of_the_comparison(name):
    """with a double precision twin standing in for the kernel: it passes; an ordinary case leaves at most 2 % of its candidates out
    of the exact comparison; a placed case leaves out none of the candidates built further from the threshold than the band"""
    c = TC.cases()[name]
    for twin in (1, 2):
        v = _judge(name, TC.evaluated(name)[twin][0], recorded=TC.recorded(name))
        assert not v["failures"], v["failures"]
    if c["family"] == "ordinary":
        assert v["left_out"] <= MAX_LEFT_OUT * v["n"], (v["left_out"], v["n"])
    for edge in c.get("edges", {}).values():
        band = np.broadcast_to(np.asarray(v["band"][edge["decision"]], np.float64), (v["n"],))[edge["rows"]]
        clear = edge["m"] > band
        assert v["keep"][edge["rows"]][clear].all(), (name, edge["decision"])


def edge_sides(verdicts):
    """per placed edge, over all its cases: the sides of the threshold that hold a candidate compared exactly"""
    sides = {}
    for name, v in verdicts.items():
        for label, edge in TC.cases()[name].get("edges", {}).items():
            d = v["dec"][edge["decision"]]
            side = np.sign(np.asarray(d["q"] - d["thr"], np.float64))[edge["rows"]]
            kept = v["keep"][edge["rows"]] & d["active"][edge["rows"]]
            sides.setdefault(label, set()).update(side[kept].astype(int).tolist())
    return sides


def test_every_placed_edge_is_compared_on_both_sides():
    verdicts = {n: _judge(n, TC.evaluated(n)[1][0]) for n in TC.names(family="placed")}
    sides = edge_sides(verdicts)
    print(sides)
    assert len(sides) >= 18
    for label, seen in sides.items():
        assert {-1, 1} <= seen, (label, seen)


# the case on which each deliberately wrong statement is caught (found by running all of them; kept so that a change of the cases
# that loses one is seen)
CAUGHT_ON = {"no_pull": "stereo_radtan", "jac_b_at_hp": "stereo_radtan", "no_half_baseline": "stereo_radtan", "size_b_for_a": "placed_errA",
             "a01_sign": "placed_dot", "fu_a_only": "placed_chi2_own", "p3_diagonal": "project_radtan", "u_offdiag_once": "gate_radtan",
             "gate_floor": "placed_gate_negative", "gate_le": "placed_gate_chi2"}


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_a_wrong_statement_is_caught(mut):
    """no_pull: the pull factor 0.8 dropped; jac_b_at_hp: B's Jacobians at hp instead of the pulled point; no_half_baseline: T_AB / 2
    left out of diff; size_b_for_a: B's keypoint size in A's error; a01_sign: a01's sign not following a10's; fu_a_only: A's fu instead
    of the smaller; p3_diagonal: P3's off-diagonals dropped; u_offdiag_once: U[0][1] read for both off-diagonals (exchanging the two changes
    nothing: chi2, the determinant and the norm are symmetric in them); gate_floor: a floor `> -1`
    under the verified chi2 (the reference has none: its truncated integer is < 4 for every negative chi2); gate_le: `<=` at chi2 = 4.
    Each leaves a bound at least tenfold or flips a compared flag."""
    name = CAUGHT_ON[mut]
    c = TC.cases()[name]
    got = S.FUNCTIONS[c["entry"]](S.Ctx(np.float64, mut=mut), *TC.args(c))
    v = _judge(name, got, recorded=TC.recorded(name))
    flipped = any("differ at compared" in f for f in v["failures"])
    tenfold = any(v["figure"][k] > 10 * v["bound"][k] for k in v["figure"])
    print(mut, name, "flags flipped" if flipped else "", {k: f"{v['figure'][k]:.1e} / {v['bound'][k]:.1e}" for k in v["figure"]})
    assert flipped or tenfold, v["failures"]


# ---- the boundary of the three entries ------------------------------------------------------------------------------------------------
def test_flag_values_and_camera_layout_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(OKVIS_FE_[A-Z0-9_]+)\s+(\d+)u?\b", hdr)}
    for prefix, names in (("TRI", ("VALID", "NOT_PARALLEL", "CAN_INIT", "RANK_DEFICIENT")),
                          ("PROJ", ("SUCCESSFUL", "OUTSIDE_IMAGE", "MASKED", "BEHIND", "INVALID")), ("GATE", ("VERIFIED", "ACCEPTED", "UNCERTAIN"))):
        for n in names:
            assert defs[f"OKVIS_FE_{prefix}_{n}"] == getattr(F, f"{prefix}_{n}") == getattr(S, f"{prefix}_{n}"), (prefix, n)
    assert [(f[0], getattr(F.CameraC, f[0]).offset) for f in F.CameraC._fields_] == [("intr", 0), ("model", 96), ("width", 100), ("height", 104),
                                                                                    ("reserved", 108)]
    body = re.search(r"typedef struct okvis_fe_camera \{(.*?)\} okvis_fe_camera;", hdr, re.S).group(1)
    assert re.findall(r"\b(intr|model|width|height|reserved)\b(?=[\[;])", body) == [f[0] for f in F.CameraC._fields_]


def test_the_three_entries_are_exported_with_the_declared_arguments():
    from okvis_amd import _lib
    L = _lib.lib()
    F.declare(L)
    hdr = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    for entry in ("stereo_triangulate", "stereo_triangulate_gn", "project_landmarks", "gate_3d2d"):
        decl = re.search(r"int okvis_fe_%s\((.*?)\);" % entry, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(getattr(L, "okvis_fe_" + entry).argtypes), entry
    cam = F.camera(TC.INTR[SAC.DIST_RADTAN], SAC.DIST_RADTAN)
    assert L.okvis_fe_stereo_triangulate_gn(None, C.byref(cam), C.byref(cam), None, None, 0, None, 0, None, 0, None, None, 0, None, None,
                                            None, None) == -1
