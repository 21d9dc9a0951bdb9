"""GPU: two properties every okvis_fe_* entry shares, whatever it computes.

  1  an optional output that is left out (a null pointer) changes nothing about the outputs that remain;
  2  what an entry returns does not depend on what the context staged before it: calls of different entries on one context, the
     staging block growing in between, equal the same calls made on a context of their own.

Everything is compared byte for byte.  Scenes: tests/vmatch_scene.py at (65, 63) and (257, 513), which cross the 64-lane block and
the 256-descriptor tile; the sample-consensus problems are recorded ones (tests/sac_cases.py); the solvers, the propagation and
the keyframe decision take seeded cases of tests/sac_solve_cases.py, tests/imu_propagate_cases.py and tests/keyframe_cases.py.
Where okvis_amd/frontend.py always passes a pointer, the library is called through the tables and ctypes directly."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_propagate_cases as IC  # noqa: E402
import keyframe_cases as KC  # noqa: E402
import sac_cases  # noqa: E402
import sac_solve_cases as SSC  # noqa: E402
import vmatch_scene as SC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402
from okvis_amd.window import DIST_EQUIDISTANT, DIST_RADTAN  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(65, 63), (257, 513)]
RATIO = 1.2


@functools.lru_cache(maxsize=None)
def inputs(k):
    """scene k (with skip masks), its candidate pairs with their sigmas, and its projections: made once, on a context of their own"""
    s = SC.scene(DIST_RADTAN if k else DIST_EQUIDISTANT, 4200 + k, *SHAPES[k], 0.15)
    fe = F.Frontend()
    pairs, _ = fe.hamming_candidates(s["desc_a"], s["desc_b"], SC.THRESHOLD, s["skip_a"], s["skip_b"])
    uv, U, _ = fe.project_landmarks(F.camera(s["intr"], s["model"]), s["T_CbW"], s["P3"], s["hp_W"])
    fe.close()
    assert len(pairs) > 100
    return s, pairs, SC.pair_sigmas(s, pairs), uv, U


def vjob(kind, s):
    cam = F.camera(s["intr"], s["model"])
    j = {"kind": kind, "desc_a": s["desc_a"], "desc_b": s["desc_b"], "kp_a": s["kp_a"], "kp_b": s["kp_b"], "cam_a": cam, "cam_b": cam,
         "skip_a": s["skip_a"], "skip_b": s["skip_b"]}
    if kind == F.MATCH_3D2D:
        j.update(hp_W=s["hp_W"], T_CbW=s["T_CbW"], P3=s["P3"])
    else:
        j.update(T_AB=s["T_AB"], UOplus=s["UOplus"])
    return j


def sac_jobs():
    g = sac_cases.golden()
    return [sac_cases.golden_job(g, 0, name) for name in sac_cases.PROBLEMS]


def solve_jobs():
    """a relative job of 65 correspondences and 9 hypotheses (one ballot word and one model tile, each plus one) and a rotation-only
    job of 257 and 65 (one 256-lane tile and one wave of samples, each plus one)"""
    return [SSC.relative_job(SSC.case(365, 65, 9)), SSC.rotation_job(SSC.case(557, 257, 65))]


def kf_arrays(res):
    """what Frontend.keyframe_decision returns for some jobs, as flat arrays"""
    ims = [im for r in res for im in r["images"]]
    a = {k: np.array([r[k] for r in res]) for k in ("decision", "overlap", "ratio")}
    a.update({k: np.concatenate([np.atleast_1d(im[k]) for im in ims]) for k in ims[0]})
    return a


def same(x, y):
    return x.keys() == y.keys() and all(x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes() for k in x)


# ---------------------------------------------------------------- 1: optional outputs

def each_left_out(call, shapes):
    """call(pointers: name -> address or None) fills arrays of `shapes` (name -> (shape, dtype)): once with all of them, once per name
    without it.  The arrays start from a byte pattern, so that a cell an entry does not write is the same cell in both runs."""
    def run(without=None):
        arrays = {k: np.empty(shape, dtype) for k, (shape, dtype) in shapes.items()}
        for a in arrays.values():
            a.view(np.uint8)[...] = 0x5A
        call({k: (None if k == without else a.ctypes.data) for k, a in arrays.items()})
        return arrays

    full = run()
    for name in shapes:
        part = run(name)
        assert (part[name].view(np.uint8) == 0x5A).all(), name
        for k in shapes:
            if k != name:
                assert part[k].tobytes() == full[k].tobytes(), (name, k)
    return full


def test_an_optional_output_left_out_changes_no_other_output():
    fe = F.Frontend()
    L, ctx = fe._L, fe._ctx
    written = 0
    for k in range(len(SHAPES)):
        s, pairs, sig, uv, U = inputs(k)
        n_a, n_b, n = len(s["kp_a"]), len(s["kp_b"]), len(pairs)
        cam = F.camera(s["intr"], s["model"])
        T_AB, UO, T_CbW, P3 = (np.ascontiguousarray(s[x], np.float64) for x in ("T_AB", "UOplus", "T_CbW", "P3"))
        sa, sb = (np.ascontiguousarray(s[x], np.uint8) for x in ("skip_a", "skip_b"))

        def check(rc):
            assert rc == 0, rc

        # triangulation: hp_a / cov / flags / gn
        r = each_left_out(lambda p: check(L.okvis_fe_stereo_triangulate_gn(
            ctx, C.byref(cam), C.byref(cam), T_AB.ctypes.data, UO.ctypes.data, n_a, s["kp_a"].ctypes.data, n_b, s["kp_b"].ctypes.data, n,
            pairs.ctypes.data, sig.ctypes.data, 1, p["hp_a"], p["cov"], p["flags"], p["gn"])),
            {"hp_a": ((n, 4), np.float64), "cov": ((n, 9), np.float64), "flags": ((n,), np.uint8), "gn": ((n, 81), np.float64)})
        written += int((r["flags"] & F.TRI_VALID != 0).sum())
        # projection: uv / U / status
        each_left_out(lambda p: check(L.okvis_fe_project_landmarks(ctx, C.byref(cam), T_CbW.ctypes.data, P3.ctypes.data, n_a,
                                                                   s["hp_W"].ctypes.data, p["uv"], p["U"], p["status"])),
                      {"uv": ((n_a, 2), np.float64), "U": ((n_a, 4), np.float64), "status": ((n_a,), np.uint8)})
        # gate: chi2 / flags
        each_left_out(lambda p: check(L.okvis_fe_gate_3d2d(ctx, n_a, uv.ctypes.data, U.ctypes.data, n_b, s["kp_b"].ctypes.data, n,
                                                           pairs.ctypes.data, p["chi2"], p["flags"])),
                      {"chi2": ((n,), np.float64), "flags": ((n,), np.uint8)})
        # candidates: dist (pairs are required)
        got = {}

        def candidates(p):
            buf, total = np.zeros((n, 2), np.int32), C.c_int32(-1)
            check(L.okvis_fe_hamming_candidates(ctx, SC.WIDTH, n_a, s["desc_a"].ctypes.data, sa.ctypes.data, n_b, s["desc_b"].ctypes.data,
                                                sb.ctypes.data, SC.THRESHOLD, n, buf.ctypes.data, p["dist"], C.byref(total)))
            assert total.value == n
            got.setdefault("pairs", buf)
            assert got["pairs"].tobytes() == buf.tobytes() == pairs.tobytes()

        each_left_out(candidates, {"dist": ((n,), np.float32)})
        # bearing vectors: all three
        each_left_out(lambda p: check(L.okvis_fe_bearing_vectors(ctx, C.byref(cam), n_b, s["kp_b"].ctypes.data, p["bearing"], p["sigma"],
                                                                 p["ok"])),
                      {"bearing": ((n_b, 3), np.float64), "sigma": ((n_b,), np.float64), "ok": ((n_b,), np.uint8)})
        # verified matching, per kind: what the kind reports besides pair_a / pair_dist / accepted
        for kind, optional in ((F.MATCH_3D2D, ("proj_status", "uv", "U", "chi2", "gate_flags")), (F.MATCH_2D2D, ("hp_a", "cov", "tri_flags"))):
            def verified(without=None):
                table, keep, (out,) = F.vmatch_job_table([vjob(kind, s)])
                for a in out.values():
                    a.view(np.uint8)[...] = 0x5A
                if without:
                    setattr(table[0], without, None)
                check(L.okvis_fe_match_verified(ctx, 1, table, SC.WIDTH, SC.THRESHOLD, 4, 1, RATIO))
                return out

            full = verified()
            written += int(full["accepted"].astype(bool).sum())
            for name in optional:
                part = verified(name)
                assert (part[name].view(np.uint8) == 0x5A).all(), name
                assert same({x: a for x, a in part.items() if x != name}, {x: a for x, a in full.items() if x != name}), (kind, name)
    # SAC: counts / best / n_inliers / inliers / scores, a batch of the five problems of a recorded case
    jobs = sac_jobs()

    def consensus(without=None):
        table, keep, out = F.sac_job_table(jobs, want_scores=True)
        for counts, scalars, inl, sc in out:
            for a in (counts, scalars, inl, sc):
                a.view(np.uint8)[...] = 0x5A
        if without:
            for j in range(len(jobs)):
                setattr(table[j], without, None)
        check(L.okvis_fe_sac_consensus(ctx, len(jobs), table))
        return [{"counts": counts, "best": scalars[:1], "n_inliers": scalars[1:], "inliers": inl, "scores": sc} for counts, scalars, inl, sc in out]

    full = consensus()
    assert sum(int(r["n_inliers"][0]) for r in full) > 50
    for name in ("counts", "best", "n_inliers", "inliers", "scores"):
        for f, p in zip(full, consensus(name)):
            assert (p[name].view(np.uint8) == 0x5A).all(), name
            for x in f:
                if x != name:
                    assert p[x].tobytes() == f[x].tobytes(), (name, x)
    # the solvers: models / valid / n_roots / essentials / counts / best / n_inliers / inliers / scores, a relative and a
    # rotation-only job in one call
    sjobs = solve_jobs()

    def solve(without=(), sigmas=True):
        table, keep, out = F.sac_solve_job_table(sjobs, want_scores=True, want_essentials=True)
        for j, o in enumerate(out):
            o["best"], o["n_inliers"] = o["scalars"][:1], o["scalars"][1:]
            del o["scalars"]
            for a in o.values():
                a.view(np.uint8)[...] = 0x5A
            for name in without:
                setattr(table[j], name, None)
            if not sigmas:
                table[j].sigma1 = table[j].sigma2 = None
        check(L.okvis_fe_sac_solve(ctx, len(sjobs), table))
        return out

    def untouched_and_same(full, part, without):
        for f, p in zip(full, part):
            for x in f:
                if x in without:
                    assert (p[x].view(np.uint8) == 0x5A).all(), (without, x)
                else:
                    assert p[x].tobytes() == f[x].tobytes(), (without, x)

    full = solve()
    assert all(f["valid"].view(np.uint8).sum() > 0 and int(f["n_inliers"][0]) > 0 for f in full)
    for name in ("models", "valid", "n_roots", "essentials", "counts", "best", "n_inliers", "inliers", "scores"):
        untouched_and_same(full, solve((name,)), (name,))
    # all five consensus outputs left out: no scoring, and then the sigmas may be left out too (the two-point solver reads none;
    # the five-point selection weighs with 1 without them, so only what it does not select is compared)
    five = ("counts", "best", "n_inliers", "inliers", "scores")
    untouched_and_same(full, solve(five), five)
    bare = solve(five, sigmas=False)
    untouched_and_same(full[1:], bare[1:], five)
    untouched_and_same([{x: full[0][x] for x in five + ("n_roots", "essentials")}], [{x: bare[0][x] for x in five + ("n_roots", "essentials")}], five)
    # propagation: cov / jac, with flags to match
    s_t, s_gyr, s_acc, ends, pjobs = IC.pool([IC.by_name(x) for x in ("steps11", "chain", "uncovered")])
    prm, s_t, s_gyr, s_acc, ends = F.imu_pools(IC.PARAMS, s_t, s_gyr, s_acc, ends)
    m = len(ends)

    def propagate(p, drop=0):
        table = F.imu_job_table([dict(j, flags=(F.IMU_COV | F.IMU_JAC) & ~drop) for j in pjobs])
        check(L.okvis_fe_imu_propagate(ctx, len(prm), prm, len(s_t), s_t.ctypes.data, s_gyr.ctypes.data, s_acc.ctypes.data, m, ends.ctypes.data,
                                       len(pjobs), table, p["T_WS"], p["sb"], p["cov"], p["jac"], p["count"]))

    def run_propagate(without=None):
        arrays = {"T_WS": np.empty((m, 7)), "sb": np.empty((m, 9)), "cov": np.empty((m, 15, 15)), "jac": np.empty((m, 15, 15)),
                  "count": np.empty(m, np.int32)}
        for a in arrays.values():
            a.view(np.uint8)[...] = 0x5A
        propagate({k: (None if k == without else a.ctypes.data) for k, a in arrays.items()}, {"cov": F.IMU_COV, "jac": F.IMU_JAC, None: 0}[without])
        return arrays

    full = run_propagate()
    assert (full["count"] > 0).sum() >= 12 and (full["count"] == -1).sum() == 2
    for name in ("cov", "jac"):
        untouched_and_same([full], [run_propagate(name)], (name,))
    # keyframe decision: its twelve outputs
    kp, matched, images, table, counts = F.keyframe_job_table(KC.cases("degenerate") + KC.cases("on_edges"))
    n_jobs = len(KC.cases("degenerate")) + len(KC.cases("on_edges"))
    shapes = {k: (a.shape, a.dtype) for k, a in F.keyframe_outputs(n_jobs, len(counts), sum(counts), want_hulls=True).items()}
    assert tuple(shapes) == F.KF_OUTPUTS and len(shapes) == 12
    r = each_left_out(lambda p: check(L.okvis_fe_keyframe_decision(ctx, len(matched), kp.ctypes.data, matched.ctypes.data, len(counts), images,
                                                                   n_jobs, table, *[p[k] for k in F.KF_OUTPUTS])), shapes)
    assert r["hull_all_size"].sum() > 20 and r["n_inside"].sum() > 0
    fe.close()
    assert written > 100


# ---------------------------------------------------------------- 2: one context, many entries

def test_entries_mixed_on_one_context_equal_each_on_a_context_of_its_own():
    (s0, pairs0, sig0, uv0, U0), (s1, pairs1, _, _, _) = inputs(0), inputs(1)
    cam0 = F.camera(s0["intr"], s0["model"])
    jobs = sac_jobs()[:1]

    def triangulate(fe):     # small: fits the first staging block
        hp, cov, flags = fe.stereo_triangulate(cam0, cam0, s0["T_AB"], s0["UOplus"], s0["kp_a"], s0["kp_b"], pairs0[:40], sig0[:40])
        return {"hp": hp, "cov": cov, "flags": flags}

    def match(s, kind):
        return lambda fe: fe.match_verified([vjob(kind, s)], SC.THRESHOLD, 4, True, RATIO)[0]

    def consensus(fe):
        r, = fe.sac_consensus(jobs, want_scores=True)
        return {k: np.asarray(v) for k, v in r.items()}

    def gate(fe):
        chi2, flags = fe.gate_3d2d(uv0, U0, s0["kp_b"], pairs0)
        return {"chi2": chi2, "flags": flags}

    def solve(fe):
        r, = fe.sac_solve(solve_jobs()[:1], want_scores=True, want_essentials=True)
        return {k: np.asarray(v) for k, v in r.items()}

    def propagate(fe):
        s_t, s_gyr, s_acc, ends, pjobs = IC.pool([IC.by_name("chain_between")])
        return dict(zip(("T_WS", "sb", "count", "cov", "jac"), fe.imu_propagate(IC.PARAMS, s_t, s_gyr, s_acc, pjobs, ends)))

    def keyframe(fe):
        return kf_arrays(fe.keyframe_decision(KC.cases("convex"), want_hulls=True))

    steps = [triangulate, match(s1, F.MATCH_2D2D), consensus, gate, match(s0, F.MATCH_3D2D), match(s1, F.MATCH_3D2D), triangulate]
    between = {1: solve, 3: propagate, 5: keyframe}      # run in front of the step of that index
    fe = F.Frontend()                       # its staging block starts empty and moves at the second step
    mixed, mixed_between = [], {}
    for i, step in enumerate(steps):
        if i in between:
            mixed_between[i] = between[i](fe)
        mixed.append(step(fe))
    fe.close()
    for step, got in list(zip(steps, mixed)) + [(between[i], mixed_between[i]) for i in between]:
        own = F.Frontend()
        want = step(own)
        own.close()
        assert same(got, want), step
    assert int(mixed_between[1]["n_inliers"]) > 0 and (mixed_between[3]["count"] > 0).all() and mixed_between[5]["hull_all_size"].sum() > 600
    assert int(mixed[1]["accepted"].sum()) > 20 and int(mixed[4]["accepted"].sum()) > 0 and int(mixed[2]["n_inliers"]) > 0
    assert (mixed[0]["flags"] & F.TRI_VALID != 0).any() and (mixed[3]["flags"] & F.GATE_VERIFIED != 0).any()
