"""The windows of the fp64 linearisation referee (tests/test_gpu_fp64_linearize.py) and what both of its halves share — TEST
INFRASTRUCTURE, host only.  tests/test_fp64_statement_host.py proves on the CPU that these inputs and the entrywise scale would
notice a wrong term; the GPU file compares the kernels on them.

Windows: every case of tests/fp32_cases.py, plus
  boundary64_*   the fused-mode boundary of fp64, 2 * SCHUR_LM_BATCH * 3 * Dp <= LinCfg<EXT, double>::STAGE_DOUBLES (256 * 23 and
                 256 * 35 doubles: Dp <= 61 with fixed extrinsics, <= 93 with free ones): K = 10 / 11 fixed (Dp = 60 / 66) and
                 K = 13 / 14 shared (Dp = 90 / 96; the six oldest speed/bias blocks fixed so that D <= MAX_D_LDS = 174 on both
                 sides and the stage alone decides);
  outliers       six observations 20 - 50 x cauchy_b off (rho' <= 2.5e-3), three with obs_sqrtw a hundredth of the rest, and one
                 landmark 1e7 m out (w = 1) whose last observation is both;
  group_*        a group that closes at exactly GROUP_OBS = 256 observations (staged kernel), one that closes at exactly
                 LIN2_PIECES = 128 pieces (monocular, piece path), okvis_ba_tuning::group_lm = 16 / 32 / 64 and a group_work cap
                 that cuts the groups earlier — each asserted from solver.index_lists (check_group_edges).

The referee of an array is the oracle built with real = long double.  e_ref(A, scale) — the bound's yardstick — is the largest
deviation from it, over ALL windows of CASES, of three CPU evaluations in fp64: the fp64 oracle, the float64 statement
(tests/fp32_statement.py) and the float64 statement summing in reverse observation order; under two scales: entrywise (what the
entry is a sum of, in absolute values) and max |A|.  It is measured on the CPU, never from a kernel; the kernels are held to
BOUND_FACTOR x e_ref.

Phase A (the landmark back-substitution) has its own statement here, phase_a(), and its own e_ref: float64 against long double
on the fp64 oracle's arrays and step, over all windows, under both dampings, with the inverse taken two ways (adjugate, LU)."""
from __future__ import annotations

import copy
import functools

import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import default_options, set_options

from . import fp32_cases
from . import fp32_statement as stmt
from . import schur_statement

BOUND_FACTOR = fp32_cases.BOUND_FACTOR     # 4: what two correct evaluations may differ by; the project's own, not tuned here
MUTATION_MARGIN = 10.0
ENTRYWISE_CEILING = 1.0e3 * 2.0 ** -53     # every entrywise e_ref stays below this (asserted on the CPU)
OLD_TOLERANCE = 1.0e-9                     # tests/test_gpu_parity.py: relative to max |A|
SCALES = ("entry", "max")
STAGE_DOUBLES = {False: 256 * 23, True: 256 * 35}        # LinCfg<EXT, double>::STAGE_DOUBLES (ba_linearize.hpp)
MAX_D_LDS, TILE_DIM, SCHUR_LM_BATCH, GROUP_OBS, LIN2_PIECES = 174, 96, 16, 256, 128
FUSED_MAX_WINDOWS, SMALL_BATCH_WINDOWS = 48, 40
FLAT = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)

_window, _keep = fp32_cases._window, fp32_cases._keep


# ---- the fused boundary in fp64 ----
def boundary64(K, ext):
    w = _window(K, 30, 210 + K, estimate_extrinsics=ext, **(dict(frame_dt=0.1) if K > 12 else {}))
    if ext != "fixed":
        w.sb_fixed = np.asarray(w.sb_fixed).copy()
        w.sb_fixed[:6] = 1
    return [w]


# ---- gross outliers, low weights, a far landmark ----
FAR_DEPTH = 1.0e7      # with w = 1: practically a point at infinity; its Jacobians are 2e6 times smaller than a landmark's at 5 m


def _predicted(w, o):
    """the pixel the statement projects observation o to"""
    ob = stmt.observation(w.pose[w.obs_pose[o]], w.pose[w.obs_ext[o]], w.lm[w.obs_lm[o]], w.cam_intr[w.obs_cam[o]],
                          int(w.cam_model[w.obs_cam[o]]), w.obs_uv[o], float(w.obs_sqrtw[o]))
    assert ob["valid"]
    return np.asarray(w.obs_uv[o], np.float64) - ob["r"] / float(w.obs_sqrtw[o])


def outliers():
    w = _window(4, 40, 231)
    rng = np.random.default_rng(231)
    w.lm, w.obs_uv, w.obs_sqrtw = (np.asarray(a, np.float64).copy() for a in (w.lm, w.obs_uv, w.obs_sqrtw))
    far = stmt.drop_landmark(w)
    of_far = np.flatnonzero(np.asarray(w.obs_lm) == far)
    o = of_far[0]
    w.lm[far, :3] = fp32_cases._camera_point_to_world(w, int(w.obs_pose[o]), int(w.obs_ext[o]), [20.0, -10.0, FAR_DEPTH])
    for o in of_far:
        w.obs_uv[o] = _predicted(w, o) + rng.normal(0.0, 0.5, 2)
    others = np.setdiff1d(np.arange(w.n_obs), of_far)
    pick = rng.choice(others, 8, replace=False)
    gross, light = list(pick[:5]) + [of_far[-1]], list(pick[5:]) + [of_far[-1]]
    for o in light:
        w.obs_sqrtw[o] *= 0.01
    for o in gross:      # the weighted residual 20 - 50 cauchy_b long
        d = rng.normal(size=2)
        w.obs_uv[o] = _predicted(w, o) + d / np.linalg.norm(d) * rng.uniform(20.0, 50.0) * float(w.cauchy_b) / w.obs_sqrtw[o]
    w.outlier_obs, w.light_obs, w.far_lm = np.array(gross), np.array(light), far
    return [w]


# ---- group edges ----
def _trim_until(w, excess_of):
    """drop the last observation of the landmark (among those excess_of names) with the most observations until excess_of says 0"""
    while True:
        excess, upto = excess_of(w)
        if excess == 0:
            return w
        counts = np.bincount(np.asarray(w.obs_lm), minlength=w.n_lm)[:upto + 1]
        l = int(np.argmax(counts))
        assert counts[l] > 2
        keep = np.ones(w.n_obs, bool)
        keep[np.flatnonzero(np.asarray(w.obs_lm) == l)[-1]] = False
        _keep(w, keep)


def _excess_over(target):
    def excess_of(w):
        cum = np.cumsum(np.bincount(np.asarray(w.obs_lm), minlength=w.n_lm))
        l = int(np.searchsorted(cum, target))      # the first landmark that reaches the target
        return int(cum[l] - target), l
    return excess_of


def group_obs_256():
    """staged kernel, groups of up to 64 landmarks: the first group's observations end at exactly 256"""
    return [_trim_until(_window(6, 50, 241, vis=0.9), _excess_over(GROUP_OBS))]


def group_pieces_128():
    """monocular (one piece per observation), groups of up to 64 landmarks: the first group's pieces end at exactly 128"""
    w = _window(8, 40, 242, vis=0.9)
    _keep(w, np.asarray(w.obs_cam) == 0)
    return [_trim_until(w, _excess_over(LIN2_PIECES))]


def group_lm_window():
    return [_window(3, 52, 243)]


CASES = dict(fp32_cases.CASES)
CASES.update({
    "boundary64_10_fixed": functools.partial(boundary64, 10, "fixed"), "boundary64_11_fixed": functools.partial(boundary64, 11, "fixed"),
    "boundary64_13_shared": functools.partial(boundary64, 13, "shared"), "boundary64_14_shared": functools.partial(boundary64, 14, "shared"),
    "outliers": outliers,
    "group_obs_256": group_obs_256, "group_pieces_128": group_pieces_128,
    "group_lm_16": group_lm_window, "group_lm_32": group_lm_window, "group_lm_64": group_lm_window, "group_work": group_lm_window,
})
NEW_CASES = tuple(n for n in CASES if n not in fp32_cases.CASES)
# the upload options a case needs for its property
CASE_OPTIONS = {
    "group_obs_256": dict(reserved0=8, tuning_group_lm=64), "group_pieces_128": dict(tuning_group_lm=64),
    "group_lm_16": dict(tuning_group_lm=16), "group_lm_32": dict(tuning_group_lm=32), "group_lm_64": dict(tuning_group_lm=64),
    "group_work": dict(tuning_group_lm=64, tuning_group_work=40),
}


def options(name=None, **kw):
    d = dict(CASE_OPTIONS.get(name, {}), fp32_linearize=0)
    d.update(kw)
    return set_options(default_options(), **d)


def group_table(w, opt, n_windows=1):
    """per group (landmarks, observations, pieces or None), from the host-side index lists"""
    from okvis_amd import solver
    lists = solver.index_lists(w, opt, n_windows)
    g = lists["groups"]
    pieces = [None] * len(g)
    if lists["piece_path"]:
        begin = list(g[:, 12]) + [int(lists["lm_piece_begin"][-1])]
        pieces = [int(begin[i + 1] - begin[i]) for i in range(len(g))]
    return [(int(r[1] - r[0]), int(r[3] - r[2]), p) for r, p in zip(g, pieces)], lists


def check_group_edges(windows):
    """the group-edge cases have the edge they are named after (index lists, no device)"""
    t, lists = group_table(windows["group_obs_256"][0], options("group_obs_256"))
    assert not lists["piece_path"] and t[0][1] == GROUP_OBS and t[0][0] < 64 and len(t) > 1, t
    t, lists = group_table(windows["group_pieces_128"][0], options("group_pieces_128"))
    assert lists["piece_path"] and t[0][2] == LIN2_PIECES and t[0][1] < GROUP_OBS and t[0][0] < 64 and len(t) > 1, t
    w = windows["group_lm_16"][0]
    for cap in (16, 32, 64):
        t, _ = group_table(w, options(f"group_lm_{cap}"))
        assert [r[0] for r in t] == [min(cap, w.n_lm - k) for k in range(0, w.n_lm, cap)], (cap, t)
        assert all(r[1] < GROUP_OBS and (r[2] is None or r[2] < LIN2_PIECES) for r in t), (cap, t)     # the cap alone closed them
    t, _ = group_table(w, options("group_work"))
    t64, _ = group_table(w, options("group_lm_64"))
    assert len(t) > len(t64) and max(r[0] for r in t) < 16, (t, t64)                                    # cut earlier than any landmark cap


def expected_route(ws, opt):
    """launch_route()'s fused / piece_path / split_small of a batch under the options, restated from batch_layout, form_chunks and
    make_plan (capi_index_build.inc, capi_launch.inc) for the fp64 stage; D, Dp and the piece path's fit come from the host-side
    index build"""
    from okvis_amd import solver
    n = len(ws)
    decision_free = int(opt.strategy) == schur_statement.STRATEGY_DOGLEG or bool(opt.gauss_newton)
    fmw = opt.tuning.fused_max_windows
    fmw = fmw if fmw > 0 else 0 if fmw < 0 else FUSED_MAX_WINDOWS
    lay_fuse = not (opt.reserved0 & 4) and opt.schur_lm_per_block == 0 and n <= fmw and decision_free
    lin2 = not (opt.reserved0 & 8) and all(solver.index_lists(w, opt, n)["piece_path"] for w in ws)
    group_chunks = lay_fuse
    for w in ws:
        c = solver.check_window(w, opt)
        has_ext = bool(np.any(np.asarray(w.pose_fixed).reshape(-1)[np.asarray(w.obs_ext)] == 0))
        group_chunks = group_chunks and c["D"] <= MAX_D_LDS and c["Dp"] <= TILE_DIM and 2 * SCHUR_LM_BATCH * 3 * c["Dp"] <= STAGE_DOUBLES[has_ext]
    split = n >= (opt.tuning.split_small_min if opt.tuning.split_small_min > 0 else SMALL_BATCH_WINDOWS)
    return dict(fused=int(group_chunks and decision_free), piece_path=int(lin2), split_small=int(split))


# ---- phase A ----
def phase_a(lm, V6, B, W, pair_lm, pair_block, off, step, lam, Dl2, dtype=np.float64, lu=False):
    """(new lm[:, :3], scale): lm + delta_l, delta_l = -(V_l + lam diag(Dl2_l))^-1 (b_l + sum_p W_p^T step[block(p)]), in `dtype`;
    scale = |lm| + |Vd^-1| (|b| + sum |W|^T |step|), float64.  The inverse is schur_statement.inverse3 (adjugate over Sarrus), or
    with lu (float64 only) numpy's LU solve: a second, differently ordered fp64 evaluation for e_ref."""
    T = dtype
    lm = np.asarray(lm, np.float64).reshape(-1, 4)
    V6, B, W = np.asarray(V6).reshape(-1, 6), np.asarray(B).reshape(-1, 3), np.asarray(W).reshape(-1, 6, 3)
    step = np.asarray(step).astype(T)
    n_lm = lm.shape[0]
    first = np.searchsorted(np.asarray(pair_lm), np.arange(n_lm + 1))
    out, scale = np.zeros((n_lm, 3), T), np.zeros((n_lm, 3), np.float64)
    for l in range(n_lm):
        t, a = B[l].astype(T), np.abs(B[l]).astype(T)
        for p in range(first[l], first[l + 1]):
            d = step[off[pair_block[p]]:off[pair_block[p]] + 6]
            t = t + W[p].astype(T).T @ d
            a = a + np.abs(W[p]).astype(T).T @ np.abs(d)
        Vd = schur_statement._sym3(V6[l], T) + np.diag(T(lam) * np.asarray(Dl2[l], T))
        Vi = schur_statement.inverse3(Vd)
        out[l] = lm[l, :3].astype(T) - (np.linalg.solve(Vd, t) if lu else Vi @ t)
        scale[l] = np.abs(lm[l, :3]) + np.asarray(np.abs(Vi) @ a, np.float64)
    assert out.dtype == T
    return out, scale


def phase_a_options(kind, **kw):
    """kind "lm": strategy = LM with gauss_newton = 1 (lambda = 1 / initial_radius, every step accepted); "dl": the default dogleg"""
    d = dict(FLAT, **(dict(strategy=schur_statement.STRATEGY_LM, gauss_newton=1) if kind == "lm" else {}))
    d.update(kw)
    return set_options(default_options(), **d)


def phase_a_damping(kind, V6):
    """(lambda, Dl2 [n_lm, 3]) of the first solve (damp_diag, ba_device.hpp; schur_statement.damping)"""
    opt = set_options(default_options(), strategy=schur_statement.STRATEGY_LM if kind == "lm" else schur_statement.STRATEGY_DOGLEG)
    lam, _, Dl2 = schur_statement.damping(opt, np.zeros(1), V6)
    return lam, Dl2


def phase_a_deviation(x, ref, scale):
    return float((np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64)) / scale).max())


def window_deviations(oracle, w, arrays):
    """{array: {"entry", "max"}} of `arrays` from the long-double oracle of ANY window, in the scales of the referee"""
    x = oracle.OracleWindow(w, extended=True)
    x.linearize()
    scale = stmt.window_arrays(w, np.float64, scales=True)["scale"]
    return {a: {"entry": stmt.deviation_entrywise(arrays[a], x.array(a), scale[a]), "max": stmt.deviation(arrays[a], x.array(a))}
            for a in stmt.ARRAYS}


class Referee:
    """Every case's windows with the long-double oracle's arrays (the referee), the entrywise scales and e_ref, computed once."""

    def __init__(self, oracle):
        assert np.finfo(np.longdouble).eps < 2e-19, "the referee needs an extended long double"
        self.oracle = oracle
        self.windows, self.ref, self.scale, self.pairs, self.o64, self.stmt64, self.e_case = {}, {}, {}, {}, {}, {}, {}
        self.e_ref = {a: {s: 0.0 for s in SCALES} for a in stmt.ARRAYS}
        self.e_ref_phase_a = 0.0
        self.e_phase_a_case, self._optimized = {}, {}
        for name, make in CASES.items():
            ws = make()
            self.windows[name] = ws
            for d in (self.ref, self.scale, self.pairs, self.o64, self.stmt64, self.e_case):
                d[name] = []
            for i, w in enumerate(ws):
                x, o = oracle.OracleWindow(w, extended=True), oracle.OracleWindow(w)
                x.linearize(), o.linearize()
                ref = {a: x.array(a) for a in stmt.ARRAYS}
                o64 = {a: o.array(a) for a in stmt.ARRAYS + ("LM",)}
                s = stmt.window_arrays(w, np.float64, scales=True)
                r = stmt.window_arrays(w, np.float64, reverse=True)
                assert np.array_equal(s["pairs"][0], o.pairs()[0]) and np.array_equal(s["pairs"][1], o.pairs()[1]), name
                e = {a: {"entry": max(stmt.deviation_entrywise(v[a], ref[a], s["scale"][a]) for v in (o64, s, r)),
                         "max": max(stmt.deviation(v[a], ref[a]) for v in (o64, s, r))} for a in stmt.ARRAYS}
                for a in stmt.ARRAYS:
                    for k in SCALES:
                        self.e_ref[a][k] = max(self.e_ref[a][k], e[a][k])
                self.ref[name].append(ref), self.scale[name].append(s["scale"]), self.pairs[name].append(o.pairs())
                self.o64[name].append(o64), self.stmt64[name].append(s), self.e_case[name].append(e)
                # phase A on the fp64 oracle's arrays and step: float64 against long double
                off = schur_statement.pose_offsets(w)
                for kind in ("lm", "dl"):
                    opt = phase_a_options(kind)
                    assert o.solve(opt.initial_radius, opt) == 0, (name, kind)
                    lam, Dl2 = phase_a_damping(kind, o64["LM_V"])
                    args = (o64["LM"], o64["LM_V"], o64["LM_B"], o64["PAIR_W"], *o.pairs(), off, o.array("STEP"), lam, Dl2)
                    ld, a = phase_a(*args, dtype=np.longdouble)
                    ea = max(phase_a_deviation(phase_a(*args, dtype=np.float64, lu=lu)[0], ld, a) for lu in (False, True))
                    self.e_phase_a_case[name, i, kind] = ea
                    self.e_ref_phase_a = max(self.e_ref_phase_a, ea)

    def optimized(self, name):
        """the fp64 oracle's optimize(10) summaries of the case's windows under the default options (computed once)"""
        if name not in self._optimized:
            self._optimized[name] = [self.oracle.OracleWindow(w).optimize(10) for w in self.case(name)]
        return self._optimized[name]

    def case(self, name):
        """fresh copies of the case's windows (an upload must not see what an earlier test did to them)"""
        return copy.deepcopy(self.windows[name])

    def bound(self, a, scale):
        return BOUND_FACTOR * self.e_ref[a][scale]

    def deviations(self, name, i, arrays):
        """{array: {"entry", "max"}} of `arrays` from the referee of window i of the case"""
        return {a: {"entry": stmt.deviation_entrywise(arrays[a], self.ref[name][i][a], self.scale[name][i][a]),
                    "max": stmt.deviation(arrays[a], self.ref[name][i][a])} for a in stmt.ARRAYS}

    def check_input_condition(self, name):
        """no observation within DEPTH_MARGIN of the validity threshold (no case is skipped or filtered)"""
        for s in self.stmt64[name]:
            d = s["depth"][np.isfinite(s["depth"])]
            assert np.all(np.abs(d - stmt.MIN_DEPTH) >= fp32_cases.DEPTH_MARGIN), (name, d)

    def table(self):
        lines = [f"FP64REF e_ref {a:13s} entrywise {self.e_ref[a]['entry']:.3e}  max-scaled {self.e_ref[a]['max']:.3e}" for a in stmt.ARRAYS]
        return lines + [f"FP64REF e_ref phase_A       entrywise {self.e_ref_phase_a:.3e}"]
