"""The windows of the Schur referee (tests/test_gpu_schur_referee.py) and what both of its halves share — TEST INFRASTRUCTURE,
host only.  tests/test_schur_statement_host.py proves on the CPU that these inputs would notice a wrong reduction; the GPU file
compares the kernels on them.

Every window is synthetic.make_window at visibility 0.35 with one landmark cut down to a single pose block.  The pose parts
(fixed extrinsics, Dp = 6 K): 18; 60, the last size of the small tiles; 66, the first beyond them; 96, exactly one tile; 102, two
tiles of which the second holds one block; 198, three tiles.  The landmark counts sit around the stage of four, the serial batch
of 12, SCHUR_LM_BATCH = 16 and the chunk: a single window's chunks are its linearise groups (16 landmarks); the `wide` cases ask
for groups of 64 (okvis_ba_tuning::group_lm) so that a chunk runs over several batches (asserted from the index lists, which need
no device).

The referee of a case is the long-double build of the oracle after linearize() and the first solve under the case's options;
e_ref(A) — the bound's yardstick — is the larger of the fp64 oracle's and the numpy statement's deviation from it in the
entrywise scale of tests/schur_statement.py, maximised over ALL windows and modes of CASES.  It is kept for the whole array, for
its pose part (the rows and columns a Schur kernel writes) and, sharpest, for the landmark-only entries of S (Solved)."""
from __future__ import annotations

import copy

import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import default_options, set_options

from . import fp32_cases
from . import schur_statement as stmt

BOUND_FACTOR = fp32_cases.BOUND_FACTOR     # 4: what two correct fp64 evaluations may differ by (order of the sums, FMA contraction)
MUTATION_MARGIN = 10.0                     # a wrong reduction exceeds BOUND_FACTOR x e_ref at least tenfold
WEIGHTED = False                           # the scale does not weight a landmark's term with cond(Vd_l): profiles/schur_referee_notes.md
VISIBILITY = 0.35
ARRAYS = ("REDUCED_S", "REDUCED_RHS")
INPUTS = ("HPP", "GRADIENT", "LM_V", "LM_B", "PAIR_W")

# the trust-region modes: options of the solver | what the referee's first solve is damped with ("dl": mu = min_mu on the
# Jacobi-scaled diagonal, the Gauss-Newton point of the first dogleg iteration — also what gauss_newton = 1 solves under the
# default strategy; "lm": 1 / initial_radius on the clamped diagonal)
MODES = {"gn": (dict(gauss_newton=1), "dl"), "dogleg": ({}, "dl"), "lm": (dict(strategy=1), "lm")}
FLAT = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


def mode_options(mode, **kw):
    return set_options(default_options(), **dict(FLAT, **MODES[mode][0]), **kw)


def single_block(w, l):
    """landmark l keeps the observations of its first pose only: one (landmark, block) pair where the extrinsics are fixed"""
    lm, pose = np.asarray(w.obs_lm), np.asarray(w.obs_pose)
    first = pose[np.flatnonzero(lm == l)[0]]
    keep = (lm != l) | (pose == first)
    for name in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_sqrtw", "obs_uv"):
        setattr(w, name, np.asarray(getattr(w, name))[keep].copy())
    return w


def _window(K, L, seed, ext="fixed"):
    kw = dict(frame_dt=0.1) if K > 12 else {}
    return single_block(synthetic.make_window(K, L, VISIBILITY, seed, estimate_extrinsics=ext, **kw), 1)


WIDE = dict(tuning_group_lm=64)
# name: (windows, referee kinds, upload options)
CASES = {
    "k3_l5": (lambda: [_window(3, 5, 301)], ("dl", "lm"), {}),
    "k3_l13": (lambda: [_window(3, 13, 302)], ("dl",), {}),
    "k3_l65_wide": (lambda: [_window(3, 65, 403)], ("dl", "lm"), WIDE),
    "k10_l17": (lambda: [_window(10, 17, 304)], ("dl", "lm"), {}),
    "k10_l30": (lambda: [_window(10, 30, 305)], ("dl",), {}),
    "k10_l67_wide": (lambda: [_window(10, 67, 306)], ("dl", "lm"), WIDE),
    "k11_l30": (lambda: [_window(11, 30, 307)], ("dl", "lm"), {}),
    "k11_l65_wide": (lambda: [_window(11, 65, 308)], ("dl",), WIDE),
    "k16_l17": (lambda: [_window(16, 17, 309)], ("dl",), {}),
    "k17_l30": (lambda: [_window(17, 30, 310)], ("dl", "lm"), {}),
    "k17_l67_wide": (lambda: [_window(17, 67, 405)], ("dl",), WIDE),
    "k33_l30": (lambda: [_window(33, 30, 312)], ("dl",), {}),
    "ext_shared": (lambda: [_window(4, 30, 400, "shared")], ("dl", "lm"), {}),
    "ext_perframe": (lambda: [_window(3, 17, 314, "perframe")], ("dl",), {}),
    "ragged": (lambda: [_window(3, 13, 315), _window(7, 30, 316), _window(10, 17, 317)], ("dl", "lm"), {}),
}
SMALL = ("k3_l5", "k3_l13", "k3_l65_wide", "k10_l17", "k10_l30", "k10_l67_wide", "ragged")     # Dp <= 60, fixed extrinsics
LARGE = ("k11_l30", "k11_l65_wide", "k16_l17", "k17_l30", "k17_l67_wide", "k33_l30")             # Dp = 66, 66, 96, 102, 102, 198
TILED = ("k17_l30", "k17_l67_wide", "k33_l30")


class Solved:
    """one window under one damping kind: the referee, the fp64 oracle, the statement, the scale and their deviations"""

    def __init__(self, oracle, w, kind):
        opt = mode_options("lm" if kind == "lm" else "dogleg")
        self.opt = opt
        x, o = oracle.OracleWindow(w, extended=True), oracle.OracleWindow(w)
        for h in (x, o):
            h.linearize()
            assert h.solve(opt.initial_radius, opt) == 0
        self.pairs = o.pairs()
        self.off = stmt.pose_offsets(w)
        self.D = o.D
        self.Dp = 6 * int((self.off >= 0).sum())
        self.ref = {a: x.array(a) for a in ARRAYS + ("STEP", "HPP", "GRADIENT")}
        self.ref["REDUCED_S"] = self.ref["REDUCED_S"].reshape(self.D, self.D)
        self.o64 = {a: o.array(a) for a in ARRAYS + ("STEP",) + INPUTS}
        self.o64["REDUCED_S"] = self.o64["REDUCED_S"].reshape(self.D, self.D)
        self.stmt64 = dict(zip(ARRAYS, self.statement(self.o64, np.float64)))
        self.a = dict(zip(ARRAYS, self._call(stmt.scale, self.o64, self.o64, weighted=WEIGHTED)))
        self.a_other = dict(zip(ARRAYS, self._call(stmt.scale, self.o64, self.o64, weighted=not WEIGHTED)))
        # [array][pose part only]: the whole array | the rows and columns of the pose part, all a Schur kernel writes
        self.e_oracle = {a: [self.deviation(a, self.o64[a], p) for p in (False, True)] for a in ARRAYS}
        self.e_stmt = {a: [self.deviation(a, self.stmt64[a], p) for p in (False, True)] for a in ARRAYS}
        self.e_oracle_other = {a: stmt.deviation(self.o64[a], self.ref[a], self.a_other[a]) for a in ARRAYS}
        self.e_step = float(np.abs(self.o64["STEP"] - self.ref["STEP"]).max() / np.abs(self.ref["STEP"]).max())
        # The landmark-only entries: the pose part's entries with U_ij = 0 (blocks of two poses that no factor but a landmark
        # couples).  There S_ij is the Schur kernel's own sum and nothing else, so a fp64 evaluation is compared with the statement
        # in long double ON THE SAME INPUTS: what is left is the rounding of the reduction alone.
        U = np.asarray(self.o64["HPP"]).reshape(self.D, self.D)
        self.landmark_only = np.zeros((self.D, self.D), bool)
        self.landmark_only[:self.Dp, :self.Dp] = (U[:self.Dp, :self.Dp] == 0.0) & (self.a["REDUCED_S"][:self.Dp, :self.Dp] > 0.0)
        ld = np.asarray(self.statement(self.o64, np.longdouble)[0], np.float64)
        self.e_landmark_only = max(self.deviation_landmark_only(self.o64["REDUCED_S"], ld), self.deviation_landmark_only(self.stmt64["REDUCED_S"], ld))

    def _call(self, fn, lin, pose_part, **kw):
        """fn on the landmark-side arrays of `lin` and HPP / GRADIENT of `pose_part`, damped as the case is (the pose part's
        diagonal from `pose_part`, the landmarks' from `lin`)"""
        lam, Dp2, Dl2 = stmt.damping(self.opt, np.diag(np.asarray(pose_part["HPP"]).reshape(self.D, self.D)), lin["LM_V"])
        return fn(pose_part["HPP"], pose_part["GRADIENT"], lin["LM_V"], lin["LM_B"], lin["PAIR_W"], self.pairs[0], self.pairs[1],
                  self.off, lam, Dp2, Dl2, **kw)

    def statement(self, lin, dtype, pose_part=None, mutate=None):
        return self._call(stmt.reduce, lin, pose_part or lin, dtype=dtype, mutate=mutate)

    def cut_pose(self, x):
        x = np.asarray(x)
        return x[:self.Dp, :self.Dp] if x.ndim == 2 else x[:self.Dp]

    def deviation(self, array, x, pose_only=False, ref=None):
        """of x from the referee (or from `ref`) in the case's scale, over the whole array or over its pose part"""
        cut = self.cut_pose if pose_only else (lambda v: v)
        ref = self.ref[array] if ref is None else np.asarray(ref, np.float64)
        return stmt.deviation(cut(np.asarray(x, np.float64).reshape(ref.shape)), cut(ref), cut(self.a[array]))


    def deviation_landmark_only(self, S, S_long_double):
        m = self.landmark_only
        d = np.abs(np.asarray(S, np.float64).reshape(self.D, self.D) - np.asarray(S_long_double, np.float64).reshape(self.D, self.D))
        return float((d[m] / self.a["REDUCED_S"][m]).max()) if m.any() else 0.0


class Referee:
    """every case's windows solved once under each of its damping kinds; e_ref per array over all of them"""

    def __init__(self, oracle):
        self.windows, self.solved = {}, {}
        self.e_ref = {a: [0.0, 0.0] for a in ARRAYS}        # [array][pose part only]
        self.e_ref_landmark_only = 0.0
        for name, (make, kinds, _) in CASES.items():
            self.windows[name] = make()
            for kind in kinds:
                self.solved[name, kind] = [Solved(oracle, w, kind) for w in self.windows[name]]
                for s in self.solved[name, kind]:
                    self.e_ref_landmark_only = max(self.e_ref_landmark_only, s.e_landmark_only)
                    for a in ARRAYS:
                        for p in (0, 1):
                            self.e_ref[a][p] = max(self.e_ref[a][p], s.e_oracle[a][p], s.e_stmt[a][p])

    def case(self, name):
        """fresh copies of the case's windows"""
        return copy.deepcopy(self.windows[name])

    def options(self, name, mode, **kw):
        return mode_options(mode, **dict(CASES[name][2], **kw))

    def of(self, name, mode):
        return self.solved[name, MODES[mode][1]]

    def bound(self, a, pose_only=False):
        return BOUND_FACTOR * self.e_ref[a][int(pose_only)]


def chunk_landmarks(lists):
    """[(lm_begin, lm_end)] of the Schur chunks, from solver.index_lists"""
    d = np.asarray(lists["chunk_desc"]).reshape(-1, 20)
    return [(int(r[0]), int(r[1])) for r in d]
