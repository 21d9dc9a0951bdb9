"""The windows of the fp32 linearisation referee (tests/test_gpu_fp32_linearize.py) and what both of its halves share — TEST
INFRASTRUCTURE, host only.  tests/test_fp32_statement_host.py proves on the CPU that these inputs would notice a wrong Jacobian
term; the GPU file compares the kernels on them.

Cameras: the generator's intrinsics with tangential coefficients of a few 1e-3 and an equidistant k4 of the same size (the stock
ones, 1e-4, would leave a wrong tangential or k4 term below the float32 noise).  The measurements keep the generator's values: the
changed model adds some tenths of a pixel to the residuals.

e_stmt(A) — the bound's yardstick — is max |A_stmt32 - A_oracle| / max |A_oracle| over ALL windows of CASES."""
from __future__ import annotations

import copy
import functools

import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import DIST_EQUIDISTANT, DIST_NONE, DIST_RADTAN, DIST_RADTAN8

from . import fp32_statement as stmt

BOUND_FACTOR = 4.0          # kernel within 4 x e_stmt: summation order, FMA contraction, device atan / log / sqrt
DEPTH_MARGIN = 1.0e-4       # no observation this close to the 0.2 m validity threshold


def referee_camera(w):
    intr = np.asarray(w.cam_intr, np.float64).copy()
    for c in range(intr.shape[0]):
        sign = 1.0 if c % 2 == 0 else -1.0
        if w.cam_model[c] in (DIST_RADTAN, DIST_RADTAN8):
            intr[c, 6:8] = [3.0e-3 * sign, 2.5e-3]
        elif w.cam_model[c] == DIST_EQUIDISTANT:
            intr[c, 7] = 3.0e-3 * sign
    w.cam_intr = intr
    return w


def _window(K, L, seed, vis=0.7, **kw):
    return referee_camera(synthetic.make_window(K, L, vis, seed, **kw))


def _keep(w, mask):
    for name in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_sqrtw", "obs_uv"):
        setattr(w, name, np.asarray(getattr(w, name))[mask].copy())
    return w


def _camera_point_to_world(w, pose_idx, ext_idx, p_C):
    """p_W of the point p_C of the camera whose extrinsics are pose block ext_idx, seen from pose block pose_idx"""
    P, E = w.pose[pose_idx], w.pose[ext_idx]
    return P[:3] + synthetic.qrot(P[3:7]) @ (E[:3] + synthetic.qrot(E[3:7]) @ np.asarray(p_C, np.float64))


# ---- the routes' windows (3 - 6 keyframes, 20 - 60 landmarks) ----
def route_small():
    return [_window(4, 40, 101)]


def route_two():
    return [_window(4, 36, 102), _window(3, 27, 103, cam_model=DIST_EQUIDISTANT)]


def route_ext_shared():
    return [_window(4, 40, 104, estimate_extrinsics="shared")]


def route_ext_perframe():
    return [_window(3, 30, 105, estimate_extrinsics="perframe")]


# ---- the fused-mode boundary: 2 * SCHUR_LM_BATCH * 3 * Dp <= stage, Dp <= 30 (fp32) / 61 (fp64), 46 / 93 with free extrinsics ----
def boundary(K, ext):
    return [_window(K, 30, 110 + K, estimate_extrinsics=ext)]


# ---- models and edges ----
def model_window(model):
    return [_window(3, 30, 120 + model, cam_model=model)]


def edge_unobserved():
    w = _window(3, 20, 27)
    return [_keep(w, np.asarray(w.obs_lm) != 5)]


def edge_too_close():
    w = _window(3, 20, 28)
    w.lm = w.lm.copy()
    w.lm[0, :3] = w.pose[0, :3] + 0.01
    return [w]


def edge_negative_w():
    w = _window(3, 20, 29)
    w.lm = w.lm.copy()
    w.lm[1] *= -1.0
    return [w]


def edge_radtan8_undefined():
    """landmark 2 far off the axis of camera 0 at pose 0 (rho = 16.25 > 9) at one metre depth: projection undefined, zeros"""
    w = _window(3, 20, 131, cam_model=DIST_RADTAN8)
    o = np.flatnonzero((np.asarray(w.obs_lm) == 2) & (np.asarray(w.obs_cam) == 0))[0]
    w.lm = w.lm.copy()
    w.lm[2, :3] = _camera_point_to_world(w, int(w.obs_pose[o]), int(w.obs_ext[o]), [4.0, 0.5, 1.0])
    return [w]


def edge_equidistant_on_axis():
    """landmark 3 on the optical axis of one of its cameras, five metres out: r = |u| at rounding level"""
    w = _window(3, 20, 132, cam_model=DIST_EQUIDISTANT)
    o = np.flatnonzero(np.asarray(w.obs_lm) == 3)[0]
    w.lm = w.lm.copy()
    w.lm[3, :3] = _camera_point_to_world(w, int(w.obs_pose[o]), int(w.obs_ext[o]), [0.0, 0.0, 5.0])
    return [w]


# ---- piece enumeration (as tests/test_gpu_piece_path.py, at the smallest sizes that keep the property) ----
def piece_monocular():
    w = _window(8, 40, 61, vis=0.9)
    return [_keep(w, np.asarray(w.obs_cam) == 0)]


def piece_odd_counts():
    rng = np.random.default_rng(62)
    w = _window(6, 50, 62, vis=0.8)
    _keep(w, rng.random(w.obs_lm.size) > 0.23)
    counts = np.bincount(np.asarray(w.obs_lm), minlength=w.lm.shape[0])
    assert (counts % 2 == 1).sum() > 10
    return [w]


def piece_three_and_four():
    w = _window(4, 30, 65)
    rng = np.random.default_rng(65)
    n = w.obs_lm.size
    extra = np.concatenate([rng.choice(n, 20, replace=False), rng.choice(n, 20, replace=False), rng.choice(n, 14, replace=False)])
    order = np.sort(np.concatenate([np.arange(n), extra]))
    uv = np.asarray(w.obs_uv)[order].copy()
    is_dup = np.r_[False, order[1:] == order[:-1]]
    uv[is_dup] += rng.uniform(-1.5, 1.5, (int(is_dup.sum()), 2))
    for name in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_sqrtw"):
        setattr(w, name, np.asarray(getattr(w, name))[order].copy())
    w.obs_uv = uv
    runs = np.diff(np.flatnonzero(np.r_[True, (np.diff(w.obs_lm) != 0) | (np.diff(w.obs_pose) != 0), True]))
    assert (runs >= 3).sum() > 5 and (runs >= 4).sum() > 1
    return [w]


def piece_beyond_128():
    """a landmark seen from more than 128 poses: the piece path refuses it, the batch runs through the staged kernel"""
    w = _window(140, 5, 66, vis=1.0, with_imu=False, frame_dt=0.05)
    _keep(w, np.asarray(w.obs_cam) == 0)
    w.pose_fixed = np.asarray(w.pose_fixed).copy()
    w.pose_fixed[:134] = 1
    w.sb_fixed = np.ones_like(np.asarray(w.sb_fixed))
    assert np.bincount(np.asarray(w.obs_lm)).max() > 128
    return [w]


def piece_beyond_64_poses():
    """72 pose blocks > LIN2_POSES: the piece path reads the poses from global memory"""
    w = _window(70, 5, 68, vis=1.0, with_imu=False, frame_dt=0.05)
    w.pose_fixed = np.asarray(w.pose_fixed).copy()
    w.pose_fixed[:62] = 1
    w.sb_fixed = np.ones_like(np.asarray(w.sb_fixed))
    assert w.pose.shape[0] > 64 and np.bincount(np.asarray(w.obs_lm)).max() == 140
    return [w]


def ragged_batch():
    return [_window(3, 20, 141), _window(5, 45, 142, cam_model=DIST_EQUIDISTANT), _window(4, 33, 143, cam_model=DIST_RADTAN8)]


CASES = {
    "route_small": route_small, "route_two": route_two, "route_ext_shared": route_ext_shared,
    "route_ext_perframe": route_ext_perframe,
    "boundary_5_fixed": functools.partial(boundary, 5, "fixed"), "boundary_6_fixed": functools.partial(boundary, 6, "fixed"),
    "boundary_5_shared": functools.partial(boundary, 5, "shared"), "boundary_6_shared": functools.partial(boundary, 6, "shared"),
    "model_none": functools.partial(model_window, DIST_NONE), "model_radtan": functools.partial(model_window, DIST_RADTAN),
    "model_equidistant": functools.partial(model_window, DIST_EQUIDISTANT), "model_radtan8": functools.partial(model_window, DIST_RADTAN8),
    "edge_unobserved": edge_unobserved, "edge_too_close": edge_too_close, "edge_negative_w": edge_negative_w,
    "edge_radtan8_undefined": edge_radtan8_undefined, "edge_equidistant_on_axis": edge_equidistant_on_axis,
    "piece_monocular": piece_monocular, "piece_odd_counts": piece_odd_counts, "piece_three_and_four": piece_three_and_four,
    "piece_beyond_128": piece_beyond_128, "piece_beyond_64_poses": piece_beyond_64_poses,
    "ragged_batch": ragged_batch,
}


class Referee:
    """Every case's windows with the float32 statement and the oracle's arrays of each, computed once; e_stmt per array."""

    def __init__(self, oracle):
        self.windows, self.stmt32, self.stmt64, self.oracle_arrays, self.oracle_pairs, self.e_case = {}, {}, {}, {}, {}, {}
        self.e_stmt = {a: 0.0 for a in stmt.ARRAYS}
        for name, make in CASES.items():
            ws = make()
            self.windows[name] = ws
            self.stmt32[name], self.stmt64[name], self.oracle_arrays[name], self.oracle_pairs[name], self.e_case[name] = [], [], [], [], []
            for w in ws:
                s32 = stmt.window_arrays(w, np.float32)
                o = oracle.OracleWindow(w)
                o.linearize()
                arrays = {a: o.array(a) for a in stmt.ARRAYS + ("IMU_RESIDUAL",)}
                e = {a: stmt.deviation(s32[a], arrays[a]) for a in stmt.ARRAYS}
                for a in stmt.ARRAYS:
                    self.e_stmt[a] = max(self.e_stmt[a], e[a])
                self.stmt32[name].append(s32)
                self.stmt64[name].append(stmt.window_arrays(w, np.float64))
                self.oracle_arrays[name].append(arrays)
                self.oracle_pairs[name].append(o.pairs())
                self.e_case[name].append(e)

    def case(self, name):
        """fresh copies of the case's windows (an upload must not see what an earlier test did to them)"""
        return copy.deepcopy(self.windows[name])

    def check_input_condition(self, name):
        """no observation within DEPTH_MARGIN of the validity threshold, and float32 takes the branches float64 takes"""
        for s32, s64 in zip(self.stmt32[name], self.stmt64[name]):
            d = s32["depth"]
            assert np.all(np.abs(d[np.isfinite(d)] - stmt.MIN_DEPTH) >= DEPTH_MARGIN), (name, d)
            assert np.all(np.abs(s64["depth"][np.isfinite(s64["depth"])] - stmt.MIN_DEPTH) >= DEPTH_MARGIN)
            assert np.array_equal(s32["defined"], s64["defined"]) and np.array_equal(s32["valid"], s64["valid"]), name
