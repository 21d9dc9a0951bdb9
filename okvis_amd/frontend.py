"""ctypes view of include/okvis_amd_frontend.h: the batched reprojection pieces of the OKVIS frontend (stereo triangulation
with uncertainty, 3D-2D projection and chi-square gating), its descriptor matching (Hamming candidates, the dense matcher's
best-match search), whole verified matching steps (the matcher under "Hamming distance and verifyMatch"), the outlier rejection
behind it (bearing vectors, consensus scoring, the two-point and five-point solvers of the 2D-2D problems, the generalised
three-point solver of the 3D-2D problem, and whole RANSAC runs with the sampler and the adaptive loop on the device), the IMU state
propagation with covariance and Jacobian, the keyframe decision (exact hulls, areas and inside counts), keypoint detection
(Harris scores, 3 x 3 maxima and greedy uniformity selection, exact) and keypoint description (the reference's gravity-aligned
angle, a 48-byte binary descriptor stated in the header, exact) on the MI355X.  No CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .window import ImuParamsC

TRI_VALID, TRI_NOT_PARALLEL, TRI_CAN_INIT, TRI_RANK_DEFICIENT = 1, 2, 4, 8
PROJ_SUCCESSFUL, PROJ_OUTSIDE_IMAGE, PROJ_MASKED, PROJ_BEHIND, PROJ_INVALID = range(5)
GATE_VERIFIED, GATE_ACCEPTED, GATE_UNCERTAIN = 1, 2, 4
SYMBOLS = ["okvis_fe_create", "okvis_fe_destroy", "okvis_fe_stereo_triangulate", "okvis_fe_stereo_triangulate_gn", "okvis_fe_project_landmarks",
           "okvis_fe_gate_3d2d", "okvis_fe_hamming_candidates", "okvis_fe_match_descriptors", "okvis_fe_bearing_vectors",
           "okvis_fe_sac_consensus", "okvis_fe_match_verified", "okvis_fe_imu_propagate", "okvis_fe_keyframe_decision",
           "okvis_fe_sac_solve", "okvis_fe_sac_solve_absolute", "okvis_fe_ransac", "okvis_fe_detect_keypoints",
           "okvis_fe_describe_keypoints", "okvis_fe_detect_and_describe", "okvis_fe_describe_tables", "okvis_fe_detect_keypoints_scaled",
           "okvis_fe_detect_scaled_and_describe"]
MATCH_3D2D, MATCH_2D2D = 1, 2
SAC_ABSOLUTE, SAC_ROTATION_ONLY, SAC_RELATIVE = 0, 1, 2
SAC_SAMPLE_ROTATION_ONLY, SAC_SAMPLE_RELATIVE, SAC_MAX_ROOTS = 2, 8, 10
SAC_SAMPLE_ABSOLUTE, SAC_MAX_ROOTS_ABSOLUTE = 4, 8
SAC_SAMPLE_SIZE = {SAC_ABSOLUTE: SAC_SAMPLE_ABSOLUTE, SAC_ROTATION_ONLY: SAC_SAMPLE_ROTATION_ONLY, SAC_RELATIVE: SAC_SAMPLE_RELATIVE}
RANSAC_STOP_CONVERGED, RANSAC_STOP_MAX_ITERATIONS, RANSAC_STOP_EXHAUSTED, RANSAC_STOP_SKIPS, RANSAC_STOP_NO_SAMPLE = range(5)
IMU_COV, IMU_JAC = 1, 2
KF_FEW_POINTS, KF_FEW_MATCHES = 1, 2
KF_MAX_KEYPOINTS, KF_MAX_CAMS = 8192, 8
DETECT_OVERFLOW, DETECT_FULL = 1, 2
DETECT_MAX_DIM, DETECT_MAX_KEYPOINTS, DETECT_MAX_CANDIDATES = 8192, 2048, 8192
DETECT_TILE_X, DETECT_TILE_Y = 64, 16            # the score kernel's tile (fe_detect.hpp: DET_TILE_X, DET_TILE_Y)
DETECT_WAVE, DETECT_SELECT_THREADS = 64, 1024    # the selection kernel's widths (DET_SEL_THREADS)
DETECT_MAX_OCTAVES, DETECT_MAX_LAYERS = 4, 5       # the scale space (fe_detect_scale.hpp: DET_MAX_OCTAVES, DET_MAX_LAYERS)
DETECT_KP_SIZE = 12.0                            # BRISK's basic size at scale 1; okvis takes sigma = 0.8 size / 12
DESCRIBE_VALID, DESCRIBE_ANGLE_UNDEFINED = 1, 2
DESCRIBE_BYTES, DESCRIBE_ROTATIONS, DESCRIBE_PAIRS, DESCRIBE_POINTS = 48, 1024, 383, 60
DESCRIBE_MARGIN = 176                            # sixteenths of a pixel (fe_describe.hpp: DSC_MARGIN)


class CameraC(C.Structure):
    """okvis_fe_camera"""
    _fields_ = [("intr", C.c_double * 12), ("model", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("reserved", C.c_int32)]


class MatchJobC(C.Structure):
    """okvis_fe_match_job"""
    _fields_ = [("n_a", C.c_int32), ("n_b", C.c_int32), ("desc_a", C.c_void_p), ("desc_b", C.c_void_p), ("skip_a", C.c_void_p),
                ("skip_b", C.c_void_p), ("pair_a", C.c_void_p), ("pair_dist", C.c_void_p), ("accepted", C.c_void_p)]


class VMatchJobC(C.Structure):
    """okvis_fe_vmatch_job"""
    _fields_ = [("kind", C.c_int32), ("n_a", C.c_int32), ("n_b", C.c_int32), ("desc_a", C.c_void_p), ("desc_b", C.c_void_p),
                ("skip_a", C.c_void_p), ("skip_b", C.c_void_p), ("kp_a", C.c_void_p), ("kp_b", C.c_void_p), ("cam_a", CameraC),
                ("cam_b", CameraC), ("hp_W", C.c_void_p), ("T_CbW", C.c_double * 7), ("P3", C.c_double * 9), ("T_AB", C.c_double * 7),
                ("UOplus", C.c_double * 36), ("pair_a", C.c_void_p), ("pair_dist", C.c_void_p), ("accepted", C.c_void_p),
                ("proj_status", C.c_void_p), ("uv", C.c_void_p), ("U", C.c_void_p), ("chi2", C.c_void_p), ("gate_flags", C.c_void_p),
                ("hp_a", C.c_void_p), ("cov", C.c_void_p), ("tri_flags", C.c_void_p)]


class SacJobC(C.Structure):
    """okvis_fe_sac_job"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("n_models", C.c_int32), ("n_cams", C.c_int32), ("threshold", C.c_double),
                ("models", C.c_void_p), ("points", C.c_void_p), ("bearing", C.c_void_p), ("sigma", C.c_void_p), ("cam_index", C.c_void_p),
                ("cam_offsets", C.c_void_p), ("cam_rotations", C.c_void_p), ("bearing1", C.c_void_p), ("bearing2", C.c_void_p),
                ("sigma1", C.c_void_p), ("sigma2", C.c_void_p), ("counts", C.c_void_p), ("best", C.c_void_p), ("n_inliers", C.c_void_p),
                ("inliers", C.c_void_p), ("scores", C.c_void_p)]


class SacSolveJobC(C.Structure):
    """okvis_fe_sac_solve_job"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("n_models", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double),
                ("bearing1", C.c_void_p), ("bearing2", C.c_void_p), ("sigma1", C.c_void_p), ("sigma2", C.c_void_p),
                ("samples", C.c_void_p), ("models", C.c_void_p), ("valid", C.c_void_p), ("n_roots", C.c_void_p),
                ("essentials", C.c_void_p), ("counts", C.c_void_p), ("best", C.c_void_p), ("n_inliers", C.c_void_p),
                ("inliers", C.c_void_p), ("scores", C.c_void_p)]


class SacAbsoluteJobC(C.Structure):
    """okvis_fe_sac_absolute_job"""
    _fields_ = [("n", C.c_int32), ("n_models", C.c_int32), ("n_cams", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double),
                ("points", C.c_void_p), ("bearing", C.c_void_p), ("sigma", C.c_void_p), ("cam_index", C.c_void_p),
                ("cam_offsets", C.c_void_p), ("cam_rotations", C.c_void_p), ("samples", C.c_void_p), ("models", C.c_void_p),
                ("valid", C.c_void_p), ("n_roots", C.c_void_p), ("candidates", C.c_void_p), ("counts", C.c_void_p), ("best", C.c_void_p),
                ("n_inliers", C.c_void_p), ("inliers", C.c_void_p), ("scores", C.c_void_p)]


class RansacJobC(C.Structure):
    """okvis_fe_ransac_job"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("n_slots", C.c_int32), ("n_cams", C.c_int32), ("max_iterations", C.c_int32),
                ("reserved", C.c_int32), ("threshold", C.c_double), ("probability", C.c_double), ("seed", C.c_uint64),
                ("points", C.c_void_p), ("bearing", C.c_void_p), ("sigma", C.c_void_p), ("cam_index", C.c_void_p),
                ("cam_offsets", C.c_void_p), ("cam_rotations", C.c_void_p), ("bearing1", C.c_void_p), ("bearing2", C.c_void_p),
                ("sigma1", C.c_void_p), ("sigma2", C.c_void_p), ("best", C.c_void_p), ("n_inliers", C.c_void_p), ("inliers", C.c_void_p),
                ("model", C.c_void_p), ("iterations", C.c_void_p), ("skipped", C.c_void_p), ("stop", C.c_void_p), ("samples", C.c_void_p),
                ("valid", C.c_void_p), ("counts", C.c_void_p), ("models", C.c_void_p)]


class ImuJobC(C.Structure):
    """okvis_fe_imu_job"""
    _fields_ = [("s_begin", C.c_int32), ("s_count", C.c_int32), ("e_begin", C.c_int32), ("e_count", C.c_int32), ("prm", C.c_int32),
                ("flags", C.c_int32), ("t_start", C.c_int64), ("T_WS", C.c_double * 7), ("sb", C.c_double * 9)]


class KfImageC(C.Structure):
    """okvis_fe_kf_image"""
    _fields_ = [("kp_begin", C.c_int32), ("kp_count", C.c_int32)]


class KfJobC(C.Structure):
    """okvis_fe_kf_job"""
    _fields_ = [("im_begin", C.c_int32), ("n_cams", C.c_int32), ("num_frames", C.c_int32), ("initialized", C.c_int32),
                ("overlap_threshold", C.c_float), ("ratio_threshold", C.c_float)]


class DetectJobC(C.Structure):
    """okvis_fe_detect_job"""
    _fields_ = [("image", C.c_void_p), ("threshold", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32),
                ("min_dist", C.c_int32), ("max_keypoints", C.c_int32), ("cand_capacity", C.c_int32), ("kp_size", C.c_float),
                ("n_keypoints", C.c_int32), ("n_candidates", C.c_int32), ("flags", C.c_int32), ("kp", C.c_void_p),
                ("response", C.c_void_p), ("pixel", C.c_void_p), ("score", C.c_void_p)]


class DetectScaleJobC(C.Structure):
    """okvis_fe_detect_scale_job"""
    _fields_ = [("image", C.c_void_p), ("threshold", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32),
                ("min_dist", C.c_int32), ("max_keypoints", C.c_int32), ("cand_capacity", C.c_int32), ("kp_size", C.c_float),
                ("octaves", C.c_int32), ("n_keypoints", C.c_int32), ("n_candidates", C.c_int32), ("flags", C.c_int32),
                ("n_layers", C.c_int32), ("n_layer_candidates", C.c_int32 * 5), ("kp", C.c_void_p), ("response", C.c_void_p),
                ("pixel", C.c_void_p), ("layer", C.c_void_p), ("scale", C.c_void_p), ("score", C.c_void_p), ("pyramid", C.c_void_p)]


class DescribeJobC(C.Structure):
    """okvis_fe_describe_job"""
    _fields_ = [("image", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("n", C.c_int32),
                ("kp", C.c_void_p), ("cam", C.POINTER(CameraC)), ("direction", C.c_double * 3), ("rot_in", C.c_void_p),
                ("n_valid", C.c_int32), ("desc", C.c_void_p), ("flags", C.c_void_p), ("rot", C.c_void_p), ("angle", C.c_void_p),
                ("angle64", C.c_void_p)]


def camera(intr, model, width=752, height=480) -> CameraC:
    c = CameraC()
    k = np.zeros(12)
    k[:len(intr)] = intr
    c.intr[:] = list(k)
    c.model, c.width, c.height = int(model), int(width), int(height)
    return c


def _f32(a, cols):
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, np.float64)
    return a if shape is None else a.reshape(shape)


def _desc(a):
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim != 2:
        raise ValueError("descriptors are [n][bytes] uint8")
    return a


def _skip(m, n):
    if m is None:
        return None
    m = np.ascontiguousarray(np.asarray(m).astype(bool), np.uint8)
    if m.shape != (n,):
        raise ValueError("a skip mask has one entry per keypoint")
    return m


def _ptr(a):
    return None if a is None else a.ctypes.data


def declare(L, prefix="okvis_fe_", with_context=True):
    """signatures of the three batch entries under `prefix` (the reference build exports them as ref_fe_* without a context)"""
    vp = C.c_void_p
    ctx = [vp] if with_context else []
    cam = C.POINTER(CameraC)
    getattr(L, prefix + "stereo_triangulate").argtypes = ctx + [cam, cam, vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp,
                                                                C.c_int32, vp, vp, vp]
    if with_context and hasattr(L, prefix + "stereo_triangulate_gn"):
        getattr(L, prefix + "stereo_triangulate_gn").argtypes = ctx + [cam, cam, vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp,
                                                                       C.c_int32, vp, vp, vp, vp]
    getattr(L, prefix + "project_landmarks").argtypes = ctx + [cam, vp, vp, C.c_int32, vp, vp, vp, vp]
    getattr(L, prefix + "gate_3d2d").argtypes = ctx + [C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp]
    if with_context:   # the matching entries: the reference build has no such entries
        i32 = C.c_int32
        L.okvis_fe_hamming_candidates.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, C.c_float, i32, vp, vp, C.POINTER(i32)]
        L.okvis_fe_match_descriptors.argtypes = [vp, i32, C.POINTER(MatchJobC), i32, C.c_float, i32, i32, C.c_float]
        L.okvis_fe_bearing_vectors.argtypes = [vp, cam, i32, vp, vp, vp, vp]
        L.okvis_fe_sac_consensus.argtypes = [vp, i32, C.POINTER(SacJobC)]
        L.okvis_fe_sac_solve.argtypes = [vp, i32, C.POINTER(SacSolveJobC)]
        L.okvis_fe_sac_solve_absolute.argtypes = [vp, i32, C.POINTER(SacAbsoluteJobC)]
        L.okvis_fe_ransac.argtypes = [vp, i32, C.POINTER(RansacJobC)]
        L.okvis_fe_match_verified.argtypes = [vp, i32, C.POINTER(VMatchJobC), i32, C.c_float, i32, i32, C.c_float]
        L.okvis_fe_imu_propagate.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, C.POINTER(ImuJobC), vp, vp, vp, vp, vp]
        L.okvis_fe_keyframe_decision.argtypes = [vp, i32, vp, vp, i32, C.POINTER(KfImageC), i32, C.POINTER(KfJobC)] + [vp] * 12
        L.okvis_fe_detect_keypoints.argtypes = [vp, i32, C.POINTER(DetectJobC)]
        L.okvis_fe_describe_keypoints.argtypes = [vp, i32, C.POINTER(DescribeJobC)]
        L.okvis_fe_detect_and_describe.argtypes = [vp, i32, C.POINTER(DetectJobC), C.POINTER(DescribeJobC)]
        L.okvis_fe_describe_tables.argtypes = [C.POINTER(vp)] * 5 + [C.POINTER(i32)]
        L.okvis_fe_detect_keypoints_scaled.argtypes = [vp, i32, C.POINTER(DetectScaleJobC)]
        L.okvis_fe_detect_scaled_and_describe.argtypes = [vp, i32, C.POINTER(DetectScaleJobC), C.POINTER(DescribeJobC)]


class Frontend:
    """One okvis_fe_context.  `api=(library, prefix)` swaps in another implementation of the same three entries (the tests
    pass the reference build); the default is the HIP library."""

    def __init__(self, device: int = 0, api=None):
        if api is None:
            self._L, self._prefix, self._ctx = _lib.lib(), "okvis_fe_", C.c_void_p()
            for s in SYMBOLS:
                getattr(self._L, s)
            declare(self._L)
            self._L.okvis_fe_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
            self._L.okvis_fe_destroy.argtypes = [C.c_void_p]
            _lib.check(self._L.okvis_fe_create(C.byref(self._ctx), int(device)), "okvis_fe_create")
        else:
            self._L, self._prefix = api
            self._ctx = None
            declare(self._L, self._prefix, with_context=False)

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.okvis_fe_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _call(self, name, *args):
        fn = getattr(self._L, self._prefix + name)
        rc = fn(self._ctx, *args) if self._ctx is not None else fn(*args)
        if self._ctx is not None:
            _lib.check(rc, name)
        elif rc != 0:
            raise RuntimeError(f"{self._prefix}{name} returned {rc}")

    def stereo_triangulate(self, cam_a: CameraC, cam_b: CameraC, T_AB, UOplus, kp_a, kp_b, pairs, sigma_ray=None,
                           want_uncertainty=True):
        """-> hp_A [n][4], cov [n][3][3], flags [n] (TRI_* bits)"""
        kp_a, kp_b = _f32(kp_a, 3), _f32(kp_b, 3)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        T_AB, UOplus = _f64(T_AB, 7), _f64(UOplus, (6, 6))
        sig = None if sigma_ray is None else _f64(sigma_ray, n)
        hp, cov, flags = np.zeros((n, 4)), np.zeros((n, 3, 3)), np.zeros(n, np.uint8)
        self._call("stereo_triangulate", C.byref(cam_a), C.byref(cam_b), T_AB.ctypes.data, UOplus.ctypes.data, len(kp_a),
                   kp_a.ctypes.data, len(kp_b), kp_b.ctypes.data, n, pairs.ctypes.data, None if sig is None else sig.ctypes.data,
                   int(bool(want_uncertainty)), hp.ctypes.data, cov.ctypes.data, flags.ctypes.data)
        return hp, cov, flags

    def stereo_triangulate_gn(self, cam_a: CameraC, cam_b: CameraC, T_AB, UOplus, kp_a, kp_b, pairs, sigma_ray=None):
        """okvis_fe_stereo_triangulate_gn -> hp_A, cov, flags, gn [n][9][9] (the Gauss-Newton matrix getUncertainty inverts)"""
        kp_a, kp_b = _f32(kp_a, 3), _f32(kp_b, 3)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        T_AB, UOplus = _f64(T_AB, 7), _f64(UOplus, (6, 6))
        sig = None if sigma_ray is None else _f64(sigma_ray, n)
        hp, cov, flags, gn = np.zeros((n, 4)), np.zeros((n, 3, 3)), np.zeros(n, np.uint8), np.zeros((n, 9, 9))
        self._call("stereo_triangulate_gn", C.byref(cam_a), C.byref(cam_b), T_AB.ctypes.data, UOplus.ctypes.data, len(kp_a),
                   kp_a.ctypes.data, len(kp_b), kp_b.ctypes.data, n, pairs.ctypes.data, None if sig is None else sig.ctypes.data,
                   1, hp.ctypes.data, cov.ctypes.data, flags.ctypes.data, gn.ctypes.data)
        return hp, cov, flags, gn

    def project_landmarks(self, cam_b: CameraC, T_CbW, P3, hp_W):
        """-> uv [n][2], U [n][2][2], status [n] (PROJ_*)"""
        hp_W = _f64(hp_W).reshape(-1, 4)
        n = len(hp_W)
        T_CbW, P3 = _f64(T_CbW, 7), _f64(P3, (3, 3))
        uv, U, st = np.zeros((n, 2)), np.zeros((n, 2, 2)), np.zeros(n, np.uint8)
        self._call("project_landmarks", C.byref(cam_b), T_CbW.ctypes.data, P3.ctypes.data, n, hp_W.ctypes.data, uv.ctypes.data,
                   U.ctypes.data, st.ctypes.data)
        return uv, U, st

    def gate_3d2d(self, uv, U, kp_b, pairs):
        """-> chi2 [n], flags [n] (GATE_* bits)"""
        uv, U, kp_b = _f64(uv).reshape(-1, 2), _f64(U).reshape(-1, 2, 2), _f32(kp_b, 3)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        chi2, flags = np.zeros(n), np.zeros(n, np.uint8)
        self._call("gate_3d2d", len(uv), uv.ctypes.data, U.ctypes.data, len(kp_b), kp_b.ctypes.data, n, pairs.ctypes.data,
                   chi2.ctypes.data, flags.ctypes.data)
        return chi2, flags

    def hamming_candidates(self, desc_a, desc_b, threshold, skip_a=None, skip_b=None):
        """-> pairs [n][2] int32 in ascending (a, b) order, dist [n] float32: the keypoints in play whose descriptors
        ([n][16 | 32 | 48 | 64] uint8) differ in fewer than `threshold` bits.  Two calls: one counts, one fills."""
        desc_a, desc_b = _desc(desc_a), _desc(desc_b)
        if desc_a.shape[1] != desc_b.shape[1]:
            raise ValueError("descriptors of different lengths")
        skip_a, skip_b = _skip(skip_a, len(desc_a)), _skip(skip_b, len(desc_b))
        n = C.c_int32(0)
        args = (desc_a.shape[1], len(desc_a), desc_a.ctypes.data, _ptr(skip_a), len(desc_b), desc_b.ctypes.data, _ptr(skip_b),
                float(threshold))
        self._call("hamming_candidates", *args, 0, None, None, C.byref(n))
        pairs, dist = np.zeros((n.value, 2), np.int32), np.zeros(n.value, np.float32)
        if n.value:
            self._call("hamming_candidates", *args, n.value, pairs.ctypes.data, dist.ctypes.data, C.byref(n))
            assert n.value == len(pairs)
        return pairs, dist

    def match_descriptors(self, jobs, threshold, num_best=4, use_ratio=False, ratio_threshold=0.0):
        """jobs: (desc_a, desc_b) or (desc_a, desc_b, skip_a, skip_b) per image pair.  -> per job (pair_a [n_b] int32, pair_dist
        [n_b] float32, accepted [n_b] bool): what okvis::DenseMatcher(1, num_best, use_ratio).match leaves in vpairs, and where it
        calls setBestMatch.  All jobs go through one call."""
        keep, out = [], []
        table = (MatchJobC * max(1, len(jobs)))()
        width = None
        for j, job in enumerate(jobs):
            da, db = _desc(job[0]), _desc(job[1])
            sa = _skip(job[2], len(da)) if len(job) > 2 else None
            sb = _skip(job[3], len(db)) if len(job) > 3 else None
            if da.shape[1] != db.shape[1] or width not in (None, da.shape[1]):
                raise ValueError("descriptors of different lengths")
            width = da.shape[1]
            pa, pd, acc = np.zeros(len(db), np.int32), np.zeros(len(db), np.float32), np.zeros(len(db), np.uint8)
            keep.append((da, db, sa, sb))
            out.append((pa, pd, acc))
            t = table[j]
            t.n_a, t.n_b = len(da), len(db)
            t.desc_a, t.desc_b, t.skip_a, t.skip_b = da.ctypes.data, db.ctypes.data, _ptr(sa), _ptr(sb)
            t.pair_a, t.pair_dist, t.accepted = pa.ctypes.data, pd.ctypes.data, acc.ctypes.data
        self._call("match_descriptors", len(jobs), table, 48 if width is None else width, float(threshold), int(num_best),
                   int(bool(use_ratio)), float(ratio_threshold))
        return [(pa, pd, acc.astype(bool)) for pa, pd, acc in out]

    def match_verified(self, jobs, threshold, num_best=4, use_ratio=False, ratio_threshold=0.0):
        """Whole matching steps under the frontend's own distance (Hamming distance under the threshold AND verifyMatch).  jobs: dicts
        with kind (MATCH_3D2D | MATCH_2D2D), desc_a, desc_b, kp_b [n_b][3], cam_b, optional skip_a / skip_b, and
        MATCH_2D2D: kp_a [n_a][3], cam_a, T_AB [7], UOplus [6][6];
        MATCH_3D2D: hp_W [n_a][4], T_CbW [7], P3 [3][3] (kp_a, cam_a optional).
        -> per job a dict: pair_a [n_b] int32, pair_dist [n_b] float32, accepted [n_b] bool, and for the accepted pairs (zeros
        elsewhere) MATCH_3D2D: chi2 [n_b], gate_flags [n_b] besides proj_status [n_a], uv [n_a][2], U [n_a][2][2];
        MATCH_2D2D: hp_a [n_b][4], cov [n_b][3][3], tri_flags [n_b].  All jobs go through one call; they must not depend on each
        other's result."""
        table, keep, out = vmatch_job_table(jobs)
        width = keep[0][0].shape[1] if keep else 48
        self._call("match_verified", len(jobs), table, width, float(threshold), int(num_best), int(bool(use_ratio)),
                   float(ratio_threshold))
        for r in out:
            r["accepted"] = r["accepted"].astype(bool)
        return out

    def bearing_vectors(self, cam: CameraC, kp):
        """kp [n][3] (x, y, size) -> bearing [n][3] unit vectors, sigma_angle [n], ok [n] bool: what the two RANSAC adapters hold
        per keypoint"""
        kp = _f32(kp, 3)
        n = len(kp)
        bearing, sigma, ok = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint8)
        self._call("bearing_vectors", C.byref(cam), n, kp.ctypes.data, bearing.ctypes.data, sigma.ctypes.data, ok.ctypes.data)
        return bearing, sigma, ok.astype(bool)

    def sac_consensus(self, jobs, want_scores=False):
        """jobs: dicts with kind (SAC_*), models [K][3][4] (or [K][3][3] for SAC_ROTATION_ONLY), threshold (default 9) and
        SAC_ABSOLUTE: points, bearing [n][3], sigma [n], cam_index [n], cam_offsets [c][3], cam_rotations [c][3][3];
        the other kinds: bearing1, bearing2 [n][3], sigma1, sigma2 [n].
        -> per job a dict: counts [K] int32, best, n_inliers, inliers [n_inliers] int32 (ascending), and scores [K][n] under
        want_scores.  All jobs go through one call."""
        table, keep, out = sac_job_table(jobs, want_scores)
        self._call("sac_consensus", len(jobs), table)
        res = []
        for counts, scalars, inl, sc in out:
            r = {"counts": counts, "best": int(scalars[0]), "n_inliers": int(scalars[1]), "inliers": inl[:int(scalars[1])].copy()}
            if want_scores:
                r["scores"] = sc
            res.append(r)
        return res

    def sac_solve(self, jobs, want_scores=False, want_essentials=False):
        """The minimal solvers of the 2D-2D outlier rejection in front of sac_consensus, all jobs in one call.  jobs: dicts with
        kind (SAC_ROTATION_ONLY or SAC_RELATIVE), bearing1, bearing2 [n][3], samples [K][2] (rotation only) or [K][8] (relative:
        five that define E, three more that pick the pose), threshold (default 9), sigma1, sigma2 [n] (may be left out of a job
        with consensus=False: the relative selection then weighs with 1), consensus (default True: score the hypotheses).
        -> per job a dict: models [K][3][3] / [K][3][4] (NaN where invalid), valid [K] bool; with consensus counts, best,
        n_inliers, inliers as sac_consensus returns them, and scores [K][n] under want_scores; relative jobs under
        want_essentials also n_roots [K] and essentials [K][10][9] (unit norm, NaN past n_roots)."""
        table, keep, out = sac_solve_job_table(jobs, want_scores, want_essentials)
        self._call("sac_solve", len(jobs), table)
        res = []
        for o in out:
            r = {"models": o["models"], "valid": o["valid"].astype(bool)}
            if "counts" in o:
                k = int(o["scalars"][1])
                r.update(counts=o["counts"], best=int(o["scalars"][0]), n_inliers=k, inliers=o["inliers"][:k].copy())
            for name in ("scores", "n_roots", "essentials"):
                if name in o:
                    r[name] = o[name]
            res.append(r)
        return res

    def sac_solve_absolute(self, jobs, want_scores=False, want_candidates=False):
        """The minimal solver of the 3D-2D outlier rejection (generalised three-point absolute pose) in front of sac_consensus, all
        jobs in one call.  jobs: dicts with points, bearing [n][3], cam_index [n], cam_offsets [c][3], cam_rotations [c][3][3] as
        sac_consensus takes them, samples [K][4] (three that define the candidates, one more that picks the pose), threshold
        (default 9), sigma [n] (may be left out of a job with consensus=False), consensus (default True: score the hypotheses).
        -> per job a dict: models [K][3][4] (body to world; NaN where invalid), valid [K] bool; with consensus counts, best,
        n_inliers, inliers as sac_consensus returns them, and scores [K][n] under want_scores; under want_candidates also n_roots
        [K] and candidates [K][8][3][4] (NaN past n_roots)."""
        table, keep, out = sac_absolute_job_table(jobs, want_scores, want_candidates)
        self._call("sac_solve_absolute", len(jobs), table)
        res = []
        for o in out:
            r = {"models": o["models"], "valid": o["valid"].astype(bool)}
            if "counts" in o:
                k = int(o["scalars"][1])
                r.update(counts=o["counts"], best=int(o["scalars"][0]), n_inliers=k, inliers=o["inliers"][:k].copy())
            for name in ("scores", "n_roots", "candidates"):
                if name in o:
                    r[name] = o[name]
            res.append(r)
        return res

    def ransac(self, jobs, want_referee=False):
        """Whole sample-consensus runs, all jobs in one call: the device draws the samples, solves and scores every slot and
        applies the loop's rule.  jobs: dicts with kind (SAC_*), the input arrays sac_consensus takes for the kind, and optionally
        n_slots (default 64), max_iterations (50), threshold (9), probability (0.99), seed (0).
        -> per job a dict: best (slot, or -1), n_inliers, inliers [n_inliers] int32 (ascending), model [3][4] / [3][3] (NaN when
        best = -1), iterations, skipped, stop (RANSAC_STOP_*); under want_referee also samples [n_slots][s], valid [n_slots] bool,
        counts [n_slots], models [n_slots][3][4] / [n_slots][3][3] (left as zeros where n is below the sample size)."""
        table, keep, out = ransac_job_table(jobs, want_referee)
        self._call("ransac", len(jobs), table)
        return [ransac_result(o) for o in out]

    def imu_propagate(self, params, s_t, s_gyr, s_acc, jobs, ends, fill=np.nan):
        """ImuError::propagation for the chains of calls of many sequences, in one call.  params: a list of ImuParams (or
        ImuParamsC); s_t [n] int64 ns, s_gyr / s_acc [n][3]: the pool of samples; ends [m] int64 ns: the pool of end times; jobs:
        dicts with s_begin, s_count (the job's deque in the sample pool), e_begin, e_count (its ascending end times), t_start,
        T_WS [7], sb [9], and optionally prm (index into params, default 0) and flags (IMU_COV | IMU_JAC, default 0).
        -> T_WS [m][7], sb [m][9], count [m] int32 (the steps of each call; -1: deque too short in time, 0: fewer than two
        samples), cov [m][15][15], jac [m][15][15].  Call k of a job starts at its end k - 1 from the state call k - 1 returned.
        Rows that no call wrote (ends of no job; cov / jac not asked for or of a call that returned early) hold `fill`."""
        table = imu_job_table(jobs)
        prm, s_t, s_gyr, s_acc, ends = imu_pools(params, s_t, s_gyr, s_acc, ends)
        m = len(ends)
        T, sb, count = np.full((m, 7), fill), np.full((m, 9), fill), np.full(m, -2, np.int32)
        cov, jac = np.full((m, 15, 15), fill), np.full((m, 15, 15), fill)
        self._call("imu_propagate", len(prm), prm, len(s_t), s_t.ctypes.data, s_gyr.ctypes.data, s_acc.ctypes.data, m, ends.ctypes.data,
                   len(jobs), table, T.ctypes.data, sb.ctypes.data, cov.ctypes.data, jac.ctypes.data, count.ctypes.data)
        return T, sb, count, cov, jac

    def keyframe_decision(self, jobs, want_hulls=False):
        """Frontend::doWeNeedANewKeyframe for many multiframes in one call.  jobs: dicts with images (a list of 1..8 (kp [n][3] or
        [n][2], matched [n]) pairs in camera order; matched is landmarkId != 0 after matchToKeyframes), and optionally num_frames
        (default 2), initialized (default True), overlap_threshold (0.6), ratio_threshold (0.2).
        -> per job a dict: decision (bool: a new keyframe is needed), overlap, ratio, and images: per image a dict with n_matched,
        hull_all_size, hull_matched_size, area_all, area_matched, n_inside, flags (KF_FEW_POINTS | KF_FEW_MATCHES) and, under
        want_hulls, hull_all / hull_matched (keypoint indices in hull order).  Exact: see okvis_fe_keyframe_decision."""
        kp, matched, images, table, counts = keyframe_job_table(jobs)
        out = keyframe_outputs(len(jobs), len(counts), sum(counts), want_hulls)
        self._call("keyframe_decision", len(matched), kp.ctypes.data, matched.ctypes.data, len(counts), images, len(jobs), table,
                   *[_ptr(out[k]) for k in KF_OUTPUTS])
        return keyframe_results(table, counts, out, want_hulls)

    def detect_keypoints(self, images, threshold, min_dist=40, max_keypoints=400, cand_capacity=DETECT_MAX_CANDIDATES,
                         kp_size=DETECT_KP_SIZE, want_score=False):
        """Harris corners with uniformity selection for many images in one call (okvis_fe_detect_keypoints; the statement is in
        the header and is not BRISK's).  images: a list of 2-D uint8 arrays whose columns are contiguous (rows may have any pitch
        >= width; sizes may differ); threshold, min_dist, max_keypoints, cand_capacity, kp_size: one value for all, or one per image.
        -> per image a dict: kp [n][3] float32 (x, y, size; strongest first: what every other entry takes as keypoints), response
        [n] float64 (the score S, exact), pixel [n][2] int32 (the integer maximum), n_candidates, flags (DETECT_OVERFLOW |
        DETECT_FULL) and, under want_score, score [h][w] int64 (0 outside the score domain)."""
        table, keep, out = detect_job_table(images, threshold, min_dist, max_keypoints, cand_capacity, kp_size, want_score)
        self._call("detect_keypoints", len(out), table)
        return detect_results(table, out)


    def describe_keypoints(self, images, kps, cams=None, directions=None, rot=None, want=("rot", "angle")):
        """Gravity-aligned 48-byte binary descriptors for the keypoints of many images in one call (okvis_fe_describe_keypoints; the
        angle is the reference's Frame::describe, the extractor is stated in the header and is not BRISK's).  images: as for
        detect_keypoints; kps: per image [n][3] (or [n][2]) float32; cams, directions: one CameraC and one 3-vector (the extraction
        direction in the camera frame, C_CW (0, 0, -1)) for all or per image; rot: per image [n] indices in 0..1023 instead, which
        skips the angle stage (an entry may be None where the camera is to be used).  want: the optional outputs among rot, angle,
        angle64.
        -> per image a dict: desc [n][48] uint8, flags [n] uint8 (DESCRIBE_VALID | DESCRIBE_ANGLE_UNDEFINED), n_valid and what was
        asked for (angle and angle64 only where the angle stage ran)."""
        table, keep, out = describe_job_table(images, kps, cams, directions, rot, want)
        self._call("describe_keypoints", len(out), table)
        return describe_results(table, out)

    def detect_and_describe(self, images, threshold, cams=None, directions=None, min_dist=40, max_keypoints=400,
                            cand_capacity=DETECT_MAX_CANDIDATES, kp_size=DETECT_KP_SIZE, want_score=False, rot=None, want=("rot", "angle")):
        """Frontend::detectAndDescribe in one call (okvis_fe_detect_and_describe): detect_keypoints, then describe_keypoints on what it
        selected, the images staged once.  rot: per image [max_keypoints] indices instead of cameras (a referee's input).
        -> the dicts of detect_keypoints extended by desc, flags, n_valid and what `want` names, cut to n_keypoints rows.  `flags`
        is the describe entry's array (one byte per keypoint); the detector's flags of the image are under `detect_flags`."""
        det, keep, out = detect_job_table(images, threshold, min_dist, max_keypoints, cand_capacity, kp_size, want_score)
        return self._describe_behind("detect_and_describe", det, out, detect_results, images, cams, directions, rot, want)

    def detect_keypoints_scaled(self, images, threshold, octaves, min_dist=40, max_keypoints=400, cand_capacity=DETECT_MAX_CANDIDATES,
                                kp_size=DETECT_KP_SIZE, want_score=False, want_pyramid=False, want_scale=False):
        """detect_keypoints over a scale space (okvis_fe_detect_keypoints_scaled; the statement is in the header and is not BRISK's):
        the detector on up to octaves + 1 half-sampled layers, a raw score comparison across layers, one selection over all layers.
        octaves: 0..DETECT_MAX_OCTAVES, one value for all or one per image; the rest as for detect_keypoints (min_dist in
        full-resolution pixels).
        -> per image the dict of detect_keypoints, where kp holds full-resolution positions and the size kp_size * scale, pixel the
        integer maximum in its layer, plus layer [n] int32, n_layers, n_layer_candidates [5] and, when asked for, scale [n] float64,
        score (a list of the layers' score images) and pyramid (a list of the layers 1..)."""
        table, keep, out = detect_scale_job_table(images, threshold, octaves, min_dist, max_keypoints, cand_capacity, kp_size, want_score,
                                                  want_pyramid, want_scale)
        self._call("detect_keypoints_scaled", len(out), table)
        return detect_scale_results(table, out)

    def detect_scaled_and_describe(self, images, threshold, octaves, cams=None, directions=None, min_dist=40, max_keypoints=400,
                                   cand_capacity=DETECT_MAX_CANDIDATES, kp_size=DETECT_KP_SIZE, want_score=False, want_pyramid=False,
                                   want_scale=False, rot=None, want=("rot", "angle")):
        """detect_and_describe with detect_keypoints_scaled as its detector (okvis_fe_detect_scaled_and_describe): keypoints of every
        layer are described at the fixed scale at their full-resolution position.  -> the dicts of detect_keypoints_scaled extended as
        detect_and_describe extends those of detect_keypoints."""
        det, keep, out = detect_scale_job_table(images, threshold, octaves, min_dist, max_keypoints, cand_capacity, kp_size, want_score,
                                                want_pyramid, want_scale)
        return self._describe_behind("detect_scaled_and_describe", det, out, detect_scale_results, images, cams, directions, rot, want)

    def _describe_behind(self, entry, det, out, results, images, cams, directions, rot, want):
        """the chain of both detectors: the describe table on max_keypoints rows per image, one call of `entry`, the detector's
        dicts (results(det, out)) extended by the describe entry's, cut to n_keypoints rows"""
        rows = [det[j].max_keypoints for j in range(len(out))]
        table, keep, out2 = describe_job_table(images, [np.zeros((r, 3), np.float32) for r in rows], cams, directions, rot, want)
        self._call(entry, len(out), det, table)
        res = results(det, out)
        for j in range(len(res)):
            table[j].n = det[j].n_keypoints
        for r, d in zip(res, describe_results(table, out2)):
            r["detect_flags"] = r.pop("flags")
            r.update(d)
        return res


def describe_tables():
    """the library's own tables (okvis_fe_describe_tables) -> dict of int64 arrays: cs [1024][2], base [60][2], ring [60], half [5],
    pairs [n_pairs][2]"""
    L = _lib.lib()
    declare(L)
    p = [C.c_void_p() for _ in range(5)]
    n = C.c_int32()
    _lib.check(L.okvis_fe_describe_tables(*[C.byref(x) for x in p], C.byref(n)), "describe_tables")
    arr = lambda ptr, ctype, shape: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=shape).astype(np.int64)
    return {"cs": arr(p[0], C.c_int32, (DESCRIBE_ROTATIONS, 2)), "base": arr(p[1], C.c_int32, (DESCRIBE_POINTS, 2)),
            "ring": arr(p[2], C.c_uint8, (DESCRIBE_POINTS,)), "half": arr(p[3], C.c_int32, (5,)), "pairs": arr(p[4], C.c_uint8, (n.value, 2))}


def landmark_covariance_in_camera(Sigma, T_CW):
    """A landmark's covariance rotated into a camera frame: ``R Sigma R^T``, R the rotation of T_CW (world to camera).  Sigma
    [..., 3, 3]: what ``WindowBatch.landmark_covariance()`` returns for a landmark (divided by w^2 when the stored homogeneous
    point has w != 1); T_CW [4, 4] or [3, 3], or a stack matching Sigma.  This is the matrix to add to P_C, the 3 x 3 point
    uncertainty the reference's 3D-2D matching gate propagates through the projection Jacobian
    (VioKeyframeWindowMatchingAlgorithm::doSetup).  numpy only."""
    Sigma, T = np.asarray(Sigma, np.float64), np.asarray(T_CW, np.float64)
    if Sigma.shape[-2:] != (3, 3) or T.shape[-2:] not in ((4, 4), (3, 3)):
        raise ValueError("Sigma is [..., 3, 3], T_CW [..., 4, 4] or [..., 3, 3]")
    R = T[..., :3, :3]
    return R @ Sigma @ np.swapaxes(R, -1, -2)


def propagated_covariance(P0, jac, cov):
    """Covariance of a propagated state: ``jac @ P0 @ jac.T + cov``.  jac, cov [..., 15, 15]: what ``Frontend.imu_propagate``
    returns for a call (flags IMU_COV | IMU_JAC); P0 [15, 15]: the covariance of the state the chain starts from, e.g.
    ``WindowBatch.state_covariance()`` of the (pose, speed/bias) blocks of that state.  All three are over the 15-vector of
    ImuError::propagation, which is the solver's tangent space of (pose, speed/bias): rows 0-2 position r, 3-5 orientation alpha,
    6-8 velocity v, 9-11 gyroscope bias b_g, 12-14 accelerometer bias b_a.  For call k > 0 of a job, jac is with respect to the
    state call k - 1 returned: chain the calls (P_k = propagated_covariance(P_{k-1}, jac_k, cov_k))."""
    P0, jac, cov = np.asarray(P0, np.float64), np.asarray(jac, np.float64), np.asarray(cov, np.float64)
    if P0.shape[-2:] != (15, 15) or jac.shape[-2:] != (15, 15) or cov.shape[-2:] != (15, 15):
        raise ValueError("P0, jac and cov are [..., 15, 15]")
    return jac @ P0 @ np.swapaxes(jac, -1, -2) + cov


def imu_pools(params, s_t, s_gyr, s_acc, ends):
    """the pools of okvis_fe_imu_propagate in the C layout: (ImuParamsC array, s_t, s_gyr, s_acc, ends)"""
    prm = (ImuParamsC * max(1, len(params)))(*[p if isinstance(p, ImuParamsC) else p.as_c() for p in params])
    s_t, ends = np.ascontiguousarray(s_t, np.int64).reshape(-1), np.ascontiguousarray(ends, np.int64).reshape(-1)
    s_gyr, s_acc = _f64(s_gyr).reshape(-1, 3), _f64(s_acc).reshape(-1, 3)
    if not len(s_t) == len(s_gyr) == len(s_acc):
        raise ValueError("arrays of different lengths")
    return prm, s_t, s_gyr, s_acc, ends


KF_OUTPUTS = ("decision", "overlap", "ratio", "n_matched", "hull_all_size", "hull_matched_size", "area_all", "area_matched", "n_inside",
              "flags", "hull_all", "hull_matched")   # in the entry's argument order


def keyframe_job_table(jobs):
    """-> (kp pool [N][3] float32, matched pool [N] uint8, okvis_fe_kf_image array, okvis_fe_kf_job array, the images' keypoint
    counts): every image of every job goes into the pools once, in job and camera order"""
    kps, ms, counts = [], [], []
    table = (KfJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        t = table[j]
        t.im_begin, t.n_cams = len(counts), len(job["images"])
        t.num_frames, t.initialized = int(job.get("num_frames", 2)), int(bool(job.get("initialized", True)))
        t.overlap_threshold, t.ratio_threshold = float(job.get("overlap_threshold", 0.6)), float(job.get("ratio_threshold", 0.2))
        for kp, m in job["images"]:
            kp = np.asarray(kp, np.float32)
            kp = kp.reshape(-1, kp.shape[-1] if kp.ndim == 2 else 3)
            if kp.shape[1] == 2:
                kp = np.concatenate([kp, np.zeros((len(kp), 1), np.float32)], axis=1)
            m = (np.asarray(m).reshape(-1) != 0).astype(np.uint8)
            if kp.shape[1] != 3 or len(m) != len(kp):
                raise ValueError("an image is (kp [n][3] or [n][2], matched [n])")
            kps.append(kp), ms.append(m), counts.append(len(kp))
    kp = np.ascontiguousarray(np.concatenate(kps) if kps else np.zeros((0, 3)), np.float32).reshape(-1, 3)
    matched = np.ascontiguousarray(np.concatenate(ms) if ms else np.zeros(0), np.uint8)
    images = (KfImageC * max(1, len(counts)))()
    at = 0
    for i, n in enumerate(counts):
        images[i].kp_begin, images[i].kp_count = at, n
        at += n
    return kp, matched, images, table, counts


def keyframe_outputs(n_jobs, n_images, n_hull, want_hulls=False):
    """the output arrays of okvis_fe_keyframe_decision by name (KF_OUTPUTS); the hull lists are None unless asked for"""
    i32 = lambda n: np.zeros(n, np.int32)
    return {"decision": np.zeros(n_jobs, np.uint8), "overlap": np.zeros(n_jobs), "ratio": np.zeros(n_jobs), "n_matched": i32(n_images),
            "hull_all_size": i32(n_images), "hull_matched_size": i32(n_images), "area_all": np.zeros(n_images),
            "area_matched": np.zeros(n_images), "n_inside": i32(n_images), "flags": np.zeros(n_images, np.uint8),
            "hull_all": i32(n_hull) if want_hulls else None, "hull_matched": i32(n_hull) if want_hulls else None}


def keyframe_results(table, counts, out, want_hulls=False):
    """the filled arrays of keyframe_outputs as one dict per job"""
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    res = []
    for j in range(len(out["decision"])):
        ims = []
        for i in range(table[j].im_begin, table[j].im_begin + table[j].n_cams):
            r = {k: out[k][i].item() for k in ("n_matched", "hull_all_size", "hull_matched_size", "area_all", "area_matched", "n_inside", "flags")}
            if want_hulls:
                r["hull_all"] = out["hull_all"][starts[i]:starts[i] + r["hull_all_size"]].copy()
                r["hull_matched"] = out["hull_matched"][starts[i]:starts[i] + r["hull_matched_size"]].copy()
            ims.append(r)
        res.append({"decision": bool(out["decision"][j]), "overlap": float(out["overlap"][j]), "ratio": float(out["ratio"][j]), "images": ims})
    return res


DETECT_OUTPUTS = ("kp", "response", "pixel", "score")


def detect_job_table(images, threshold, min_dist=40, max_keypoints=400, cand_capacity=DETECT_MAX_CANDIDATES, kp_size=DETECT_KP_SIZE,
                     want_score=False, leave_out=()):
    """-> (okvis_fe_detect_job array, what has to outlive the call, the output arrays per job by name (DETECT_OUTPUTS; None where
    not asked for or named in leave_out)).  An image is passed as it lies in memory: no copy is made of a view with a pitch."""
    table, keep, out = _detect_jobs(DetectJobC, images, threshold, min_dist, max_keypoints, cand_capacity, kp_size)
    for t, im, o in zip(table, images, out):
        o["score"] = np.zeros(im.shape, np.int64) if want_score else None
        for k in leave_out:
            o[k] = None
        t.kp, t.response, t.pixel, t.score = (_ptr(o[k]) for k in DETECT_OUTPUTS)
    return table, keep, out


def _detect_jobs(ctype, images, threshold, min_dist, max_keypoints, cand_capacity, kp_size):
    """what both detect job tables begin with: the images checked, the fields the two structs share (one value for all, or one per
    image) and the per-keypoint arrays kp, response, pixel on max_keypoints rows -> (table, keep, out)"""
    n = len(images)
    per = lambda v: list(v) if np.ndim(v) else [v] * n
    thr, md, mk, cc, ks = per(threshold), per(min_dist), per(max_keypoints), per(cand_capacity), per(kp_size)
    table, out = (ctype * max(1, n))(), []
    for j, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1) or im.strides[0] < im.shape[1]:
            raise ValueError("an image is a 2-D uint8 array with contiguous columns and a pitch of at least its width")
        t = table[j]
        t.image, t.height, t.width, t.pitch = im.ctypes.data, im.shape[0], im.shape[1], im.strides[0]
        t.threshold, t.min_dist, t.max_keypoints, t.cand_capacity, t.kp_size = int(thr[j]), int(md[j]), int(mk[j]), int(cc[j]), float(ks[j])
        rows = max(0, int(mk[j]))
        out.append({"kp": np.zeros((rows, 3), np.float32), "response": np.zeros(rows), "pixel": np.zeros((rows, 2), np.int32)})
    return table, list(images), out


def detect_results(table, out):
    """the filled arrays of detect_job_table as one dict per image, cut to n_keypoints rows"""
    res = []
    for j, o in enumerate(out):
        n = table[j].n_keypoints
        r = {k: o[k][:n].copy() for k in ("kp", "response", "pixel") if o[k] is not None}
        if o["score"] is not None:
            r["score"] = o["score"]
        r.update(n_candidates=int(table[j].n_candidates), flags=int(table[j].flags))
        res.append(r)
    return res


DETECT_SCALE_OUTPUTS = ("kp", "response", "pixel", "layer", "scale", "score", "pyramid")


def detect_layers(width, height, octaves):
    """-> [(w_l, h_l)] of the layers that exist (the header's pyramid rule)"""
    out = [(int(width), int(height))]
    while len(out) <= min(int(octaves), DETECT_MAX_OCTAVES) and (out[-1][0] >> 1) >= 5 and (out[-1][1] >> 1) >= 5:
        out.append((out[-1][0] >> 1, out[-1][1] >> 1))
    return out


def detect_scale_job_table(images, threshold, octaves, min_dist=40, max_keypoints=400, cand_capacity=DETECT_MAX_CANDIDATES,
                           kp_size=DETECT_KP_SIZE, want_score=False, want_pyramid=False, want_scale=False, leave_out=()):
    """-> (okvis_fe_detect_scale_job array, what has to outlive the call, the output arrays per job by name (DETECT_SCALE_OUTPUTS; None
    where not asked for or named in leave_out)).  score and pyramid are flat: the layers one behind the other."""
    table, keep, out = _detect_jobs(DetectScaleJobC, images, threshold, min_dist, max_keypoints, cand_capacity, kp_size)
    octs = list(octaves) if np.ndim(octaves) else [octaves] * len(images)
    for j, (t, im, o) in enumerate(zip(table, images, out)):
        t.octaves = int(octs[j])
        rows = len(o["kp"])
        layers = detect_layers(im.shape[1], im.shape[0], max(0, t.octaves))
        o.update(layer=np.zeros(rows, np.int32), scale=np.zeros(rows) if want_scale else None,
                 score=np.zeros(sum(w * h for w, h in layers), np.int64) if want_score else None,
                 pyramid=np.zeros(max(1, sum(w * h for w, h in layers[1:])), np.uint8) if want_pyramid else None)
        for k in leave_out:
            o[k] = None
        t.kp, t.response, t.pixel, t.layer, t.scale, t.score, t.pyramid = (_ptr(o[k]) for k in DETECT_SCALE_OUTPUTS)
    return table, keep, out


def detect_scale_results(table, out):
    """the filled arrays of detect_scale_job_table as one dict per image, cut to n_keypoints rows; score and pyramid as lists of
    2-D arrays, one per layer (pyramid: the layers 1..)"""
    res = []
    for j, o in enumerate(out):
        t = table[j]
        n = t.n_keypoints
        r = {k: o[k][:n].copy() for k in ("kp", "response", "pixel", "layer", "scale") if o[k] is not None}
        layers = detect_layers(t.width, t.height, t.octaves)
        assert len(layers) == t.n_layers
        for name, which in (("score", layers), ("pyramid", layers[1:])):
            if o[name] is not None:
                at, r[name] = 0, []
                for w, h in which:
                    r[name].append(o[name][at:at + w * h].reshape(h, w))
                    at += w * h
        r.update(n_candidates=int(t.n_candidates), flags=int(t.flags), n_layers=int(t.n_layers),
                 n_layer_candidates=np.array(list(t.n_layer_candidates), np.int32))
        res.append(r)
    return res


DESCRIBE_OUTPUTS = ("desc", "flags", "rot", "angle", "angle64")


def describe_job_table(images, kps, cams=None, directions=None, rot=None, want=("rot", "angle"), leave_out=()):
    """-> (okvis_fe_describe_job array, what has to outlive the call, the output arrays per job by name (DESCRIBE_OUTPUTS; None
    where not asked for or named in leave_out)).  An image is passed as it lies in memory."""
    n = len(images)
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
    cams, rots = per(cams), per(rot)
    dirs = [None] * n if directions is None else (list(np.asarray(directions, np.float64)) if np.ndim(directions) == 2 else [directions] * n)
    table, keep, out = (DescribeJobC * max(1, n))(), [], []
    for j, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1) or im.strides[0] < im.shape[1]:
            raise ValueError("an image is a 2-D uint8 array with contiguous columns and a pitch of at least its width")
        kp = np.asarray(kps[j], np.float32)
        kp = kp.reshape(-1, kp.shape[-1] if kp.ndim == 2 else 3)
        if kp.shape[1] == 2:
            kp = np.concatenate([kp, np.zeros((len(kp), 1), np.float32)], axis=1)
        if kp.shape[1] != 3:
            raise ValueError("keypoints are [n][3] or [n][2]")
        kp = np.ascontiguousarray(kp, np.float32)
        rows = len(kp)
        t = table[j]
        t.image, t.height, t.width, t.pitch, t.n = im.ctypes.data, im.shape[0], im.shape[1], im.strides[0], rows
        kp_mem = kp if rows else np.zeros((1, 3), np.float32)          # a pointer even for no keypoints
        t.kp = kp_mem.ctypes.data
        r_in = None
        if rots[j] is not None:
            r_in = np.ascontiguousarray(rots[j], np.int32).reshape(-1)
            if len(r_in) != rows:
                raise ValueError("rot has one entry per keypoint")
            r_in = r_in if rows else np.zeros(1, np.int32)
            t.rot_in = r_in.ctypes.data
        if cams[j] is not None:
            t.cam = C.pointer(cams[j])
            t.direction[:] = [float(v) for v in np.asarray(dirs[j], np.float64).reshape(3)]
        elif r_in is None:
            raise ValueError("a job needs a camera and a direction, or rot")
        room = max(1, rows)
        o = {"desc": np.zeros((room, DESCRIBE_BYTES), np.uint8), "flags": np.zeros(room, np.uint8),
             "rot": np.zeros(room, np.int32) if "rot" in want else None, "angle": np.zeros(room, np.float32) if "angle" in want else None,
             "angle64": np.zeros(room, np.float64) if "angle64" in want else None}
        for k in leave_out:
            o[k] = None
        t.desc, t.flags, t.rot, t.angle, t.angle64 = (_ptr(o[k]) for k in DESCRIBE_OUTPUTS)
        keep += [im, kp_mem, r_in, cams[j]]
        out.append(o)
    return table, keep, out


def describe_results(table, out):
    """the filled arrays of describe_job_table as one dict per image, cut to n rows; angle and angle64 only where the stage ran"""
    res = []
    for j, o in enumerate(out):
        n = table[j].n
        skip = ("angle", "angle64") if table[j].rot_in else ()
        r = {k: o[k][:n].copy() for k in DESCRIBE_OUTPUTS if o[k] is not None and k not in skip}
        r["n_valid"] = int(table[j].n_valid)
        res.append(r)
    return res


def imu_job_table(jobs):
    """-> the okvis_fe_imu_job array (a job holds no pointers: nothing else has to outlive the call)"""
    table = (ImuJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        t = table[j]
        t.s_begin, t.s_count, t.e_begin, t.e_count = int(job["s_begin"]), int(job["s_count"]), int(job["e_begin"]), int(job["e_count"])
        t.prm, t.flags, t.t_start = int(job.get("prm", 0)), int(job.get("flags", 0)), int(job["t_start"])
        t.T_WS[:] = list(_f64(job["T_WS"], 7))
        t.sb[:] = list(_f64(job["sb"], 9))
    return table


def sac_job_table(jobs, want_scores=False):
    """-> (okvis_fe_sac_job array, the input arrays it points into, per job the output arrays (counts, [best, n_inliers], inliers,
    scores)); both lists have to outlive the call"""
    keep, out = [], []
    table = (SacJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        kind = int(job["kind"])
        if kind not in (SAC_ABSOLUTE, SAC_ROTATION_ONLY, SAC_RELATIVE):
            raise ValueError("kind is one of SAC_ABSOLUTE, SAC_ROTATION_ONLY, SAC_RELATIVE")
        models = _f64(job["models"]).reshape(-1, 9 if kind == SAC_ROTATION_ONLY else 12)
        t = table[j]
        t.kind, t.n_models, t.threshold, t.models = kind, len(models), float(job.get("threshold", 9.0)), models.ctypes.data
        if kind == SAC_ABSOLUTE:
            a, b = _f64(job["points"]).reshape(-1, 3), _f64(job["bearing"]).reshape(-1, 3)
            s1, ci = _f64(job["sigma"]).reshape(-1), np.ascontiguousarray(job["cam_index"], np.int32).reshape(-1)
            off, rot = _f64(job["cam_offsets"]).reshape(-1, 3), _f64(job["cam_rotations"]).reshape(-1, 9)
            if not (len(a) == len(b) == len(s1) == len(ci)) or len(off) != len(rot):
                raise ValueError("arrays of different lengths")
            t.n, t.n_cams = len(a), len(off)
            t.points, t.bearing, t.sigma, t.cam_index = a.ctypes.data, b.ctypes.data, s1.ctypes.data, ci.ctypes.data
            t.cam_offsets, t.cam_rotations = off.ctypes.data, rot.ctypes.data
            keep.append((models, a, b, s1, ci, off, rot))
        else:
            a, b = _f64(job["bearing1"]).reshape(-1, 3), _f64(job["bearing2"]).reshape(-1, 3)
            s1, s2 = _f64(job["sigma1"]).reshape(-1), _f64(job["sigma2"]).reshape(-1)
            if not (len(a) == len(b) == len(s1) == len(s2)):
                raise ValueError("arrays of different lengths")
            t.n = len(a)
            t.bearing1, t.bearing2, t.sigma1, t.sigma2 = a.ctypes.data, b.ctypes.data, s1.ctypes.data, s2.ctypes.data
            keep.append((models, a, b, s1, s2))
        n, K = t.n, len(models)
        counts, scalars, inl = np.zeros(K, np.int32), np.zeros(2, np.int32), np.zeros(max(n, 1), np.int32)
        sc = np.zeros((K, n)) if want_scores else None
        t.counts, t.best, t.n_inliers, t.inliers = counts.ctypes.data, scalars.ctypes.data, scalars.ctypes.data + 4, inl.ctypes.data
        t.scores = _ptr(sc)
        out.append((counts, scalars, inl, sc))
    return table, keep, out


RANSAC_SCALARS = ("best", "n_inliers", "iterations", "skipped", "stop")


def ransac_job_table(jobs, want_referee=False):
    """-> (okvis_fe_ransac_job array, the input arrays it points into, per job the dict of output arrays); both lists have to
    outlive the call"""
    keep, out = [], []
    table = (RansacJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        kind = int(job["kind"])
        if kind not in (SAC_ABSOLUTE, SAC_ROTATION_ONLY, SAC_RELATIVE):
            raise ValueError("kind is one of SAC_ABSOLUTE, SAC_ROTATION_ONLY, SAC_RELATIVE")
        t = table[j]
        t.kind, t.n_slots, t.max_iterations = kind, int(job.get("n_slots", 64)), int(job.get("max_iterations", 50))
        t.threshold, t.probability, t.seed = float(job.get("threshold", 9.0)), float(job.get("probability", 0.99)), int(job.get("seed", 0))
        if kind == SAC_ABSOLUTE:
            a, b = _f64(job["points"]).reshape(-1, 3), _f64(job["bearing"]).reshape(-1, 3)
            s1, ci = _f64(job["sigma"]).reshape(-1), np.ascontiguousarray(job["cam_index"], np.int32).reshape(-1)
            off, rot = _f64(job["cam_offsets"]).reshape(-1, 3), _f64(job["cam_rotations"]).reshape(-1, 9)
            if not (len(a) == len(b) == len(s1) == len(ci)) or len(off) != len(rot):
                raise ValueError("arrays of different lengths")
            t.n, t.n_cams = len(a), len(off)
            t.points, t.bearing, t.sigma, t.cam_index = a.ctypes.data, b.ctypes.data, s1.ctypes.data, ci.ctypes.data
            t.cam_offsets, t.cam_rotations = off.ctypes.data, rot.ctypes.data
            keep.append((a, b, s1, ci, off, rot))
        else:
            a, b = _f64(job["bearing1"]).reshape(-1, 3), _f64(job["bearing2"]).reshape(-1, 3)
            s1, s2 = _f64(job["sigma1"]).reshape(-1), _f64(job["sigma2"]).reshape(-1)
            if not (len(a) == len(b) == len(s1) == len(s2)):
                raise ValueError("arrays of different lengths")
            t.n = len(a)
            t.bearing1, t.bearing2, t.sigma1, t.sigma2 = a.ctypes.data, b.ctypes.data, s1.ctypes.data, s2.ctypes.data
            keep.append((a, b, s1, s2))
        n, K, cols = t.n, t.n_slots, 3 if kind == SAC_ROTATION_ONLY else 4
        o = {"scalars": np.zeros(len(RANSAC_SCALARS), np.int32), "inliers": np.zeros(max(n, 1), np.int32), "model": np.zeros((3, cols))}
        for i, name in enumerate(RANSAC_SCALARS):
            setattr(t, name, o["scalars"].ctypes.data + 4 * i)
        t.inliers, t.model = o["inliers"].ctypes.data, o["model"].ctypes.data
        if want_referee:
            o.update(samples=np.zeros((max(K, 0), SAC_SAMPLE_SIZE[kind]), np.int32), valid=np.zeros(max(K, 0), np.uint8),
                     counts=np.zeros(max(K, 0), np.int32), models=np.zeros((max(K, 0), 3, cols)))
            for name in ("samples", "valid", "counts", "models"):
                setattr(t, name, o[name].ctypes.data)
        out.append(o)
    return table, keep, out


def ransac_result(o):
    """the filled arrays of one job of ransac_job_table as the dict Frontend.ransac returns"""
    r = {name: int(o["scalars"][i]) for i, name in enumerate(RANSAC_SCALARS)}
    r.update(inliers=o["inliers"][:r["n_inliers"]].copy(), model=o["model"])
    for name in ("samples", "counts", "models"):
        if name in o:
            r[name] = o[name]
    if "valid" in o:
        r["valid"] = o["valid"].astype(bool)
    return r


def ransac_2d2d_outcome(n, rotation_only_inliers, rel_pose_inliers):
    """What Frontend::runRansac2d2d makes of its two runs (okvis_frontend/src/Frontend.cpp:688-733), with its `float` ratios.
    n: the number of correspondences (n >= 1); the two arguments: the inlier counts of the rotation-only and of the relative-pose
    run.  -> dict: rotation_only_ratio, rel_pose_ratio (float32), rotation_only (the rotation-only ratio is larger than the
    relative-pose ratio or above 0.8), rotation_only_success, rel_pose_success (more than 10 inliers, and the respective choice),
    inliers_from ("rotation_only", "rel_pose" or None: whose inlier set decides which observations are removed)."""
    n, k_rot, k_rel = int(n), int(rotation_only_inliers), int(rel_pose_inliers)
    r_rot, r_rel = np.float32(k_rot) / np.float32(n), np.float32(k_rel) / np.float32(n)
    rotation_only = bool(r_rot > r_rel or float(r_rot) > 0.8)     # :711 compares the float with the double literal: 4 / 5 passes
    rot_success = bool(rotation_only and k_rot > 10)
    rel_success = bool(not rotation_only and k_rel > 10)
    return {"rotation_only_ratio": r_rot, "rel_pose_ratio": r_rel, "rotation_only": rotation_only, "rotation_only_success": rot_success,
            "rel_pose_success": rel_success, "inliers_from": "rotation_only" if rot_success else "rel_pose" if rel_success else None}


def sac_solve_job_table(jobs, want_scores=False, want_essentials=False):
    """-> (okvis_fe_sac_solve_job array, the input arrays it points into, per job the dict of output arrays); both lists have to
    outlive the call"""
    keep, out = [], []
    table = (SacSolveJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        kind = int(job["kind"])
        if kind not in (SAC_ROTATION_ONLY, SAC_RELATIVE):
            raise ValueError("kind is SAC_ROTATION_ONLY or SAC_RELATIVE")
        relative = kind == SAC_RELATIVE
        a, b = _f64(job["bearing1"]).reshape(-1, 3), _f64(job["bearing2"]).reshape(-1, 3)
        q = np.ascontiguousarray(job["samples"], np.int32).reshape(-1, SAC_SAMPLE_RELATIVE if relative else SAC_SAMPLE_ROTATION_ONLY)
        s1 = None if job.get("sigma1") is None else _f64(job["sigma1"]).reshape(-1)
        s2 = None if job.get("sigma2") is None else _f64(job["sigma2"]).reshape(-1)
        if len(a) != len(b) or any(s is not None and len(s) != len(a) for s in (s1, s2)):
            raise ValueError("arrays of different lengths")
        n, K = len(a), len(q)
        t = table[j]
        t.kind, t.n, t.n_models, t.threshold = kind, n, K, float(job.get("threshold", 9.0))
        t.bearing1, t.bearing2, t.sigma1, t.sigma2, t.samples = a.ctypes.data, b.ctypes.data, _ptr(s1), _ptr(s2), q.ctypes.data
        keep.append((a, b, s1, s2, q))
        o = {"models": np.zeros((K, 3, 4 if relative else 3)), "valid": np.zeros(K, np.uint8)}
        t.models, t.valid = o["models"].ctypes.data, o["valid"].ctypes.data
        if relative and want_essentials:
            o["n_roots"], o["essentials"] = np.zeros(K, np.int32), np.zeros((K, SAC_MAX_ROOTS, 9))
            t.n_roots, t.essentials = o["n_roots"].ctypes.data, o["essentials"].ctypes.data
        if job.get("consensus", True):
            o["counts"], o["scalars"], o["inliers"] = np.zeros(K, np.int32), np.zeros(2, np.int32), np.zeros(max(n, 1), np.int32)
            t.counts, t.best, t.n_inliers = o["counts"].ctypes.data, o["scalars"].ctypes.data, o["scalars"].ctypes.data + 4
            t.inliers = o["inliers"].ctypes.data
            if want_scores:
                o["scores"] = np.zeros((K, n))
                t.scores = o["scores"].ctypes.data
        out.append(o)
    return table, keep, out


def sac_absolute_job_table(jobs, want_scores=False, want_candidates=False):
    """-> (okvis_fe_sac_absolute_job array, the input arrays it points into, per job the dict of output arrays); both lists have to
    outlive the call"""
    keep, out = [], []
    table = (SacAbsoluteJobC * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        a, b = _f64(job["points"]).reshape(-1, 3), _f64(job["bearing"]).reshape(-1, 3)
        ci = np.ascontiguousarray(job["cam_index"], np.int32).reshape(-1)
        off, rot = _f64(job["cam_offsets"]).reshape(-1, 3), _f64(job["cam_rotations"]).reshape(-1, 9)
        q = np.ascontiguousarray(job["samples"], np.int32).reshape(-1, SAC_SAMPLE_ABSOLUTE)
        s = None if job.get("sigma") is None else _f64(job["sigma"]).reshape(-1)
        if not (len(a) == len(b) == len(ci)) or len(off) != len(rot) or (s is not None and len(s) != len(a)):
            raise ValueError("arrays of different lengths")
        n, K = len(a), len(q)
        t = table[j]
        t.n, t.n_models, t.n_cams, t.threshold = n, K, len(off), float(job.get("threshold", 9.0))
        t.points, t.bearing, t.sigma, t.cam_index = a.ctypes.data, b.ctypes.data, _ptr(s), ci.ctypes.data
        t.cam_offsets, t.cam_rotations, t.samples = off.ctypes.data, rot.ctypes.data, q.ctypes.data
        keep.append((a, b, s, ci, off, rot, q))
        o = {"models": np.zeros((K, 3, 4)), "valid": np.zeros(K, np.uint8)}
        t.models, t.valid = o["models"].ctypes.data, o["valid"].ctypes.data
        if want_candidates:
            o["n_roots"], o["candidates"] = np.zeros(K, np.int32), np.zeros((K, SAC_MAX_ROOTS_ABSOLUTE, 3, 4))
            t.n_roots, t.candidates = o["n_roots"].ctypes.data, o["candidates"].ctypes.data
        if job.get("consensus", True):
            o["counts"], o["scalars"], o["inliers"] = np.zeros(K, np.int32), np.zeros(2, np.int32), np.zeros(max(n, 1), np.int32)
            t.counts, t.best, t.n_inliers = o["counts"].ctypes.data, o["scalars"].ctypes.data, o["scalars"].ctypes.data + 4
            t.inliers = o["inliers"].ctypes.data
            if want_scores:
                o["scores"] = np.zeros((K, n))
                t.scores = o["scores"].ctypes.data
        out.append(o)
    return table, keep, out


def vmatch_job_table(jobs):
    """-> (okvis_fe_vmatch_job array, the input arrays it points into, per job the dict of output arrays); both lists have to
    outlive the call"""
    keep, out = [], []
    table = (VMatchJobC * max(1, len(jobs)))()
    width = None
    for j, job in enumerate(jobs):
        kind = int(job["kind"])
        if kind not in (MATCH_3D2D, MATCH_2D2D):
            raise ValueError("kind is MATCH_3D2D or MATCH_2D2D")
        da, db = _desc(job["desc_a"]), _desc(job["desc_b"])
        if da.shape[1] != db.shape[1] or width not in (None, da.shape[1]):
            raise ValueError("descriptors of different lengths")
        width = da.shape[1]
        na, nb = len(da), len(db)
        sa, sb = _skip(job.get("skip_a"), na), _skip(job.get("skip_b"), nb)

        def rows(a, n, cols, dtype):   # [n][cols], never a NULL pointer
            a = np.ascontiguousarray(a, dtype).reshape(-1, cols)
            if len(a) != n:
                raise ValueError("arrays of different lengths")
            return a if n else np.zeros((1, cols), dtype)

        kb = rows(job["kp_b"], nb, 3, np.float32)
        ka = rows(job["kp_a"], na, 3, np.float32) if job.get("kp_a") is not None else None
        t = table[j]
        t.kind, t.n_a, t.n_b = kind, na, nb
        t.desc_a, t.desc_b, t.skip_a, t.skip_b = da.ctypes.data, db.ctypes.data, _ptr(sa), _ptr(sb)
        t.kp_a, t.kp_b = _ptr(ka), kb.ctypes.data
        t.cam_b = job["cam_b"]
        t.cam_a = job.get("cam_a", job["cam_b"])
        r = {"pair_a": np.zeros(nb, np.int32), "pair_dist": np.zeros(nb, np.float32), "accepted": np.zeros(nb, np.uint8)}
        hp = None
        if kind == MATCH_3D2D:
            hp = rows(job["hp_W"], na, 4, np.float64)
            t.hp_W = hp.ctypes.data
            t.T_CbW[:] = list(_f64(job["T_CbW"], 7))
            t.P3[:] = list(_f64(job["P3"], 9))
            r.update(proj_status=np.zeros(na, np.uint8), uv=np.zeros((na, 2)), U=np.zeros((na, 2, 2)), chi2=np.zeros(nb),
                     gate_flags=np.zeros(nb, np.uint8))
        else:
            if ka is None:
                raise ValueError("MATCH_2D2D needs kp_a")
            t.T_AB[:] = list(_f64(job["T_AB"], 7))
            t.UOplus[:] = list(_f64(job["UOplus"], 36))
            r.update(hp_a=np.zeros((nb, 4)), cov=np.zeros((nb, 3, 3)), tri_flags=np.zeros(nb, np.uint8))
        for name, arr in r.items():
            setattr(t, name, arr.ctypes.data)
        keep.append((da, db, sa, sb, ka, kb, hp))
        out.append(r)
    return table, keep, out
