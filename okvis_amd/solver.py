"""Host-side handle of a batch of windows on one MI355X (thin wrapper over the C-ABI).

Mirrors how ``okvis::Estimator`` drives its backend: upload the window structure (what
``addStates/addLandmark/addObservation`` build in the reference, okvis_ceres/src/Estimator.cpp:110-365,
implementation/Estimator.hpp:43-90), ``optimize(numIter)`` (Estimator.cpp:843-906), read the states back
(``get_T_WS/getSpeedAndBias/getLandmark``, Estimator.cpp:933-1200).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from .window import LimitsC, OptionsC, SummaryC, Window, WindowC, default_options

# okvis_ba_download's arrays (include/okvis_amd_ba.h, enum okvis_ba_array).  IMU_LIN: [n_imu][511], per IMU factor of the accepted
# buffer H = J^T J as the packed lower triangle (index a (a + 1) / 2 + b) over the factor's own columns pose0(6) | sb0(9) |
# pose1(6) | sb1(9) (465), g = J^T r (30), the weighted residual r (15), the cost (1) — reshape(-1, 511).
ARR = dict(POSE=0, SB=1, LM=2, OBS_RESIDUAL=3, LM_V=4, LM_B=5, LM_HQ=6, PAIR_W=7, REDUCED_S=8,
           REDUCED_RHS=9, STEP=10, LM_QUALITY=11, GRADIENT=12, IMU_RESIDUAL=13, HPP=14, DAMPING=15, IMU_SB_REF=16, IMU_LIN=17, PROF=99, IMU_REDO_COUNT=98, CTRL=97, SLOTS=96, GROUP_RECS=95)
_dp = C.POINTER(C.c_double)


def limits() -> dict:
    lim = LimitsC()
    _lib.lib().okvis_ba_get_limits(C.byref(lim))
    return {n: getattr(lim, n) for n, _ in lim._fields_}


def check_window(window: Window, options: OptionsC | None = None) -> dict:
    """Host-only structure check (no GPU needed): the index building okvis_ba_upload performs."""
    window.validate()
    wc, keep = window.as_c()
    st = (C.c_int64 * 8)()
    _lib.check(_lib.lib().okvis_ba_check_window(C.byref(wc), C.byref(options) if options is not None else None, st),
               "check_window")
    del keep
    return dict(D=st[0], Dp=st[1], n_pair=st[2], n_group=st[3], n_chunk=st[4], n_task=st[5], gpart=st[6],
                arena_bytes=st[7])


INDEX_LISTS = ("groups", "lm_obs_begin", "lm_pair_begin", "pair_lm", "pair_block", "pair_off", "pair_role", "lm_piece_begin",
               "pair_piece", "pair_list_begin", "pair_list", "tasks", "task_list", "chunks", "chunk_diag_begin", "chunk_diag_out",
               "chunk_desc", "piece_path", "ldl_comp", "chain", "chunk_recs", "group_recs", "plan")   # OKVIS_BA_LIST_* in this order


def index_lists(window: Window, options: OptionsC | None = None, n_windows: int = 1) -> dict:
    """The index lists okvis_ba_upload would build for `window` as one of `n_windows` (host only; okvis_ba_check_window_lists)."""
    wc, keep = window.as_c()
    L = _lib.lib()
    po = C.byref(options) if options is not None else None
    out = {}
    for which, name in enumerate(INDEX_LISTS):
        n = C.c_int64()
        rc = L.okvis_ba_check_window_lists(C.byref(wc), po, n_windows, which, None, 0, C.byref(n))
        if rc != 0 and not (rc == -1 and n.value > 0):
            _lib.check(rc, "check_window_lists")
        a = np.zeros(max(n.value, 1), np.int32)
        if n.value:
            _lib.check(L.okvis_ba_check_window_lists(C.byref(wc), po, n_windows, which, a.ctypes.data_as(C.POINTER(C.c_int32)), n.value,
                                                     C.byref(n)), "check_window_lists")
        out[name] = a[:n.value]
    del keep
    out["groups"] = out["groups"].reshape(-1, 16)
    out["tasks"] = out["tasks"].reshape(-1, 6)
    out["chunks"] = out["chunks"].reshape(-1, 2)
    out["chunk_recs"] = out["chunk_recs"].reshape(-1, 128)
    out["group_recs"] = out["group_recs"].reshape(-1, 32)
    out["piece_path"] = int(out["piece_path"][0])
    out["ldl_comp"] = int(out["ldl_comp"][0]) & 0xFFFFFFFF
    out["chain"] = int(out["chain"][0])
    return out


class WindowStore:
    """Host-side window container with O(edit) structure updates (okvis_ba_store_*; no GPU needed)."""

    def __init__(self, window: Window):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        wc, keep = window.as_c()
        _lib.check(self._L.okvis_ba_store_create(C.byref(wc), C.byref(self._h)), "store_create")
        del keep

    def patch(self, patch) -> int:
        """Apply a :class:`okvis_amd.window.Patch`; returns the status (0 = applied, otherwise the window is untouched)."""
        pc, keep = patch.as_c()
        rc = self._L.okvis_ba_store_patch(self._h, C.byref(pc))
        del keep
        return rc

    def view(self) -> Window:
        from .window import window_from_c
        wc = WindowC()
        _lib.check(self._L.okvis_ba_store_view(self._h, C.byref(wc)), "store_view")
        return window_from_c(wc)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.okvis_ba_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowBatch:
    """A batch of independent sliding windows resident in the HBM of one GPU."""

    def __init__(self, windows: Sequence[Window], device: int = 0, options: OptionsC | None = None, patchable: bool = False):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        _lib.check(self._L.okvis_ba_create(C.byref(self._h), int(device)), "create")
        self.options = options or default_options()
        _lib.check(self._L.okvis_ba_set_options(self._h, C.byref(self.options)), "set_options")
        if patchable:   # the solver keeps a container of every uploaded window (okvis_ba_patch_window)
            _lib.check(self._L.okvis_ba_set_patchable(self._h, 1), "set_patchable")
        self.upload(windows)

    def patch(self, w: int, patch):
        """okvis_ba_patch_window: edit window w on the solver (blocks that stay keep the device's values)."""
        pc, keep = patch.as_c()
        _lib.check(self._L.okvis_ba_patch_window(self._h, int(w), C.byref(pc)), "patch_window")
        del keep
        self.windows[w] = self.patched_view(w)

    def patched_view(self, w: int) -> Window:
        """The solver's container of window w as a :class:`Window` (current device values)."""
        from .window import window_from_c
        wc = WindowC()
        _lib.check(self._L.okvis_ba_patched_view(self._h, int(w), C.byref(wc)), "patched_view")
        return window_from_c(wc)

    def upload(self, windows: Sequence[Window]):
        """okvis_ba_upload on this solver: replaces the windows.  Device allocations are kept (grow-only) and so are the captured
        launch graphs when the new windows have the shapes of the old ones."""
        self.windows = list(windows)
        arr = (WindowC * len(self.windows))()
        keep = []
        for i, w in enumerate(self.windows):
            w.validate()
            wc, k = w.as_c()
            arr[i] = wc
            keep.append(k)
        _lib.check(self._L.okvis_ba_upload(self._h, len(self.windows), arr), "upload")
        del keep

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.okvis_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.windows)

    # ---- options ----
    def set_options(self, options: OptionsC):
        _lib.check(self._L.okvis_ba_set_options(self._h, C.byref(options)), "set_options")
        self.options = options

    # ---- hot path ----
    def optimize(self, num_iter: int):
        s = (SummaryC * len(self))()
        _lib.check(self._L.okvis_ba_optimize(self._h, int(num_iter), s), "optimize")
        return [x.as_dict() for x in s]

    def optimize_timed(self, max_iter: int, min_iter: int, time_limit_s: float):
        s = (SummaryC * len(self))()
        _lib.check(self._L.okvis_ba_optimize_timed(self._h, int(max_iter), int(min_iter), float(time_limit_s), s),
                   "optimize_timed")
        return [x.as_dict() for x in s]

    def begin(self):
        _lib.check(self._L.okvis_ba_begin(self._h), "begin")

    def iterate(self, n: int):
        _lib.check(self._L.okvis_ba_iterate(self._h, int(n)), "iterate")

    def finish(self):
        s = (SummaryC * len(self))()
        _lib.check(self._L.okvis_ba_finish(self._h, s), "finish")
        return [x.as_dict() for x in s]

    def evaluate_cost(self):
        c = np.zeros(len(self))
        _lib.check(self._L.okvis_ba_evaluate_cost(self._h, c.ctypes.data_as(_dp)), "evaluate_cost")
        return c

    def marginalize(self, w: int, pose_marg, sb_marg, prior=None) -> dict:
        """okvis_ba_marginalize on window w (all its landmarks + the flagged blocks are eliminated)."""
        from .window import marg_call
        win = self.windows[w]
        st, out = marg_call(lambda sp, rs: self._L.okvis_ba_marginalize(self._h, int(w), sp, rs), win.n_pose, win.n_sb,
                            pose_marg, sb_marg, prior)
        _lib.check(st, "marginalize")
        return out

    def marginalize_batch(self, w0: int, jobs) -> list:
        """okvis_ba_marginalize_batch on windows w0 .. w0 + len(jobs) - 1: jobs[i] = (pose_marg, sb_marg, prior_or_None) for window
        w0 + i.  One linearisation, one copy each way and one synchronisation for the whole range; per window the dict (and the
        bits) ``marginalize`` returns."""
        self.marginalize_batch_begin(w0, jobs)
        return self.marginalize_batch_end()

    def marginalize_batch_begin(self, w0: int, jobs):
        """First half of :meth:`marginalize_batch`: checks every window's arguments and enqueues the work.  Until
        :meth:`marginalize_batch_end` the solver takes no edits and hands out no results."""
        from .window import marg_marshal_batch
        jobs = list(jobs)
        w0 = int(w0)
        if w0 < 0 or w0 + len(jobs) > len(self.windows):
            raise IndexError(f"windows {w0} .. {w0 + len(jobs) - 1} of a batch of {len(self.windows)}")
        shapes = [(self.windows[w0 + i].n_pose, self.windows[w0 + i].n_sb) for i in range(len(jobs))]
        specs, results, outs, keep = marg_marshal_batch(shapes, jobs)
        _lib.check(self._L.okvis_ba_marginalize_batch_begin(self._h, w0, len(jobs), specs, results), "marginalize_batch_begin")
        self._marg_batch = (results, outs, keep)

    def marginalize_batch_end(self) -> list:
        """Second half of :meth:`marginalize_batch`: waits and returns the list of results."""
        if getattr(self, "_marg_batch", None) is None:
            _lib.check(-2, "marginalize_batch_end")   # OKVIS_BA_ERR_STATE: no batch has been begun
        results, outs, keep = self._marg_batch
        self._marg_batch = None
        _lib.check(self._L.okvis_ba_marginalize_batch_end(self._h, results), "marginalize_batch_end")
        from .window import marg_unpack
        del keep
        return [marg_unpack(results[i], outs[i]) for i in range(len(outs))]

    def newest_state_blocks(self, w: int) -> list:
        """[(BLOCK_POSE, i), (BLOCK_SPEEDBIAS, j)]: the pose and speed/bias blocks window w's last IMU term ends at."""
        from .window import BLOCK_POSE, BLOCK_SPEEDBIAS
        W = self.windows[w]
        if W.n_imu < 1:
            raise ValueError(f"window {w} has no IMU term: name the blocks")
        return [(BLOCK_POSE, int(np.asarray(W.imu_pose1).reshape(-1)[-1])), (BLOCK_SPEEDBIAS, int(np.asarray(W.imu_sb1).reshape(-1)[-1]))]

    # ---- what state_covariance, landmark_covariance and predicted_measurement share ----
    def _window_range(self, w0, n):
        """(w0, n) of a call on windows w0 .. w0 + n - 1 (n = None: to the end of the batch)"""
        w0 = int(w0)
        n = len(self.windows) - w0 if n is None else int(n)
        if w0 < 0 or n < 1 or w0 + n > len(self.windows):
            raise IndexError(f"windows {w0} .. {w0 + n - 1} of a batch of {len(self.windows)}")
        return w0, n

    def _tap_dims(self, w0, n) -> list:
        """(D, Dp, n_lm, n_pair) of windows w0 .. w0 + n - 1: the sizes of the referee's taps S0, Spp, V, W"""
        dims = []
        for w in range(w0, w0 + n):
            W = self.windows[w]
            np_ = C.c_int32()
            _lib.check(self._L.okvis_ba_pair_count(self._h, w, C.byref(np_)))
            dims.append((self.reduced_dim(w), 6 * int((np.asarray(W.pose_fixed).reshape(-1) == 0).sum()), int(W.n_lm), np_.value))
        return dims

    def _covariance_results(self, st, what, n, unpack) -> list:
        """The end of a covariance call that returned status st: [unpack(i) for the n windows], raised inside BackendError (as its
        ``results``) when st is OKVIS_BA_ERR_NUMERIC; any other failure has no results."""
        if st not in (0, -5):
            _lib.check(st, what)
        res = [unpack(i) for i in range(n)]
        if st != 0:
            err = _lib.BackendError(st, what)
            err.results = res
            raise err
        return res

    def state_covariance(self, blocks=None, w0: int = 0, n: int | None = None, want_S0: bool = False) -> list:
        """okvis_ba_state_covariance on windows w0 .. w0 + n - 1 (default: to the end of the batch): the marginal covariance of the
        listed free blocks at the state the solver holds, rows and columns of the inverse of the undamped reduced system, in the
        order of the list and in the solver's tangent coordinates (pose-type block: r, alpha; speed/bias block: v, b_g, b_a).
        blocks: one list of (block type, index) pairs (``window.BLOCK_POSE`` / ``BLOCK_SPEEDBIAS``) for every window, a list of
        such lists (one per window), or None = the newest state: the pose and speed/bias blocks the window's last IMU term ends
        at (ValueError for a window without IMU terms).  One linearisation, one copy each way and one synchronisation for the
        range; the solver is left as it was.  Per window a dict cov [dim][dim], dim, info, min_pivot and, with want_S0, S0 [D][D]
        (the matrix the kernel inverted).  A window with info = 1 has cov filled with NaN; the call then raises BackendError
        (OKVIS_BA_ERR_NUMERIC) whose ``results`` attribute holds the list."""
        from .window import cov_marshal_batch
        w0, n = self._window_range(w0, n)
        if blocks is None:
            sels = [self.newest_state_blocks(w0 + i) for i in range(n)]
        elif len(blocks) > 0 and isinstance(blocks[0], (list, tuple)) and len(blocks[0]) > 0 and isinstance(blocks[0][0], (list, tuple)):
            sels = [list(b) for b in blocks]
            if len(sels) != n:
                raise ValueError(f"{len(sels)} selections for {n} windows")
        else:
            sels = [list(blocks)] * n
        dims = [self.reduced_dim(w0 + i) for i in range(n)] if want_S0 else [0] * n
        specs, results, outs, keep = cov_marshal_batch(sels, dims, want_S0)
        st = self._L.okvis_ba_state_covariance(self._h, w0, n, specs, results)
        del keep

        def unpack(i):
            k = int(results[i].dim)
            r = dict(cov=outs[i]["cov"][:k * k].reshape(k, k).copy(), dim=k, info=int(results[i].info), min_pivot=float(results[i].min_pivot))
            if want_S0:
                r["S0"] = outs[i]["S0"].reshape(dims[i], dims[i]).copy()
            return r
        return self._covariance_results(st, "state_covariance", n, unpack)

    def last_covariance_ms(self) -> dict:
        """okvis_ba_last_covariance_ms: HIP-event times of the last state_covariance call's assembly launches and of cov_kernel"""
        a, k = C.c_float(), C.c_float()
        _lib.check(self._L.okvis_ba_last_covariance_ms(self._h, C.byref(a), C.byref(k)), "last_covariance_ms")
        return dict(assembly=a.value, kernel=k.value)

    def landmark_covariance(self, landmarks=None, w0: int = 0, n: int | None = None, want_taps: bool = False) -> list:
        """okvis_ba_landmark_covariance on windows w0 .. w0 + n - 1 (default: to the end of the batch): for every selected landmark
        the 3 x 3 diagonal block of the inverse of the full undamped normal matrix at the state the solver holds,
        ``V^-1 + G^T P[rows, rows] G`` with ``G = W V^-1`` and P the pose-type part of the inverse of the reduced system, in the
        tangent coordinates of the homogeneous point (a step on its first three coordinates; metres^2 in the world frame for
        w = 1, otherwise divide by w^2).  landmarks: None = every landmark of every window in window order, one list of indices
        for every window, or a list of lists (an entry may be None).  One linearisation, one copy each way and one synchronisation
        for the range; the solver is left as it was.  Per window a dict cov [m][3][3], flags [m] (bool: True = no covariance, the
        row is NaN: a landmark without observations from a free block, or a V that is not positive definite), info, min_pivot and,
        with want_taps, S0 [D][D], Spp [Dp][Dp], V [n_lm][6], W [n_pair][18]: the arrays the kernels read.  A window with
        info = 1 has every row NaN and every flag set; the call then raises BackendError (OKVIS_BA_ERR_NUMERIC) whose ``results``
        attribute holds the list."""
        from .window import lmcov_marshal_batch
        w0, n = self._window_range(w0, n)
        if landmarks is None:
            sels = [None] * n
        elif len(landmarks) > 0 and (landmarks[0] is None or isinstance(landmarks[0], (list, tuple, np.ndarray))):
            sels = list(landmarks)
            if len(sels) != n:
                raise ValueError(f"{len(sels)} selections for {n} windows")
        else:
            sels = [landmarks] * n
        counts = [int(self.windows[w0 + i].n_lm) for i in range(n)]
        taps = self._tap_dims(w0, n) if want_taps else None
        specs, results, outs, keep = lmcov_marshal_batch(sels, counts, taps)
        st = self._L.okvis_ba_landmark_covariance(self._h, w0, n, specs, results)
        del keep

        def unpack(i):
            m = int(results[i].n)
            r = dict(cov=outs[i]["cov"][:m].reshape(m, 3, 3).copy(), flags=outs[i]["flags"][:m].astype(bool), info=int(results[i].info),
                     min_pivot=float(results[i].min_pivot))
            if want_taps:
                r.update({k: outs[i][k].copy() for k in ("S0", "Spp", "V", "W")})
            return r
        return self._covariance_results(st, "landmark_covariance", n, unpack)

    def last_landmark_covariance_ms(self) -> dict:
        """okvis_ba_last_landmark_covariance_ms: HIP-event times of the last landmark_covariance call's assembly launches, of the
        inverse stage (all pose-type columns of the reduced system's inverse) and of the landmark stage"""
        a, k, l = C.c_float(), C.c_float(), C.c_float()
        _lib.check(self._L.okvis_ba_last_landmark_covariance_ms(self._h, C.byref(a), C.byref(k), C.byref(l)), "last_landmark_covariance_ms")
        return dict(assembly=a.value, inverse=k.value, landmark=l.value)

    def newest_state_queries(self, w: int = 0) -> np.ndarray:
        """The default queries of predicted_measurement for window w, [n_q][4] (lm, pose, ext, cam): every landmark into the newest
        state — the pose block the window's last IMU term ends at, or without IMU terms the highest pose index an observation
        names — through each (extrinsics, camera) pair the window uses for it: the pairs of that state's own observations, or,
        where it observes nothing yet, those of the newest state that does.  Camera by camera, landmarks in window order."""
        W = self.windows[w]
        op, oe, oc = (np.asarray(a).reshape(-1) for a in (W.obs_pose, W.obs_ext, W.obs_cam))
        if op.size == 0:
            return np.zeros((0, 4), np.int32)
        newest = int(np.asarray(W.imu_pose1).reshape(-1)[-1]) if W.n_imu else int(op.max())
        at = op == (newest if np.any(op == newest) else int(op.max()))
        pairs = sorted(set(zip(oc[at].tolist(), oe[at].tolist())))
        lm = np.arange(W.n_lm)
        return np.concatenate([np.stack([lm, np.full_like(lm, newest), np.full_like(lm, e), np.full_like(lm, c)], 1) for c, e in pairs]).astype(np.int32)

    def predicted_measurement(self, queries=None, w0: int = 0, n: int | None = None, want_taps: bool = False) -> list:
        """okvis_ba_predicted_measurement on windows w0 .. w0 + n - 1 (default: to the end of the batch): for every query (lm, pose,
        ext, cam) — the meaning of an observation row; it need not be one — the predicted pixel uv and its 2 x 2 covariance under the
        joint uncertainty of landmark, pose and extrinsics at the state the solver holds, ``J_l V^-1 J_l^T + A P[R, R] A^T`` with
        ``A = J_x E_x - J_l G^T E_l`` (include/okvis_amd_ba.h has the definition).  No keypoint noise is included.  queries: None =
        newest_state_queries of every window, one [n_q][4] integer array for every window, or a list of such arrays (an entry may
        be None).  One linearisation, one copy each way and one synchronisation for the range; the solver is left as it was.  Per
        window a dict uv [n_q][2], cov [n_q][2][2], flags [n_q] (uint8: bit 1 = no covariance, cov NaN; bit 2 = the point does not
        project, uv and cov NaN), info, min_pivot and, with want_taps, S0, Spp, V, W (the arrays the kernels read) and jac
        [n_q][30] (J_l | J_p | J_e as the kernel formed them).  uv and cov go unchanged into ``Frontend.gate_3d2d``.  A window with
        info = 1 has every cov NaN and bit 1 set everywhere; the call then raises BackendError (OKVIS_BA_ERR_NUMERIC) whose
        ``results`` attribute holds the list."""
        from .window import predcov_marshal_batch
        w0, n = self._window_range(w0, n)
        if queries is None:
            qs = [None] * n
        elif isinstance(queries, np.ndarray) and queries.ndim == 2:
            qs = [queries] * n
        else:
            qs = list(queries)
            if len(qs) != n:
                raise ValueError(f"{len(qs)} query lists for {n} windows")
        qs = [self.newest_state_queries(w0 + i) if q is None else np.asarray(q, np.int32).reshape(-1, 4) for i, q in enumerate(qs)]
        taps = self._tap_dims(w0, n) if want_taps else None
        specs, results, outs, keep = predcov_marshal_batch(qs, taps)
        st = self._L.okvis_ba_predicted_measurement(self._h, w0, n, specs, results)
        del keep

        def unpack(i):
            m = int(results[i].n)
            r = dict(uv=outs[i]["uv"][:m].copy(), cov=outs[i]["cov"][:m].reshape(m, 2, 2).copy(), flags=outs[i]["flags"][:m].copy(),
                     info=int(results[i].info), min_pivot=float(results[i].min_pivot))
            if want_taps:
                r.update({k: outs[i][k].copy() for k in ("S0", "Spp", "V", "W")})
                r["jac"] = outs[i]["jac"][:m].copy()
            return r
        return self._covariance_results(st, "predicted_measurement", n, unpack)

    def last_predicted_measurement_ms(self) -> dict:
        """okvis_ba_last_predicted_measurement_ms: HIP-event times of the last predicted_measurement call's assembly launches, of the
        inverse stage (all pose-type columns of the reduced system's inverse) and of the query stage"""
        a, k, q = C.c_float(), C.c_float(), C.c_float()
        _lib.check(self._L.okvis_ba_last_predicted_measurement_ms(self._h, C.byref(a), C.byref(k), C.byref(q)), "last_predicted_measurement_ms")
        return dict(assembly=a.value, inverse=k.value, query=q.value)

    def synchronize(self):
        _lib.check(self._L.okvis_ba_synchronize(self._h), "synchronize")

    # ---- results ----
    def get_state(self, w: int = 0):
        W = self.windows[w]
        pose, sb, lm = np.zeros((W.n_pose, 7)), np.zeros((W.n_sb, 9)), np.zeros((W.n_lm, 4))
        _lib.check(self._L.okvis_ba_get_state(self._h, w, pose.ctypes.data_as(_dp), sb.ctypes.data_as(_dp),
                                              lm.ctypes.data_as(_dp)), "get_state")
        return pose, sb, lm

    def fetch_results(self, w: int = 0):
        """okvis_ba_fetch_results: state, landmark quality and the IMU caches' reference biases with one synchronisation."""
        W = self.windows[w]
        pose, sb, lm = np.zeros((W.n_pose, 7)), np.zeros((W.n_sb, 9)), np.zeros((W.n_lm, 4))
        q, ref = np.zeros(W.n_lm), np.zeros((W.n_imu, 9))
        _lib.check(self._L.okvis_ba_fetch_results(self._h, w, pose.ctypes.data_as(_dp), sb.ctypes.data_as(_dp), lm.ctypes.data_as(_dp),
                                                  q.ctypes.data_as(_dp), ref.ctypes.data_as(_dp)), "fetch_results")
        return dict(pose=pose, sb=sb, lm=lm, quality=q, imu_sb_ref=ref)

    def fetch_imu_caches(self, w: int = 0):
        """okvis_ba_fetch_imu_caches: the preintegration records of window w's IMU terms, [n_imu, 290] (Window.imu_cache, flag 2)."""
        from .window import IMU_CACHE_DOUBLES
        out = np.zeros((self.windows[w].n_imu, IMU_CACHE_DOUBLES))
        _lib.check(self._L.okvis_ba_fetch_imu_caches(self._h, w, out.ctypes.data_as(_dp)), "fetch_imu_caches")
        return out

    def set_state(self, w: int, pose=None, sb=None, lm=None):
        def p(a):
            return None if a is None else np.ascontiguousarray(a, np.float64)
        pose, sb, lm = p(pose), p(sb), p(lm)
        _lib.check(self._L.okvis_ba_set_state(
            self._h, w, None if pose is None else pose.ctypes.data_as(_dp),
            None if sb is None else sb.ctypes.data_as(_dp), None if lm is None else lm.ctypes.data_as(_dp)), "set_state")

    def array(self, name: str, w: int = 0) -> np.ndarray:
        """okvis_ba_download of the array ARR[name] of window w, flat (ARR's comment has the layout of IMU_LIN)"""
        n = C.c_int64()
        _lib.check(self._L.okvis_ba_array_size(self._h, w, ARR[name], C.byref(n)), f"array_size {name}")
        out = np.zeros(max(n.value, 0))
        _lib.check(self._L.okvis_ba_download(self._h, w, ARR[name], out.ctypes.data_as(_dp), n.value), f"download {name}")
        return out

    def reduced_dim(self, w: int = 0) -> int:
        d = C.c_int32()
        _lib.check(self._L.okvis_ba_reduced_dim(self._h, w, C.byref(d)))
        return d.value

    def pairs(self, w: int = 0):
        n = C.c_int32()
        _lib.check(self._L.okvis_ba_pair_count(self._h, w, C.byref(n)))
        a, b = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        ip = C.POINTER(C.c_int32)
        _lib.check(self._L.okvis_ba_pairs(self._h, w, a.ctypes.data_as(ip), b.ctypes.data_as(ip)))
        return a, b

    # ---- measurement hooks ----
    def last_iterate_ms(self) -> float:
        t = C.c_float()
        _lib.check(self._L.okvis_ba_last_iterate_ms(self._h, C.byref(t)))
        return t.value

    def profile_iterations(self, n: int):
        ms = (C.c_float * 4)()
        _lib.check(self._L.okvis_ba_profile_iterations(self._h, int(n), ms))
        return dict(schur=ms[0], solve=ms[1], small=ms[2], linearize=ms[3])

    def profile_launches(self, n: int):
        """per-iteration launch durations [n][3] in ms: schur, solve, linearise (incl. the IMU / prior workgroups)"""
        ms = (C.c_float * (4 * int(n)))()
        _lib.check(self._L.okvis_ba_profile_launches(self._h, int(n), ms))
        a = np.array(ms[:], dtype=np.float64).reshape(int(n), 4)
        return dict(schur=a[:, 0], solve=a[:, 1], linearize=a[:, 2] + a[:, 3])

    def helper_timeouts(self) -> int:
        """okvis_ba_helper_timeouts: solve launches whose helper workgroups were late (0 in a healthy run)"""
        n = C.c_int64()
        _lib.check(self._L.okvis_ba_helper_timeouts(self._h, C.byref(n)))
        return n.value

    def pause_count(self) -> int:
        """okvis_ba_pause_count: windows the three-launch iteration's solve kernel paused since begin() (0 in a steady run)"""
        n = C.c_int64()
        _lib.check(self._L.okvis_ba_pause_count(self._h, C.byref(n)))
        return n.value

    ROUTE = ("windows", "fused", "decision_free_schur", "piece_path", "split_small", "sub_batches", "sub_batch_max_windows",
             "schur_kernel", "solve_dbuf", "solve_tiled", "solve_helpers", "graph", "max_chunks", "slots", "solve_mode", "small_rides",
             "lin_records", "three_launch")

    def launch_route(self) -> dict:
        """okvis_ba_launch_route: which launches this batch takes under the current options (read-only)"""
        r = (C.c_int32 * len(self.ROUTE))()
        _lib.check(self._L.okvis_ba_launch_route(self._h, r), "launch_route")
        return {n: int(r[i]) for i, n in enumerate(self.ROUTE)}

    def algorithmic_bytes(self):
        v = [C.c_int64() for _ in range(4)]
        _lib.check(self._L.okvis_ba_algorithmic_bytes(self._h, *[C.byref(x) for x in v]))
        return dict(linearize=v[0].value, schur=v[1].value, solve=v[2].value, small=v[3].value)
