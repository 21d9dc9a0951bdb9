"""The query lists of the predicted-measurement referee — TEST INFRASTRUCTURE, host only.  The windows are those of
tests/lmcov_cases.py (A ... F, H, U; K = 3 ... 12, L = 30 ... 120): the smallest shapes at which the kernel can go wrong.
tests/test_predicted_measurement_host.py proves on the CPU that these inputs can tell the right definition from wrong ones;
tests/test_gpu_predicted_measurement.py compares the kernel on them.  Every case's list (queries(name)) holds, in this order,

    newest    every landmark into the newest state, landmark l through camera l mod 2 and the extrinsics block the window's
              observations pair with that state and camera (most of these coincide with an observation; the others are a landmark
              seen from a pose that does not observe it; U's landmark without pairs is among them)
    observed  three rows of the window's own observation list: the first, the middle one, the last
    unseen    up to three (landmark, pose) combinations no observation of the window has (none in D and H: visibility 1)
    crossed   with per-frame extrinsics (C, H): a state seen through the extrinsics block of another frame
    fixed     where a pose is fixed (F): two landmarks from that pose — with fixed extrinsics rows_x is empty
    behind    one query whose point does not project, the farthest behind of its kind: a landmark with pairs seen from the newest state through
              ANOTHER BODY POSE taken as T_SC (a query need not be an observation).  The landmark itself is not moved: a landmark
              with observations moved behind its cameras has V = 0 and W = 0 and takes the window's S0 with it
    repeats   the first row and the `behind` row once more

H: every landmark touches all 12 free blocks (72 rows = Dp, more than a wave has lanes); the query's blocks are among them, so
|R| = 72 — 84 rows need a window with 14 free pose-type blocks around one landmark, which the cases' limit Dp <= 72 excludes.
A, D, E, F, U have fixed extrinsics (rows_x is the pose alone), B shared and C, H per-frame free ones."""
from __future__ import annotations

import numpy as np

from . import lmcov_cases as lc
from . import predcov_statement as ps

CASES = lc.CASES
NC = 2
_cache = {}


def _ext_of(w, pose, cam):
    """the extrinsics block the window's observations pair with (pose, cam); where that state has none with this camera, the one
    the camera's observations use most recently"""
    op, oe, oc = (np.asarray(a).reshape(-1) for a in (w.obs_pose, w.obs_ext, w.obs_cam))
    at = np.flatnonzero((op == pose) & (oc == cam))
    if at.size == 0:
        at = np.flatnonzero(oc == cam)
        at = at[op[at] == op[at].max()]
    return int(oe[at[0]])


def _depth(T_WS, T_SC, hp):
    """z of the point in the camera frame, in metres"""
    from okvis_amd import synthetic
    p_S = synthetic.qrot(T_WS[3:]).T @ (hp[:3] / hp[3] - T_WS[:3])
    return float((synthetic.qrot(T_SC[3:]).T @ (p_S - T_SC[:3]))[2])


def keyframes(name):
    return lc.cc.KEYFRAMES[{"H": "A", "U": "A"}.get(name, name)]


def queries(name):
    """(window, queries [n, 4] int32, tags [n]) of a case, computed once"""
    if name in _cache:
        return _cache[name]
    from . import oracle_lib as ol
    w = lc.window(name)
    K = keyframes(name)
    ol_, op, oe, oc = (np.asarray(a).reshape(-1).astype(np.int64) for a in (w.obs_lm, w.obs_pose, w.obs_ext, w.obs_cam))
    n_lm = int(np.asarray(w.lm).reshape(-1, 4).shape[0])
    fixed = np.asarray(w.pose_fixed).reshape(-1) != 0
    q, tags = [], []

    def add(tag, l, p, e, c):
        q.append((int(l), int(p), int(e), int(c)))
        tags.append(tag)

    ext_new = [_ext_of(w, K - 1, c) for c in range(NC)]
    for l in range(n_lm):
        add("newest", l, K - 1, ext_new[l % NC], l % NC)
    for o in (0, ol_.size // 2, ol_.size - 1):
        add("observed", ol_[o], op[o], oe[o], oc[o])
    seen = set(zip(ol_.tolist(), op.tolist()))
    unseen = [(l, k) for k in range(K) for l in range(n_lm) if (l, k) not in seen and not fixed[k]][:3]
    for l, k in unseen:
        add("unseen", l, k, _ext_of(w, k, 1), 1)
    if name in ("C", "H"):
        add("crossed", 2, K - 1, _ext_of(w, 0, 0), 0)
        add("crossed", 3, 0, _ext_of(w, K - 1, 1), 1)
    for k in np.flatnonzero(fixed[:K]):
        add("fixed", 1, k, _ext_of(w, k, 0), 0)
        add("fixed", 4, k, _ext_of(w, k, 1), 1)
    paired = set(ol_[~fixed[op]].tolist()) | set(ol_[~fixed[oe]].tolist())
    pose, lm = np.asarray(w.pose, np.float64).reshape(-1, 7), np.asarray(w.lm, np.float64).reshape(-1, 4)
    depth = {(l, k): _depth(pose[K - 1], pose[k], lm[l]) for l in sorted(paired) for k in range(K - 1)}
    l, k = min(depth, key=depth.get)                        # the farthest behind: it stays there when the state is optimised
    assert depth[(l, k)] < -1.0 and not ps.jacobians(ol.lib(), w, (l, K - 1, k, 0))[2], name
    add("behind", l, K - 1, k, 0)
    add("repeats", *q[0])
    add("repeats", *q[-2])
    _cache[name] = (w, np.array(q, np.int32).reshape(-1, 4), np.array(tags))
    return _cache[name]


def expected_flags(w, terms, Q, projects):
    """flags [n] a healthy window's query list must come back with: 1 = the landmark has no pair, 2 = the point does not project"""
    return np.array([(0 if terms[int(q[0])][0].size else 1) | (0 if ok else 2) for q, ok in zip(Q, projects)], np.uint8)
