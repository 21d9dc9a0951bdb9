"""Named, seeded cases for the referee of okvis_fe_stereo_triangulate, okvis_fe_project_landmarks and okvis_fe_gate_3d2d
(tests/tri_statement.py).  TEST INFRASTRUCTURE ONLY: imports nothing from the product.

A case is a dict with `entry` ("stereo" | "project" | "gate"), `family` ("ordinary" | "size" | "placed"), the arguments of the entry
and, for a placed case, `edges`: {edge name: {"decision": name in the statement's record, "rows": candidates, "m": the distance from
the threshold each was built at (in units of the decision's scale), "side": -1 below / +1 above}}.  A size case carries `parent` and
`rows`: it is the first rows of that ordinary case, to be compared row by row with it.

Placed edges are solved, not drawn: place() bisects one scalar input of every candidate until the long double statement's decision
quantity sits at the requested distance from its threshold.  Keypoints are float32, so an edge that only keypoints can move is placed
no closer than about 1e-4; the edges that a double input moves (sigma_ray, hp_W, uv, U) go down to a few bands."""
import functools

import numpy as np

import tri_statement as S
from sac_statement import DIST_EQUI, DIST_NONE, DIST_RADTAN, DIST_RADTAN8, _distort

INTR = {DIST_EQUI: np.array([458.654, 457.296, 367.215, 248.375, -0.0129, 0.0077, -0.0041, 0.0009]),
        DIST_RADTAN: np.array([458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]),
        DIST_RADTAN8: np.array([350.0, 360.0, 378.0, 238.0, -0.16, 0.15, 0.0003, 0.0002, 0.01, 0.02, -0.01, 0.005]),
        DIST_NONE: np.array([350.0, 360.0, 378.0, 238.0])}
NAMES = {DIST_NONE: "none", DIST_RADTAN: "radtan", DIST_EQUI: "equi", DIST_RADTAN8: "radtan8"}
M_DOUBLE = (0.3, 1e-3, 1e-6, 3e-8, 1e-10)   # stereo edges moved by sigma_ray: the bands there are 1e-12 ... 1e-11
M_FLOAT = (0.3, 1e-2, 1e-3)               # edges only float32 keypoints can move
M_EXACT = (0.3, 1e-4, 1e-8, 1e-12, 1e-13, 2e-14)   # projection and gate: the bands are 8 ulp = 1.8e-15


def quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.r_[axis * np.sin(angle / 2), np.cos(angle / 2)]


def rot(q):
    return np.asarray(S.rotation(S.Ctx(np.float64), q), np.float64)


def forward(cam, p):
    """pixel of the points p [n][3] in the camera's frame, in double (for building scenes only; no status)"""
    x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    xd, yd, _ = _distort(cam["model"], cam["intr"][4:], x, y)
    return np.c_[cam["intr"][0] * xd + cam["intr"][2], cam["intr"][1] * yd + cam["intr"][3]]


def uoplus(full, seed, trans=1.69e-2, rotv=1e-8):
    U = np.diag([trans] * 3 + [rotv] * 3)
    if full:
        rng = np.random.default_rng(seed)
        A = rng.normal(size=(6, 6)) * 0.3 + np.eye(6)
        d = np.sqrt(np.diag(U))
        U = (A @ A.T) * np.outer(d, d)
    return U


# ---- ordinary scenes -----------------------------------------------------------------------------------------------------------------
def stereo_scene(model_a, model_b, seed, n=100, full=False, sigma="none", b_other=False):
    """points in front of A seen by B = A moved by T_AB; keypoints = projections + 0.5 px noise; candidates = the true matches, wrong
    matches, repeated keypoints and the last keypoint of each array"""
    rng = np.random.default_rng(seed)
    cam_a = S.camera(INTR[model_a], model_a)
    intr_b = INTR[model_b].copy()
    if b_other:
        intr_b[:4] = [420.0, 415.0, 330.0, 210.0]
    cam_b = S.camera(intr_b, model_b, 680, 440) if b_other else S.camera(intr_b, model_b)
    T_AB = np.r_[0.11 * np.array([1.0, 0.05, -0.02]), quat(rng.normal(size=3), 0.02)]
    depth = rng.uniform(0.6, 25.0, n)
    depth[:4] = [0.12, 0.15, 300.0, 2000.0]            # nearer than 0.2 (zero Jacobians), and far: parallel rays
    p_A = np.c_[rng.uniform(-0.5, 0.5, n) * depth, rng.uniform(-0.35, 0.35, n) * depth, depth]
    p_A[:2, :2] = [[0.05, 0.0], [0.06, 0.01]]
    p_B = (p_A - T_AB[:3]) @ rot(T_AB[3:])
    uvA = forward(cam_a, p_A) + rng.normal(size=(n, 2)) * 0.5
    uvB = forward(cam_b, p_B) + rng.normal(size=(n, 2)) * 0.5
    uvA[:4], uvB[:4] = forward(cam_a, p_A[:4]), forward(cam_b, p_B[:4])
    # keypoints far outside the image: undistort runs out of steps.  Not so far that RADTAN8's distort refuses inside the loop
    # (rho > 9), where the reference reads values it never set
    far = 0.6 if DIST_RADTAN8 in (model_a, model_b) else 2.5 if DIST_RADTAN in (model_a, model_b) else 1.0
    uvA[4] = cam_a["intr"][2:4] + far * np.array([760.0, -540.0])
    uvB[5] = cam_b["intr"][2:4] + far * np.array([-700.0, 610.0])
    size = rng.choice([4.0, 8.0, 12.0, 31.0], n)
    kpA, kpB = np.c_[uvA, size].astype(np.float32), np.c_[uvB, rng.permutation(size)].astype(np.float32)
    true = np.c_[np.arange(n), np.arange(n)]
    wrong = np.c_[rng.integers(0, n, n // 4), rng.integers(0, n, n // 4)]
    repeat = np.array([[7, 7], [7, 7], [7, 8], [n - 1, n - 1], [n - 1, 0], [0, n - 1]])
    pairs = np.r_[true, wrong, repeat].astype(np.int32)
    sig = None
    if sigma != "none":
        sig = 2 ** 0.25 * 0.8 * rng.choice([4.0, 8.0, 31.0], len(pairs)) / 12.0 / cam_a["intr"][0]
        if sigma == "minus":
            sig = np.where(rng.random(len(pairs)) < 0.4, -1.0, sig)
    return {"entry": "stereo", "family": "ordinary", "cam_a": cam_a, "cam_b": cam_b, "T_AB": T_AB, "UOplus": uoplus(full, seed),
            "kp_a": kpA, "kp_b": kpB, "pairs": pairs, "sigma_ray": sig}


def project_scene(model, seed, n=300, width=752, height=480):
    """landmarks all around the camera: in front, behind, outside the image, w < 0, w = 0, w = 1e-3 and one on the principal plane"""
    rng = np.random.default_rng(seed)
    cam = S.camera(INTR[model], model, width, height)
    T = np.r_[rng.normal(size=3), quat(rng.normal(size=3), 0.4)]
    p_C = np.c_[rng.uniform(-8, 8, n), rng.uniform(-6, 6, n), rng.uniform(-4, 12, n)]
    p_C[::3, :2] *= 0.3                                    # a good share inside the image
    p_C[0] = [1.0, 1.0, 0.0]
    w = rng.choice([1.0, 1.0, 1.0, 0.5, -1.0, 0.0, 1e-3], n)
    hp_W = np.c_[(p_C - w[:, None] * T[:3]) @ rot(T[3:]), w]
    A = rng.normal(size=(3, 3)) * 0.4 + np.eye(3)
    P3 = (A @ A.T) * (1.69e-2 if seed % 2 else 4e-6)       # full, non-diagonal
    return {"entry": "project", "family": "ordinary", "cam": cam, "T_CbW": T, "P3": P3, "hp_W": hp_W}


def gate_scene(proj, seed):
    """keypoints near the successful projections of a project case (some within 2 sigma, some not), random pairs, and U with
    U[0][1] != U[1][0]"""
    rng = np.random.default_rng(seed)
    res = S.project_landmarks(S.Ctx(np.float64), proj["cam"], proj["T_CbW"], proj["P3"], proj["hp_W"])
    idx = np.flatnonzero(res["status"] == S.PROJ_SUCCESSFUL)
    uv, U = np.asarray(res["uv"], np.float64), np.asarray(res["U"], np.float64).copy()
    U[:, 0, 1] *= 1.0 + 0.5 * rng.random(len(U))          # not symmetric
    kp = np.c_[uv[idx] + rng.normal(size=(len(idx), 2)) * rng.choice([0.3, 2.0, 6.0], len(idx))[:, None],
               rng.choice([4.0, 8.0, 16.0, 60.0], len(idx))].astype(np.float32)
    pairs = np.r_[np.c_[idx, np.arange(len(idx))], np.c_[rng.choice(idx, 220), rng.integers(0, len(idx), 220)],
                  [[idx[-1], len(idx) - 1], [idx[0], len(idx) - 1]]].astype(np.int32)
    return {"entry": "gate", "family": "ordinary", "uv": uv, "U": U, "kp_b": kp, "pairs": pairs}


def cut(parent_name, parent, rows):
    c = dict(parent)
    c.update(family="size", parent=parent_name, rows=rows)
    if parent["entry"] == "stereo":
        c["pairs"] = parent["pairs"][:rows]
        c["sigma_ray"] = None if parent["sigma_ray"] is None else parent["sigma_ray"][:rows]
    elif parent["entry"] == "project":
        c["hp_W"] = parent["hp_W"][:rows]
    else:
        c["pairs"] = parent["pairs"][:rows]
    return c


# ---- placed edges --------------------------------------------------------------------------------------------------------------------
def run(case, cx=None, **kw):
    """the statement on a case -> (result, decisions)"""
    cx = cx or S.Ctx()
    if case["entry"] == "stereo":
        res = S.stereo(cx, case["cam_a"], case["cam_b"], case["T_AB"], case["UOplus"], case["kp_a"], case["kp_b"], case["pairs"],
                       case["sigma_ray"], **kw)
    elif case["entry"] == "project":
        res = S.project_landmarks(cx, case["cam"], case["T_CbW"], case["P3"], case["hp_W"])
    else:
        res = S.gate(cx, case["uv"], case["U"], case["kp_b"], case["pairs"])
    return res, cx.dec


def targets(thr, ms, zero_scale=None):
    """(target quantity, m, side) for every m on both sides: below thr (1 - m), above thr / (1 - m), so that the distance in units
    of max(|thr|, |q|) is m; around a zero threshold -m and +m in units of the scale the decision uses"""
    out = []
    for m in ms:
        if thr == 0:
            out += [(-m, m, -1), (m, m, 1)]
        else:
            out += [(thr * (1 - m), m, -1), (thr / (1 - m), m, 1)]
    return out


def place(build, decision, tg, lo, hi, iters=64, relative=False, **kw):
    """bisect t [k] in [lo, hi] until decision's quantity of candidate i of build(t) is tg[i][0] (in units of its scale with
    `relative`, for a zero threshold) -> t"""
    want = np.array([t[0] for t in tg], np.longdouble)
    lo, hi = np.full(len(tg), lo, np.float64), np.full(len(tg), hi, np.float64)

    def q(t):
        d = run(build(t), **kw)[1][decision]
        return d["q"] / d["scale"] if relative else d["q"]
    rising = q(hi) > q(lo)
    for _ in range(iters):
        mid = (lo + hi) / 2
        up = (q(mid) < want) == rising
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return (lo + hi) / 2


def edge(decision, tg, first=0):
    return {"decision": decision, "rows": np.arange(first, first + len(tg)), "m": np.array([t[1] for t in tg]),
            "side": np.array([t[2] for t in tg])}


def _pairs(k):
    return np.c_[np.arange(k), np.arange(k)].astype(np.int32)


def _stereo_base(model=DIST_RADTAN, wide=False):
    intr = INTR[model].copy()
    cam = S.camera(intr, model)
    if wide:
        intr[:4] = [350.0, 350.0, 2000.0, 1500.0]
        cam = S.camera(intr, model, 4000, 3000)
    return cam, np.r_[0.11, 0.004, -0.002, quat([0.3, 1.0, 0.2], 0.015)]


def _placed_stereo(build, decision, thr, ms, lo, hi, name, relative=False, **kw):
    tg = targets(thr, ms)
    case = build(place(build, decision, tg, lo, hi, relative=relative, **kw))
    case.update(family="placed", edges={name: edge(decision, tg)})
    return case


def placed_sigma(which):
    """`chi2 > 9` and the parallel branch's `|e1 x e2| < 6 sigma`: the candidate's own sigma_ray (a double) is what moves"""
    cam, T_AB = _stereo_base()
    C = rot(T_AB[3:])
    k = 2 * len(M_DOUBLE)
    depth = np.linspace(2.0, 9.0, k) if which == "chi2" else np.linspace(900.0, 2500.0, k)
    p_A = np.c_[0.2 * depth, -0.1 * depth, depth]
    kpA = np.c_[forward(cam, p_A), np.full(k, 12.0)].astype(np.float32)
    kpB = np.c_[forward(cam, (p_A - T_AB[:3]) @ C) + [0.0, 0.6 if which == "chi2" else 0.15], np.full(k, 12.0)].astype(np.float32)

    def build(t):
        return {"entry": "stereo", "cam_a": cam, "cam_b": cam, "T_AB": T_AB, "UOplus": uoplus(False, 0), "kp_a": kpA, "kp_b": kpB,
                "pairs": _pairs(k), "sigma_ray": np.asarray(t, np.float64)}
    if which == "chi2":
        return _placed_stereo(build, "chi2", 9.0, M_DOUBLE, 1e-6, 1e-1, "chi2 > 9", want_uncertainty=False)
    tg = targets(1.0, M_DOUBLE)            # the threshold is 6 sigma itself: place cross / (6 sigma) around 1

    def ratio(t):
        d = run(build(t), want_uncertainty=False)[1]["cross"]
        return d["q"] / d["thr"]
    lo, hi = np.full(k, 1e-7), np.full(k, 1e-1)
    want = np.array([t[0] for t in tg], np.longdouble)
    for _ in range(64):
        mid = (lo + hi) / 2
        big = ratio(mid) > want            # the ratio falls as sigma grows
        lo, hi = np.where(big, mid, lo), np.where(big, hi, mid)
    case = build((lo + hi) / 2)
    case.update(family="placed", edges={"cross < 6 sigma": edge("cross", tg)})
    return case


def placed_keypoint(which):
    """edges that a keypoint of B moves: |det| <= 1e-6 (disparity), errA / errB > 4 (offset along the epipolar normal), |r_B|^2 < 4
    (depth), the undistort loop's early exit (radius)"""
    model = {"det": DIST_NONE, "det_radtan": DIST_RADTAN, "exit_equi": DIST_EQUI}.get(which, DIST_RADTAN)
    cam, T_AB = _stereo_base(model)
    cam_b = cam
    if which == "chi2_own":                # sigma_ray = -1: 0.5 / min(fu_A, fu_B), and B's is the smaller
        intr_b = INTR[model].copy()
        intr_b[:4] = [420.0, 415.0, 330.0, 210.0]
        cam_b = S.camera(intr_b, model, 680, 440)
    if which.startswith("det"):
        T_AB = np.r_[0.11, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    C = rot(T_AB[3:])
    k = 2 * len(M_FLOAT)
    depth = np.linspace(2.5, 6.0, k)
    p_A = np.c_[0.15 * depth, 0.1 * depth, depth]
    uvA, uvB = forward(cam, p_A), forward(cam_b, (p_A - T_AB[:3]) @ C)
    sa, sb = (12.0, 31.0) if which == "errA" else (31.0, 12.0) if which == "errB" else (12.0, 12.0)
    sig = np.full(k, 1e-1 if which in ("errA", "errB") else 1e-2)

    def build(t):
        a, b = uvA.copy(), uvB.copy()
        if which.startswith("det"):
            b = a - np.c_[t, np.zeros(k)]
        elif which in ("errA", "errB", "chi2_own"):
            b = b + np.c_[np.zeros(k), t]
        elif which == "rB":
            p = np.c_[0.15 * t, 0.1 * t, t]
            a, b = forward(cam, p), forward(cam, (p - T_AB[:3]) @ C)
        else:
            ctr = cam["intr"][2:4]
            a = ctr + np.c_[t, 0.6 * t]
            b = a - [8.0, 0.0]
        return {"entry": "stereo", "cam_a": cam, "cam_b": cam_b, "T_AB": T_AB, "UOplus": uoplus(False, 0),
                "kp_a": np.c_[a, np.full(k, sa)].astype(np.float32), "kp_b": np.c_[b, np.full(k, sb)].astype(np.float32),
                "pairs": _pairs(k), "sigma_ray": None if which == "rB" else np.full(k, -1.0) if which == "chi2_own" else sig}
    if which.startswith("det"):
        return _placed_stereo(build, "det", 1.0e-6, M_FLOAT, 0.05, 3.0, "|det| <= 1e-6", want_uncertainty=False)
    if which in ("errA", "errB"):
        return _placed_stereo(build, which, 4.0, M_FLOAT, 0.3, 12.0, which + " > 4", want_uncertainty=False)
    if which == "chi2_own":
        return _placed_stereo(build, "chi2", 9.0, (0.3, 0.05, 1e-2), 0.05, 6.0, "chi2 > 9", want_uncertainty=False)
    if which == "rB":
        return _placed_stereo(build, "rB", 4.0, M_FLOAT, 2.0, 40.0, "|r_B|^2 < 4")
    step = "A_undistort_exit2" if which == "exit_radtan" else "A_undistort_exit1"
    return _placed_stereo(build, step, 1.0e-15, M_FLOAT, 2.0, 330.0, "undistort exit at 1e-15", want_uncertainty=False)


def placed_dot():
    """the `dot < 0` flip: two wide cameras and skew rays (a wrong match) under a sigma_ray large enough to pass chi2; between
    converging and diverging the midpoint passes the plane through the baseline's centre.  The rows after the edge's look at each
    other at more than a right angle: the `a10 < 0` branch ("wrong viewing direction")."""
    cam, _ = _stereo_base(DIST_NONE, wide=True)
    T_AB = np.r_[0.11, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    tg = targets(0.0, M_FLOAT)
    k = len(tg)
    opposed = np.array([-3.0, -2.2, -1.5, -1.0])

    def build(t):
        a = np.tile([[1.5, 0.0, 1.0]], (k + len(opposed), 1))
        b = np.c_[np.r_[t, opposed], np.full(k + len(opposed), 1.0), np.ones(k + len(opposed))]
        return {"entry": "stereo", "cam_a": cam, "cam_b": cam, "T_AB": T_AB, "UOplus": uoplus(False, 0),
                "kp_a": np.c_[forward(cam, a), np.full(len(a), 12.0)].astype(np.float32),
                "kp_b": np.c_[forward(cam, b), np.full(len(a), 12.0)].astype(np.float32), "pairs": _pairs(len(a)),
                "sigma_ray": np.full(len(a), 1e3)}

    def q(t):
        d = run(build(t), want_uncertainty=False)[1]["dot"]
        return (d["q"] / d["scale"])[:k]
    lo, hi = np.full(k, 1.9), np.full(k, 2.4)
    want = np.array([t[0] for t in tg], np.longdouble)
    for _ in range(50):
        mid = (lo + hi) / 2
        high = q(mid) > want                # the quantity falls as B's ray turns outwards
        lo, hi = np.where(high, mid, lo), np.where(high, hi, mid)
    case = build((lo + hi) / 2)
    case.update(family="placed", edges={"dot < 0": edge("dot", tg)})
    return case


def placed_rank():
    """rank 8 against 9.  Below: points nearer than 0.2 to both cameras, whose Jacobians the reprojection error zeroes (the point
    block of H is exactly zero).  Above and around: the rotation part of UOplus scaled down until the smallest |R_ii| is the given
    multiple of the threshold for the first candidate."""
    cam, _ = _stereo_base(DIST_NONE, wide=True)
    T_AB = np.r_[0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    p = np.array([[0.02, 0.01, 0.15], [0.03, -0.01, 0.12], [0.01, 0.0, 0.18], [0.2, 0.1, 3.0], [0.3, -0.2, 5.0], [-0.4, 0.1, 4.0]])
    k = len(p)
    base = {"entry": "stereo", "cam_a": cam, "cam_b": cam, "T_AB": T_AB, "kp_a": np.c_[forward(cam, p), np.full(k, 12.0)].astype(np.float32),
            "kp_b": np.c_[forward(cam, p - T_AB[:3]), np.full(k, 12.0)].astype(np.float32), "pairs": _pairs(k), "sigma_ray": np.full(k, 1e-1)}
    cases = {}
    for label, mult in (("clear", None), ("x1000", 1000.0), ("x8", 8.0), ("x1", 1.0), ("x0.1", 0.1)):
        lo, hi = -40.0, -8.0                       # log10 of the rotation variance
        if mult is not None:
            for _ in range(50):
                mid = (lo + hi) / 2
                c = dict(base, UOplus=uoplus(False, 0, rotv=10.0 ** mid))
                if run(c)[1]["rank"]["q"][3] < mult:
                    lo = mid
                else:
                    hi = mid
        c = dict(base, UOplus=uoplus(False, 0, rotv=10.0 ** hi), family="placed")
        c["edges"] = {"rank 8 against 9": {"decision": "rank", "rows": np.arange(k), "m": np.full(k, np.nan), "side": np.zeros(k, int)}}
        cases["placed_rank_" + label] = c
    return cases


def placed_project(which):
    """|z| < 1e-12, the image border of a 640 x 400 image, RADTAN8's rho > 9: hp_W is a double, the pose the identity"""
    model = DIST_RADTAN8 if which == "rho" else DIST_NONE
    cam = S.camera(INTR[model], model, 640, 400)
    T = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    P3 = np.array([[2.0, 0.3, -0.1], [0.3, 1.0, 0.2], [-0.1, 0.2, 1.5]]) * 1e-2
    fu, fv, cu, cv = cam["intr"][:4]
    dec, thr, zero = {"z": ("z_small", 1e-12, False), "z_neg": ("z_small", 1e-12, False), "rho": ("rho", 9.0, False), "u_low": ("u_low", 0.0, True),
                      "v_low": ("v_low", 0.0, True), "u_high": ("u_high", 640.0, False), "v_high": ("v_high", 400.0, False)}[which]
    tg = targets(thr, M_EXACT)
    k = len(tg)
    w = np.where(np.arange(k) % 3 == 2, -1.0, 1.0)        # every third through the w < 0 branch

    def build(t):
        if which in ("z", "z_neg"):
            h = np.c_[0.1 * t, -0.05 * t, t if which == "z" else -t, np.ones(k)]
        elif which == "rho":
            h = np.c_[t * 0.8, t * 0.6, np.ones(k), np.ones(k)]
        elif which.startswith("u"):
            h = np.c_[t, np.full(k, 0.1), np.ones(k), np.ones(k)]
        else:
            h = np.c_[np.full(k, 0.1), t, np.ones(k), np.ones(k)]
        h[:, :3] *= w[:, None]
        h[:, 3] = w
        return {"entry": "project", "cam": cam, "T_CbW": T, "P3": P3, "hp_W": h}
    lo, hi = {"z": (1e-14, 1e-10), "z_neg": (1e-14, 1e-10), "rho": (1.0, 5.0), "u_low": (-2.0, 0.0), "v_low": (-2.0, 0.0),
              "u_high": (0.0, 2.0), "v_high": (0.0, 2.0)}[which]
    case = build(place(build, dec, tg, lo, hi, iters=80, relative=zero))
    label = {"z": "|z| < 1e-12", "z_neg": "|z| < 1e-12, z < 0", "rho": "rho > 9", "u_low": "u < 0", "v_low": "v < 0", "u_high": "u >= width",
             "v_high": "v >= height"}[which]
    case.update(family="placed", edges={label: edge(dec, tg)})
    return case


def placed_gate(which):
    """chi2 around 4 (both the `< 4` of verifyMatch and the `> 4` of setBestMatch read it), negative chi2 (a U that is not positive
    definite: the truncated integer is still < 4) and the UNCERTAIN norm; uv and U are doubles, U[0][1] != U[1][0] throughout"""
    if which == "negative":
        chi = np.array([-5.0, -1.5, -1.0 - 1e-9, -1.0, -1.0 + 1e-9, -0.5])
        k = len(chi)
        U = np.tile(np.array([[-3.0, 0.0], [0.0, 1.0]]), (k, 1, 1))
        s2 = float(np.float64(0.8) * 12.0 / 12.0) ** 2
        uv = np.c_[100.0 + np.sqrt(-chi * (3.0 - s2)), np.full(k, 50.0)]
        kp = np.tile(np.array([[100.0, 50.0, 12.0]], np.float32), (k, 1))
        return {"entry": "gate", "family": "placed", "uv": uv, "U": U, "kp_b": kp, "pairs": _pairs(k),
                "edges": {"chi2 < 4 (verifyMatch)": {"decision": "gate_chi2_lt", "rows": np.arange(k), "m": np.full(k, 0.5), "side": -np.ones(k, int)}}}
    tg = targets(4.0 if which == "chi2" else 1.0, M_EXACT)
    k = len(tg)
    kp = np.c_[np.linspace(90.0, 400.0, k), np.linspace(60.0, 300.0, k), np.tile([8.0, 12.0, 16.0], k)[:k]].astype(np.float32)
    Ub = np.array([[1.1, 0.45], [0.15, 0.8]])

    def build(t):
        if which == "chi2":
            return {"entry": "gate", "uv": kp[:, :2].astype(np.float64) + np.c_[t, -0.7 * t], "U": np.tile(Ub, (k, 1, 1)), "kp_b": kp,
                    "pairs": _pairs(k)}
        return {"entry": "gate", "uv": kp[:, :2].astype(np.float64) + [0.4, -0.3], "U": Ub[None] * t[:, None, None], "kp_b": kp, "pairs": _pairs(k)}
    if which == "chi2":
        case = build(place(build, "gate_chi2_lt", tg, 0.0, 40.0, iters=80))
        # one more row with chi2 = 4 in every arithmetic: powers of two throughout (the keypoint's variance vanishes under 2^70)
        case["uv"] = np.r_[case["uv"], [[2.0 ** 36, 0.0]]]
        case["U"] = np.r_[case["U"], [[[2.0 ** 70, 0.0], [0.0, 2.0 ** 70]]]]
        case["kp_b"] = np.r_[case["kp_b"], np.array([[0.0, 0.0, 12.0]], np.float32)]
        case["pairs"] = _pairs(k + 1)
        case["exact"] = np.array([k])
        case.update(family="placed", edges={"chi2 < 4 (verifyMatch)": edge("gate_chi2_lt", tg), "chi2 > 4 (setBestMatch)": edge("gate_chi2_gt", tg)})
        return case

    def ratio(t):
        d = run(build(t))[1]["gate_norm"]
        return d["q"] / d["thr"]
    lo, hi = np.full(k, 0.0), np.full(k, 1e4)
    want = np.array([t[0] for t in tg], np.longdouble)
    for _ in range(90):
        mid = (lo + hi) / 2
        small = ratio(mid) < want
        lo, hi = np.where(small, mid, lo), np.where(small, hi, mid)
    case = build((lo + hi) / 2)
    case.update(family="placed", edges={"UNCERTAIN norm": edge("gate_norm", tg)})
    return case


# ---- the list ------------------------------------------------------------------------------------------------------------------------
STEREO_SIZES, FLAT_SIZES = (1, 63, 64, 65, 129), (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for model in (DIST_NONE, DIST_RADTAN, DIST_EQUI, DIST_RADTAN8):
        c["stereo_" + NAMES[model]] = stereo_scene(model, model, 10 + model, full=model % 2 == 1,
                                                   sigma=("none", "array", "minus", "array")[model])
    c["stereo_equi_radtan8"] = stereo_scene(DIST_EQUI, DIST_RADTAN8, 21, full=True, sigma="minus", b_other=True)
    c["stereo_radtan_none"] = stereo_scene(DIST_RADTAN, DIST_NONE, 22, full=False, sigma="none", b_other=True)
    for rows in STEREO_SIZES:
        c[f"stereo_size_{rows}"] = cut("stereo_radtan", c["stereo_radtan"], rows)
    for model in (DIST_NONE, DIST_RADTAN, DIST_EQUI, DIST_RADTAN8):
        name = "project_" + NAMES[model]
        c[name] = project_scene(model, 30 + model, width=752 if model != DIST_RADTAN else 640, height=480 if model != DIST_RADTAN else 400)
        c["gate_" + NAMES[model]] = gate_scene(c[name], 40 + model)
    for rows in FLAT_SIZES:
        c[f"project_size_{rows}"] = cut("project_radtan8", c["project_radtan8"], rows)
        c[f"gate_size_{rows}"] = cut("gate_radtan8", c["gate_radtan8"], rows)
    c["placed_chi2"] = placed_sigma("chi2")
    c["placed_cross"] = placed_sigma("cross")
    for which in ("det", "det_radtan", "errA", "errB", "chi2_own", "rB", "exit_radtan", "exit_equi"):
        c["placed_" + which] = placed_keypoint(which)
    c["placed_dot"] = placed_dot()
    c.update(placed_rank())
    for which in ("z", "z_neg", "rho", "u_low", "v_low", "u_high", "v_high"):
        c["placed_project_" + which] = placed_project(which)
    for which in ("chi2", "negative", "norm"):
        c["placed_gate_" + which] = placed_gate(which)
    return c


def names(entry=None, family=None):
    return [n for n, c in cases().items() if entry in (None, c["entry"]) and family in (None, c["family"])]


def args(case):
    """the arguments of the statement's function (tri_statement.FUNCTIONS[case["entry"]]) after the context"""
    if case["entry"] == "stereo":
        return (case["cam_a"], case["cam_b"], case["T_AB"], case["UOplus"], case["kp_a"], case["kp_b"], case["pairs"], case["sigma_ray"])
    if case["entry"] == "project":
        return (case["cam"], case["T_CbW"], case["P3"], case["hp_W"])
    return (case["uv"], case["U"], case["kp_b"], case["pairs"])


def arrays(case):
    """every input of a case as plain arrays, by name (what the golden file keeps)"""
    out = {}
    for k, v in case.items():
        if k in ("entry", "family", "edges", "parent", "rows", "exact") or v is None:
            continue
        if isinstance(v, dict):                       # a camera
            out[k] = np.r_[v["intr"], v["model"], v["width"], v["height"]]
        else:
            out[k] = np.asarray(v)
    return out


def call(fe, camera, case, gn=True, **kw):
    """the case through a Frontend-like object `fe` (`camera` builds its camera struct) -> dict of outputs named as the statement's"""
    cam = lambda c: camera(c["intr"], c["model"], c["width"], c["height"])
    if case["entry"] == "stereo":
        a = (cam(case["cam_a"]), cam(case["cam_b"]), case["T_AB"], case["UOplus"], case["kp_a"], case["kp_b"], case["pairs"], case["sigma_ray"])
        if gn and not kw:
            hp, cov, flags, g = fe.stereo_triangulate_gn(*a)
            return {"hp": hp, "cov": cov, "flags": flags, "gn": g}
        hp, cov, flags = fe.stereo_triangulate(*a, **kw)
        return {"hp": hp, "cov": cov, "flags": flags}
    if case["entry"] == "project":
        uv, U, st = fe.project_landmarks(cam(case["cam"]), case["T_CbW"], case["P3"], case["hp_W"])
        return {"uv": uv, "U": U, "status": st}
    chi2, flags = fe.gate_3d2d(case["uv"], case["U"], case["kp_b"], case["pairs"])
    return {"chi2": chi2, "flags": flags}


def in_golden(case):
    """the reference build has a triangulator for one camera geometry with a distortion, and every projection and gate"""
    if case["family"] == "size":
        return False
    if case["entry"] == "stereo":
        return case["cam_a"]["model"] == case["cam_b"]["model"] != DIST_NONE
    return True


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """the statement and its two twins on a case, computed once for every test that needs them"""
    c = cases()[name]
    return S.evaluate(S.FUNCTIONS[c["entry"]], *args(c))


def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_gate.npz"))


def recorded(name, g=None):
    """the reference build's outputs for a case, or None where the golden file has none"""
    g = g if g is not None else golden()
    keys = [k for k in g.files if k.startswith(name + "/ref/")]
    return {k.split("/")[2]: g[k] for k in keys} or None
