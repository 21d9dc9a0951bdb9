"""The referee of okvis_fe_sac_solve_absolute: the generalised three-point absolute pose solver of the 3D-2D outlier rejection,
stated from its mathematical definition (NOT pinned to OpenGV, whose source is not in the reference tree).

Convention (the consensus entry's): a hypothesis (R, t) takes a body point to the world, X = R p + t.

Definition.  Correspondence k = 0..2 of a sample: c_k its camera's offset, d_k = (its camera's rotation) (its bearing), X_k its
world point.  The candidates are all real (l0, l1, l2), every l_k > 0, with |(c_a + l_a d_a) - (c_b + l_b d_b)|^2 = |X_a - X_b|^2
for (a, b) = (0, 1), (0, 2), (1, 2).  With p_k = c_k + l_k d_k the candidate is R = a1 b1^T + a2 b2^T + a3 b3^T from the frames
(a1, a2, a3) = (u / |u|, (a1 x v) / |.|, a1 x a2), u = X_1 - X_0, v = X_2 - X_0, and (b1, b2, b3) alike from the p_k; t = X_0 - R p_0.
The hypothesis is the candidate with the smallest |reprojection - bearing|^2 of the fourth correspondence.  Invalid: |u x v| zero
or not finite, or no candidate.

gp3p(..., ctx=MP) is the statement: mpmath at DPS digits.  The resultant in l0 of the two quadrics that hold it, reduced modulo
the third to A(l1) + B(l1) l2, the octic in l1, ALL its roots through mpmath.polyroots, l2 = -A / B and l0 from the difference of
the first two quadrics (linear in l0), Newton on the three quadrics to the working precision, then the frames and the selection.
gp3p(..., ctx=NP) evaluates the same definition in float64 with numpy.roots.

Per sample: separation = the smaller of the smallest distance between the depth vectors of two real solutions and the smallest
|depth| over all real solutions (of either sign); margin = the relative gap between the best and the second-best candidate's
score on the fourth correspondence.

gp3p_near is the statement on inputs that differ from a solved sample's in the last place: Newton on the three quadrics from the
solved sample's depths at DPS digits to its fixed point, then the frames.  For a sample whose separation and margin are far above
2^-53 that is what the full evaluation returns (test_sac_abs_host checks it)."""
import mpmath as mp
import numpy as np

DPS = 60
SEPARATION_MIN, MARGIN_MIN, MAX_EXCLUDED = 1e-3, 1e-6, 0.02


class MP:
    name = "mpmath"

    @staticmethod
    def num(x):
        return mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x

    sqrt = staticmethod(mp.sqrt)

    @staticmethod
    def roots(p):          # ascending coefficients -> [(root, is real)]
        out = []
        for r in mp.polyroots(list(reversed(p)), maxsteps=500, extraprec=4 * DPS):
            real = abs(mp.im(r)) <= mp.mpf(10) ** (-DPS // 2) * max(1, abs(r))
            out.append((mp.re(r) if real else r, real))
        return out


class NP:
    name = "numpy"
    num = staticmethod(np.float64)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def roots(p):
        return [(r.real if r.imag == 0.0 else r, r.imag == 0.0) for r in np.roots(np.array(list(reversed(p)), np.float64))]


# ---- polynomials in one variable as ascending lists; the coefficients are numbers of either arithmetic, or numpy arrays ------------------
def _mul(p, q):
    r = [0 * p[0]] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            r[i + j] = r[i + j] + a * b
    return r


def _add(p, q, s=1):
    n = max(len(p), len(q))
    zero = 0 * p[0]
    return [(p[i] if i < len(p) else zero) + s * (q[i] if i < len(q) else zero) for i in range(n)]


def _eval(p, x):
    s = p[-1]
    for c in reversed(p[:-1]):
        s = s * x + c
    return s


# polynomials in (x, y) as lists over the powers of y of polynomials in x
def _mul2(P, Q):
    R = [None] * (len(P) + len(Q) - 1)
    for i, a in enumerate(P):
        for j, b in enumerate(Q):
            R[i + j] = _mul(a, b) if R[i + j] is None else _add(R[i + j], _mul(a, b))
    return R


def _add2(P, Q, s=1):
    zero = [0 * P[0][0]]
    return [_add(P[i] if i < len(P) else zero, Q[i] if i < len(Q) else zero, s) for i in range(max(len(P), len(Q)))]


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _sub(u, v):
    return [u[0] - v[0], u[1] - v[1], u[2] - v[2]]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def quadric(ca, da, Xa, cb, db, Xb):
    """(la^2, lb^2, la lb, la, lb, 1) of |(ca + la da) - (cb + lb db)|^2 - |Xa - Xb|^2"""
    w, D = _sub(ca, cb), _sub(Xa, Xb)
    return [_dot(da, da), _dot(db, db), -2 * _dot(da, db), 2 * _dot(da, w), -2 * _dot(db, w), _dot(w, w) - _dot(D, D)]


def elimination(q01, q02, q12):
    """-> (octic in l1, A, B, the linear equation of l0: (n0(x), n1(y), m0(x), m1(y)) with l0 = -(n0 + n1) / (m0 + m1))"""
    a, b, c = q01[0], [q01[3], q01[2]], [q01[5], q01[4], q01[1]]          # in l0, over x = l1
    a_, b_, c_ = q02[0], [q02[3], q02[2]], [q02[5], q02[4], q02[1]]        # in l0, over y = l2
    inx = lambda p: [p]                                     # a polynomial in x as one in (x, y)
    iny = lambda p: [[v] for v in p]                        # a polynomial in y
    sc = lambda s, p: [s * v for v in p]
    u = _add2(iny(sc(a, c_)), inx(sc(a_, c)), -1)
    v = _add2(iny(sc(a, b_)), inx(sc(a_, b)), -1)
    z = _add2(_mul2(inx(b), iny(c_)), _mul2(iny(b_), inx(c)), -1)
    G = _add2(_mul2(u, u), _mul2(v, z), -1)
    g = [G[j] if j < len(G) else [0 * a] for j in range(5)]
    e, l, k = q12[1], [q12[4], q12[2]], [q12[5], q12[3], q12[0]]
    m1, m0 = sc(-1 / e, l), sc(-1 / e, k)
    s = _add(_mul(m1, m1), m0)
    m1m0 = _mul(m1, m0)
    t3, t4 = _add(_mul(s, m1), m1m0), _mul(s, m0)
    A = _add(_add(_add(g[0], _mul(g[2], m0)), _mul(g[3], m1m0)), _mul(g[4], t4))
    B = _add(_add(_add(g[1], _mul(g[2], m1)), _mul(g[3], s)), _mul(g[4], t3))
    P = _add(_add(sc(e, _mul(A, A)), _mul(l, _mul(A, B)), -1), _mul(k, _mul(B, B)))
    # a' f01 - a f02 = (a' b - a b') l0 + (a' c - a c')
    return P[:9], A, B, (sc(a_, c), sc(-a, c_), sc(a_, b), sc(-a, b_))


def residual(c, d, X, lam):
    """the three quadrics in their geometric form and their Jacobian"""
    p = [[c[k][e] + lam[k] * d[k][e] for e in range(3)] for k in range(3)]
    F, J = [], []
    for a, b in ((0, 1), (0, 2), (1, 2)):
        r, D = _sub(p[a], p[b]), _sub(X[a], X[b])
        F.append(_dot(r, r) - _dot(D, D))
        row = [0 * lam[0]] * 3
        row[a], row[b] = 2 * _dot(r, d[a]), -2 * _dot(r, d[b])
        J.append(row)
    return F, J


def newton(ctx, c, d, X, lam, steps):
    for _ in range(steps):
        F, J = residual(c, d, X, lam)
        if ctx is MP:
            delta = mp.lu_solve(mp.matrix(J), -mp.matrix(F))
            lam = [lam[k] + delta[k] for k in range(3)]
        else:
            lam = list(np.array(lam) + np.linalg.solve(np.array(J, np.float64), -np.array(F, np.float64)))
    return lam


def frame(ctx, P):
    """(a1, a2, a3) of the triangle P [3][3], or None"""
    u, v = _sub(P[1], P[0]), _sub(P[2], P[0])
    n = ctx.sqrt(_dot(u, u))
    if not n > 0:
        return None
    a1 = [x / n for x in u]
    w = _cross(a1, v)
    n = ctx.sqrt(_dot(w, w))
    if not n > 0:
        return None
    a2 = [x / n for x in w]
    return a1, a2, _cross(a1, a2)


def transformation(ctx, c, d, X, lam):
    """(R, t) of the depths lam, or None"""
    p = [[c[k][e] + lam[k] * d[k][e] for e in range(3)] for k in range(3)]
    fa, fb = frame(ctx, X), frame(ctx, p)
    if fa is None or fb is None:
        return None
    R = [[sum(fa[i][r] * fb[i][col] for i in range(3)) for col in range(3)] for r in range(3)]
    return R, [X[0][r] - _dot(R[r], p[0]) for r in range(3)]


def fourth_score(ctx, R, t, X3, f3, c3, C3):
    """|reprojection - bearing|^2 of the fourth correspondence: the absolute score of okvis_fe_sac_consensus without sigma"""
    g = _sub(X3, t)
    body = [sum(R[j][k] * g[j] for j in range(3)) for k in range(3)]          # R^T (X - t)
    dd = _sub(body, c3)
    r = [sum(C3[j][k] * dd[j] for j in range(3)) for k in range(3)]           # C^T (body - c)
    n = ctx.sqrt(_dot(r, r))
    e = [r[k] / n - f3[k] for k in range(3)]
    return _dot(e, e)


def _inputs(ctx, points, bearing, offsets, rotations):
    num = ctx.num
    X = [[num(v) for v in row] for row in np.asarray(points, np.float64).reshape(4, 3)]
    f = [[num(v) for v in row] for row in np.asarray(bearing, np.float64).reshape(4, 3)]
    c = [[num(v) for v in row] for row in np.asarray(offsets, np.float64).reshape(4, 3)]
    C = [[[num(v) for v in row] for row in M] for M in np.asarray(rotations, np.float64).reshape(4, 3, 3)]
    d = [[_dot(C[k][r], f[k]) for r in range(3)] for k in range(4)]
    return X, f, c, C, d


def _floats(R, t):
    return np.array([[float(x) for x in row] for row in R]), np.array([float(x) for x in t])


def gp3p(points, bearing, offsets, rotations, ctx=MP):
    """points, bearing, offsets [4][3], rotations [4][3][3]: the sample's world points and bearing vectors with the offset and
    rotation of each one's camera (the first three define the candidates, the fourth picks).
    -> dict: valid, R [3][3], t [3] (float64 arrays, NaN when invalid), n_roots (candidates), candidates [n_roots][3][4], n_real
    (real solutions of either sign), separation, margin, and `exact`: the depths of the choice in the arithmetic of ctx."""
    if ctx is MP:
        mp.mp.dps = DPS
    X, f, c, C, d = _inputs(ctx, points, bearing, offsets, rotations)
    res = {"valid": False, "R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "n_roots": 0, "candidates": np.zeros((0, 3, 4)),
           "n_real": 0, "separation": np.inf, "margin": np.inf, "exact": None}
    w = _cross(_sub(X[1], X[0]), _sub(X[2], X[0]))
    nn = float(ctx.sqrt(_dot(w, w)))
    if not (nn > 0.0 and np.isfinite(nn)):
        return res
    q01, q02, q12 = (quadric(c[a], d[a], X[a], c[b], d[b], X[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    P, A, B, (n0, n1, m0, m1) = elimination(q01, q02, q12)
    sols = []
    for x, real in ctx.roots(P):
        if not real:
            continue
        try:
            with np.errstate(all="ignore"):
                y = -_eval(A, x) / _eval(B, x)
                l0 = -(_eval(n0, x) + _eval(n1, y)) / (_eval(m0, x) + _eval(m1, y))
                lam = newton(ctx, c, d, X, [l0, x, y], 4)
        except (ZeroDivisionError, np.linalg.LinAlgError):
            continue
        if all(np.isfinite(float(v)) for v in lam):
            sols.append(lam)
    res["n_real"] = len(sols)
    sep = np.inf
    for i, u in enumerate(sols):
        sep = min(sep, min(abs(float(v)) for v in u))
        for v in sols[i + 1:]:
            sep = min(sep, float(ctx.sqrt(sum((u[k] - v[k]) ** 2 for k in range(3)))))
    res["separation"] = sep
    cands = []
    for lam in sols:
        if not all(v > 0 for v in lam):
            continue
        T = transformation(ctx, c, d, X, lam)
        if T is not None:
            cands.append((fourth_score(ctx, T[0], T[1], X[3], f[3], c[3], C[3]), T[0], T[1], lam))
    res["n_roots"] = len(cands)
    if cands:
        res["candidates"] = np.array([np.concatenate([_floats(R, t)[0], _floats(R, t)[1][:, None]], axis=1) for _, R, t, _ in cands])
        cands.sort(key=lambda cand: cand[0])
        score, R, t, lam = cands[0]
        res["valid"] = True
        res["R"], res["t"] = _floats(R, t)
        res["exact"] = lam
        if len(cands) > 1:
            second = cands[1][0]
            res["margin"] = float((second - score) / second) if second > 0 else 0.0
    return res


def gp3p_near(points, bearing, offsets, rotations, base):
    """the statement's (R, t) on inputs within rounding of those `base` (a gp3p(..., ctx=MP) result) was solved for"""
    mp.mp.dps = DPS
    X, f, c, C, d = _inputs(MP, points, bearing, offsets, rotations)
    lam = newton(MP, c, d, X, list(base["exact"]), 6)          # quadratic from 1e-16: 1e-32, 1e-64, then the working precision
    return _floats(*transformation(MP, c, d, X, lam))


# ---- float64, vectorised over many samples ------------------------------------------------------------------------------------------
def count_candidates(X, c, d):
    """X, c, d [N][3][3] -> (real solutions of either sign, candidates = real solutions with three positive depths) per sample,
    float64: the same elimination with arrays for coefficients, the roots as eigenvalues of the companion matrices"""
    vec = lambda a, k: [a[:, k, 0], a[:, k, 1], a[:, k, 2]]
    q = [quadric(vec(c, a), vec(d, a), vec(X, a), vec(c, b), vec(d, b), vec(X, b)) for a, b in ((0, 1), (0, 2), (1, 2))]
    P, A, B, (n0, n1, m0, m1) = elimination(*q)
    P = np.stack(P, axis=1)
    N = len(P)
    M = np.zeros((N, 8, 8))
    M[:, 0, :] = -P[:, 7::-1] / P[:, 8:9]
    M[:, np.arange(1, 8), np.arange(0, 7)] = 1.0
    roots = np.linalg.eigvals(M)
    real = roots.imag == 0.0
    x = roots.real
    with np.errstate(all="ignore"):
        ev = lambda p, v: _eval([np.asarray(k)[:, None] if np.ndim(k) else k for k in p], v)
        y = -ev(A, x) / ev(B, x)
        l0 = -(ev(n0, x) + ev(n1, y)) / (ev(m0, x) + ev(m1, y))
        pos = real & (x > 0) & (y > 0) & (l0 > 0)
    return real.sum(axis=1), pos.sum(axis=1)


def score_absolute(R, t, points, bearing, cam_index, offsets, rotations):
    """float64: |reprojection - bearing|^2 of all correspondences [n] under (R, t) (divide by sigma for the consensus score)"""
    body = (points - t) @ R                                     # R^T (X - t)
    dd = body - offsets[cam_index]
    r = np.einsum("njk,nj->nk", rotations[cam_index], dd)       # C^T (body - c)
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    return ((r - bearing) ** 2).sum(axis=1)


def pose_distance(R, t, R0, t0):
    """max(|R - R0|_F, |t - t0|)"""
    return max(float(np.linalg.norm(np.asarray(R) - np.asarray(R0))), float(np.linalg.norm(np.asarray(t) - np.asarray(t0))))


def excluded(st):
    return st["separation"] < SEPARATION_MIN or st["margin"] < MARGIN_MIN
