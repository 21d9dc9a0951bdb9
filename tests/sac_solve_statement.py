"""The referee of okvis_fe_sac_solve: the two minimal solvers of the 2D-2D outlier rejection, stated from their published
definitions (NOT pinned to OpenGV, whose source is not in the reference tree).

Convention: a point of frame 2 is R12 p2 + t12 in frame 1; R f2 ~ f1; f1^T E f2 = 0 with E = [t12]x R12.

five_point(..., ctx=MP) is the statement: mpmath at DPS digits.  Null space of the 5x9 epipolar matrix, the ten cubics
(det E = 0, 2 E E^T E - tr(E E^T) E = 0) expanded in E = x X + y Y + z Z + W, elimination to the 10x10 action matrix of
"multiply by x" on the quotient ring's basis (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1), its eigenvalues and eigenvectors through
mpmath's general eigen solver, the four decompositions of every real root from its singular vectors, and the selection over all
eight correspondences.  five_point(..., ctx=NP) evaluates the same definition in float64 with numpy.linalg.svd / eig / solve.

Per sample: separation = the smaller of the least |Im| among the complex eigenvalues and the least gap between consecutive real
ones, relative to max(1, |root|); margin = the relative gap between the best and the second-best passing candidate's score sum.

five_point_near is the statement on bearings that differ from a solved sample's in the last place: the same root and the same
decomposition, followed by Newton on the definition at DPS digits to its fixed point.  For a sample whose margin is far above
2^-53 that is what the full evaluation returns (test_sac_solve_host checks it), at a fiftieth of the cost.

two_point is the rotation-only statement, operation for operation in float64."""
import itertools

import mpmath as mp
import numpy as np

DPS = 60
SEPARATION_MIN, MARGIN_MIN, MAX_EXCLUDED = 1e-3, 1e-6, 0.02

# monomials of degree three in (x, y, z, 1) = variables (0, 1, 2, 3), graded: the ten cubic ones, then the basis of the quotient ring
MONO = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (0, 2, 2), (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 2, 2),
        (0, 0, 3), (0, 1, 3), (0, 2, 3), (1, 1, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]
# x times basis monomial i: ("row", k) = cubic monomial k, to be reduced; ("unit", j) = basis monomial j
X_TIMES = [("row", 0), ("row", 1), ("row", 2), ("row", 3), ("row", 4), ("row", 5), ("unit", 0), ("unit", 1), ("unit", 2), ("unit", 6)]


class MP:
    name = "mpmath"

    @staticmethod
    def num(x):
        return mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x

    sqrt = staticmethod(mp.sqrt)

    @staticmethod
    def null_space(A):          # rows of a 4x9: the last columns of Q in A^T = Q R
        Q, _ = mp.qr(mp.matrix(A).T)
        return [[Q[e, 5 + i] for e in range(9)] for i in range(4)]

    @staticmethod
    def solve(M1, M2):
        X = mp.inverse(mp.matrix(M1)) * mp.matrix(M2)
        return [[X[i, j] for j in range(X.cols)] for i in range(X.rows)]

    @staticmethod
    def eig(A):
        vals, vecs = mp.eig(mp.matrix(A))
        out = []
        for k, lam in enumerate(vals):
            real = abs(mp.im(lam)) <= mp.mpf(10) ** (-DPS // 2) * max(1, abs(lam))
            v = [vecs[i, k] / vecs[9, k] for i in range(10)] if real else None
            out.append((lam, real, None if v is None else [mp.re(v[6]), mp.re(v[7]), mp.re(v[8])]))
        return out

    @staticmethod
    def svd3(E):
        U, S, V = mp.svd_r(mp.matrix(E))
        return [[U[i, j] for j in range(3)] for i in range(3)], [[V[i, j] for j in range(3)] for i in range(3)]


class NP:
    name = "numpy"
    num = staticmethod(np.float64)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def null_space(A):
        return np.linalg.svd(np.array(A, np.float64))[2][5:].tolist()

    @staticmethod
    def solve(M1, M2):
        return np.linalg.solve(np.array(M1, np.float64), np.array(M2, np.float64)).tolist()

    @staticmethod
    def eig(A):
        vals, vecs = np.linalg.eig(np.array(A, np.float64))
        out = []
        for k, lam in enumerate(vals):
            real = lam.imag == 0.0
            v = (vecs[:, k] / vecs[9, k]).real if real else None
            out.append((lam, real, None if v is None else [v[6], v[7], v[8]]))
        return out

    @staticmethod
    def svd3(E):
        U, _, Vt = np.linalg.svd(np.array(E, np.float64))
        return U.tolist(), Vt.tolist()


# ---- polynomials in four variables as {sorted tuple of variables: coefficient} ---------------------------------------------------------
def _padd(p, q, s=1):
    r = dict(p)
    for k, v in q.items():
        r[k] = r[k] + s * v if k in r else s * v
    return r


def _pmul(p, q):
    r = {}
    for (k1, v1), (k2, v2) in itertools.product(p.items(), q.items()):
        k = tuple(sorted(k1 + k2))
        r[k] = r[k] + v1 * v2 if k in r else v1 * v2
    return r


def _pscale(p, s):
    return {k: s * v for k, v in p.items()}


def cubics(B, half):
    """the 10x20 coefficient matrix of the ten cubics in the order of MONO; B: the four basis matrices as rows of 9"""
    E = [[{(i,): B[i][3 * r + c] for i in range(4)} for c in range(3)] for r in range(3)]
    EEt = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for k in range(3):
            s = {}
            for m in range(3):
                s = _padd(s, _pmul(E[r][m], E[k][m]))
            EEt[r][k] = s
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    eqs = []
    for r in range(3):
        for c in range(3):
            s = {}
            for k in range(3):
                lam = _padd(EEt[r][k], _pscale(tr, half), -1) if k == r else EEt[r][k]
                s = _padd(s, _pmul(lam, E[k][c]))
            eqs.append(s)
    det = {}
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        minor = _padd(_pmul(E[1][b], E[2][c]), _pmul(E[1][c], E[2][b]), -1)
        det = _padd(det, _pmul(E[0][a], minor))
    eqs.append(det)
    return [[eq[m] for m in MONO] for eq in eqs]


# ---- geometry in either arithmetic -------------------------------------------------------------------------------------------------
def _matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _T(A):
    return [list(r) for r in zip(*A)]


def _det3(A):
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
            + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def rays_and_score(ctx, R, t, f1, f2, s1, s2):
    """the two ray parameters of the two-view midpoint method and the relative-pose score (fe_sac.hpp: sac_midpoint,
    sac_score_relative), as mathematics"""
    g = [_dot(R[k], f2) for k in range(3)]
    b0, b1 = _dot(t, f1), _dot(t, g)
    a00, a10, a11 = _dot(f1, f1), _dot(f1, g), -_dot(g, g)
    a01 = -a10
    det = a00 * a11 - a01 * a10
    l0, l1 = (a11 * b0 - a01 * b1) / det, (a00 * b1 - a10 * b0) / det
    p = [(l0 * f1[k] + t[k] + l1 * g[k]) / 2 for k in range(3)]
    d = [p[k] - t[k] for k in range(3)]
    q = [sum(R[j][k] * d[j] for j in range(3)) for k in range(3)]
    pn, qn = ctx.sqrt(_dot(p, p)), ctx.sqrt(_dot(q, q))
    e1 = [p[k] / pn - f1[k] for k in range(3)]
    e2 = [q[k] / qn - f2[k] for k in range(3)]
    return l0, l1, _dot(e1, e1) / (2 * s1) + _dot(e2, e2) / (2 * s2)


def decompositions(ctx, E):
    """the four (R, t) of an essential matrix from its singular vectors: R = U W V^T, U W^T V^T with det +1, t = +-u3"""
    U, Vt = ctx.svd3(E)
    one, zero = ctx.num(1), ctx.num(0)
    W = [[zero, -one, zero], [one, zero, zero], [zero, zero, one]]
    t = [U[k][2] for k in range(3)]
    n = ctx.sqrt(_dot(t, t))
    t = [x / n for x in t]
    out = []
    for Wk in (W, _T(W)):
        R = _matmul(_matmul(U, Wk), Vt)
        if _det3(R) < 0:
            R = [[-x for x in row] for row in R]
        for sg in (1, -1):
            out.append((R, [sg * x for x in t]))
    return out


def five_point(f1, f2, sigma1=None, sigma2=None, ctx=MP):
    """f1, f2 [8][3]: the sample's bearing vectors (the first five define E); sigma1, sigma2 [8] or None (= 1).
    -> dict: valid, R [3][3], t [3] (float64 arrays, NaN when invalid), n_roots, essentials [n_roots][9] (unit norm), separation,
    margin, and `exact`: R, t, E of the choice in the arithmetic of ctx (for five_point_near)."""
    if ctx is MP:
        mp.mp.dps = DPS
    num = ctx.num
    f1 = [[num(x) for x in row] for row in np.asarray(f1, np.float64).reshape(8, 3)]
    f2 = [[num(x) for x in row] for row in np.asarray(f2, np.float64).reshape(8, 3)]
    s1 = [num(1.0 if sigma1 is None else sigma1[k]) for k in range(8)]
    s2 = [num(1.0 if sigma2 is None else sigma2[k]) for k in range(8)]
    A = [[f1[k][r] * f2[k][c] for r in range(3) for c in range(3)] for k in range(5)]
    B = ctx.null_space(A)
    M = cubics(B, num(0.5))
    Bm = ctx.solve([row[:10] for row in M], [row[10:] for row in M])
    zero, one = num(0), num(1)
    At = []
    for what, k in X_TIMES:
        At.append([-x for x in Bm[k]] if what == "row" else [one if j == k else zero for j in range(10)])
    roots = ctx.eig(At)
    reals = sorted([r for r in roots if r[1]], key=lambda r: float(mp.re(r[0]) if ctx is MP else r[0].real))
    sep = np.inf
    for lam, real, _ in roots:
        if not real:
            sep = min(sep, float(abs(lam.imag) / max(1, abs(lam))))
    vals = [mp.re(r[0]) if ctx is MP else r[0].real for r in reals]
    for u, v in zip(vals[:-1], vals[1:]):
        sep = min(sep, float((v - u) / max(1, abs(u), abs(v))))
    essentials, cands = [], []
    for _, _, (x, y, z) in reals:
        E = [x * B[0][e] + y * B[1][e] + z * B[2][e] + B[3][e] for e in range(9)]
        n = ctx.sqrt(sum(e * e for e in E))
        E = [e / n for e in E]
        essentials.append(E)
        E3 = [E[0:3], E[3:6], E[6:9]]
        for R, t in decompositions(ctx, E3):
            ok, total = True, zero
            for k in range(8):
                l0, l1, s = rays_and_score(ctx, R, t, f1[k], f2[k], s1[k], s2[k])
                ok = ok and l0 > 0 and l1 > 0
                total = total + s
            if ok:
                cands.append((total, R, t, E3))
    res = {"n_roots": len(reals), "essentials": np.array([[float(e) for e in E] for E in essentials]).reshape(-1, 9), "separation": sep,
           "valid": bool(cands), "R": np.full((3, 3), np.nan), "t": np.full(3, np.nan), "margin": np.inf, "exact": None}
    if cands:
        cands.sort(key=lambda c: c[0])
        total, R, t, E3 = cands[0]
        res["R"], res["t"] = np.array([[float(x) for x in row] for row in R]), np.array([float(x) for x in t])
        res["exact"] = (R, t, E3)
        if len(cands) > 1:
            second = cands[1][0]
            res["margin"] = float((second - total) / second) if second > 0 else 0.0
    return res


def _residual_and_jacobian(B, c):
    """the ten cubics at E = sum c_i B_i (mpmath) and their derivatives along the basis: 10-vector, 10x4"""
    E = mp.matrix(3, 3)
    for e in range(9):
        E[e // 3, e % 3] = sum(c[i] * B[i][e] for i in range(4))
    H, G = E * E.T, E.T * E
    half_tr = (H[0, 0] + H[1, 1] + H[2, 2]) / 2
    K = mp.matrix(3, 3)
    for r in range(3):
        for q in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (q + 1) % 3, (q + 2) % 3
            K[r, q] = E[r1, c1] * E[r2, c2] - E[r1, c2] * E[r2, c1]
    Rm = (H - half_tr * mp.eye(3)) * E
    res = [Rm[e // 3, e % 3] for e in range(9)] + [sum(E[0, q] * K[0, q] for q in range(3))]
    J = mp.matrix(10, 4)
    for i in range(4):
        D = mp.matrix(3, 3)
        for e in range(9):
            D[e // 3, e % 3] = B[i][e]
        tr = sum(E[a, b] * D[a, b] for a in range(3) for b in range(3))
        dR = D * G + E * (D.T * E) + H * D - tr * E - half_tr * D
        for e in range(9):
            J[e, i] = dR[e // 3, e % 3]
        J[9, i] = sum(K[a, b] * D[a, b] for a in range(3) for b in range(3))
    return mp.matrix(res), J


def five_point_near(f1, f2, base):
    """the statement's (R, t) on bearings within rounding of those `base` (a five_point(..., ctx=MP) result) was solved for:
    the root of `base` followed into the new null space by Newton on the ten cubics, and the decomposition of `base`'s kind"""
    mp.mp.dps = DPS
    R0, t0, E0 = base["exact"]
    f1 = [[MP.num(x) for x in row] for row in np.asarray(f1, np.float64).reshape(8, 3)]
    f2 = [[MP.num(x) for x in row] for row in np.asarray(f2, np.float64).reshape(8, 3)]
    A = [[f1[k][r] * f2[k][c] for r in range(3) for c in range(3)] for k in range(5)]
    B = MP.null_space(A)
    flat = [E0[r][c] for r in range(3) for c in range(3)]
    c = mp.matrix([sum(B[i][e] * flat[e] for e in range(9)) for i in range(4)])
    c = c / mp.norm(c)
    for _ in range(6):      # quadratic from 1e-16: 1e-32, 1e-64, then the working precision
        res, J = _residual_and_jacobian(B, c)
        N = J.T * J + c * c.T
        c = c + mp.lu_solve(N, -(J.T * res))
        c = c / mp.norm(c)
    E = [sum(c[i] * B[i][e] for i in range(4)) for e in range(9)]
    best = None
    for R, t in decompositions(MP, [E[0:3], E[3:6], E[6:9]]):
        d = max(mp.sqrt(sum((R[i][j] - R0[i][j]) ** 2 for i in range(3) for j in range(3))), mp.sqrt(sum((t[i] - t0[i]) ** 2 for i in range(3))))
        if best is None or d < best[0]:
            best = (d, R, t)
    return np.array([[float(x) for x in row] for row in best[1]]), np.array([float(x) for x in best[2]])


# ---- a vectorised float64 root count, for searching many samples --------------------------------------------------------------------
def _tables():
    i2 = {}
    for i in range(4):
        for j in range(i, 4):
            i2[(i, j)] = len(i2)
    P2, P3 = np.zeros((4, 4, 10)), np.zeros((10, 4, 20))
    for i in range(4):
        for j in range(4):
            P2[i, j, i2[tuple(sorted((i, j)))]] = 1.0
    for (i, j), m in i2.items():
        for k in range(4):
            P3[m, k, MONO.index(tuple(sorted((i, j, k))))] = 1.0
    return P2, P3


def count_real_roots(f1, f2):
    """f1, f2 [N][5][3] -> the number of real roots of each sample, float64: the same definition through batched einsum products,
    numpy.linalg.svd, solve and eigvals"""
    P2, P3 = _tables()
    A = np.einsum("nkr,nkc->nkrc", f1, f2).reshape(len(f1), 5, 9)
    L = np.linalg.svd(A)[2][:, 5:, :].reshape(-1, 4, 3, 3).transpose(0, 2, 3, 1)          # [N][r][c][i]
    EEt = np.einsum("nrmi,nkmj,ijp->nrkp", L, L, P2)
    tr = EEt[:, 0, 0] + EEt[:, 1, 1] + EEt[:, 2, 2]
    lam = EEt - 0.5 * np.einsum("rk,np->nrkp", np.eye(3), tr)
    eq = np.einsum("nrkp,nkcl,plq->nrcq", lam, L, P3).reshape(len(f1), 9, 20)
    det = np.zeros((len(f1), 20))
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        minor = np.einsum("ni,nj,ijp->np", L[:, 1, b], L[:, 2, c], P2) - np.einsum("ni,nj,ijp->np", L[:, 1, c], L[:, 2, b], P2)
        det += np.einsum("np,nl,plq->nq", minor, L[:, 0, a], P3)
    M = np.concatenate([eq, det[:, None, :]], axis=1)
    Bm = np.linalg.solve(M[:, :, :10], M[:, :, 10:])
    At = np.zeros((len(f1), 10, 10))
    for i, (what, k) in enumerate(X_TIMES):
        if what == "row":
            At[:, i, :] = -Bm[:, k, :]
        else:
            At[:, i, k] = 1.0
    return (np.linalg.eigvals(At).imag == 0.0).sum(axis=1)


def score_relative(R, t, f1, f2, s1, s2):
    """float64: the relative-pose scores of all correspondences [n] under (R, t)"""
    return np.array([float(rays_and_score(NP, R.tolist(), list(t), f1[k], f2[k], s1[k], s2[k])[2]) for k in range(len(f1))])


def score_rotation_only(R, f1, f2, s1, s2):
    e1, e2 = f2 @ R.T - f1, f1 @ R - f2
    return (e1 * e1).sum(axis=1) * 0.5 / s1 + (e2 * e2).sum(axis=1) * 0.5 / s2


def pose_distance(R, t, R0, t0):
    """max(|R - R0|_F, |t - t0|)"""
    return max(float(np.linalg.norm(np.asarray(R) - np.asarray(R0))), float(np.linalg.norm(np.asarray(t) - np.asarray(t0))))


def excluded(st):
    return st["separation"] < SEPARATION_MIN or st["margin"] < MARGIN_MIN


# ---- two points -------------------------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def _frame(fi, fj):
    c = _cross(fi, fj)
    n = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not (n > 0.0) or not np.isfinite(n):
        return None
    a2 = np.array([c[0] / n, c[1] / n, c[2] / n])
    return a2, _cross(fi, a2)


def two_point(bearing1, bearing2, i, j):
    """-> (R [3][3], valid); R all NaN when invalid.  float64, every product and sum rounded on its own, in the order of the
    header's statement."""
    with np.errstate(all="ignore"):
        f1i, f1j, f2i, f2j = (np.asarray(x, np.float64) for x in (bearing1[i], bearing1[j], bearing2[i], bearing2[j]))
        a = _frame(f1i, f1j) if i != j else None
        b = _frame(f2i, f2j) if i != j else None
        if a is None or b is None:
            return np.full((3, 3), np.nan), False
        R = np.empty((3, 3))
        for r in range(3):
            for c in range(3):
                R[r, c] = (f1i[r] * f2i[c] + a[0][r] * b[0][c]) + a[1][r] * b[1][c]
        return R, True
