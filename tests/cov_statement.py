"""An independent statement of the marginal state covariance — TEST INFRASTRUCTURE, host only (numpy, scipy, mpmath).

    S0      = U - sum_l W_l V_l^-1 W_l^T          (tests/schur_statement.reduce with lam = 0, Dp2 = 0, Dl2 = 0, long double)
    Sigma_K = rows and columns K of S0^-1

The reference inverse X* is mpmath's at 60 digits of a matrix given exactly: every long double entry as the sum of two doubles.
A full 60-digit inverse of a 174 x 174 matrix takes mpmath 20 s, so X* is formed for a set of columns C only (Cholesky once, one
pair of triangular solves per column): the C x C block of the inverse, C the union of the rows any selection of the case names.
Every distance below is taken on such a block,

    e(X, X*) = max_ij |X_ij - X*_ij| / sqrt(X*_ii X*_jj) .
"""
from __future__ import annotations

import numpy as np

from . import schur_statement as stmt

DIGITS = 60
INPUTS = ("HPP", "GRADIENT", "LM_V", "LM_B", "PAIR_W")


def offsets(w):
    """(reduced offset of every pose-type block, of every speed/bias block, D); -1 for a fixed block"""
    po = stmt.pose_offsets(w)
    Dp = 6 * int((po >= 0).sum())
    free = np.asarray(w.sb_fixed).reshape(-1) == 0
    so = np.full(free.size, -1, np.int64)
    so[free] = Dp + 9 * np.arange(int(free.sum()))
    return po, so, Dp + 9 * int(free.sum())


def rows_of(w, blocks):
    """the reduced rows of a list of (block type, index) pairs, in list order"""
    po, so, _ = offsets(w)
    out = []
    for t, i in blocks:
        off = int(po[i] if t == 0 else so[i])
        assert off >= 0, "a fixed block"
        out += list(range(off, off + (6 if t == 0 else 9)))
    return np.array(out, np.int64)


def linearized(oracle, w, extended=False, optimize=0):
    """the arrays of the oracle (fp64 or long double build) linearised at the uploaded state or after optimize(n)"""
    o = oracle.OracleWindow(w, extended=extended)
    if optimize:
        o.optimize(optimize)
    o.linearize()
    lin = {a: o.array(a) for a in INPUTS}
    lin["pairs"] = o.pairs()
    lin["D"] = o.D
    return lin


def S0_of(w, lin, lam=0.0, vinv_of=None):
    """S0 in long double.  lam: damping added the way the first dogleg solve would (a mutation); vinv_of(l, V) -> a 3 x 3 that
    replaces V_l^-1 for landmark l, or None (a mutation)."""
    D = lin["D"]
    U = np.asarray(lin["HPP"]).reshape(D, D)
    assert np.array_equal(U, U.T)
    off = stmt.pose_offsets(w)
    n_lm = np.asarray(lin["LM_V"]).reshape(-1, 6).shape[0]
    T = np.longdouble
    if lam == 0.0 and vinv_of is None:
        S, _ = stmt.reduce(U, lin["GRADIENT"], lin["LM_V"], lin["LM_B"], lin["PAIR_W"], lin["pairs"][0], lin["pairs"][1], off,
                           lam=0.0, Dp2=np.zeros(D), Dl2=np.zeros((n_lm, 3)), dtype=T)
        return (S + S.T) / T(2)      # (a landmark's product Y W^T is symmetric only up to rounding)
    Dp2 = np.diag(U).copy()
    Dl2 = np.asarray(lin["LM_V"]).reshape(-1, 6)[:, [0, 3, 5]].copy()
    S = U.astype(T)
    S[np.arange(D), np.arange(D)] += T(lam) * Dp2.astype(T)
    for l, rows, Wl, Vi, _, _, Vd in stmt._landmark_terms(lin["LM_V"], lin["LM_B"], lin["PAIR_W"], lin["pairs"][0], lin["pairs"][1], off,
                                                           lam, Dl2, T, None):
        alt = vinv_of(l, np.asarray(Vd, np.float64)) if vinv_of is not None else None
        if alt is not None:
            Vi = np.asarray(alt).astype(T)
        S[np.ix_(rows, rows)] -= (Wl @ Vi) @ Wl.T
    return (S + S.T) / T(2)


def pinv_rank2(V):
    """the pseudo-inverse of V with its smallest eigenvalue set to zero: what a rule that truncates a weak direction would use"""
    lam, Q = np.linalg.eigh(V)
    lam[0] = 0.0
    return np.linalg.pinv((Q * lam) @ Q.T, rcond=1e-12, hermitian=True)


def two_doubles(S):
    """a long double matrix as (hi, lo) doubles with hi + lo == S exactly (64-bit mantissa <= 2 x 53)"""
    S = np.asarray(S, np.longdouble)
    hi = S.astype(np.float64)
    lo = (S - hi.astype(np.longdouble)).astype(np.float64)
    assert np.array_equal(hi.astype(np.longdouble) + lo.astype(np.longdouble), S)
    return hi, lo


def inverse_block_mp(S, cols):
    """the cols x cols block of the inverse of S (long double or double, symmetric positive definite) by mpmath at DIGITS digits,
    rounded to double"""
    import mpmath as mp
    hi, lo = two_doubles(S)
    n = hi.shape[0]
    cols = [int(c) for c in cols]
    with mp.workdps(DIGITS):
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpf(float(hi[i, j])) + mp.mpf(float(lo[i, j]))
        Lm = mp.cholesky(M)
        L = [[Lm[i, k] for k in range(i + 1)] for i in range(n)]           # rows of L
        Lt = [[L[i][k] for i in range(k, n)] for k in range(n)]            # columns of L from the diagonal down
        out = np.zeros((len(cols), len(cols)))
        for b, c in enumerate(cols):
            y = [mp.mpf(0)] * n
            y[c] = 1 / L[c][c]
            for i in range(c + 1, n):
                y[i] = -mp.fdot(L[i][c:i], y[c:i]) / L[i][i]
            x = [mp.mpf(0)] * n
            for i in range(n - 1, c - 1, -1):          # (rows below c come from the columns before, by symmetry)
                x[i] = (y[i] - mp.fdot(Lt[i][1:], x[i + 1:])) / L[i][i]
            for a, r in enumerate(cols):
                if r >= c:
                    out[a, b] = out[b, a] = float(x[r])
    return out


def e(X, Xs):
    """the error measure of the module docstring"""
    X, Xs = np.asarray(X, np.float64), np.asarray(Xs, np.float64)
    assert X.shape == Xs.shape
    d = np.sqrt(np.diag(Xs))
    if not np.all(np.isfinite(X)):
        return float("inf")
    return float((np.abs(X - Xs) / np.outer(d, d)).max())


def host_inverses(S, cols):
    """the cols x cols blocks of two fp64 host inverses of S: Cholesky (scipy.linalg.cho_solve) and LU (numpy.linalg.inv)"""
    import scipy.linalg
    S = np.asarray(S, np.float64)
    ix = np.ix_(cols, cols)
    chol = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), np.eye(S.shape[0]))
    return chol[ix], np.linalg.inv(S)[ix]
