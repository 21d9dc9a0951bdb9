"""An independent statement of the landmark covariance — TEST INFRASTRUCTURE, host only (numpy, scipy, mpmath).

    S0      = U - sum_l W_l V_l^-1 W_l^T                     (tests/cov_statement.S0_of)
    P       = (S0^-1)[0:Dp, 0:Dp]                            Dp = 6 x the free pose-type blocks
    G_l     = W_l V_l^-1                                     W_l [6 n_l, 3]: the landmark's pairs' 6 x 3 blocks stacked
    Sigma_l = V_l^-1 + G_l^T P[rows_l, rows_l] G_l           rows_l: the reduced rows of those blocks

the landmark's diagonal block of the inverse of the full undamped normal matrix.  The reference X* is evaluated with mpmath at 60
digits from inputs given exactly (a long double as the sum of two doubles); P comes from cov_statement.inverse_block_mp, which
rounds the 60-digit inverse to double — a relative 1.1e-16 on a term that is positive semi-definite in P, far below every error
measured here.  Per landmark

    e(X, X*) = max_ij |X_ij - X*_ij| / sqrt(X*_ii X*_jj) .
"""
from __future__ import annotations

import numpy as np

from . import cov_statement as cs
from . import schur_statement as stmt

UT = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # the order of OKVIS_BA_ARR_LM_V


def pose_dim(w):
    return 6 * int((np.asarray(w.pose_fixed).reshape(-1) == 0).sum())


def landmark_terms(w, V6, W18, pairs, drop_first=False, w_3x6=False):
    """[(rows [6 n_l], W_l [6 n_l, 3], V6_l [6])] for every landmark in window order.  drop_first: without the landmark's first pair;
    w_3x6: every pair's 18 numbers read as 3 x 6 and transposed (two mutations)."""
    V6 = np.asarray(V6).reshape(-1, 6)
    W18 = np.asarray(W18).reshape(-1, 18)
    pair_lm, pair_block = (np.asarray(p) for p in pairs)
    off = stmt.pose_offsets(w)
    first = np.searchsorted(pair_lm, np.arange(V6.shape[0] + 1))
    out = []
    for l in range(V6.shape[0]):
        ps = list(range(first[l], first[l + 1]))[1 if drop_first else 0:]
        rows = np.concatenate([off[pair_block[p]] + np.arange(6) for p in ps]).astype(np.int64) if ps else np.zeros(0, np.int64)
        assert np.all(rows >= 0)
        blocks = [(W18[p].reshape(3, 6).T if w_3x6 else W18[p].reshape(6, 3)) for p in ps]
        out.append((rows, np.concatenate(blocks, axis=0) if ps else np.zeros((0, 3), W18.dtype), V6[l]))
    return out


def sym3(v6):
    m = np.zeros((3, 3), np.asarray(v6).dtype)
    for e, (i, j) in enumerate(UT):
        m[i, j] = m[j, i] = v6[e]
    return m


def inv3sym_np(v6):
    """the cofactor inverse of ba_math.hpp's inv3sym restated in numpy (float64, no fused operations)"""
    a, b, c, d, e, f = (np.float64(x) for x in v6)
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    i = np.float64(1.0) / (a * c00 + b * c01 + c * c02)
    o = (c00 * i, c01 * i, c02 * i, (a * f - c * c) * i, (b * c - a * e) * i, (a * d - b * b) * i)
    return sym3(np.array(o))


def sigma_np(term, P, vinv="inv"):
    """Sigma_l in float64 from one landmark's term and P [Dp, Dp]; vinv: 'inv' (numpy.linalg.inv), 'cofactor' (inv3sym_np) or
    'only' (V^-1 alone, a mutation)"""
    rows, Wl, v6 = term
    if rows.size == 0:
        return np.full((3, 3), np.nan)
    V = sym3(np.asarray(v6, np.float64))
    Vi = inv3sym_np(v6) if vinv == "cofactor" else np.linalg.inv(V)
    if vinv == "only":
        return Vi
    G = np.asarray(Wl, np.float64) @ Vi
    return Vi + G.T @ (np.asarray(P, np.float64)[np.ix_(rows, rows)] @ G)


def _mp_rows(mp, A):
    """a double or long double matrix as rows of mpf, every entry exactly"""
    hi, lo = cs.two_doubles(np.atleast_2d(A))
    return [[mp.mpf(float(h)) + mp.mpf(float(l_)) for h, l_ in zip(hr, lr)] for hr, lr in zip(hi, lo)]


def sigma_mp(term, Pm):
    """Sigma_l at 60 digits from one landmark's term and P as rows of mpf (_mp_rows), every input taken exactly; rounded to
    double.  Call under mp.workdps(cs.DIGITS)."""
    import mpmath as mp
    rows, Wl, v6 = term
    if rows.size == 0:
        return np.full((3, 3), np.nan)
    Vi = mp.inverse(mp.matrix(_mp_rows(mp, sym3(np.asarray(v6)))))
    Vi = [[(Vi[i, j] + Vi[j, i]) / 2 for j in range(3)] for i in range(3)]
    Vc = [[Vi[k][j] for k in range(3)] for j in range(3)]                          # columns of V^-1
    G = [[mp.fdot(wr, Vc[j]) for j in range(3)] for wr in _mp_rows(mp, Wl)]        # [R][3]
    Gc = [[g[j] for g in G] for j in range(3)]                                     # columns of G
    T = [[mp.fdot([Pm[r][c] for c in rows], Gc[j]) for j in range(3)] for r in rows]
    Tc = [[t[j] for t in T] for j in range(3)]
    X = [[Vi[i][j] + mp.fdot(Gc[i], Tc[j]) for j in range(3)] for i in range(3)]
    return np.array([[float((X[i][j] + X[j][i]) / 2) for j in range(3)] for i in range(3)])


def sigma_all(terms, P, how="mp", **kw):
    """Sigma_l [n_lm, 3, 3] of every term: how = 'mp' (the 60-digit statement) or 'np' (float64, kw to sigma_np)"""
    if how != "mp":
        return np.array([sigma_np(t, P, **kw) for t in terms]).reshape(-1, 3, 3)
    import mpmath as mp
    with mp.workdps(cs.DIGITS):
        Pm = _mp_rows(mp, P)
        return np.array([sigma_mp(t, Pm) for t in terms]).reshape(-1, 3, 3)


def e(X, Xs):
    """the error measure of the module docstring, per landmark [n]; a landmark without covariance (X* NaN) must be NaN in X too
    and counts 0"""
    X, Xs = np.asarray(X, np.float64).reshape(-1, 3, 3), np.asarray(Xs, np.float64).reshape(-1, 3, 3)
    assert X.shape == Xs.shape
    out = np.zeros(X.shape[0])
    for l in range(X.shape[0]):
        if np.isnan(Xs[l]).all():
            out[l] = 0.0 if np.isnan(X[l]).all() else np.inf
        elif not np.all(np.isfinite(X[l])):
            out[l] = np.inf
        else:
            d = np.sqrt(np.diag(Xs[l]))
            out[l] = (np.abs(X[l] - Xs[l]) / np.outer(d, d)).max()
    return out
