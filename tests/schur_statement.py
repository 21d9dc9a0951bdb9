"""An independent statement of the landmark Schur reduction — TEST INFRASTRUCTURE, host only (numpy).

    S   = U + lambda diag(Dp2) - sum_l W_l (V_l + lambda diag(Dl2_l))^-1 W_l^T
    rhs = -g                   + sum_l W_l (V_l + lambda diag(Dl2_l))^-1 b_l

(oracle/orc_window.cpp solve_damped; the kernels of ba_schur.hpp and ba_schur2.hpp).  W_l stacks the 6 x 3 blocks of the
(landmark, block) pairs of landmark l, at the reduced offsets of their pose blocks.  It differs from the oracle on purpose: the
inverse of V is the adjugate over the determinant by Sarrus' rule (six products, no cofactor shared with the adjugate), the
landmarks are summed in REVERSE order, and a landmark's whole contribution is one numpy product over all its blocks.  `dtype` is
the arithmetic: numpy.float64 restates the oracle, numpy.longdouble is the isolating referee of the GPU test.

The entrywise scale: what every entry of the result is a sum OF, with absolute values —

    a_ij = |U_ij| + lambda Dp2_i delta_ij + sum_l c_l (|W_l| |Vd_l^-1| |W_l|^T)_ij ,   a_i = |g_i| + sum_l c_l (|W_l| |Vd_l^-1| |b_l|)_i

with c_l = 1 (unweighted) or c_l = cond_2(Vd_l) (weighted: the relative error of an inverse formed in floating point is
cond x eps, so a landmark whose V is nearly singular may move its own term by that much and no more).
deviation(X, ref, a) = max |X - ref| / a over a > 0; where a = 0 nothing was ever added and X must be an exact zero.

`mutate` breaks the reduction the way a kernel could (tests/test_schur_statement_host.py proves that the cases notice):

    "ragged_last"   the last landmark of the window (the ragged last stage of its chunk) left out
    "drop_pair"     one (landmark, block) pair left out
    "drop_vb"       one landmark's V^-1 b left out of the right-hand side
    "no_lm_damping" lambda Dl2 not added to V (LM mode: lambda = 1 / radius)
    "transpose"     one off-diagonal 6 x 6 block of the landmark part transposed
"""
from __future__ import annotations

import numpy as np

MUTATIONS = ("ragged_last", "drop_pair", "drop_vb", "no_lm_damping", "transpose")
STRATEGY_DOGLEG, STRATEGY_LM = 0, 1
DL_MIN_MU = 1.0e-8     # mu of the first dogleg iteration (Ceres DoglegStrategy min_mu)
_UT = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def pose_offsets(w):
    """reduced offset of every pose-type block: the free ones in index order, six rows each; -1 for a fixed block"""
    free = np.asarray(w.pose_fixed).reshape(-1) == 0
    off = np.full(free.size, -1, np.int64)
    off[free] = 6 * np.arange(int(free.sum()))
    return off


def damping(opt, U_diag, V6):
    """(lambda, Dp2 [D], Dl2 [n_lm, 3]) of the FIRST solve of an optimisation under the options: LM clamps the diagonal and damps
    with 1 / initial_radius; DOGLEG (also with gauss_newton) clamps the Jacobi-scaled diagonal and solves its Gauss-Newton point
    with mu = min_mu."""
    h = np.asarray(U_diag, np.float64)
    v = np.asarray(V6, np.float64).reshape(-1, 6)[:, [0, 3, 5]]
    lo, hi = float(opt.min_lm_diagonal), float(opt.max_lm_diagonal)
    if int(opt.strategy) == STRATEGY_DOGLEG:
        def d(x):
            sc = 1.0 / (1.0 + np.sqrt(x)) if opt.jacobi_scaling else np.ones_like(x)
            return np.clip(sc * sc * x, lo, hi) / (sc * sc)
        return DL_MIN_MU, d(h), d(v)
    return 1.0 / float(opt.initial_radius), np.clip(h, lo, hi), np.clip(v, lo, hi)


def _sym3(v6, T):
    m = np.zeros((3, 3), T)
    for e, (i, j) in enumerate(_UT):
        m[i, j] = m[j, i] = T(v6[e])
    return m


def inverse3(m):
    """adjugate / determinant of a symmetric 3 x 3, every cofactor written out, the determinant by Sarrus' rule"""
    a, b, c = m[0, 0], m[0, 1], m[0, 2]
    d, e, f = m[1, 1], m[1, 2], m[2, 2]
    det = a * d * f + b * e * c + c * b * e - c * d * c - b * b * f - a * e * e
    adj = np.array([[d * f - e * e, c * e - b * f, b * e - c * d],
                    [c * e - b * f, a * f - c * c, b * c - a * e],
                    [b * e - c * d, b * c - a * e, a * d - b * b]], dtype=m.dtype)
    return adj / det


def _landmark_terms(V6, B, W, pair_lm, pair_block, off, lam, Dl2, T, mutate):
    """per landmark, last first: (l, rows, W_l [6 n, 3], Vd_l^-1, b_l, in_rhs, Vd_l)"""
    V6 = np.asarray(V6).reshape(-1, 6)
    B = np.asarray(B).reshape(-1, 3)
    W = np.asarray(W).reshape(-1, 6, 3)
    pair_lm, pair_block = np.asarray(pair_lm), np.asarray(pair_block)
    n_lm, n_pair = V6.shape[0], pair_lm.size
    assert W.shape[0] == n_pair and np.all(np.diff(pair_lm) >= 0)
    first = np.searchsorted(pair_lm, np.arange(n_lm + 1))
    dropped_pair = n_pair // 2 if mutate == "drop_pair" else -1
    no_vb = n_lm // 2 if mutate == "drop_vb" else -1
    for l in range(n_lm - 1, -1, -1):
        if mutate == "ragged_last" and l == n_lm - 1:
            continue
        ps = [p for p in range(first[l], first[l + 1]) if p != dropped_pair]
        Vd = _sym3(V6[l], T)
        if mutate != "no_lm_damping":
            Vd = Vd + np.diag((T(lam) * np.asarray(Dl2[l], T)))
        rows = np.concatenate([off[pair_block[p]] + np.arange(6) for p in ps]).astype(np.int64) if ps else np.zeros(0, np.int64)
        assert np.all(rows >= 0)
        Wl = np.concatenate([W[p].astype(T) for p in ps], axis=0) if ps else np.zeros((0, 3), T)
        yield l, rows, Wl, inverse3(Vd), B[l].astype(T), l != no_vb, Vd


def reduce(U, g, V6, B, W, pair_lm, pair_block, off, lam, Dp2, Dl2, dtype=np.float64, mutate=None):
    """(S [D, D], rhs [D]) in `dtype`"""
    T = dtype
    g = np.asarray(g).astype(T)
    D = g.size
    S = np.asarray(U).astype(T).reshape(D, D).copy()
    S[np.arange(D), np.arange(D)] += T(lam) * np.asarray(Dp2).astype(T)
    rhs = -g
    L = np.zeros((D, D), T)          # the landmark part: sum_l Y_l W_l^T
    for l, rows, Wl, Vi, b, in_rhs, _ in _landmark_terms(V6, B, W, pair_lm, pair_block, off, lam, Dl2, T, mutate):
        Y = Wl @ Vi
        L[np.ix_(rows, rows)] += Y @ Wl.T
        if in_rhs:
            rhs[rows] += Y @ b
    if mutate == "transpose":
        i, j = _first_offdiagonal_block(L)
        blk = L[6 * i:6 * i + 6, 6 * j:6 * j + 6].T.copy()
        L[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk
        L[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk.T
    assert S.dtype == T and rhs.dtype == T and L.dtype == T
    return S - L, rhs


def _first_offdiagonal_block(L):
    n = L.shape[0] // 6
    for i in range(1, n):
        for j in range(i):
            if np.any(L[6 * i:6 * i + 6, 6 * j:6 * j + 6] != 0):
                return i, j
    raise AssertionError("no off-diagonal block carries a landmark term")


def scale(U, g, V6, B, W, pair_lm, pair_block, off, lam, Dp2, Dl2, weighted):
    """(a_S [D, D], a_rhs [D]) of the module docstring, float64"""
    T = np.float64
    g = np.asarray(g, T)
    D = g.size
    aS = np.abs(np.asarray(U, T).reshape(D, D))
    aS[np.arange(D), np.arange(D)] += lam * np.asarray(Dp2, T)
    ar = np.abs(g)
    for l, rows, Wl, Vi, b, _, Vd in _landmark_terms(V6, B, W, pair_lm, pair_block, off, lam, Dl2, T, None):
        c = float(np.linalg.cond(Vd)) if weighted else 1.0
        Ya = np.abs(Wl) @ np.abs(Vi)
        aS[np.ix_(rows, rows)] += c * (Ya @ np.abs(Wl).T)
        ar[rows] += c * (Ya @ np.abs(b))
    return aS, ar


def deviation(x, ref, a):
    """max |x - ref| / a over a > 0 (float); entries with a = 0 must be exact zeros of x (asserted)"""
    x, ref, a = (np.asarray(v, np.float64) for v in (x, ref, a))
    assert x.shape == ref.shape == a.shape, (x.shape, ref.shape, a.shape)
    assert np.all(x[a == 0.0] == 0.0), "an entry nothing sums into is not an exact zero"
    on = a > 0.0
    return float((np.abs(x - ref)[on] / a[on]).max()) if on.any() else 0.0


def worst_entry(x, ref, a):
    """(deviation, flat index) of the worst entry — to locate a fault from the entry pattern"""
    x, ref, a = (np.asarray(v, np.float64) for v in (x, ref, a))
    e = np.where(a > 0.0, np.abs(x - ref) / np.where(a > 0.0, a, 1.0), 0.0)
    k = int(np.argmax(e))
    return float(e.reshape(-1)[k]), k
