"""An independent statement of the predicted measurement covariance — TEST INFRASTRUCTURE, host only (numpy, mpmath).

A query (lm, pose, ext, cam) projects landmark l through T_WS = pose[pose] and T_SC = pose[ext]; J_l (2 x 3), J_p, J_e (2 x 6) are
the derivatives of the pixel in the solver's tangent coordinates.  With V_l, W_l, rows_l, G_l = W_l V_l^-1 and P as in
tests/lmcov_statement.py, rows_x the reduced rows of the query's free blocks and R = rows_l u rows_x:

    form A      A = J_x E_x - J_l G_l^T E_l,      U = J_l V_l^-1 J_l^T + A P[R, R] A^T
    block form  Sigma_l  = V_l^-1 + G_l^T P[rows_l, rows_l] G_l,   Sigma_xx = P[rows_x, rows_x],   Sigma_lx = -G_l^T P[rows_l, rows_x]
                U = J_l Sigma_l J_l^T + J_x Sigma_xx J_x^T + J_l Sigma_lx J_x^T + (J_l Sigma_lx J_x^T)^T

Both are J Sigma J^T for J = [J_l J_p J_e] and Sigma the block of the inverse of the full undamped normal matrix.  Each is
evaluated with mpmath at 60 digits from inputs given exactly, and in float64 numpy; form A works on R in ascending order, the block
form never forms A: two independent orders.  Per query

    e(U, U*) = max_ij |U_ij - U*_ij| / sqrt(U*_ii U*_jj) .
"""
from __future__ import annotations

import numpy as np

from . import cov_statement as cs
from . import lmcov_statement as ls
from . import schur_statement as stmt


def jacobians(L, w, q, pose=None, lm=None):
    """(uv [2], jac [30] = J_l | J_p | J_e row-major, projects) of one query from an oracle library's reprojection factor (L:
    oracle_lib.lib() or lib_ld()) with unit information and the measurement at the origin: the residual is -uv and its Jacobians
    are -J.  pose / lm: the state (default: the window's).  Where the point does not project the factor leaves zeros; NaN here."""
    from . import oracle_lib as ol
    pose = np.asarray(w.pose if pose is None else pose, np.float64).reshape(-1, 7)
    lm = np.asarray(w.lm if lm is None else lm, np.float64).reshape(-1, 4)
    l, p, e, c = (int(x) for x in q)
    r, Jp, Jl, Je = np.zeros(2), np.zeros((2, 6)), np.zeros((2, 3)), np.zeros((2, 6))
    intr = np.ascontiguousarray(np.asarray(w.cam_intr, np.float64).reshape(-1, 12)[c])
    st = L.orc_reprojection(ol._p(ol._arr(pose[p])), ol._p(ol._arr(lm[l])), ol._p(ol._arr(pose[e])), ol._p(intr),
                            int(np.asarray(w.cam_model).reshape(-1)[c]), ol._p(np.zeros(2)), ol._p(np.eye(2).reshape(4).copy()),
                            ol._p(r), ol._p(Jp), ol._p(Jl), ol._p(Je))
    if not st & 1:
        return np.full(2, np.nan), np.full(30, np.nan), False
    return -r, -np.concatenate([Jl.reshape(-1), Jp.reshape(-1), Je.reshape(-1)]), True


def jacobians_all(L, w, queries, pose=None, lm=None):
    """(uv [n, 2], jac [n, 30], projects [n]) of a query list"""
    out = [jacobians(L, w, q, pose, lm) for q in queries]
    return (np.array([o[0] for o in out]).reshape(-1, 2), np.array([o[1] for o in out]).reshape(-1, 30),
            np.array([o[2] for o in out], bool))


def split(jac):
    jac = np.asarray(jac)
    return jac[:6].reshape(2, 3), jac[6:18].reshape(2, 6), jac[18:30].reshape(2, 6)


def rows_x_of(w, q):
    """(rows_x [6 k], the pose and the extrinsics part's offsets or -1) of a query: the reduced rows of its free blocks"""
    off = stmt.pose_offsets(w)
    op, oe = int(off[int(q[1])]), int(off[int(q[2])])
    rows = [o + np.arange(6) for o in (op, oe) if o >= 0]
    return (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int64), op, oe


def n_rows(w, term, q):
    """|R| of a query"""
    return int(np.union1d(term[0], rows_x_of(w, q)[0]).size)


def _jx(jac, op, oe, dtype=np.float64):
    _, Jp, Je = split(jac)
    parts = [J for J, o in ((Jp, op), (Je, oe)) if o >= 0]
    return np.concatenate(parts, axis=1).astype(dtype) if parts else np.zeros((2, 0), dtype)


# ---- float64 numpy ------------------------------------------------------------------------------------
def u_np(w, term, q, jac, P, form="A", vinv="inv", mutate=None):
    """U in float64.  form 'A' or 'block'; vinv as lmcov_statement.sigma_np; mutate: None, 'no cross' (the cross term dropped),
    'marginal' (J_l Sigma_l J_l^T alone) or 'G sign' (the sign of G flipped) — wrong definitions."""
    rows_l, Wl, v6 = term
    if rows_l.size == 0 or not np.all(np.isfinite(jac)):
        return np.full((2, 2), np.nan)
    P = np.asarray(P, np.float64)
    Jl = split(jac)[0]
    rows_x, op, oe = rows_x_of(w, q)
    Jx = _jx(jac, op, oe)
    Vi = ls.inv3sym_np(v6) if vinv == "cofactor" else np.linalg.inv(ls.sym3(np.asarray(v6, np.float64)))
    G = np.asarray(Wl, np.float64) @ Vi
    if mutate == "G sign":
        G = -G
    if form == "A" and mutate in (None, "G sign"):
        Dp = P.shape[0]
        A = np.zeros((2, Dp))
        A[:, rows_l] -= Jl @ G.T
        if rows_x.size:
            A[:, rows_x] += Jx
        R = np.union1d(rows_l, rows_x)
        AR = A[:, R]
        return Jl @ Vi @ Jl.T + AR @ (P[np.ix_(R, R)] @ AR.T)
    Sl = Vi + G.T @ (P[np.ix_(rows_l, rows_l)] @ G)
    U = Jl @ Sl @ Jl.T
    if mutate == "marginal" or rows_x.size == 0:
        return U
    U = U + Jx @ P[np.ix_(rows_x, rows_x)] @ Jx.T
    if mutate == "no cross":
        return U
    Cx = Jl @ (-(G.T @ P[np.ix_(rows_l, rows_x)])) @ Jx.T
    return U + Cx + Cx.T


# ---- 60 digits ----------------------------------------------------------------------------------------
def _m(mp, A):
    A = np.atleast_2d(A)
    return mp.matrix(ls._mp_rows(mp, A)) if A.size else mp.matrix(A.shape[0], A.shape[1])


def _sub(mp, Pm, r, c):
    return mp.matrix([[Pm[int(i)][int(j)] for j in c] for i in r]) if len(r) and len(c) else mp.matrix(len(r), len(c))


def _round(mp, U):
    return np.array([[float((U[i, j] + U[j, i]) / 2) for j in range(2)] for i in range(2)])


def u_mp(w, term, q, jac, Pm, form="A"):
    """U at 60 digits from one query's inputs, every input taken exactly, Pm = P as rows of mpf (lmcov_statement._mp_rows); rounded
    to double.  Call under mp.workdps(cs.DIGITS)."""
    import mpmath as mp
    rows_l, Wl, v6 = term
    if rows_l.size == 0 or not np.all(np.isfinite(jac)):
        return np.full((2, 2), np.nan)
    Jl = _m(mp, split(jac)[0])
    rows_x, op, oe = rows_x_of(w, q)
    Jx = _m(mp, _jx(jac, op, oe))
    Vi = mp.inverse(_m(mp, ls.sym3(np.asarray(v6))))
    G = _m(mp, Wl) * Vi
    if form == "A":
        R = np.union1d(rows_l, rows_x)
        at = {int(r): i for i, r in enumerate(R)}
        A = mp.matrix(2, len(R))
        JG = Jl * G.T
        for k, r in enumerate(rows_l):
            for i in range(2):
                A[i, at[int(r)]] -= JG[i, k]
        for k, r in enumerate(rows_x):
            for i in range(2):
                A[i, at[int(r)]] += Jx[i, k]
        return _round(mp, Jl * Vi * Jl.T + A * _sub(mp, Pm, R, R) * A.T)
    Sl = Vi + G.T * _sub(mp, Pm, rows_l, rows_l) * G
    U = Jl * Sl * Jl.T
    if rows_x.size:
        Cx = Jl * (-(G.T * _sub(mp, Pm, rows_l, rows_x))) * Jx.T
        U = U + Jx * _sub(mp, Pm, rows_x, rows_x) * Jx.T + Cx + Cx.T
    return _round(mp, U)


def u_all(w, terms, queries, jac, P, how="mp", **kw):
    """U [n, 2, 2] of every query: how = 'mp' (60 digits; kw: form) or 'np' (float64; kw to u_np)"""
    queries = np.asarray(queries).reshape(-1, 4)
    if how != "mp":
        return np.array([u_np(w, terms[int(q[0])], q, j, P, **kw) for q, j in zip(queries, jac)]).reshape(-1, 2, 2)
    import mpmath as mp
    with mp.workdps(cs.DIGITS):
        Pm = ls._mp_rows(mp, P)
        return np.array([u_mp(w, terms[int(q[0])], q, j, Pm, **kw) for q, j in zip(queries, jac)]).reshape(-1, 2, 2)


def e(U, Us):
    """the error measure of the module docstring, per query [n]; a query without covariance (U* NaN) must be NaN in U too and
    counts 0"""
    U, Us = np.asarray(U, np.float64).reshape(-1, 2, 2), np.asarray(Us, np.float64).reshape(-1, 2, 2)
    assert U.shape == Us.shape
    out = np.zeros(U.shape[0])
    for k in range(U.shape[0]):
        if np.isnan(Us[k]).all():
            out[k] = 0.0 if np.isnan(U[k]).all() else np.inf
        elif not np.all(np.isfinite(U[k])):
            out[k] = np.inf
        else:
            d = np.sqrt(np.diag(Us[k]))
            out[k] = (np.abs(U[k] - Us[k]) / np.outer(d, d)).max()
    return out


# ---- the dense full normal matrix ---------------------------------------------------------------------
def full_normal_matrix(w, lin):
    """H [D + 3 n_lm, D + 3 n_lm] of the oracle's arrays: the reduced ordering first, then three rows per landmark in window order"""
    D = lin["D"]
    V6 = np.asarray(lin["LM_V"], np.float64).reshape(-1, 6)
    W18 = np.asarray(lin["PAIR_W"], np.float64).reshape(-1, 18)
    pair_lm, pair_block = (np.asarray(p) for p in lin["pairs"])
    off = stmt.pose_offsets(w)
    n = D + 3 * V6.shape[0]
    H = np.zeros((n, n))
    H[:D, :D] = np.asarray(lin["HPP"], np.float64).reshape(D, D)
    for l in range(V6.shape[0]):
        H[D + 3 * l:D + 3 * l + 3, D + 3 * l:D + 3 * l + 3] = ls.sym3(V6[l])
    for p in range(W18.shape[0]):
        r, c = int(off[pair_block[p]]), D + 3 * int(pair_lm[p])
        H[r:r + 6, c:c + 3] = W18[p].reshape(6, 3)
        H[c:c + 3, r:r + 6] = W18[p].reshape(6, 3).T
    return H


def full_jacobian(w, D, q, jac):
    """(columns of the full ordering the query's J touches, J [2, their number])"""
    Jl = split(jac)[0]
    rows_x, op, oe = rows_x_of(w, q)
    cols = np.concatenate([D + 3 * int(q[0]) + np.arange(3), rows_x]).astype(np.int64)
    return cols, np.concatenate([Jl, _jx(jac, op, oe)], axis=1)
