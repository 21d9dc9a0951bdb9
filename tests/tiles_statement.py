"""What the tiled multi-workgroup Cholesky of the reduced camera system (okvis_amd/csrc/ba_chol_tiles.hpp: chol_tile_task,
chol_chain_task, chol_backsub_task, ct_ldl_inv48 — the solver behind every window with D > 174) is held to, stated on the CPU.
Test infrastructure, no GPU.  The rule is the LDS solvers' (tests/solve_statement.py): reference, e, rho and BOUND_FACTOR are
taken from there unchanged.

  fp64 peers        numpy.linalg.solve, a LAPACK Cholesky solve (scipy.linalg.cho_factor / cho_solve) and tiled_emulation below:
                    the data flow of ba_chol_tiles.hpp in plain numpy loops, not its wave roles — padded to 48 nT with the
                    identity, left-looking by tile columns, diagonal tile -> L_jj and the explicit Linv_j,
                    y_j = Linv_j (r_j - sum_k L_jk y_k) riding along, L_ij = C Linv_j^T, the back-substitution
                    x_j = Linv_j^T (y_j - sum_(i>j) L_ij^T x_i) from the last tile row up;
  kernel arithmetic tiled_kernel_arithmetic: the same flow with the arithmetic of ct_ldl_inv48 restated (LDL^T over three 16-wide
                    panels, each diagonal 16-block eliminated in place with reciprocal pivots and fused updates, NOT compensated;
                    Lt^-1 by block products; rows scaled by sqrt(dinv)) and the tile products as fused chains over the inner
                    index — the CPU evidence for how far behind an ill-conditioned prior the kernel may sit from the plain peers
                    (tiles_cases.ROTATED_RHO_FACTOR).  Not a bit-exact model: the hardware reciprocal and square root and the
                    matrix core's internal order are not restated;
  mutations         of tiled_emulation, each broken the way the kernel could be (MUTATIONS).

The bound of a family of cases: the largest e its peers reach against the reference over the family's cases, and the largest rho
of the two Cholesky peers (LAPACK, tiled_emulation) — numpy's pivoted LU leaves a rho ten times larger on the graded family, under
which no unpivoted solver could fail; measured by tests/test_tiles_statement_host.py, recorded in tests/tiles_cases.FAMILY_REF; a
kernel must stay within BOUND_FACTOR times both."""
import numpy as np

from tests.solve_statement import BOUND_FACTOR, _mfma_chain, e, fma, reference, rho   # noqa: F401  (the statement, re-exported)

TB = 48   # CT_TB

MUTATIONS = ("skip_chain_last_update",   # the chain's last update (k = j - 1) of diagonal tile j = 1 left out
             "skip_forward_term",        # the forward substitution's L_jk y_k left out for j = 1, k = 0
             "transpose_sub",            # L_(1,0) stored transposed
             "skip_far_tile",            # the far tile (2, 0) skipped in the back-substitution of tile row 0
             "tile_index_shift",         # an update of a tile of row i >= 3 reads L_(i,k), k >= 1, at the index of (i, k - 1)
             "zero_padding")             # the padding taken as zero instead of the identity


def n_tiles(n):
    return (n + TB - 1) // TB


def pad(S, g, identity=True):
    """(tiles {(i, j): 48 x 48, i >= j}, rhs [nT][48]) of the system padded to 48 nT (okvis_ba_dense_solve, large_export_kernel)"""
    n = S.shape[0]
    nT = n_tiles(n)
    M = np.eye(TB * nT) if identity else np.zeros((TB * nT, TB * nT))
    M[:n, :n] = S
    r = np.zeros(TB * nT)
    r[:n] = g
    return {(i, j): M[TB * i:TB * i + TB, TB * j:TB * j + TB].copy() for i in range(nT) for j in range(i + 1)}, r.reshape(nT, TB).copy()


def _chol48(C):
    """(L, L^-1) of a 48 x 48 tile, the lower triangle referenced: column Cholesky and the inverse by forward substitution on the
    identity.  A pivot that is not positive is not guarded here (the kernel's guard reports it; a peer has nothing to report to)"""
    A = np.tril(C).copy()
    L = np.zeros_like(A)
    for c in range(TB):
        d = np.sqrt(A[c, c])
        L[c, c] = d
        L[c + 1:, c] = A[c + 1:, c] / d
        A[c + 1:, c + 1:] -= np.tril(np.outer(L[c + 1:, c], L[c + 1:, c]))
    X = np.zeros_like(A)
    for r in range(TB):
        row = -(L[r, :r] @ X[:r, :])
        row[r] += 1.0
        X[r] = row / L[r, r]
    return L, np.tril(X)


def _ldl_inv48(C):
    """L^-1 of a 48 x 48 tile by the steps and the arithmetic of ct_ldl_inv48: a blocked LDL^T with 16-wide panels, each diagonal
    block eliminated in place (ldl16_pivot<K, true, GUARD, COMP = false>: multiplier = the pivot COLUMN's entry, row factor =
    -(the pivot ROW's entry) x the RECIPROCAL of the pivot, one fused update per entry, factorisation and unit-lower inverse in
    the same registers), everything between the blocks 16 x 16 x 16 products (fused chains), Lt^-1's off-diagonal blocks by block
    products, rows scaled by sqrt(1 / d)"""
    M = np.tril(C) + np.tril(C, -1).T        # (the kernel references the lower triangle)
    M = M.copy()
    X = np.zeros((TB, TB))
    R = np.zeros((TB, TB))
    dinv = np.zeros(TB)
    lower = np.tril(np.ones((16, 16), bool), -1)
    blk = lambda A, I, J: A[16 * I:16 * I + 16, 16 * J:16 * J + 16]
    prod = lambda A, B: _mfma_chain(np.zeros((16, 16)), np.ascontiguousarray(A.T), B)     # A B, fused over the inner index

    def eliminate(b):
        W = blk(M, b, b)
        W = np.tril(W) + np.tril(W, -1).T
        di = np.zeros(16)
        for K in range(16):
            rd = 1.0 / W[K, K] if W[K, K] > 0.0 else 0.0       # (GUARD: a pivot that is not positive is left out, the kernel reports it)
            di[K] = rd
            v = -W[K, :] * rd
            v[K] = 0.0
            m = W[K + 1:, K].copy()
            W[K + 1:, :] = fma(m[:, None], v[None, :], W[K + 1:, :])
        dinv[16 * b:16 * b + 16] = di
        blk(X, b, b)[:] = np.where(lower, -W * di[None, :], 0.0) + np.eye(16)      # (c: -L^-1 D below the diagonal)

    def update(I, J, k):                     # A_IJ -= R_kI^T D_k^-1 R_kJ (lower blocks; the product first, then one subtraction)
        v = prod((blk(R, k, I) * dinv[16 * k:16 * k + 16, None]).T, blk(R, k, J))
        blk(M, I, J)[:] -= v if I > J else np.tril(v)

    eliminate(0)
    for J in (1, 2):
        blk(R, 0, J)[:] = prod(blk(X, 0, 0), blk(M, J, 0).T)
    for I, J in ((1, 1), (2, 1), (2, 2)):
        update(I, J, 0)
    eliminate(1)
    blk(R, 1, 2)[:] = prod(blk(X, 1, 1), blk(M, 2, 1).T)
    update(2, 2, 1)
    eliminate(2)
    Lt = lambda I, J: (blk(R, J, I) * dinv[16 * J:16 * J + 16, None]).T             # Lt_IJ = R_JI^T D_J^-1
    T10, T21, T20 = prod(Lt(1, 0), blk(X, 0, 0)), prod(Lt(2, 1), blk(X, 1, 1)), prod(Lt(2, 0), blk(X, 0, 0))
    blk(X, 1, 0)[:] = -prod(blk(X, 1, 1), T10)
    blk(X, 2, 1)[:] = -prod(blk(X, 2, 2), T21)
    T20 = T20 + prod(Lt(2, 1), blk(X, 1, 0))
    blk(X, 2, 0)[:] = -prod(blk(X, 2, 2), T20)
    return X * np.sqrt(dinv)[:, None]


def _gemm_nt_fused(acc, A, B, sign):
    """acc + sign A B^T the way ct_gemm_nt adds it: one fused multiply-add per inner index, in the order of the index"""
    for k in range(TB):
        acc = fma(sign * A[:, k][:, None], B[:, k][None, :], acc)
    return acc


def tiled_emulation(S, g, mutation=None, kernel_arithmetic=False):
    """x with S x = g by the steps of ba_chol_tiles.hpp"""
    assert mutation is None or mutation in MUTATIONS
    n = S.shape[0]
    nT = n_tiles(n)
    T, r = pad(np.asarray(S, np.float64), np.asarray(g, np.float64), identity=mutation != "zero_padding")
    Linv, y = [None] * nT, np.zeros((nT, TB))
    if kernel_arithmetic:
        sub = lambda C, A, B: _gemm_nt_fused(C, A, B, -1.0)
        times_t = lambda C, Li: _gemm_nt_fused(np.zeros((TB, TB)), C, Li, 1.0)
    else:
        sub = lambda C, A, B: C - A @ B.T
        times_t = lambda C, Li: C @ Li.T

    def L_of(i, k):      # the tile an update reads as L_(i,k)
        if mutation == "tile_index_shift" and i >= 3 and k >= 1:
            return T[(i, k - 1)]
        return T[(i, k)]

    with np.errstate(all="ignore"):          # (the zero padding divides by zero: its x is not finite, which is the point)
        for j in range(nT):
            # the diagonal tile: every update k < j in the order of k (tile task k < j - 1, the chain k = j - 1), then L_jj^-1
            C, rj = T[(j, j)], r[j].copy()
            for k in range(j):
                Ljk = L_of(j, k)
                if not (mutation == "skip_chain_last_update" and j == 1 and k == 0):
                    C = sub(C, Ljk, Ljk)
                if not (mutation == "skip_forward_term" and j == 1 and k == 0):
                    rj -= Ljk @ y[k]
            if kernel_arithmetic:
                Linv[j] = _ldl_inv48(C)
            else:
                T[(j, j)], Linv[j] = _chol48(C)
            y[j] = Linv[j] @ rj
            # the tiles below it: L_ij = (A_ij - sum_(k<j) L_ik L_jk^T) Linv_j^T
            for i in range(j + 1, nT):
                C = T[(i, j)]
                for k in range(j):
                    C = sub(C, L_of(i, k), L_of(j, k))
                C = times_t(C, Linv[j])
                T[(i, j)] = C.T.copy() if (mutation == "transpose_sub" and (i, j) == (1, 0)) else C
        x = np.zeros((nT, TB))
        for j in reversed(range(nT)):
            t = y[j].copy()
            for i in range(nT - 1, j, -1):   # the far tiles from the last tile row up, the near one (j + 1, j) last
                if mutation == "skip_far_tile" and (i, j) == (2, 0):
                    continue
                t -= T[(i, j)].T @ x[i]
            x[j] = Linv[j].T @ t
    return x.reshape(-1)[:n].copy()


def tiled_kernel_arithmetic(S, g):
    """tiled_emulation with the kernel's arithmetic restated where it differs from plain numpy (see the module's docstring)"""
    return tiled_emulation(S, g, kernel_arithmetic=True)


def lapack_cholesky(S, g):
    try:
        from scipy.linalg import cho_factor, cho_solve
        return cho_solve(cho_factor(S, lower=True), g)
    except ImportError:
        L = np.linalg.cholesky(S)
        return np.linalg.solve(L.T, np.linalg.solve(L, g))


CHOLESKY_PEERS = ("lapack", "tiled")


def peers(S, g):
    """{name: x} of the fp64 peers"""
    return {"numpy": np.linalg.solve(S, g), "lapack": lapack_cholesky(S, g), "tiled": tiled_emulation(S, g)}
