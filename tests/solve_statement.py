"""What the LDS-resident solvers of the reduced camera system (okvis_amd/csrc/ba_ldl16.hpp::ldl16_solve, ba_chain.hpp::chain_solve) are
held to, stated on the CPU.  Test infrastructure, no GPU.

  reference(H, g)   the solution of H x = g by a Cholesky factorisation in 50-digit mpmath of the fp64 inputs (converted exactly),
                    rounded to fp64 at the end;
  e(x, x_ref)       max |x - x_ref| / max |x_ref|;
  rho(H, g, x)      the Jacobi-scaled residual  ||d^-1 (H x - g)||_inf / (||d^-1 H d^-1||_inf ||d x||_inf + ||d^-1 g||_inf),
                    d = sqrt(diag H), formed in long double: an axis-aligned 1e16 on the diagonal scales away, a rotated one does not;
  fp64 peers        numpy.linalg.solve, tests/chain_emulation.chain_solve (chain-structured systems) and ldl16_emulation below: the
                    blocked LDL^T with 16-wide panels in the solver's order (L16::perm), the right-hand side as column D, products
                    with zero blocks skipped — the data flow of ldl16_solve in plain loops, not its wave roles;
  kernel arithmetic ldl16_kernel_arithmetic: the same solve with the kernel's arithmetic restated (in-place elimination, reciprocal
                    multipliers, fused updates, the compensated second update of comp_mask) — the CPU evidence for how far from
                    the better plain peer the kernels may sit behind the rotated prior (solve_cases.ROTATED_RHO_FACTOR);
  mutations         of the two emulations, each broken the way a kernel could be (MUTATIONS_LDL16, MUTATIONS_CHAIN; the chain's
                    live in chain_emulation.chain_solve(mutation=...)).

The bound of a family of cases: the largest e and rho its peers reach against the reference over the family's cases (measured by
tests/test_solve_statement_host.py, recorded in tests/solve_cases.FAMILY_REF); a kernel must stay within BOUND_FACTOR times that."""
import numpy as np

BOUND_FACTOR = 4.0   # (the other referees' factor)

MUTATIONS_LDL16 = ("skip_last_column_update",    # the trailing update of the last block column (the one with the rhs) left out in the last step that has one
                   "stale_zero_flag",            # a block that was zero on input is skipped after it has filled in
                   "rhs_wrong_column_npl0",      # D a multiple of 16: the right-hand side taken from column 1 of the last block, not column npl = 0
                   "transpose_coupling")         # block (0, 1) transposed when it is loaded
MUTATIONS_CHAIN = ("drop_col_64", "drop_col_128",   # one column of [pose couplings | rhs] left out of the pose system's update
                   "no_share",                      # the right sweep's share not added to the middle block
                   "transpose_coupling")            # the coupling of the first step of the left sweep transposed


def reference(H, g):
    """x with H x = g: Cholesky in 50 digits over rows (mpmath.fdot), the lower triangle of H (what the kernels read)"""
    import mpmath
    n = H.shape[0]
    with mpmath.workdps(50):
        mpf, fdot = mpmath.mpf, mpmath.fdot
        A = [[mpf(float(H[i, j])) for j in range(i + 1)] for i in range(n)]
        L = [[None] * (i + 1) for i in range(n)]
        for i in range(n):
            Li = L[i]
            for j in range(i):
                Li[j] = (A[i][j] - fdot(Li[:j], L[j][:j])) / L[j][j]
            s = A[i][i] - fdot(Li[:i], Li[:i])
            if not s > 0:
                raise ValueError("not positive definite")
            Li[i] = mpmath.sqrt(s)
        y = []
        for i in range(n):
            y.append((mpf(float(g[i])) - fdot(L[i][:i], y)) / L[i][i])
        x = [None] * n
        for i in reversed(range(n)):
            x[i] = (y[i] - fdot([L[k][i] for k in range(i + 1, n)], x[i + 1:])) / L[i][i]
        return np.array([float(v) for v in x])


def e(x, x_ref):
    return float(np.abs(x - x_ref).max() / np.abs(x_ref).max())


def rho(H, g, x):
    ld = np.longdouble
    Hl, gl, xl = H.astype(ld), g.astype(ld), np.asarray(x).astype(ld)
    d = np.sqrt(np.diag(Hl))
    r = np.abs((Hl @ xl - gl) / d).max()
    Hs = np.abs(Hl / d[:, None] / d[None, :]).sum(axis=1).max()
    return float(r / (Hs * np.abs(d * xl).max() + np.abs(gl / d).max()))


def ldl16_emulation(H, g, Dp=None, mutation=None):
    """x with H x = g by the steps of ba_ldl16.hpp::ldl16_solve.  Dp < D: the speed/bias rows (reduced index >= Dp) come first in
    the solver's order (L16::perm with Ds = D - Dp)."""
    assert mutation is None or mutation in MUTATIONS_LDL16
    D = H.shape[0]
    Dp = D if Dp is None else Dp
    Ds = D - Dp
    nb = (D + 1 + 15) // 16
    npl = D - 16 * (nb - 1)
    perm = np.array([i + Ds if i < Dp else i - Dp for i in range(D)])
    n = 16 * nb
    M = np.zeros((n, n))
    M[np.ix_(perm, perm)] = H
    M[perm, D] = g
    M[D, perm] = g      # (the last diagonal block is held full; row npl is never a pivot row)
    blk = lambda I, J: M[16 * I:16 * I + 16, 16 * J:16 * J + 16]
    A = {(I, J): blk(I, J).copy() for I in range(nb) for J in range(I, nb)}
    if mutation == "transpose_coupling" and nb >= 2:
        A[(0, 1)] = A[(0, 1)].T.copy()
    zero_in = {key: not np.any(a) for key, a in A.items()}
    Linv, dinv, R = [None] * nb, [None] * nb, {}
    for k in range(nb):
        npiv = npl if k == nb - 1 else 16
        # the diagonal block: Gauss elimination in LDL^T form on [A | I]; the columns beyond the pivots (the rhs) ride along
        W = A[(k, k)].copy()
        Li = np.eye(16)
        di = np.zeros(16)
        for K in range(npiv):
            rd = 1.0 / W[K, K]
            di[K] = rd
            v = W[K, :] * rd                       # the pivot row over d
            m = W[:, K].copy()                     # the pivot column: the multipliers
            rows = np.arange(K + 1, 16)
            W[np.ix_(rows, np.arange(K + 1, 16))] -= np.outer(m[rows], v[K + 1:])
            Li[rows, :] -= np.outer(m[rows] * rd, Li[K, :])
        Linv[k], dinv[k] = Li, di
        if k == nb - 1:
            y_last = W[:, npl].copy()              # L^-1 b of the last block in its rows < npl
            break
        # the panel row R_J = L_kk^-1 A_kJ; a block that is still exactly zero stays zero and is flagged
        z = {}
        for J in range(k + 1, nb):
            a = A[(k, J)]
            z[J] = not np.any(a) or (mutation == "stale_zero_flag" and zero_in[(k, J)])
            R[(k, J)] = np.zeros((16, 16)) if z[J] else Li @ a
        # the trailing update A_IJ -= R_I^T D^-1 R_J, skipped where a factor is a zero block
        for I in range(k + 1, nb):
            for J in range(I, nb):
                if z[I] or z[J]:
                    continue
                if mutation == "skip_last_column_update" and J == nb - 1 and k == nb - 2:
                    continue
                A[(I, J)] -= R[(k, I)].T @ (di[:, None] * R[(k, J)])
    # back-substitution from the last block: x[D] = -1 makes the rhs one more column
    xb = np.zeros((nb, 16))
    for K in reversed(range(nb)):
        if K == nb - 1:
            t = np.where(np.arange(16) < npl, y_last, 0.0)
        else:
            t = np.zeros(16)
            for J in range(nb - 1, K + 1, -1):      # the slots in the fixed order, then the super-diagonal block
                t -= R[(K, J)] @ xb[J]
            t -= R[(K, K + 1)] @ xb[K + 1]
        xk = Linv[K].T @ (dinv[K] * t)
        if K == nb - 1:
            at = 1 if (mutation == "rhs_wrong_column_npl0" and npl == 0) else npl
            xk = np.where(np.arange(16) == at, -1.0, np.where(np.arange(16) < npl, xk, 0.0))
        xb[K] = xk
    xs = xb.reshape(-1)[:D]
    return xs[perm]


def fma(a, b, c):
    """a * b + c with one rounding, elementwise, in plain fp64: the product exactly (Veltkamp / Dekker), the sum exactly (Knuth),
    then the two error terms folded in — the fused result except in rare double-rounding ties"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b
    ta, tb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    ep = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    es = (p - (s - bb)) + (c - bb)
    return s + (es + ep)


def _mfma_chain(acc, A, B):
    """acc + A^T B (A, B: [16][16], the inner dimension first) the way four v_mfma_f64_16x16x4_f64 add it: one fused multiply-add
    per inner index, in the order of the index"""
    for k in range(A.shape[0]):
        acc = fma(A[k][:, None], B[k][None, :], acc)
    return acc


def ldl16_kernel_arithmetic(H, g, Dp=None, comp_mask=0):
    """ldl16_emulation with the kernel's arithmetic restated where it differs from plain numpy: the elimination of a diagonal
    block column per lane IN PLACE (the inverse of the unit-lower factor grows in the columns left of the pivot, as -L^-1 D),
    multiplier = row entry times the RECIPROCAL of the pivot, every update a fused multiply-add, the compensated second update
    for the blocks of comp_mask (ldl16_pivot<.., COMP>), the panel and trailing products as fused chains over the inner index
    with D^-1 rounded into one operand first, the back-substitution through D^-1 Bh D^-1.  A peer for the question how far the
    kernel's arithmetic alone may sit from the better of the plain peers — not a bit-exact model (the hardware reciprocal's two
    Newton steps and the matrix core's internal order are not restated)."""
    D = H.shape[0]
    Dp = D if Dp is None else Dp
    Ds = D - Dp
    nb = (D + 1 + 15) // 16
    npl = D - 16 * (nb - 1)
    perm = np.array([i + Ds if i < Dp else i - Dp for i in range(D)])
    n = 16 * nb
    M = np.zeros((n, n))
    M[np.ix_(perm, perm)] = H
    M[perm, D] = g
    M[D, perm] = g
    A = {(I, J): M[16 * I:16 * I + 16, 16 * J:16 * J + 16].copy() for I in range(nb) for J in range(I, nb)}
    Linv, dinv, XB, R = [None] * nb, [None] * nb, [None] * nb, {}
    lower = np.tril(np.ones((16, 16), bool), -1)
    for k in range(nb):
        npiv = npl if k == nb - 1 else 16
        comp = bool((comp_mask >> k) & 1)
        W = A[(k, k)].copy()
        di = np.zeros(16)
        for K in range(npiv):
            rd = 1.0 / W[K, K]
            di[K] = rd
            row = W[K, :].copy()
            v = -row * rd
            vl = fma(-row, rd, -v) if comp else None
            v[K] = 0.0
            m = W[K + 1:, K].copy()
            W[K + 1:, :] = fma(m[:, None], v[None, :], W[K + 1:, :])
            if comp:
                vl[K] = 0.0
                W[K + 1:, :] = fma(m[:, None], vl[None, :], W[K + 1:, :])
        # what the consumers make of the published columns: L^-1 = -(G) D^-1 below the diagonal, D^-1 Bh D^-1 for the way back
        Li = np.where(lower, W * (-di)[None, :], 0.0) + np.eye(16)
        Linv[k], dinv[k] = Li, di
        XB[k] = np.where(lower, -(W * di[:, None] * di[None, :]), 0.0) + np.diag(di)
        if k == nb - 1:
            y_last = W[:, npl].copy()
            break
        z = {}
        for J in range(k + 1, nb):
            a = A[(k, J)]
            z[J] = not np.any(a)
            R[(k, J)] = np.zeros((16, 16)) if z[J] else _mfma_chain(np.zeros((16, 16)), Li.T.copy(), a)
        for I in range(k + 1, nb):
            for J in range(I, nb):
                if not (z[I] or z[J]):
                    A[(I, J)] = _mfma_chain(A[(I, J)], R[(k, I)], R[(k, J)] * (-di)[:, None])
    xb = np.zeros((nb, 16))
    for K in reversed(range(nb)):
        if K == nb - 1:
            t = np.where(np.arange(16) < npl, y_last, 0.0)
        else:
            t = np.zeros(16)
            for J in range(nb - 1, K + 1, -1):
                t -= R[(K, J)] @ xb[J]
            for c in range(16):
                t = fma(-xb[K + 1][c], R[(K, K + 1)][:, c], t)
        xk = np.zeros(16)
        for c in range(16):
            xk = fma(t[c], XB[K][c, :], xk)
        if K == nb - 1:
            xk = np.where(np.arange(16) == npl, -1.0, np.where(np.arange(16) < npl, xk, 0.0))
        xb[K] = xk
    return xb.reshape(-1)[:D][perm]


def kernel_arithmetic_peer(H, g, Dp, mode, comp_mask):
    """the solve of `mode` ("dense" | "chain") with ldl16_kernel_arithmetic where the kernel runs ldl16_solve: the whole system, or
    the pose system behind the chain emulation's sweeps"""
    if mode == "dense":
        return ldl16_kernel_arithmetic(H, g, Dp, comp_mask)
    from tests.chain_emulation import chain_solve
    return chain_solve(H, g, Dp, pose_solver=lambda S, r: ldl16_kernel_arithmetic(S, r, None, comp_mask))


def peers(H, g, Dp, chain):
    """{name: x} of the fp64 peers that apply to the system"""
    from tests.chain_emulation import chain_solve, is_chain_structured
    out = {"numpy": np.linalg.solve(H, g), "ldl16": ldl16_emulation(H, g, Dp)}
    if chain and Dp >= 6 and Dp < H.shape[0] and is_chain_structured(H, Dp):
        out["chain"] = chain_solve(H, g, Dp)
    return out
