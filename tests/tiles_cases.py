"""The cases of the tiled Cholesky's referee (tests/test_tiles_statement_host.py on the CPU, tests/test_gpu_tiles_referee.py on the GPU):
seeded SPD systems at the tile edges of ba_chol_tiles.hpp (48) and at the panel edges of ct_ldl_inv48 (16).  Test infrastructure,
no GPU.

A case is (family, name, n, kind, seed); system(case) builds S, g once, reference_of(case) the 50-digit solution once (neither is
ever modified).  The sizes are the smallest at which each part of the kernel first runs: nT = 1 .. 6, both sides of every tile
edge, exact multiples of 48 (no padding) at nT = 2 .. 6, the three 16-panels inside one tile, the smallest D a window sends here
(175).  nT = 3 is the first size with a diagonal task's k < j - 1 sums, a general tile (i, j >= 1) and a far tile in the
back-substitution; nT = 4 the first with a general tile that has a k >= 1 update.

Families — the unit over which a bound is taken (tiles_statement's docstring):
  dense      J^T J as in solve_cases._dense_spd
  struct     tile structures: block-diagonal by tiles (every off-diagonal tile exactly zero), diagonal, arrow (dense last tile row
             only), reverse arrow (dense first tile column only), tridiagonal by tiles
  graded     S -> d S d with d = 10^U(0, 4), the right-hand side scaled alike
  axis       1e16 added to diagonal entries at and next to tile and panel edges: Jacobi scaling removes it, the bound stays tight
  rotated    1e16 n n^T with a random unit n on rows 3 .. 5 (the project's yaw prior, inside tile 0) and on rows 46 .. 48
             (straddling the first tile edge): the plain peers themselves scatter over orders of magnitude in e here; the family
             cannot referee structure, it referees the claim that the uncompensated tile elimination is good enough"""
import functools
from collections import namedtuple

import numpy as np

from tests import tiles_statement as ts
from tests.solve_cases import _dense_spd

Case = namedtuple("Case", "family name n kind seed")

# What the fp64 peers reach against the reference over each family's cases (e_ref: the worst of the three peers; rho_ref: the worst
# of the two Cholesky peers), measured on the CPU by tests/test_tiles_statement_host.py::test_family_bounds, which fails when the
# peers leave them by more than a quarter (LAPACK's last bits differ between builds) or when they are more than 1.5 x what the
# peers reach (rounded up to two digits; profiles/tiles_referee_notes.md has the per-case figures).  Never from a kernel.
FAMILY_REF = {
    "dense": (1.3e-15, 1.2e-16),
    "struct": (1.1e-15, 1.5e-16),
    "graded": (2.8e-14, 6.8e-17),       # (e: numpy's pivoted LU, 1.5e-14 .. 2.8e-14; the two Cholesky peers 2.5e-16 .. 8.6e-16)
    "axis": (1.2e-15, 8.7e-17),
    "rotated": (9.4e-4, 8.3e-17),
}

# Behind the rotated prior: how far from the better of a case's plain peers (in rho) a CPU peer sits that restates the kernel's
# arithmetic (tiles_statement.tiled_kernel_arithmetic: ct_ldl_inv48's in-place elimination with reciprocal pivots and fused updates,
# not compensated), the largest ratio over the family's cases; measured by
# tests/test_tiles_statement_host.py::test_rotated_factor_of_the_kernel_arithmetic, rounded up.  The GPU test holds the kernel's rho,
# case by case, to this multiple of the better peer's.  Measured, case by case (rotated3-97, rotated46-97, rotated3-193, ..):
# 39850, 1.8, 33614, 0.6, 602, 3.0 — with the prior inside one 16-block of tile 0 (rows 3 .. 5) the uncompensated elimination
# leaves rho = 6.3e-15 .. 6.1e-13, 19 to 1850 times the family's bound; with the prior across the tile edge (rows 46 .. 48, the
# last pivots of tile 0 and the first of tile 1) it is an ordinary peer.  Recorded: the largest, 39850, plus the quarter by which
# LAPACK's last bits move the plain peers between builds (the allowance of FAMILY_REF; the better peer of rotated3-193, numpy's LU,
# was seen at 3.7e-18 on one host and 9.6e-18 on another), rounded up.
ROTATED_RHO_FACTOR = 5.0e4
# The cases on which that CPU peer leaves the family's rho bound (asserted by the same host test): there the kernel's rho is held to
# ROTATED_RHO_FACTOR alone and recorded, as the LDS referee does for a comp_mask that leaves the prior's block uncovered; e is held
# to the family's bound everywhere.
ROTATED_UNCOMPENSATED = ("rotated3-97", "rotated3-193", "rotated3-240")

DENSE_N = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97, 143, 144, 145, 175, 191, 192, 193, 240, 241, 288]
STRUCT_N = [144, 193, 240]
STRUCT_KINDS = ["blockdiag48", "diagonal", "arrow", "reverse_arrow", "tridiag48"]
COND_N = [97, 193, 240]
AXIS_ROWS = [(3,), (15, 16), (47, 48), (-1,)]
ROTATED_ROWS = [3, 46]


def _cases():
    out = [Case("dense", f"dense-{n}", n, "dense", 100 + n) for n in DENSE_N]
    for n in STRUCT_N:
        out += [Case("struct", f"{kind}-{n}", n, kind, 2000 + n) for kind in STRUCT_KINDS]
    for n in COND_N:
        out.append(Case("graded", f"graded-{n}", n, "graded", 5000 + n))
        for rows in AXIS_ROWS:
            rows = tuple(r % n for r in rows)
            out.append(Case("axis", f"axis{'_'.join(map(str, rows))}-{n}", n, ("axis", rows), 3000 + n))
        out += [Case("rotated", f"rotated{r0}-{n}", n, ("rotated", r0), 4000 + n + r0) for r0 in ROTATED_ROWS]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = list(FAMILY_REF)


def _tile_structure(rng, n, kind):
    nT = ts.n_tiles(n)
    S = np.zeros((n, n))
    if kind == "diagonal":
        S[np.arange(n), np.arange(n)] = rng.uniform(0.5, 50.0, n)
        return S
    sl = [slice(ts.TB * I, min(ts.TB * I + ts.TB, n)) for I in range(nT)]
    for s in sl:
        S[s, s] = _dense_spd(rng, s.stop - s.start)
    if kind == "blockdiag48":
        return S
    pairs = {"arrow": [(nT - 1, J) for J in range(nT - 1)], "reverse_arrow": [(I, 0) for I in range(1, nT)],
             "tridiag48": [(I + 1, I) for I in range(nT - 1)]}[kind]
    for I, J in pairs:
        C = rng.standard_normal((sl[I].stop - sl[I].start, sl[J].stop - sl[J].start))
        S[sl[I], sl[J]] = C
        S[sl[J], sl[I]] = C.T
    # the couplings scaled against the diagonal so that the matrix stays well inside the positive definite
    lam = np.linalg.eigvalsh(S)[0]
    if lam < 10.0:
        S[np.arange(n), np.arange(n)] += 10.0 - lam
    return S


@functools.lru_cache(maxsize=None)
def system(case):
    """(S, g) of the case: read-only arrays"""
    rng = np.random.default_rng(case.seed)
    n, kind = case.n, case.kind
    if kind in STRUCT_KINDS:
        S, g = _tile_structure(rng, n, kind), rng.standard_normal(n)
    else:
        S, g = _dense_spd(rng, n), rng.standard_normal(n)
        if kind == "graded":
            d = 10.0 ** rng.uniform(0.0, 4.0, n)
            S, g = d[:, None] * S * d[None, :], d * g
        elif isinstance(kind, tuple) and kind[0] == "axis":
            for r in kind[1]:
                S[r, r] += 1e16
        elif isinstance(kind, tuple) and kind[0] == "rotated":
            v = rng.standard_normal(3)
            v /= np.linalg.norm(v)
            rows = np.arange(kind[1], kind[1] + 3)
            S[np.ix_(rows, rows)] += 1e16 * np.outer(v, v)
    S = np.ascontiguousarray(0.5 * (S + S.T))
    g = np.ascontiguousarray(g)
    assert np.array_equal(S, S.T)
    S.setflags(write=False)
    g.setflags(write=False)
    return S, g


@functools.lru_cache(maxsize=None)
def reference_of(case):
    x = ts.reference(*system(case))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def peers_of(case):
    """{peer: (e, rho)} of the case's fp64 peers against its reference"""
    S, g = system(case)
    xr = reference_of(case)
    return {name: (ts.e(x, xr), ts.rho(S, g, x)) for name, x in ts.peers(S, g).items()}


def family_reach(family):
    """(e, rho) the family's peers reach: e the worst of all peers, rho the worst of the two Cholesky peers"""
    we = wr = 0.0
    for c in (c for c in CASES if c.family == family):
        p = peers_of(c)
        we = max(we, max(v[0] for v in p.values()))
        wr = max(wr, max(p[k][1] for k in ts.CHOLESKY_PEERS))
    return we, wr


def bound(family):
    e_ref, rho_ref = FAMILY_REF[family]
    return ts.BOUND_FACTOR * e_ref, ts.BOUND_FACTOR * rho_ref


def better_peer(case):
    """(e, rho) of the better of the case's peers, each figure on its own"""
    p = peers_of(case)
    return min(v[0] for v in p.values()), min(v[1] for v in p.values())
