"""The cases of the solver referee (tests/test_solve_statement_host.py on the CPU, tests/test_gpu_solve_referee.py on the GPU): seeded
reduced systems at the block and chunk edges of ba_ldl16.hpp / ba_chain.hpp.  Test infrastructure, no GPU.

A case is (family, name, D, Dp, kind, seed) and the solvers it goes through; system(case) builds H, g once, reference_of(case) the
50-digit solution once (shared by the dense, chain and mask tests of one system; neither is ever modified).

Families — the unit over which a bound is taken (solve_statement's docstring):
  dense      random dense SPD, Dp = D (no reordering), no zero block
  chain      chain-structured systems without a prior (tests/chain_emulation.chain_structured_system): the dense solver with the
             speed/bias rows first, and the chain solver
  struct     the same shapes with other couplings, and 16-block structures (block-diagonal, diagonal, arrow, reverse arrow)
  axis       a 1e16 added to diagonal entries at and next to a 16-block edge: Jacobi scaling removes it, the bound stays tight
  rotated    the project's rotated prior 1e16 n n^T on the first pose: the fp64 peers themselves scatter over orders of magnitude
             here, seed by seed; the family referees the compensated elimination only (comp_mask), not the solver's structure"""
import functools
from collections import namedtuple

import numpy as np

from tests import solve_statement as st
from tests.chain_emulation import chain_structured_system

Case = namedtuple("Case", "family name D Dp kind seed modes")

# What the fp64 peers reach against the reference over each family's cases (e_ref, rho_ref), measured on the CPU by
# tests/test_solve_statement_host.py::test_family_bounds, which fails when the peers leave them by more than a quarter (LAPACK's
# last bits differ between builds) or when they are more than 1.5 x what the peers reach (rounded up to two digits;
# profiles/solve_referee_notes.md has the per-case figures).  Never from a kernel.
FAMILY_REF = {
    "dense": (1.1e-15, 1.2e-16),
    "chain": (4.2e-15, 1.2e-16),
    "struct": (4.0e-15, 1.7e-16),
    "axis": (4.1e-15, 7.0e-17),
    "rotated": (3.2e-5, 5.9e-17),
}

# Behind the rotated prior, with the comp_mask of the index build: how far from the better of a case's plain peers (in rho) a CPU peer
# sits that restates the kernel's arithmetic (solve_statement.ldl16_kernel_arithmetic: in-place elimination, reciprocal multipliers,
# fused updates, the compensated second update), the largest ratio over the family's cases, per solver; measured by
# tests/test_solve_statement_host.py::test_rotated_factor_of_the_kernel_arithmetic (12.8 and 6.8), rounded up.  The GPU test holds the
# kernel's rho, case by case, to this multiple of the better peer's — BOUND_FACTOR raised as far as that peer reaches, no further.
ROTATED_RHO_FACTOR = {"dense": 13.0, "chain": 6.9}

DENSE_D = [1, 2, 3, 6, 14, 15, 16, 17] + [16 * k + o for k in range(2, 11) for o in (-1, 0, 1)] + [173, 174]
REORDERED = [(48, 12), (48, 30), (96, 24), (96, 60), (144, 36), (144, 54), (144, 90), (144, 126), (150, 60), (168, 6), (174, 12), (174, 48)]
CHAIN_ONLY = [(15, 6), (24, 6), (33, 6),                                   # Ks = 1, 2, 3
              (57, 48), (66, 48), (105, 96), (114, 96), (153, 144),        # npl = 0 in the pose system
              (69, 60), (78, 60), (75, 66), (84, 66),                      # the 64-column edge of the column waves
              (135, 126), (144, 126), (141, 132), (150, 132),              # the 128-column edge
              (165, 156), (156, 120)]                                      # the largest that fit
CHAIN_UNFIT = [(162, 144), (174, 156), (174, 120), (171, 162)]             # the upload's fit rule refuses them (the guard test)
STRUCT_SB_SHAPES = [(48, 30), (75, 66), (141, 132), (144, 54)]             # a multiple of 16, both chunk edges
STRUCT_SB_KINDS = ["all_poses", "no_poses", "last_pose", "no_neighbours"]  # ("neighbours" is the chain family itself)
STRUCT_16_D = [48, 81, 144, 174]
STRUCT_16_KINDS = ["blockdiag16", "diagonal", "arrow", "reverse_arrow"]
AXIS_ROWS = [(3,), (15, 16), (0, 47)]
COND_SHAPES = [(48, 48), (96, 60), (144, 54), (141, 132)]                  # (D, Dp); Dp = D: the dense family's system


def _cases():
    out = []
    for D in DENSE_D:
        out.append(Case("dense", f"dense-{D}", D, D, "dense", 100 + D, ("dense",)))
    seen = set()
    for D, Dp in REORDERED + CHAIN_ONLY:
        if (D, Dp) in seen:
            continue
        seen.add((D, Dp))
        modes = (("dense",) if (D, Dp) in REORDERED else ()) + ("chain",)
        out.append(Case("chain", f"chain-{D}-{Dp}", D, Dp, "neighbours", 1000 * D + Dp, modes))
    for D, Dp in STRUCT_SB_SHAPES:
        for kind in STRUCT_SB_KINDS:
            out.append(Case("struct", f"{kind}-{D}-{Dp}", D, Dp, kind, 1000 * D + Dp + 7, ("dense", "chain")))
        out.append(Case("struct", f"diagonal-{D}-{Dp}", D, Dp, "diagonal", 1000 * D + Dp + 9, ("dense", "chain")))
    for D in STRUCT_16_D:
        for kind in STRUCT_16_KINDS:
            out.append(Case("struct", f"{kind}-{D}", D, D, kind, 2000 + D, ("dense",)))
    for D, Dp in COND_SHAPES:
        modes = ("dense",) if Dp == D else ("dense", "chain")
        for rows in AXIS_ROWS:
            out.append(Case("axis", f"axis{'_'.join(map(str, rows))}-{D}-{Dp}", D, Dp, ("axis", rows), 3000 + D + Dp, modes))
        if Dp < D:
            out.append(Case("rotated", f"rotated-{D}-{Dp}", D, Dp, "rotated", 4000 + D + Dp, modes))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def runs():
    """(case, mode) for every solver a case goes through, the sizes ascending"""
    return sorted(((c, m) for c in CASES for m in c.modes), key=lambda cm: (cm[0].D, cm[0].Dp, cm[0].name, cm[1]))


def _dense_spd(rng, D):
    J = rng.standard_normal((3 * D + 8, D))
    return J.T @ J


def _sb_structure(rng, D, Dp, kind):
    """chain_structured_system's construction with other couplings of the speed/bias blocks"""
    n_pose, n_sb = Dp // 6, (D - Dp) // 9
    H = np.zeros((D, D))
    Jp = rng.standard_normal((4 * Dp + 8, Dp))
    H[:Dp, :Dp] = Jp.T @ Jp
    for k in range(n_sb):
        cols = list(range(Dp + 9 * k, Dp + 9 * k + 9))
        if k + 1 < n_sb and kind != "no_neighbours":
            cols += list(range(Dp + 9 * (k + 1), Dp + 9 * (k + 1) + 9))
        poses = {"all_poses": range(n_pose), "no_poses": (), "last_pose": (n_pose - 1,),
                 "no_neighbours": (min(k, n_pose - 1), min(k + 1, n_pose - 1))}[kind]
        for p in poses:
            cols += list(range(6 * p, 6 * p + 6))
        cols = sorted(set(cols))
        Jk = rng.standard_normal((len(cols) + 6, len(cols)))
        H[np.ix_(cols, cols)] += Jk.T @ Jk
    H[np.arange(Dp, D), np.arange(Dp, D)] += 1e-3
    return 0.5 * (H + H.T)


def _block16_structure(rng, D, kind):
    nb = (D + 15) // 16
    H = np.zeros((D, D))
    if kind == "diagonal":
        H[np.arange(D), np.arange(D)] = rng.uniform(0.5, 50.0, D)
        return H
    for I in range(nb):
        s = slice(16 * I, min(16 * I + 16, D))
        H[s, s] = _dense_spd(rng, s.stop - s.start)
    if kind in ("arrow", "reverse_arrow") and nb > 1:
        # the coupling of one block row to every other block, scaled so that the matrix stays well inside the positive definite
        hub = slice(16 * (nb - 1), D) if kind == "arrow" else slice(0, 16)
        rest = np.setdiff1d(np.arange(D), np.arange(hub.start, hub.stop))
        C = rng.standard_normal((hub.stop - hub.start, rest.size))
        H[hub, rest] = C
        H[rest, hub] = C.T
        lam = np.linalg.eigvalsh(H)[0]
        if lam < 10.0:
            H[np.arange(D), np.arange(D)] += 10.0 - lam
    return H


@functools.lru_cache(maxsize=None)
def system(case):
    """(H, g) of the case: read-only arrays"""
    rng = np.random.default_rng(case.seed)
    D, Dp, kind = case.D, case.Dp, case.kind
    if kind == "dense":
        H, g = _dense_spd(rng, D), rng.standard_normal(D)
    elif kind == "neighbours":
        H, g, _ = chain_structured_system(rng, Dp // 6, (D - Dp) // 9, pose_prior=0.0)
    elif kind == "rotated":
        H, g, _ = chain_structured_system(rng, Dp // 6, (D - Dp) // 9, pose_prior=1e16)
    elif kind in STRUCT_SB_KINDS:
        H, g = _sb_structure(rng, D, Dp, kind), rng.standard_normal(D)
    elif kind in STRUCT_16_KINDS:
        H, g = _block16_structure(rng, D, kind), rng.standard_normal(D)
    elif kind[0] == "axis":
        if Dp == D:
            H, g = _dense_spd(rng, D), rng.standard_normal(D)
        else:
            H, g, _ = chain_structured_system(rng, Dp // 6, (D - Dp) // 9, pose_prior=0.0)
        for r in kind[1]:
            H[r, r] += 1e16
    else:
        raise ValueError(kind)
    H, g = np.ascontiguousarray(H), np.ascontiguousarray(g)
    assert np.array_equal(H, H.T)
    H.setflags(write=False)
    g.setflags(write=False)
    return H, g


@functools.lru_cache(maxsize=None)
def reference_of(case):
    x = st.reference(*system(case))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def peers_of(case):
    """{peer: (e, rho)} of the case's fp64 peers against its reference"""
    H, g = system(case)
    xr = reference_of(case)
    return {n: (st.e(x, xr), st.rho(H, g, x)) for n, x in st.peers(H, g, case.Dp, "chain" in case.modes).items()}


SOLVE_LDS_LIMIT_CHAIN = 144 * 1024     # ba_solve.hpp


def chain_doubles(D, Dp):
    """LChain::make(D, Dp).total (ba_chain.hpp), restated"""
    nb16 = lambda n: (n + 16) // 16
    area = lambda n: max(nb16(n) * (nb16(n) + 1) // 2 * 256, 2 * nb16(n) * 256 + 3 * nb16(n) * 288 + 1024 + 2 * nb16(n) * 16 + 288)
    Ks, NP = (D - Dp) // 9, (Dp + 2) & ~1
    oA = nb16(Dp) * (nb16(Dp) + 1) // 2 * 256
    oX = oA + Ks * 90 + max(Ks - 1, 1) * 180 + Ks * 90
    oN = (max(oX + 90 + 9 * NP, area(Dp)) + 1) & ~1
    return oN + Ks * 9 * NP + 2 * Ks * 90 + Ks * 10 + 12


def chain_launch_bytes(doubles, D):
    """solve_smem_chain (capi_launch.inc) of a launch with that many chain doubles and a largest reduced dimension D"""
    return (doubles + 4 * ((D + 5) // 6) * 6) * 8 + 16


def chain_fits(D, Dp):
    """the fit rule of the index build (BuildCtx::layout) for a forced chain solve"""
    return Dp >= 6 and D > Dp and (Dp + 1 + 63) // 64 <= 3 and chain_launch_bytes(chain_doubles(D, Dp), D) <= SOLVE_LDS_LIMIT_CHAIN


def bound(family):
    e_ref, rho_ref = FAMILY_REF[family]
    return st.BOUND_FACTOR * e_ref, st.BOUND_FACTOR * rho_ref


def better_peer_rho(case):
    return min(v[1] for v in peers_of(case).values())


def prior_mask(case, mode):
    """the comp_mask the index build derives for a prior on the first pose: the 16-blocks that hold reduced rows 0 .. 5, in the
    order of the solver that factorises them (dense: speed/bias rows first, L16::perm; chain: the pose system's own blocks)"""
    first = 0 if (mode == "chain" or case.Dp == case.D) else case.D - case.Dp
    return (1 << (first >> 4)) | (1 << ((first + 5) >> 4))
