"""CPU: the statement the tiled Cholesky is refereed against (tests/tiles_statement.py) and its cases (tests/tiles_cases.py), checked
without a GPU — what the fp64 peers reach per family (the bound of tests/test_gpu_tiles_referee.py, printed here: run with -s),
every mutation of the tile emulation beyond that bound on every case it changes, and how far the kernel's arithmetic, restated,
sits from the better plain peer behind the rotated prior."""
import numpy as np
import pytest

from tests import tiles_cases as tc
from tests import tiles_statement as ts

# the least factor by which a mutation must leave a family's bound (measured: 1.9e12 and more in the four tight families, 4.9e6 and
# more behind the rotated prior; the per-mutation figures are in profiles/tiles_referee_notes.md)
MUTATION_MARGIN = {"dense": 1e11, "struct": 1e11, "graded": 1e11, "axis": 1e11, "rotated": 1e6}


def test_emulation_is_a_solver_and_the_restated_arithmetic_an_ordinary_peer_where_nothing_cancels():
    # an exact system: powers of four on the diagonal of two tiles (every root and quotient is exact), the padding behind them
    n = 50
    S = np.diag(4.0 ** (np.arange(n) % 5))
    g = np.arange(1.0, n + 1)
    assert np.array_equal(ts.tiled_emulation(S, g), g / np.diag(S))
    for name in ("dense-49", "dense-97", "axis15_16-97", "graded-97"):
        c = tc.BY_NAME[name]
        S, g = tc.system(c)
        x = ts.tiled_kernel_arithmetic(S, g)
        ek, rk = ts.e(x, tc.reference_of(c)), ts.rho(S, g, x)
        print(f"  kernel arithmetic {name:16s} e {ek:.2e} rho {rk:.2e}")
        assert ek <= tc.bound(c.family)[0] and rk <= tc.bound(c.family)[1]


@pytest.mark.parametrize("where", [0, 15, 16, 47, 48, 96])
def test_guard_restated_leaves_the_pivot_out_and_everything_finite(where):
    """ldl16_pivot<.., GUARD>: a pivot that is not positive takes no part in the elimination.  Restated, x is finite, zero in that
    row and elsewhere the solution of the system without that row and column (replacing the pivot by 1, as the kernel did until this
    referee, overflows: the multipliers of a dense block are squared into what is left at every later pivot that fails in turn)"""
    S, g = tc.system(tc.BY_NAME["dense-97"])
    keep = np.arange(97) != where
    want = np.linalg.solve(S[np.ix_(keep, keep)], g[keep])
    for value in (-1.0, 0.0):
        Sb = S.copy()
        Sb[where, where] = value
        x = ts.tiled_kernel_arithmetic(Sb, g)
        assert x[where] == 0.0 and np.abs(x[keep] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_family_bounds(family):
    """e_ref = the largest e the three peers reach over the family's cases, rho_ref = the largest rho of the two Cholesky peers: the
    recorded pair holds them and is tight"""
    for c in (c for c in tc.CASES if c.family == family):
        for peer, (e, r) in tc.peers_of(c).items():
            print(f"  peer {c.name:20s} {peer:6s} e {e:.2e} rho {r:.2e}")
    worst_e, worst_r = tc.family_reach(family)
    e_ref, rho_ref = tc.FAMILY_REF[family]
    print(f"family {family}: e_ref {worst_e:.3e} (recorded {e_ref:.1e})  rho_ref {worst_r:.3e} (recorded {rho_ref:.1e})")
    # (LAPACK's last bits depend on the build and its thread count: the recorded pair must be what the peers reach to within a
    #  quarter, not to the digit)
    assert worst_e <= 1.25 * e_ref <= 1.875 * worst_e and worst_r <= 1.25 * rho_ref <= 1.875 * worst_r


def test_rotated_factor_of_the_kernel_arithmetic():
    """behind the rotated prior: rho of the peer that restates ct_ldl_inv48's uncompensated elimination against the better of the
    case's plain peers; the recorded factor holds that peer and is tight"""
    worst = 0.0
    for c in (c for c in tc.CASES if c.family == "rotated"):
        S, g = tc.system(c)
        be, br = tc.better_peer(c)
        x = ts.tiled_kernel_arithmetic(S, g)
        ek, rk = ts.e(x, tc.reference_of(c)), ts.rho(S, g, x)
        print(f"  kernel arithmetic {c.name:16s} e {ek:.2e} = {ek / be:8.2f} x the better peer's {be:.2e}   rho {rk:.2e} = {rk / br:8.1f} x the better peer's {br:.2e}")
        worst = max(worst, rk / br)
        # where the restated arithmetic leaves the family's rho bound the kernel's rho is recorded, not held to that bound
        assert (rk > tc.bound("rotated")[1]) == (c.name in tc.ROTATED_UNCOMPENSATED), c.name
        assert ek <= tc.bound("rotated")[0], c.name
    f = tc.ROTATED_RHO_FACTOR
    print(f"rotated: the kernel-arithmetic peer reaches {worst:.2f} x the better peer in rho (recorded {f})")
    # (the recorded factor is what that peer reaches plus a quarter for LAPACK's last bits in the plain peers, no more)
    assert 1.25 * worst <= 1.02 * f and f <= 1.5 * worst


def test_every_case_is_what_its_name_says():
    assert len(tc.CASES) == 23 + 15 + 3 + 12 + 6
    assert {ts.n_tiles(c.n) for c in tc.CASES if c.family == "dense"} == {1, 2, 3, 4, 5, 6}
    assert {c.n for c in tc.CASES if c.family == "dense" and c.n % 48 == 0} == {48, 96, 144, 192, 240, 288}
    for c in tc.CASES:
        S, g = tc.system(c)
        assert S.shape == (c.n, c.n) and g.shape == (c.n,) and np.all(np.diag(S) > 0)
    tile = lambda S, I, J: S[48 * I:48 * I + 48, 48 * J:48 * J + 48]
    for n in tc.STRUCT_N:
        nT = ts.n_tiles(n)
        off = [(I, J) for I in range(nT) for J in range(I)]
        full = {"blockdiag48": [], "diagonal": [], "arrow": [(nT - 1, J) for J in range(nT - 1)],
                "reverse_arrow": [(I, 0) for I in range(1, nT)], "tridiag48": [(I + 1, I) for I in range(nT - 1)]}
        for kind, want in full.items():
            S, _ = tc.system(tc.BY_NAME[f"{kind}-{n}"])
            assert [p for p in off if np.any(tile(S, *p))] == sorted(want), (kind, n)
    for c in (c for c in tc.CASES if c.family in ("axis", "rotated")):
        S, _ = tc.system(c)
        big = np.nonzero(np.diag(S) > 1e14)[0]
        if c.family == "axis":
            assert set(big) == set(c.kind[1]), c.name
        else:       # (a component of the unit vector may be small)
            assert len(big) >= 2 and set(big) <= set(range(c.kind[1], c.kind[1] + 3)), c.name


def _mutants(name):
    """(case, x of the mutated emulation) for every case the mutation changes a bit of"""
    for c in tc.CASES:
        S, g = tc.system(c)
        x0, x1 = ts.tiled_emulation(S, g), ts.tiled_emulation(S, g, mutation=name)
        if not np.array_equal(x0, x1, equal_nan=True):
            yield c, x1


# What no referee of x can see, measured: row n - 1 = 96 is alone in the last tile of axis96-97 and carries the 1e16, so x_2 is 1e-16
# of the solution and L_(2,0) 1e-8 of the matrix — the far tile's term is below the last bit of t_0's rounding error, and an
# emulation without it stays inside the bound (factor 0.6).  A kernel with that defect is right to working precision on that system.
UNSEEN = {("skip_far_tile", "axis96-97")}

# the tile counts from which a mutation has something to change (the padding: every n that is no multiple of 48)
FIRST_NT = {"skip_chain_last_update": 2, "skip_forward_term": 2, "transpose_sub": 2, "skip_far_tile": 3, "tile_index_shift": 4}


@pytest.mark.parametrize("name", ts.MUTATIONS)
def test_the_cases_notice_every_mutation(name):
    """an emulation broken the way the kernel could be leaves its family's bound on every case it touches: by more than 1e11 where the
    family is well conditioned, graded or axis-aligned, by more than 1e6 behind the rotated prior (MUTATION_MARGIN) — but for the
    one pair of UNSEEN, which is asserted to stay inside.  A mutation that finds zero tiles where it strikes (the tile structures)
    changes no bit there and is not counted; every family must still have a case that it changes"""
    least, touched = {}, set()
    for c, x in _mutants(name):
        S, g = tc.system(c)
        be, br = tc.bound(c.family)
        f = max(ts.e(x, tc.reference_of(c)) / be, ts.rho(S, g, x) / br) if np.all(np.isfinite(x)) else np.inf
        print(f"  mutation {name:24s} {c.name:20s} beyond the bound by {f:.1e}")
        touched.add(c.name)
        if (name, c.name) in UNSEEN:
            assert f <= 1.0, (c.name, f)      # (a record that has gone stale is an error too)
            continue
        least[c.family] = min(least.get(c.family, np.inf), f)
    print(f"mutation {name}: least factor beyond the bound per family {({k: float(f'{v:.2g}') for k, v in least.items()})}")
    assert set(least) == set(tc.FAMILIES), least
    assert all(f > MUTATION_MARGIN[fam] for fam, f in least.items()), least
    # every dense case the mutation can reach is touched
    for c in (c for c in tc.CASES if c.family == "dense"):
        reach = c.n % 48 != 0 if name == "zero_padding" else ts.n_tiles(c.n) >= FIRST_NT[name]
        assert (c.name in touched) == reach, c.name
