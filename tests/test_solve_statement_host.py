"""CPU: the statement the LDS solvers are refereed against (tests/solve_statement.py) and its cases (tests/solve_cases.py), checked
without a GPU — the 50-digit reference, what the fp64 peers reach per family (the bound of tests/test_gpu_solve_referee.py, printed
here: run with -s), every mutation of the two emulations far beyond that bound, the LDS arithmetic behind the chain solver's fit
rule, and the refusals of okvis_ba_reduced_solve that need no device."""
import ctypes as C

import numpy as np
import pytest

from okvis_amd import _lib
from okvis_amd.window import SOLVE_CHAIN, SOLVE_DENSE
from tests import solve_cases as sc
from tests import solve_statement as st
from tests.chain_emulation import chain_solve, chain_structured_system, is_chain_structured

FAMILIES = list(sc.FAMILY_REF)
ERR_ARG = -1


def test_reference_solves_to_the_last_bit_of_an_exact_system():
    # powers of two: every quotient is exact, so the rounded 50-digit solution is the solution
    H = np.diag([1.0, 2.0, 4.0, 0.5])
    g = np.array([3.0, 5.0, -7.0, 0.25])
    assert np.array_equal(st.reference(H, g), g / np.diag(H))
    # integers: a system whose solution is known in closed form
    n = 12
    H = np.minimum.outer(np.arange(1, n + 1), np.arange(1, n + 1)).astype(float)      # min(i, j): inverse is the second difference
    x = np.arange(1.0, n + 1)
    assert np.array_equal(st.reference(H, H @ x), x)
    rng = np.random.default_rng(1)
    Hc, gc, _ = chain_structured_system(rng, 4, 4, pose_prior=1e16)
    xr = st.reference(Hc, gc)
    assert st.rho(Hc, gc, xr) < 2.0 ** -52 and st.e(xr, xr) == 0.0


@pytest.mark.parametrize("family", FAMILIES)
def test_family_bounds(family):
    """e_ref, rho_ref of the family = the largest its fp64 peers reach over its cases: the recorded pair holds them and is tight"""
    worst_e = worst_r = 0.0
    for c in (c for c in sc.CASES if c.family == family):
        for peer, (e, r) in sc.peers_of(c).items():
            print(f"  peer {c.name:24s} {peer:6s} e {e:.2e} rho {r:.2e}")
            worst_e, worst_r = max(worst_e, e), max(worst_r, r)
    e_ref, rho_ref = sc.FAMILY_REF[family]
    print(f"family {family}: e_ref {worst_e:.3e} (recorded {e_ref:.1e})  rho_ref {worst_r:.3e} (recorded {rho_ref:.1e})")
    # (numpy.linalg.solve goes through LAPACK, whose last bits depend on the build and its thread count: the recorded pair must
    #  be what the peers reach to within a quarter, not to the digit)
    assert worst_e <= 1.25 * e_ref <= 1.875 * worst_e and worst_r <= 1.25 * rho_ref <= 1.875 * worst_r


def test_rotated_factor_of_the_kernel_arithmetic():
    """behind the rotated prior the plain peers' rho sit at a tenth of the unit roundoff; a peer that restates the kernel's arithmetic
    sits up to 12.8 (dense) and 6.8 (chain solver's pose system) times above the better of them with the index build's mask — and
    at 1e-13, thousands of times above, without it: the recorded factors hold that peer and are tight"""
    for mode in ("dense", "chain"):
        worst = 0.0
        for c in (c for c in sc.CASES if c.family == "rotated"):
            H, g = sc.system(c)
            xr, better = sc.reference_of(c), sc.better_peer_rho(c)
            for mask in (sc.prior_mask(c, mode), 0):
                x = st.kernel_arithmetic_peer(H, g, c.Dp, mode, mask)
                r = st.rho(H, g, x)
                print(f"  kernel arithmetic {c.name:18s} {mode:5s} mask {mask:#4x} e {st.e(x, xr):.2e} rho {r:.2e} = {r / better:8.1f} x the better peer's {better:.2e}")
                if mask:
                    worst = max(worst, r / better)
        f = sc.ROTATED_RHO_FACTOR[mode]
        print(f"rotated, {mode}: the kernel-arithmetic peer reaches {worst:.2f} x the better peer (recorded {f})")
        assert st.BOUND_FACTOR <= worst <= 1.1 * f <= 1.25 * worst
    # the same peer is an ordinary peer where nothing cancels: within the family bounds on a well-conditioned and an axis case
    for name in ("dense-96", "chain-96-60", "axis3-96-60"):
        c = sc.BY_NAME[name]
        H, g = sc.system(c)
        for mode in c.modes:
            x = st.kernel_arithmetic_peer(H, g, c.Dp, mode, 0xFFFFFFFF)
            assert st.e(x, sc.reference_of(c)) <= sc.bound(c.family)[0] and st.rho(H, g, x) <= sc.bound(c.family)[1]


def test_every_case_is_what_its_name_says():
    for c in sc.CASES:
        H, g = sc.system(c)
        assert H.shape == (c.D, c.D) and (c.D - c.Dp) % 9 == 0 and np.all(np.diag(H) > 0)
        if "chain" in c.modes:
            assert is_chain_structured(H, c.Dp) and sc.chain_fits(c.D, c.Dp), c.name
    multiples = [c for c in sc.CASES if c.D % 16 == 0]
    assert {c.D for c in multiples if c.family == "dense"} == {16 * k for k in range(1, 11)}
    assert {c.Dp for c in sc.CASES if "chain" in c.modes and c.Dp % 16 == 0} >= {48, 96, 144}
    # a block that is zero on input and fills in: the reverse arrow's, and the speed/bias chain's in the dense solver's order
    H, _ = sc.system(sc.BY_NAME["reverse_arrow-81"])
    assert not np.any(H[16:32, 32:48]) and np.any(H[0:16, 16:32]) and np.any(H[0:16, 32:48])


def _mutants(name):
    """(case, x of the mutated emulation) for every case the mutation changes a bit of"""
    chain = name.startswith("chain:")
    for c in sc.CASES:
        H, g = sc.system(c)
        if chain:
            if "chain" not in c.modes:
                continue
            x0, x1 = chain_solve(H, g, c.Dp), chain_solve(H, g, c.Dp, mutation=name[6:])
        else:
            x0, x1 = st.ldl16_emulation(H, g, c.Dp), st.ldl16_emulation(H, g, c.Dp, mutation=name)
        if not np.array_equal(x0, x1):
            yield c, x1


@pytest.mark.parametrize("name", list(st.MUTATIONS_LDL16) + ["chain:" + m for m in st.MUTATIONS_CHAIN])
def test_the_cases_notice_every_mutation(name):
    """an emulation broken the way a kernel could be leaves its family's bound on every case it touches: by more than 1e9 (asserted;
    measured: 1e12 and more) where the family is well conditioned or axis-aligned, by more than 1 behind the rotated prior
    (asserted; measured: 4e7 and more, through rho)"""
    least = {}
    for c, x in _mutants(name):
        H, g = sc.system(c)
        be, br = sc.bound(c.family)
        f = max(st.e(x, sc.reference_of(c)) / be, st.rho(H, g, x) / br)
        print(f"  mutation {name:28s} {c.name:24s} beyond the bound by {f:.1e}")
        least[c.family] = min(least.get(c.family, np.inf), f)
    print(f"mutation {name}: least factor beyond the bound per family {({k: float(f'{v:.2g}') for k, v in least.items()})}")
    tight = [f for fam, f in least.items() if fam != "rotated"]
    assert tight and min(tight) > 1e9, least
    assert all(f > 1.0 for f in least.values()), least


def test_chain_lds_arithmetic_of_the_fit_rule_and_of_mixed_batches():
    assert sc.chain_doubles(156, 120) == 17740
    for D, Dp in sc.CHAIN_ONLY + sc.REORDERED:
        assert sc.chain_fits(D, Dp), (D, Dp)
    for D, Dp in sc.CHAIN_UNFIT:
        assert not sc.chain_fits(D, Dp), (D, Dp)
    # two windows that fit alone and not together: the launch is sized from the larger LChain::total and the larger dimension
    for D, Dp in [(174, 12), (174, 30), (174, 48), (171, 18), (171, 36), (171, 54)]:
        assert sc.chain_fits(D, Dp) and sc.chain_doubles(D, Dp) < 17740
        assert sc.chain_launch_bytes(17740, max(D, 156)) == 147504 > sc.SOLVE_LDS_LIMIT_CHAIN
    # every pair that overflows contains (156, 120), four speed/bias blocks: below the eight SOLVE_AUTO asks for (CHAIN_AUTO_MIN_BLOCKS),
    # so only a forced SOLVE_CHAIN reaches the batch check of build_batch; under AUTO such a batch is dense by the per-window rule
    fit = [(D, Dp) for Dp in range(6, 175, 6) for D in range(Dp + 9, 175, 9) if sc.chain_fits(D, Dp)]
    over = [(a, b) for i, a in enumerate(fit) for b in fit[i:]
            if sc.chain_launch_bytes(max(sc.chain_doubles(*a), sc.chain_doubles(*b)), max(a[0], b[0])) > sc.SOLVE_LDS_LIMIT_CHAIN]
    assert len(over) == 6 and all((156, 120) in p for p in over), over


def _status(H, g, Dp, mode):
    D = H.shape[0]
    dp = C.POINTER(C.c_double)
    Hc, gc, x = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(g, np.float64), np.zeros(D)
    ticks, info = C.c_int64(), C.c_int32()
    return _lib.lib().okvis_ba_reduced_solve(0, D, Dp, mode, 0, Hc.ctypes.data_as(dp), gc.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                             C.byref(ticks), C.byref(info), 1, None, 0)


def test_reduced_solve_refuses_before_any_device_call():
    """chain mode: a speed/bias block coupled beyond its neighbours, and the shapes the upload would not lay out for the chain solver
    (no device is needed for a refusal; tests/test_gpu_solve_referee.py has the calls that are accepted)"""
    rng = np.random.default_rng(3)
    H, g, Dp = chain_structured_system(rng, 4, 4, pose_prior=0.0)
    for a, b in ((0, 2), (3, 0), (1, 3)):
        Hb = H.copy()
        Hb[Dp + 9 * a + 4, Dp + 9 * b + 2] = 1e-30
        assert _status(Hb, g, Dp, SOLVE_CHAIN) == ERR_ARG, (a, b)
        assert _status(Hb.T.copy(), g, Dp, SOLVE_CHAIN) == ERR_ARG, (a, b)
    for D, Dp_ in sc.CHAIN_UNFIT + [(174, 192), (15, 0), (60, 60)]:
        assert _status(np.eye(D), np.ones(D), Dp_, SOLVE_CHAIN) == ERR_ARG, (D, Dp_)
    assert _status(np.eye(175), np.ones(175), 175, SOLVE_DENSE) == ERR_ARG
