"""The launch plan's three-launch iteration, on the host (make_plan, capi_launch.inc, through OKVIS_BA_LIST_PLAN).

An iteration is Schur -> solve -> linearise exactly where the factors' launch of an iteration is small_prepare_kernel alone (the
factors ride in the decision-free Schur launch: piece path, factors in a launch of their own, small tiles) AND the strategy keeps an
iteration budget (DOGLEG, with or without gauss_newton).  OKVIS_BA_TUNE_FOUR_LAUNCH, the LM strategy, the fused route and every
route whose factors do not ride keep their launches.  The captured graphs of the two routes have different keys."""
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import (TUNE_FOUR_LAUNCH, TUNE_NO_SMALL_RIDE, TUNE_SCHUR_DECIDES, TUNE_SCHUR_VALU, default_options)

PLAN = ("three", "rides", "prepare", "budget", "fused", "solve", "key_three", "key_four")
STRATEGY_DOGLEG, STRATEGY_LM = 0, 1


def _plan(w, n_windows, strategy=STRATEGY_DOGLEG, gn=0, flags=0, split_small_min=1, fused_max_windows=-1):
    o = default_options()
    o.strategy, o.gauss_newton = strategy, gn
    o.tuning.flags = flags
    o.tuning.split_small_min = split_small_min
    o.tuning.fused_max_windows = fused_max_windows
    p = solver.index_lists(w, o, n_windows)["plan"]
    assert len(p) == len(PLAN), p
    return dict(zip(PLAN, (int(x) for x in p)))


@pytest.fixture(scope="module")
def windows():
    return [synthetic.small_window(seed=3, K=4, L=40), synthetic.small_window(seed=4, K=6, L=150), synthetic.make_window(10, 400, 1.0, 20240923)]


@pytest.mark.parametrize("gn", [0, 1])
def test_three_launches_where_the_factors_ride_under_a_budget(windows, gn):
    for w in windows:
        p = _plan(w, 3, gn=gn)
        assert p["rides"] == 1 and p["prepare"] == 1 and p["budget"] == 1 and p["fused"] == 0, p
        assert p["three"] == 1, p


def test_the_flagship_batch_and_its_small_sibling(windows):
    """the default tuning: 64 windows ride (factors in a launch of their own from 40 windows on), 8 windows do not"""
    w = windows[2]
    assert _plan(w, 64, gn=1, split_small_min=0, fused_max_windows=0)["three"] == 1
    assert _plan(w, 256, gn=1, split_small_min=0, fused_max_windows=0)["three"] == 1
    p = _plan(w, 8, gn=1, split_small_min=0, fused_max_windows=0)
    assert p["three"] == 0 and p["prepare"] == 0, p


def test_the_tuning_bit_forces_four_launches(windows):
    for w in windows:
        p = _plan(w, 3, gn=1, flags=TUNE_FOUR_LAUNCH)
        assert p["rides"] == 1 and p["prepare"] == 1 and p["budget"] == 1, p   # (the route is the same one ...)
        assert p["three"] == 0, p                                               # (... with the prepare launch in every slot)


@pytest.mark.parametrize("gn", [0, 1])
def test_the_lm_strategy_keeps_its_launches(windows, gn):
    """LM keeps no iteration budget: with gauss_newton its factors may ride, the prepare launch stays in every slot"""
    for w in windows:
        p = _plan(w, 3, strategy=STRATEGY_LM, gn=gn)
        assert p["budget"] == 0 and p["three"] == 0, p
        if not gn:
            assert p["rides"] == 0 and p["prepare"] == 0, p


def test_the_fused_route_keeps_its_launches(windows):
    for w in windows:
        p = _plan(w, 3, gn=1, fused_max_windows=0)   # (0 = the default: fused up to 48 windows)
        assert p["fused"] == 1 and p["rides"] == 0 and p["three"] == 0, p


@pytest.mark.parametrize("flags", [TUNE_NO_SMALL_RIDE, TUNE_SCHUR_DECIDES, TUNE_SCHUR_VALU])
def test_routes_whose_factors_do_not_ride_keep_their_launches(windows, flags):
    for w in windows:
        p = _plan(w, 3, gn=1, flags=flags)
        assert p["rides"] == 0 and p["prepare"] == 0 and p["three"] == 0, p


def test_factors_in_the_linearise_launch_keep_their_launches(windows):
    p = _plan(windows[0], 3, gn=1, split_small_min=40)
    assert p["rides"] == 0 and p["three"] == 0, p


def test_the_graph_key_separates_the_routes(windows):
    p = _plan(windows[0], 3, gn=1)
    assert p["key_three"] != p["key_four"], p
    q = _plan(windows[0], 3, gn=1, flags=TUNE_FOUR_LAUNCH)
    assert (q["key_three"], q["key_four"]) == (p["key_three"], p["key_four"]), (p, q)   # (a key names call length and route, nothing else)
