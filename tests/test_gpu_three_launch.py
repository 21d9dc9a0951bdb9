"""The three-launch iteration (Schur -> solve -> linearise) against the four-launch one, on the GPU.

Where the IMU / prior factors ride in the Schur launch and the strategy keeps an iteration budget, small_prepare_kernel is no longer
part of every slot: the solve kernel's tail repeats the bias check of imu_factor<1> with a margin, pauses the windows whose
preintegration records need that launch, and the host runs it for them (okvis_ba_iterate's entry, okvis_ba_finish) and grants the
slots they sat out.  OKVIS_BA_TUNE_FOUR_LAUNCH keeps the launch in every slot and is the referee.  Every window performs the same
evaluations, decisions and re-preintegrations on both routes, so everything is compared with numpy.array_equal: states, summaries,
the IMU records' reference biases and re-preintegration counts, the reduced system and its right-hand side (debug_arrays = 1).

The route is forced at small sizes by tuning.split_small_min = 1 and tuning.fused_max_windows = -1.  Windows "at rest" start from
their own optimum (no term moves its gyro bias by 1e-4 / dt any more); windows "on the move" start with gyro biases 0.02 rad/s off,
so that the first steps carry them far past the threshold and their terms re-preintegrate in the first slots."""
import copy

import numpy as np
import pytest

from okvis_amd import solver, synthetic
from okvis_amd.window import TUNE_FOUR_LAUNCH, default_options

pytestmark = pytest.mark.gpu

ROUTES = {"three": 0, "four": TUNE_FOUR_LAUNCH}
THRESHOLD = 1e-4   # ImuError.cpp:549: |b_g - b_g,ref| * dt above it re-preintegrates
MARGIN = 1e-6      # the solve kernel's check treats anything above THRESHOLD * (1 - MARGIN) as not quiet


def _opts(mode, route, **kw):
    o = default_options()
    o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    o.gauss_newton = 1 if mode == "gn" else 0
    o.tuning.split_small_min = 1         # the IMU / prior factors in a launch of their own, as from 40 windows on
    o.tuning.fused_max_windows = -1      # no fused linearise + reduce launch
    o.tuning.flags = ROUTES[route]
    o.debug_arrays = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _batch(ws, mode, route, **kw):
    b = solver.WindowBatch(ws, options=_opts(mode, route, **kw))
    r = b.launch_route()
    assert r["fused"] == 0 and r["piece_path"] == 1 and r["split_small"] == 1 and r["small_rides"] == 1, r
    assert r["three_launch"] == (1 if route == "three" else 0), (route, r)
    return b


def _results(b, sm, n_windows):
    out = {"cost": np.array([[x["initial_cost"], x["final_cost"]] for x in sm]),
           "steps": np.array([[x["iterations"], x["successful_steps"], x["termination"]] for x in sm])}
    for i in range(n_windows):
        out[f"pose{i}"], out[f"sb{i}"], out[f"lm{i}"] = (np.array(a) for a in b.get_state(i))
        for a in ("IMU_SB_REF", "IMU_REDO_COUNT", "REDUCED_S", "REDUCED_RHS"):
            out[f"{a}{i}"] = np.array(b.array(a, i))
    return out


def _run(ws, mode, route, calls, **kw):
    """begin, iterate(n) for n in calls (None: optimize(sum)), finish.  Returns the results, the pauses and the slots after each call."""
    b = _batch(ws, mode, route, **kw)
    slots = []
    if calls is None:
        sm = b.optimize(10)
    else:
        b.begin()
        for n in calls:
            b.iterate(n)
            slots.append(b.launch_route()["slots"])
        sm = b.finish()
    out = _results(b, sm, len(ws))
    pauses, late = b.pause_count(), b.helper_timeouts()
    b.close()
    assert late == 0
    return out, pauses, slots


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
        assert np.isfinite(a[k]).all(), (what, k)


def _moved(w, delta):
    """w with every gyro bias delta off (rad/s, along x and z)"""
    v = copy.deepcopy(w)
    v.sb[:, 3] += delta
    v.sb[:, 5] -= 0.5 * delta
    return v


@pytest.fixture(scope="module")
def rest():
    """three small windows at their own optimum (of different sizes: 3, 4 and 5 IMU terms)"""
    ws = [synthetic.small_window(seed=21, K=4, L=40), synthetic.small_window(seed=22, K=5, L=90), synthetic.small_window(seed=23, K=6, L=150)]
    b = _batch(ws, "gn", "four")
    b.optimize(25)
    out = []
    for i, w in enumerate(ws):
        v = copy.deepcopy(w)
        pose, sb, lm = b.get_state(i)
        v.pose[:], v.sb[:], v.lm[:] = pose, sb, lm
        out.append(v)
    b.close()
    return out


# ---- (a) forced re-preintegrations next to windows at rest ----
@pytest.mark.parametrize("calls", [None, (3, 7)], ids=["optimize10", "iterate3+7"])
@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_forced_repreintegrations(rest, mode, calls):
    ws = [_moved(rest[0], 0.02), rest[1], _moved(rest[2], -0.02), rest[0]]
    three, pauses, _ = _run(ws, mode, "three", calls)
    four, none, _ = _run(ws, mode, "four", calls)
    _same(three, four, ("forced", mode, calls))
    assert none == 0 and pauses >= 2, (pauses, none)   # (the two windows on the move paused, at least once each)
    redo = [three[f"IMU_REDO_COUNT{i}"] for i in range(4)]
    assert (redo[0] >= 2).all() and (redo[2] >= 2).all(), redo   # (first use + the first slots)
    assert (redo[1] == 1).all() and (redo[3] == 1).all(), redo   # (first use alone: at rest)
    assert (three["steps"][:, 0] >= 1).all(), three["steps"]


# ---- (b) the threshold ----
def _one_slot(w, route):
    b = _batch([w], "gn", route)
    b.begin()
    b.iterate(1)
    sm = b.finish()
    out = _results(b, sm, 1)
    pauses = b.pause_count()
    b.close()
    return out, pauses


def test_threshold(rest):
    """Term 0's start bias is moved by d along x: the first step pulls it back, so |b_g,trial - b_g,ref| * dt of term 0 grows with d.
    Bisection on d (four-launch route: does term 0 re-preintegrate behind the first step?) finds the d at which it reaches the
    threshold; just above it the three-launch route pauses and re-preintegrates, inside the conservative margin it pauses and does
    not, well below it does neither."""
    base = rest[1]

    def at(d):
        v = copy.deepcopy(base)
        v.sb[0, 3] += d
        return v

    def redone(d):
        return _one_slot(at(d), "four")[0]["IMU_REDO_COUNT0"][0] > 1

    lo, hi = 0.0, 4e-3
    assert not redone(lo) and redone(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if redone(mid):
            hi = mid
        else:
            lo = mid
        if hi - lo <= 1e-9 * hi:
            break
    assert hi - lo <= 1e-8 * hi, (lo, hi)
    # (the quantity is linear in d to far better than the margin over such a step: the start is the optimum but for d)
    cases = {"above": hi * (1 + 1e-3), "margin": hi * (1 - 0.5 * MARGIN), "below": hi * 0.9}
    got = {}
    for name, d in cases.items():
        three, pauses = _one_slot(at(d), "three")
        four, none = _one_slot(at(d), "four")
        _same(three, four, ("threshold", name))
        got[name] = (pauses, int(three["IMU_REDO_COUNT0"][0]))
        assert none == 0
        print(f"threshold case {name}: d = {d:.12e}, pauses {pauses}, re-preintegrations of term 0: {got[name][1]}")
    assert got["above"] == (1, 2), got     # pauses and re-preintegrates
    assert got["margin"] == (1, 1), got    # pauses, imu_factor<1> decides exactly: no re-preintegration
    assert got["below"] == (0, 1), got     # neither


# ---- (c) a steady batch ----
@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_steady_windows_never_pause(rest, mode):
    three, pauses, slots = _run(rest, mode, "three", (4, 6))
    four, _, slots4 = _run(rest, mode, "four", (4, 6))
    _same(three, four, ("steady", mode))
    assert pauses == 0
    assert slots[0] == 4, slots                      # after the first call: the requested iterations, no slot more
    if mode == "gn":
        assert slots == [4, 10] and slots4 == [4, 10], (slots, slots4)
    for i in range(len(rest)):
        assert (three[f"IMU_REDO_COUNT{i}"] == 1).all()


# ---- (d) pauses at the edges of calls ----
@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_pauses_at_the_edges_of_calls(rest, mode):
    """iterate(1) six times: the only slot of a call is its first and its last, so a pause is met at the entry of the next call (or in
    okvis_ba_finish, for the last) — against one iterate(6) and against the four-launch route"""
    ws = [_moved(rest[0], 0.02), rest[1], _moved(rest[2], 0.01)]
    ones, p1, _ = _run(ws, mode, "three", (1,) * 6)
    whole, p6, _ = _run(ws, mode, "three", (6,))
    four, _, _ = _run(ws, mode, "four", (1,) * 6)
    four6, _, _ = _run(ws, mode, "four", (6,))
    _same(ones, four, ("edges", mode, "1 x 6"))
    _same(whole, four6, ("edges", mode, "6"))
    _same(ones, whole, ("edges", mode, "1 x 6 against 6"))
    assert p1 >= 2 and p6 >= 2, (p1, p6)


def test_a_pause_in_the_last_slot_before_finish(rest):
    """one call, one slot: the pause is found by okvis_ba_finish alone"""
    ws = [_moved(rest[2], 0.02), rest[0]]
    three, pauses, _ = _run(ws, "gn", "three", (1,))
    four, _, _ = _run(ws, "gn", "four", (1,))
    _same(three, four, "last slot")
    assert pauses == 1 and (three["IMU_REDO_COUNT0"] == 2).all(), (pauses, three["IMU_REDO_COUNT0"])


# ---- (e) pause, finish, get_state ----
@pytest.mark.parametrize("mode", ["gn", "dogleg"])
def test_pause_then_finish_then_get_state(rest, mode):
    ws = [rest[1], _moved(rest[0], 0.02)]
    state = {}
    for route in ROUTES:
        b = _batch(ws, mode, route)
        b.begin()
        b.iterate(5)
        sm = b.finish()
        state[route] = [np.array(a) for i in range(2) for a in b.get_state(i)] + [np.array([x["final_cost"] for x in sm])]
        pauses = b.pause_count()
        assert (pauses >= 1) == (route == "three"), (route, pauses)
        b.close()
    for a, c in zip(state["three"], state["four"]):
        assert np.array_equal(a, c) and np.isfinite(a).all()


def test_the_next_optimisation_starts_on_four_launches_after_a_pause(rest):
    """a solver whose last begin ... finish paused, or re-preintegrated, runs the next one with the prepare launch in every slot (no
    pause can occur, although the second optimisation meets the moved start again); results as on the four-launch route throughout"""
    ws = [_moved(rest[0], 0.02), rest[1]]
    b3, b4 = _batch(ws, "gn", "three"), _batch(ws, "gn", "four")
    pauses = []
    for k in range(3):
        s3, s4 = b3.optimize(6), b4.optimize(6)
        _same(_results(b3, s3, 2), _results(b4, s4, 2), ("next", k))
        pauses.append(b3.pause_count())
        if k == 0:   # the second optimisation meets the same start again: on the move, but on four launches
            for b in (b3, b4):
                for i, w in enumerate(ws):
                    b.set_state(i, w.pose, w.sb, w.lm)
    assert pauses[0] >= 1 and pauses[1] == 0 and pauses[2] == 0, pauses
    b3.close()
    b4.close()
