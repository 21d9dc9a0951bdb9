"""TEST INFRASTRUCTURE: the cases of okvis_fe_imu_propagate (tests/test_imu_propagate_host.py, tests/test_gpu_imu_propagate.py,
tests/golden/make_imu_propagation_golden.py) and the yardstick they are judged by.

The sample streams are synthetic.make_window's (200 Hz, white noise at the configured densities), edited by hand where a case needs
it.  A spec is one job: a deque (a range of a stream), a start time, ascending end times, the state at the start, flags, a parameter
set.  The smallest shapes at which the kernel can go wrong:

  1  1, 2, 11, 33 and 101 steps, start and end on sample stamps (101 > the 64-sample window of a wave: one refill)
  2  start and end strictly between stamps: in different intervals, in the SAME interval (one step, both interpolations), and a
     start on a stamp with an end between two
  3  the IMU-rate chain: a 300-sample deque, start = stamp 289, ends = stamps 290 .. 299: ten one-step calls, each behind 289 or
     more skipped samples (five rounds of the 64-wide scan), covariance and Jacobian
  4  the same chain with start and ends between stamps
  5  saturation: one gyroscope sample above g_max and one accelerometer sample above a_max in the middle of an 11-step call
  6  zero rotation: gyr == b_g exactly for every sample: the small-angle branches of sinc and rightJacobian
  7  an end the deque does not cover: count = -1, outputs = inputs.  Ends ascend, so every end behind an uncovered one is
     uncovered too: the chain is (covered, uncovered, uncovered), and what continues behind the -1 is the carried state
  8  a deque of one sample: count = 0 for every end
  9  batch(): 130 jobs drawn from 1-8, two parameter sets, flags 0 1 2 3 side by side, lengths 1 to 101 next to each other: more
     jobs than waves in a workgroup, divergent trip counts

The yardstick of one call and one array: error = max |x - referee| / max |referee|, limit = 4 * max(e_oracle, n_steps * 2^-52),
e_oracle = the fp64 oracle's error against the long double referee on that same call; n_steps * 2^-52 is one rounding per step, the
factor 4 the margin the project gives device arithmetic over an independent evaluation (tests/test_gpu_fp32_linearize.py)."""
import ctypes as C
import functools
import os

import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import ImuParams

try:
    from tests import oracle_lib
except ImportError:   # (imported with tests/ itself on the path)
    import oracle_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_propagation.npz")
PARAMS = [ImuParams(), ImuParams(sigma_g_c=2.0e-3, sigma_a_c=5.0e-3, sigma_gw_c=1.0e-5, sigma_aw_c=1.0e-4, g=9.80665, g_max=5.0,
                                 a_max=150.0)]
BIAS = np.r_[0, 0, 0, 1e-3, -2e-3, 1e-3, 0.01, 0.02, -0.01]   # as tests/test_estimator_host.py
DT = 5_000_000                                                 # ns between two stamps
ARRAYS = ("T_WS", "sb", "cov", "jac")
EPS = 2.0 ** -52
COV, JAC = 1, 2


@functools.lru_cache(maxsize=None)
def streams():
    """name -> (t [n] int64, gyr [n][3], acc [n][3]), n = 305: the plain stream, one with two saturated samples, one whose
    gyroscope reads the bias exactly"""
    w = synthetic.make_window(4, 10, 1.0, 77)
    t, g, a = w.imu_s_t.copy(), w.imu_s_gyr.copy(), w.imu_s_acc.copy()
    assert len(t) >= 303 and (np.diff(t) == DT).all()
    gs, as_ = g.copy(), a.copy()
    gs[45, 1], as_[47, 0] = 9.0, -200.0     # above g_max = 7.8 (and 5.0), a_max = 176 (and 150)
    gz = np.tile(BIAS[3:6], (len(t), 1))
    out = {"plain": (t, g, a), "saturated": (t, gs, as_), "still": (t, gz, a)}
    for arrays in out.values():
        for x in arrays:
            x.setflags(write=False)
    return out


def state_at(t_ns):
    """the true state at t_ns with the bias offset: T_WS [7], sb [9]"""
    p, v, _, R, _ = synthetic.truth_at(t_ns * 1e-9)
    return np.r_[p, synthetic.rot_to_quat(R)], np.r_[v, 0, 0, 0, 0, 0, 0] + BIAS


def _spec(name, case, stream, s_begin, s_count, t_start, ends, flags=COV | JAC, prm=0):
    T, sb = state_at(t_start)
    return dict(name=name, case=case, stream=stream, s_begin=int(s_begin), s_count=int(s_count), t_start=int(t_start),
                ends=[int(e) for e in ends], T_WS=T, sb=sb, flags=flags, prm=prm)


@functools.lru_cache(maxsize=None)
def specs():
    s = []
    for n in (1, 2, 11, 33, 101):            # one sample of margin on both sides, like the frontend's deques
        s.append(_spec(f"steps{n}", 1, "plain", 9, n + 3, 10 * DT, [(10 + n) * DT]))
    s.append(_spec("between", 2, "plain", 9, 16, 10 * DT + 1_700_000, [21 * DT + 3_100_000]))
    s.append(_spec("same_interval", 2, "plain", 9, 4, 10 * DT + 1_200_000, [10 * DT + 3_900_000]))
    s.append(_spec("end_between", 2, "plain", 9, 8, 10 * DT, [13 * DT + 4_999_999]))
    s.append(_spec("chain", 3, "plain", 0, 300, 289 * DT, [(290 + k) * DT for k in range(10)]))
    s.append(_spec("chain_between", 4, "plain", 0, 300, 288 * DT + 3_300_000, [(289 + k) * DT + 1_300_000 for k in range(10)]))
    s.append(_spec("saturated", 5, "saturated", 39, 14, 40 * DT, [51 * DT]))
    s.append(_spec("still", 6, "still", 9, 14, 10 * DT, [21 * DT]))
    s.append(_spec("uncovered", 7, "plain", 9, 14, 10 * DT, [15 * DT, 23 * DT, 24 * DT]))   # the deque ends at stamp 22
    s.append(_spec("one_sample", 8, "plain", 10, 1, 10 * DT, [11 * DT, 12 * DT]))
    return s


def by_name(name):
    return next(s for s in specs() if s["name"] == name)


@functools.lru_cache(maxsize=None)
def batch():
    """case 9: 130 jobs; job j has flags j % 4 and parameter set (j // 4) % 2, and neighbours differ in length"""
    base = specs()
    order = np.random.default_rng(9).permutation(130)
    out = []
    for j in range(130):
        s = dict(base[int(order[j]) % len(base)])
        s["flags"], s["prm"], s["name"] = j % 4, (j // 4) % 2, f"{s['name']}#{j}"
        out.append(s)
    return out


def deque_of(spec):
    t, g, a = streams()[spec["stream"]]
    r = slice(spec["s_begin"], spec["s_begin"] + spec["s_count"])
    return t[r], g[r], a[r]


def pool(spec_list):
    """the pools and the job table of one call: every job brings its own deque and its own ends.
    -> s_t, s_gyr, s_acc, ends, jobs (dicts for okvis_amd.frontend.imu_propagate)"""
    ts, gs, as_, ends, jobs = [], [], [], [], []
    n_s = n_e = 0
    for s in spec_list:
        t, g, a = deque_of(s)
        ts.append(t), gs.append(g), as_.append(a), ends.extend(s["ends"])
        jobs.append(dict(s_begin=n_s, s_count=len(t), e_begin=n_e, e_count=len(s["ends"]), prm=s["prm"], flags=s["flags"],
                         t_start=s["t_start"], T_WS=s["T_WS"], sb=s["sb"]))
        n_s, n_e = n_s + len(t), n_e + len(s["ends"])
    return np.concatenate(ts), np.concatenate(gs), np.concatenate(as_), np.array(ends, np.int64), jobs


# ------------------------------------------------------------------------------------------------ single calls and the yardstick

def call(fn, spec, T, sb, t0, t1):
    """one propagation call through fn = an entry of the signature of orc_imu_propagation -> dict(T_WS, sb, cov, jac, count)"""
    t, g, a = (np.ascontiguousarray(x) for x in deque_of(spec))
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    T, sb = np.array(T, np.float64), np.array(sb, np.float64)
    cov, jac = np.zeros((15, 15)), np.zeros((15, 15))
    pc = spec.get("params", PARAMS[spec["prm"]]).as_c()   # ("params": a parameter set of the test's own)
    n = fn(C.c_int(len(t)), t.ctypes.data_as(lp), g.ctypes.data_as(dp), a.ctypes.data_as(dp), C.byref(pc), T.ctypes.data_as(dp),
           sb.ctypes.data_as(dp), C.c_int64(int(t0)), C.c_int64(int(t1)), cov.ctypes.data_as(dp), jac.ctypes.data_as(dp))
    return dict(T_WS=T, sb=sb, cov=cov, jac=jac, count=int(n))


def referee(spec, T, sb, t0, t1):
    return call(oracle_lib.lib_ld().orc_imu_propagation, spec, T, sb, t0, t1)


def oracle(spec, T, sb, t0, t1):
    return call(oracle_lib.lib().orc_imu_propagation, spec, T, sb, t0, t1)


def error(x, ref):
    return float(np.abs(np.asarray(x) - ref).max() / np.abs(ref).max())


def judge(spec, T, sb, t0, t1):
    """the referee's result of one covered call and the limit of each array -> (referee dict, {array: limit})"""
    ref, orc = referee(spec, T, sb, t0, t1), oracle(spec, T, sb, t0, t1)
    assert ref["count"] == orc["count"] >= 0
    return ref, {k: 4.0 * max(error(orc[k], ref[k]), ref["count"] * EPS) for k in ARRAYS}


def calls(spec):
    """(k, start, end) of the spec's chain"""
    starts = [spec["t_start"]] + spec["ends"][:-1]
    return [(k, t0, t1) for k, (t0, t1) in enumerate(zip(starts, spec["ends"]))]


def covered(spec, t1):
    t, _, _ = deque_of(spec)
    return len(t) >= 2 and t[-1] >= t1


def chain(fn, spec):
    """the spec's whole chain through fn, every call from the state the call before it returned: a list of call() results.  A
    deque of fewer than two samples never reaches fn: Frontend::propagation returns 0 before it (Frontend.cpp:281-286)."""
    T, sb, out = spec["T_WS"], spec["sb"], []
    for _, t0, t1 in calls(spec):
        if spec["s_count"] < 2:
            r = dict(T_WS=np.array(T), sb=np.array(sb), cov=np.zeros((15, 15)), jac=np.zeros((15, 15)), count=0)
        else:
            r = call(fn, spec, T, sb, t0, t1)
        out.append(r)
        T, sb = r["T_WS"], r["sb"]
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def golden_chain(spec):
    """what the compiled reference returned for the chain of the base spec of `spec` (tests/golden/imu_propagation.npz)"""
    g, name = golden(), spec["name"].split("#")[0]
    n = len(spec["ends"])
    return [dict(count=int(g[f"{name}/count"][k]), **{a: g[f"{name}/{a}"][k] for a in ARRAYS}) for k in range(n)]
