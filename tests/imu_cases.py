"""The factors of the IMU referee (tests/test_gpu_imu_referee.py) and what both of its halves share — TEST INFRASTRUCTURE, host
only.  tests/test_imu_statement_host.py proves on the CPU that these inputs would notice a wrong factor and pins the oracle to the
compiled reference on them; the GPU file compares the kernel (okvis_amd/csrc/ba_imu.hpp) on them.

Every case is one small window (3 poses, 10 landmarks, synthetic.make_window) — `ragged` is two — whose IMU streams, imu_t0 and
imu_t1 are replaced.  Samples lie on a grid of PERIOD (5 ms; `long`: 1.25 ms) and follow the analytic truth trajectory plus white
noise; the factor's second state is the reference's own propagation of the first over the stream, and all states are then
perturbed (pose 0.01, speed 0.01, gyro bias 0.001, accelerometer bias 0.01) so that no residual is near zero.  A window's two
factors take the case's stream shape with different samples.  The integer time logic decides the shape:

  aligned_k / unaligned_k   k integration steps, k in STEP_COUNTS (the device stages IMU_N = 32 steps per chunk): end points on
                            sample times, or t0 a quarter and t1 a third of a period inside a sample interval
  inside_one                t0 and t1 strictly inside one sample interval: both interpolations fall on one step
  dup                       64 steps, two repeated timestamps, one of them where the second chunk begins
  dup_run                   ten equal timestamps in the middle of the first chunk (more than the 8 spare words of the device's
                            staged timestamps), then normal samples
  lead300                   300 samples at or before t0 in front of 40 steps
  tail                      20 samples beyond t1
  sat                       40 unaligned steps, one gyroscope sample above g_max and one accelerometer sample above a_max
  long                      416 steps at 800 Hz
  ragged                    a batch of two windows with 2 and 4 factors of 20, 45 | 33, 7, 64, 90 steps

THE YARDSTICK (the convention of tests/schur_cases.py and tests/fp32_cases.py).  The referee of a factor is the long-double build
of the oracle (orc_imu_evaluate_record).  A quantity X is compared entrywise, deviation = max |X - ref| / a, where a is what the
entry is a sum of, in absolute values, taken from the referee:
  H = J^T J      |J|^T |J|                  information = sqrt_info^T sqrt_info     |sqrt_info|^T |sqrt_info|
  g = J^T r      |J|^T |r|                  cost = r.r / 2                          sum |r_i| max |r|  (see below)
  r, the four integrals, the three bias Jacobians      the largest entry of the block
  Delta_q        absolute
sqrt_info is judged through the information it stands for and through H, never factor against factor (its conditioning is the
covariance's, 1e9 and more).  e_ref of a factor and quantity is the larger of two deviations from the referee, the fp64 oracle's
and the float64 numpy statement's (tests/imu_statement.py), computed when the test runs; the bound is
BOUND_FACTOR * max(e_ref, (n_steps + 15) * 2^-52): one rounding per step and one per row of the 15x15 algebra, needed because some
e_ref are exactly zero.

The cost is one number and an exact function of r.  Its own two deviations are two samples of a sum of signed errors that may
cancel by chance (after three iterations, unaligned_33: 1.4e-12 of the cost on one route's state, 1.7e-11 on the next), so they are
no yardstick alone.  What r is allowed carries over: an r within e_r max |r| entrywise moves r.r / 2 by at most e_r max |r|
sum |r_i| to first order.  The cost is therefore measured in the scale sum |r_i| max |r| and e_ref(cost) is the larger of its own
two deviations and e_ref(r).  (The first GPU run had it in the scale of the cost itself with its own two deviations only: every
first evaluation passed, one factor of each window after three iterations on the fused route did not — 5.6 and 3.0 x that bound
with r at 0.13 and 0.11 of its own; the device's cost is r.r / 2 of its own r to 3.4e-16, test_gpu_imu_referee.py `cost alone`.)"""
from __future__ import annotations

import copy

import numpy as np

from okvis_amd import synthetic
from okvis_amd.window import IMU_CACHE_DOUBLES

from . import fp32_cases
from . import imu_statement as stmt

BOUND_FACTOR = fp32_cases.BOUND_FACTOR     # 4: what two correct fp64 evaluations may differ by (order of the sums, FMA contraction)
MUTATION_MARGIN = 10.0                     # a wrong factor exceeds the bound at least tenfold
PERIOD = 5_000_000                         # ns between samples (200 Hz)
STEP_COUNTS = (1, 2, 31, 32, 33, 64, 65)
EPS = 2.0 ** -52

# the preintegration record okvis_ba_fetch_imu_caches hands out (ImuCacheD, okvis_amd/csrc/ba_types.hpp), in doubles
RECORD = dict(Delta_q=(0, 4), C_integral=(4, 13), C_doubleintegral=(13, 22), acc_integral=(22, 25), acc_doubleintegral=(25, 28),
              dalpha_db_g=(28, 37), dv_db_g=(37, 46), dp_db_g=(46, 55), sqrt_info=(55, 280), sb_ref=(280, 289))
RECORD_FLAGS = 289                         # the last double: int32 valid | int32 redo_count
assert RECORD_FLAGS + 1 == IMU_CACHE_DOUBLES and RECORD["sb_ref"][1] == RECORD_FLAGS
BLOCKS = ("C_integral", "C_doubleintegral", "acc_integral", "acc_doubleintegral", "dalpha_db_g", "dv_db_g", "dp_db_g")
QUANTITIES = ("H", "g", "r", "cost", "information", "Delta_q") + BLOCKS
# OKVIS_BA_ARR_IMU_LIN per factor: H packed lower (465) | g (30) | r (15) | cost (1)
LIN = dict(H=(0, 465), g=(465, 495), r=(495, 510), cost=(510, 511))
LIN_DOUBLES = 511


def decode_record(rec):
    """one factor's 290 doubles -> the fields, valid, redo_count"""
    rec = np.ascontiguousarray(rec, np.float64)
    assert rec.size == IMU_CACHE_DOUBLES
    out = {k: rec[a:b].copy() for k, (a, b) in RECORD.items()}
    flags = rec[RECORD_FLAGS:].view(np.int32)
    out["valid"], out["redo_count"] = int(flags[0]), int(flags[1])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(lead, steps, tail, period):
    """sample indices: `lead` samples before the one at index 0, `steps` intervals, `tail` samples behind"""
    return np.arange(-lead, steps + tail + 1, dtype=np.int64) * period


def shape_aligned(k, lead=1, tail=1, period=PERIOD):
    t = _grid(lead, k, tail, period)
    return t, 0, k * period


def shape_unaligned(k, lead=1, tail=1, period=PERIOD):
    t = _grid(lead, k, tail, period)
    return t, period // 4, (k - 1) * period + period // 3


def shape_inside_one():
    t = _grid(1, 1, 1, PERIOD)
    return t, PERIOD // 5, (7 * PERIOD) // 10


def shape_dup():
    t, t0, t1 = shape_unaligned(64)
    # (sample 0 opens step 0: sample 32 opens step 32, the first of the second chunk; sample 10 lies inside the first)
    t = np.sort(np.concatenate([t, [10 * PERIOD, 32 * PERIOD]]))
    return t, t0, t1


def shape_dup_run():
    t, t0, t1 = shape_unaligned(40)
    t = np.sort(np.concatenate([t, [12 * PERIOD] * 9]))      # ten samples at 12 * PERIOD
    return t, t0, t1


SHAPES = {
    "inside_one": (shape_inside_one, 1),
    "dup": (shape_dup, 64),
    "dup_run": (shape_dup_run, 40),
    "lead300": (lambda: shape_unaligned(40, lead=300), 40),
    "tail": (lambda: shape_unaligned(40, tail=20), 40),
    "sat": (lambda: shape_unaligned(40), 40),
    "long": (lambda: shape_unaligned(416, period=PERIOD // 4), 416),
}
SINGLE = tuple(f"{a}_{k}" for k in STEP_COUNTS for a in ("aligned", "unaligned")) + tuple(SHAPES)


def shape(name):
    """(sample times, t0, t1) relative to the factor's origin, and the integration steps the reference makes of them"""
    if name in SHAPES:
        return SHAPES[name][0](), SHAPES[name][1]
    kind, k = name.rsplit("_", 1)
    return dict(aligned=shape_aligned, unaligned=shape_unaligned)[kind](int(k)), int(k)


def _samples(rng, prm, t_abs, period):
    gyr, acc = np.zeros((t_abs.size, 3)), np.zeros((t_abs.size, 3))
    g_W = np.array([0.0, 0.0, prm.g])
    for j, tj in enumerate(t_abs):
        _, _, a, R, w = synthetic.truth_at(tj * 1e-9)
        gyr[j], acc[j] = w, R.T @ (a + g_W)
    dt = period * 1e-9
    gyr += rng.standard_normal(gyr.shape) * prm.sigma_g_c / np.sqrt(dt)
    acc += rng.standard_normal(acc.shape) * prm.sigma_a_c / np.sqrt(dt)
    return gyr, acc


def make(shapes, seed, K=None):
    """a window of len(shapes) + 1 poses whose factor f has the stream shape shapes[f]"""
    from . import oracle_lib
    K = len(shapes) + 1 if K is None else K
    built = [shape(s)[0] for s in shapes]
    mean = float(np.mean([(t1 - t0) * 1e-9 for _, t0, t1 in built]))
    # (frames 2 s after the origin of time: room for 300 leading samples)
    w = synthetic.make_window(K, 10, 1.0, seed, frame_dt=max(mean, 0.02), frame_offset_s=2.0017)
    rng = np.random.default_rng(seed + 7)
    prm = w.imu_params
    frames = np.asarray(w.meta["t_frame_ns"], np.int64)
    pose, sb = np.array(w.pose, np.float64), np.array(w.sb, np.float64)
    ts, gs, as_, begin, count, t0s, t1s = [], [], [], [], [], [], []
    at = 0
    for f, (name, (t, t0, t1)) in enumerate(zip(shapes, built)):
        period = int(np.diff(np.unique(t)).min())
        origin = int(frames[f] // period * period)
        t_abs = t + origin
        gyr, acc = _samples(rng, prm, t_abs, period)
        if name == "sat":
            j = int(np.flatnonzero(t == 9 * period)[0])
            gyr[j, 1] = 1.3 * prm.g_max
            acc[j + 14, 2] = -1.2 * prm.a_max
        pose[f + 1], s1, _, _, n = oracle_lib.imu_propagation(t_abs, gyr, acc, prm, pose[f], sb[f], origin + t0, origin + t1)
        assert n == shape(name)[1], (name, n)
        sb[f + 1] = s1
        ts.append(t_abs), gs.append(gyr), as_.append(acc), begin.append(at), count.append(t_abs.size)
        t0s.append(origin + t0), t1s.append(origin + t1)
        at += t_abs.size
    nf = len(shapes)
    for k in range(nf + 1):
        pose[k] = synthetic.pose_oplus(pose[k], rng.normal(0, 0.01, 6))
        sb[k, 0:3] += rng.normal(0, 0.01, 3)
        sb[k, 3:6] += rng.normal(0, 0.001, 3)
        sb[k, 6:9] += rng.normal(0, 0.01, 3)
    w.pose, w.sb = pose, sb
    w.imu_pose0 = w.imu_sb0 = np.arange(0, nf, dtype=np.int32)
    w.imu_pose1 = w.imu_sb1 = np.arange(1, nf + 1, dtype=np.int32)
    w.imu_t0, w.imu_t1 = np.array(t0s, np.int64), np.array(t1s, np.int64)
    w.imu_s_begin, w.imu_s_count = np.array(begin, np.int32), np.array(count, np.int32)
    w.imu_s_t, w.imu_s_gyr, w.imu_s_acc = np.concatenate(ts), np.concatenate(gs), np.concatenate(as_)
    w.meta["imu_shapes"] = tuple(shapes)
    w.validate()
    return w


def _ragged():
    return [make(("unaligned_20", "unaligned_45"), 930), make(("unaligned_33", "unaligned_7", "unaligned_64", "unaligned_90"), 931)]


# name: the windows of the case (one batch)
CASES = {**{name: (lambda name=name, i=i: [make((name, name), 900 + i)]) for i, name in enumerate(SINGLE)}, "ragged": _ragged}
OTHER_ROUTES = ("unaligned_33", "dup_run", "sat", "ragged")     # the cases every route besides the default one runs


def factor_inputs(w, f, pose=None, sb=None):
    """what the factor-level entry points take, from the window (or from the given states)"""
    pose = np.asarray(w.pose if pose is None else pose, np.float64).reshape(-1, 7)
    sb = np.asarray(w.sb if sb is None else sb, np.float64).reshape(-1, 9)
    b, c = int(w.imu_s_begin[f]), int(w.imu_s_count[f])
    return (np.asarray(w.imu_s_t)[b:b + c], np.asarray(w.imu_s_gyr)[b:b + c], np.asarray(w.imu_s_acc)[b:b + c], w.imu_params,
            int(w.imu_t0[f]), int(w.imu_t1[f]), pose[w.imu_pose0[f]], sb[w.imu_sb0[f]], pose[w.imu_pose1[f]], sb[w.imu_sb1[f]])


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def quantities(J, r, record, T=np.float64):
    """every judged quantity from J [15][30], r [15] and the record's fields, formed in the number type T"""
    J, r = np.asarray(J, T), np.asarray(r, T)
    H, g = stmt.linearisation(J, r, T)
    SI = np.asarray(record["sqrt_info"], T).reshape(15, 15)
    q = dict(H=stmt.pack_lower(H), g=g, r=r, cost=np.array([T(0.5) * np.dot(r, r)], dtype=T), information=SI.T @ SI,
             Delta_q=np.asarray(record["Delta_q"], T))
    for k in BLOCKS:
        q[k] = np.asarray(record[k], T).reshape(-1)
    return q


def scales(J, r, record):
    T = np.longdouble
    aJ, ar = np.abs(np.asarray(J, T)), np.abs(np.asarray(r, T))
    aS = np.abs(np.asarray(record["sqrt_info"], T).reshape(15, 15))
    a = dict(H=stmt.pack_lower(aJ.T @ aJ), g=aJ.T @ ar, r=np.full(15, ar.max()), cost=np.array([ar.sum() * ar.max()]),
             information=aS.T @ aS, Delta_q=np.ones(4, T))
    for k in BLOCKS:
        v = np.abs(np.asarray(record[k], T).reshape(-1))
        a[k] = np.full(v.size, v.max())
    return a


def deviation(x, ref, a):
    """max |x - ref| / a; an entry nothing sums into (a = 0) must be the referee's to the bit"""
    x, ref, a = (np.asarray(v, np.longdouble).reshape(-1) for v in (x, ref, a))
    assert x.shape == ref.shape == a.shape, (x.shape, ref.shape, a.shape)
    d = np.abs(x - ref)
    if not np.all(np.isfinite(d)):
        return float("inf")
    if np.any(d[a == 0] != 0):
        return float("inf")
    m = a > 0
    return float((d[m] / a[m]).max()) if m.any() else 0.0


class Factor:
    """one factor at one set of states: the referee, the two fp64 evaluations, the scales, e_ref and the bound per quantity"""

    def __init__(self, oracle, inputs, sb_ref=None, label=""):
        self.inputs, self.sb_ref, self.label = inputs, sb_ref, label
        r, Js, rec, steps, redo = oracle.imu_evaluate_record(*inputs, sb_ref=sb_ref, extended=True)
        self.J, self.r, self.n_steps, self.redo_count = np.concatenate(Js, 1), r, steps, redo
        self.record = {k: rec[a:b] for k, (a, b) in RECORD.items()}
        self.ref = quantities(self.J, self.r, self.record, np.longdouble)
        self.a = scales(self.J, self.r, self.record)
        r6, Js6, rec6, steps6, redo6 = oracle.imu_evaluate_record(*inputs, sb_ref=sb_ref)
        assert (steps6, redo6) == (steps, redo), (label, steps6, redo6, steps, redo)
        self.o64 = quantities(np.concatenate(Js6, 1), r6, {k: rec6[a:b] for k, (a, b) in RECORD.items()})
        s = stmt.evaluate(*inputs, sb_ref=sb_ref)
        assert (s["n_steps"], s["redo_count"]) == (steps, redo), (label, s["n_steps"], s["redo_count"], steps, redo)
        self.s64 = quantities(s["J"], s["r"], s)
        self.e_oracle = {q: deviation(self.o64[q], self.ref[q], self.a[q]) for q in QUANTITIES}
        self.e_stmt = {q: deviation(self.s64[q], self.ref[q], self.a[q]) for q in QUANTITIES}
        self.e_ref = {q: max(self.e_oracle[q], self.e_stmt[q]) for q in QUANTITIES}
        self.e_ref["cost"] = max(self.e_ref["cost"], self.e_ref["r"])      # (the cost inherits what r is allowed: module docstring)
        self.floor = (self.n_steps + 15) * EPS

    def bound(self, q):
        return BOUND_FACTOR * max(self.e_ref[q], self.floor)

    def statement(self, dtype=np.float64, mutate=None):
        s = stmt.evaluate(*self.inputs, sb_ref=self.sb_ref, dtype=dtype, mutate=mutate)
        q = quantities(s["J"], s["r"], s, dtype)
        if mutate == "wrong_permutation":      # (the statement's H and g ARE the mutation: J itself is in the natural order)
            q["H"], q["g"] = stmt.pack_lower(s["H"]), s["g"]
        return q

    def judge(self, lin, rec):
        """the device's IMU_LIN entry [511] and record [290] of this factor -> {quantity: deviation}"""
        lin = np.asarray(lin, np.float64)
        assert lin.size == LIN_DOUBLES
        d = decode_record(rec)
        got = {k: lin[a:b] for k, (a, b) in LIN.items()}
        SI = d["sqrt_info"].reshape(15, 15).astype(np.longdouble)
        got["information"] = SI.T @ SI
        for k in ("Delta_q",) + BLOCKS:
            got[k] = d[k]
        return {q: deviation(got[q], self.ref[q], self.a[q]) for q in QUANTITIES}, d


class Referee:
    """the factors of every case, evaluated once"""

    def __init__(self, oracle, names=None):
        self.oracle = oracle
        self.windows, self.factors = {}, {}
        for name in (CASES if names is None else names):
            self.windows[name] = CASES[name]()
            self.factors[name] = [[Factor(oracle, factor_inputs(w, f), label=f"{name} w{i} f{f}") for f in range(w.n_imu)]
                                  for i, w in enumerate(self.windows[name])]

    def case(self, name):
        """fresh copies of the case's windows"""
        return copy.deepcopy(self.windows[name])

    def all(self):
        for name, per_window in self.factors.items():
            for i, fs in enumerate(per_window):
                for f, fac in enumerate(fs):
                    yield name, i, f, fac
