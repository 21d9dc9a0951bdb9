"""Time ONE okvis_fe_imu_propagate call that carries a frame time's worth of propagation for 64 sequences, next to the same work as a
loop over the CPU oracle's orc_imu_propagation on one core.

Per sequence (its own 200 Hz stream, a 300-sample deque):
  - one frame job: the state from stamp 279 + 1.7 ms to stamp 289 + 1.7 ms (11 steps), state only         (Estimator::addStates)
  - one IMU-rate chain: start = stamp 289, ends = stamps 290 .. 299, covariance and Jacobian at every end   (imuConsumerLoop)
so 128 jobs, 704 calls, 1344 integration steps, 640 covariances and Jacobians per call of the entry.

The host clock is around the C entry (tables and output arrays made beforehand), which returns after a stream synchronise: packing
into the pinned block, the copy in, the kernel, the copy back and the scatter to the callers' arrays included.

    python scripts/bench_propagate.py [--sequences 64] [--warmup 200] [--rounds 3] [--calls 2000] [--cpu-passes 20] [--profile]

--profile: warm-up and one round only, no CPU loop (for a run under rocprofv3 --kernel-trace --stats).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from okvis_amd import frontend as F, synthetic  # noqa: E402
from okvis_amd.window import ImuParams  # noqa: E402

DT = 5_000_000
BIAS = np.r_[0, 0, 0, 1e-3, -2e-3, 1e-3, 0.01, 0.02, -0.01]


def workload(n_seq):
    ts, gs, as_, ends, jobs = [], [], [], [], []
    for q in range(n_seq):
        w = synthetic.make_window(4, 10, 1.0, 1000 + q)
        t, g, a = w.imu_s_t[:300], w.imu_s_gyr[:300], w.imu_s_acc[:300]
        assert len(t) == 300 and (np.diff(t) == DT).all()
        for t_start, e, flags in ((279 * DT + 1_700_000, [289 * DT + 1_700_000], 0), (289 * DT, [(290 + k) * DT for k in range(10)], 3)):
            p, v, _, R, _ = synthetic.truth_at(t_start * 1e-9)
            jobs.append(dict(s_begin=300 * q, s_count=300, e_begin=len(ends), e_count=len(e), prm=0, flags=flags, t_start=t_start,
                             T_WS=np.r_[p, synthetic.rot_to_quat(R)], sb=np.r_[v, 0, 0, 0, 0, 0, 0] + BIAS))
            ends.extend(e)
        ts.append(t), gs.append(g), as_.append(a)
    return np.concatenate(ts), np.concatenate(gs), np.concatenate(as_), np.array(ends, np.int64), jobs


def stats(x):
    x = np.asarray(x) * 1e6
    return {"median_us": float(np.median(x)), "p10_us": float(np.percentile(x, 10)), "p90_us": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--cpu-passes", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    params = [ImuParams()]
    s_t, s_gyr, s_acc, ends, jobs = workload(a.sequences)
    fe = F.Frontend()
    prm, s_t, s_gyr, s_acc, ends = F.imu_pools(params, s_t, s_gyr, s_acc, ends)
    table = F.imu_job_table(jobs)
    m = len(ends)
    T, sb, cov, jac, cnt = np.zeros((m, 7)), np.zeros((m, 9)), np.zeros((m, 225)), np.zeros((m, 225)), np.zeros(m, np.int32)
    args = (fe._ctx, 1, C.addressof(prm), len(s_t), s_t.ctypes.data, s_gyr.ctypes.data, s_acc.ctypes.data, m, ends.ctypes.data, len(jobs), table,
            T.ctypes.data, sb.ctypes.data, cov.ctypes.data, jac.ctypes.data, cnt.ctypes.data)
    entry = fe._L.okvis_fe_imu_propagate

    def once():
        t0 = time.perf_counter()
        rc = entry(*args)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    for _ in range(a.warmup):
        once()
    out = {"sequences": a.sequences, "jobs": len(jobs), "calls_of_propagation": m, "integration_steps": int(cnt.sum()),
           "covariances": sum(j["e_count"] for j in jobs if j["flags"] & 1)}
    assert (cnt > 0).all()
    out["gpu_call"] = [stats([once() for _ in range(a.calls)]) for _ in range(1 if a.profile else a.rounds)]
    if not a.profile:
        # the same work on one core: the CPU oracle's restatement, call by call, each chain from its own carried state
        from tests import oracle_lib
        fn = oracle_lib.lib().orc_imu_propagation
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        pc = params[0].as_c()
        Tc, sbc, covc, jacc = np.zeros((m, 7)), np.zeros((m, 9)), np.zeros((m, 225)), np.zeros((m, 225))

        def cpu_pass():
            for j in jobs:
                b, n = j["s_begin"], j["s_count"]
                t, g, ac = s_t[b:b + n], s_gyr[b:b + n], s_acc[b:b + n]
                Tj, sj, t0 = np.array(j["T_WS"]), np.array(j["sb"]), j["t_start"]
                want = j["flags"] != 0
                for k in range(j["e_count"]):
                    e = j["e_begin"] + k
                    fn(n, t.ctypes.data_as(lp), g.ctypes.data_as(dp), ac.ctypes.data_as(dp), C.byref(pc), Tj.ctypes.data_as(dp),
                       sj.ctypes.data_as(dp), C.c_int64(t0), C.c_int64(int(ends[e])), covc[e].ctypes.data_as(dp) if want else None,
                       jacc[e].ctypes.data_as(dp) if want else None)
                    Tc[e], sbc[e], t0 = Tj, sj, int(ends[e])

        cpu_pass()
        per = []
        for _ in range(a.cpu_passes):
            t0 = time.perf_counter()
            cpu_pass()
            per.append(time.perf_counter() - t0)
        out["cpu_loop_one_core"] = stats(per)
        out["cpu_loop_over_gpu_call"] = out["cpu_loop_one_core"]["median_us"] / float(np.median([r["median_us"] for r in out["gpu_call"]]))
        rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())  # noqa: E731
        has = np.array([e for j in jobs if j["flags"] for e in range(j["e_begin"], j["e_begin"] + j["e_count"])])
        out["gpu_vs_cpu_oracle"] = {"T_WS": rel(T, Tc), "sb": rel(sb, sbc), "cov": rel(cov[has], covc[has]), "jac": rel(jac[has], jacc[has])}
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
