#!/usr/bin/env python3
"""Times okvis_fe_sac_solve_absolute on a frame's 3D-2D work for 64 sequences: one absolute problem each, n = 300 correspondences
over two cameras and 50 samples (64 jobs, 3 200 samples), in one fused call.  Next to it: the solve-only call, the unfused pair
(solve-only call, then okvis_fe_sac_consensus on its hypotheses) and the same samples through the host side of the core as a loop
on one CPU core (tools/sac_abs_cpu_loop.cpp), whose hypotheses have to equal the device's bit for bit.  Host clock, median.  The
two kernels' own times come from a kernel-trace run of this script (rocprofv3 --kernel-trace --stats -- python
scripts/bench_sac_abs.py --calls 20 --no-cpu), taken on its own, with no counters.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_abs_cases as AC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402


def frame_jobs(sequences=64, n=300, k=50, seed=0):
    rng = np.random.default_rng(seed)
    jobs = []
    for _ in range(sequences):
        c = AC.scene(rng, n)
        c["sigma"] = rng.uniform(0.5e-6, 2e-6, n)
        jobs.append(AC.job(c, AC.samples(rng, n, k), threshold=9.0))
    return jobs


def median_ms(f, calls):
    f()
    times = []
    for _ in range(calls):
        t = time.perf_counter()
        f()
        times.append(time.perf_counter() - t)
    return 1e3 * float(np.median(times))


def cpu_loop_ms(jobs):
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "sac_abs_cpu_loop.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "sac_abs_cpu_loop.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        table, keep, out = F.sac_absolute_job_table([dict(j, consensus=False) for j in jobs])
        L.sac_abs_cpu.argtypes = [C.c_int32, C.POINTER(F.SacAbsoluteJobC)]
        t = time.perf_counter()
        L.sac_abs_cpu(len(jobs), table)
        return 1e3 * (time.perf_counter() - t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    jobs = frame_jobs()
    fe = F.Frontend()
    solve_only = [dict(j, consensus=False) for j in jobs]
    fused_table = F.sac_absolute_job_table(jobs)
    solve_table = F.sac_absolute_job_table(solve_only)
    models = fe.sac_solve_absolute(solve_only)
    cons_table = F.sac_job_table([dict(j, kind=F.SAC_ABSOLUTE, models=m["models"]) for j, m in zip(jobs, models)])
    res = {"jobs": len(jobs), "samples": sum(len(j["samples"]) for j in jobs), "n": 300,
           "valid_fraction": float(np.mean(np.concatenate([m["valid"] for m in models])))}
    res["fused_ms"] = median_ms(lambda: fe._call("sac_solve_absolute", len(jobs), fused_table[0]), a.calls)
    res["solve_only_ms"] = median_ms(lambda: fe._call("sac_solve_absolute", len(jobs), solve_table[0]), a.calls)
    res["consensus_only_ms"] = median_ms(lambda: fe._call("sac_consensus", len(jobs), cons_table[0]), a.calls)
    res["unfused_ms"] = median_ms(lambda: (fe._call("sac_solve_absolute", len(jobs), solve_table[0]), fe._call("sac_consensus", len(jobs), cons_table[0])), a.calls)
    if not a.no_cpu:
        res["cpu_loop_one_core_ms"], out = cpu_loop_ms(jobs)
        res["cpu_loop_equals_device_bitwise"] = all(o["models"].tobytes() == m["models"].tobytes() for o, m in zip(out, models))
    fe.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
