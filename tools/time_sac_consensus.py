"""Times one okvis_fe_sac_consensus call that carries a frame's worth of outlier rejection: one absolute-pose problem (n = 300
correspondences over 2 cameras, 50 hypotheses) and, for 2 cameras x 3 keyframes, a rotation-only and a relative-pose problem each
(n = 150, 50 hypotheses): 13 problems, 105000 (hypothesis, correspondence) cells.

    python tools/time_sac_consensus.py [--calls N] [--rounds R] [--no-cpu]

Prints one JSON line: the median (and 10th / 90th percentile) host time of a call, which ends in a stream synchronise, per round;
and the same work as a loop on one CPU core (tools/sac_cpu_loop.cpp: the score functions the kernel uses, compiled for the host).
The kernel's share of the call comes from a separate run under rocprofv3 --kernel-trace --stats (profiles/sac_notes.md).
Needs a GPU; there is no fall-back."""
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
import sac_cases as SC  # noqa: E402
import sac_statement as S  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402


def frame_jobs(seed=1):
    rng = np.random.default_rng(seed)
    jobs = [SC.random_job(rng, S.ABSOLUTE, 300, 50)]
    jobs[0]["cam_index"] = (np.arange(300) % 2).astype(np.int32)
    jobs[0]["cam_offsets"], jobs[0]["cam_rotations"] = np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1))
    for _ in range(6):
        jobs += [SC.random_job(rng, S.ROTATION_ONLY, 150, 50), SC.random_job(rng, S.RELATIVE, 150, 50)]
    return jobs


def percentiles(t):
    t = np.sort(np.asarray(t)) * 1e6
    return {"median_us": round(float(np.median(t)), 2), "p10_us": round(float(t[len(t) // 10]), 2), "p90_us": round(float(t[(9 * len(t)) // 10]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    jobs = frame_jobs()
    cells = sum(len(j["models"]) * len(j["sigma"] if j["kind"] == S.ABSOLUTE else j["sigma1"]) for j in jobs)
    fe = F.Frontend()
    table, keep, out = F.sac_job_table(jobs)
    call = fe._L.okvis_fe_sac_consensus
    for _ in range(a.warmup):
        assert call(fe._ctx, len(jobs), table) == 0
    rounds = []
    for _ in range(a.rounds):
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call(fe._ctx, len(jobs), table)
            t.append(time.perf_counter() - t0)
        rounds.append(percentiles(t))
    gpu_counts = [o[0].copy() for o in out]
    result = {"what": "okvis_fe_sac_consensus, one frame", "jobs": len(jobs), "cells": cells, "calls_per_round": a.calls, "gpu_call": rounds}
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as d:
            so = os.path.join(d, "sac_cpu_loop.so")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "sac_cpu_loop.cpp"), "-o", so])
            L = C.CDLL(so)
            L.sac_cpu_consensus.argtypes = [C.c_int32, C.POINTER(F.SacJobC)]
            for _ in range(20):
                L.sac_cpu_consensus(len(jobs), table)
            t = []
            for _ in range(300):
                t0 = time.perf_counter()
                L.sac_cpu_consensus(len(jobs), table)
                t.append(time.perf_counter() - t0)
            result["cpu_one_core_loop"] = percentiles(t)
            result["cpu_counts_equal_gpu_counts"] = all((o[0] == g).all() for o, g in zip(out, gpu_counts))
    fe.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
