#!/usr/bin/env python3
"""Timing of ONE okvis_ba_state_covariance call for 64 windows of BASELINE configs[1] (newest-state covariance, 15 x 15 each)
next to the loop of 64 single calls and to scipy's Cholesky inverse of the 64 tap matrices on one core.

    python scripts/bench_covariance.py [--windows 64] [--repeat 30] [--optimize 5]

Prints the median of one call (host clock around the entry), the share of the assembly launches and of cov_kernel (HIP events,
okvis_ba_last_covariance_ms), the loop of single calls and the host figure; the last line is one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from okvis_amd import solver, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--optimize", type=int, default=5)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")   # (the host figure is one core's)
    import scipy.linalg
    b = solver.WindowBatch(synthetic.config_batch(a.windows))
    if a.optimize:
        b.optimize(a.optimize)
    b.state_covariance()                            # warm-up: scratch allocation, code objects
    t_call, t_asm, t_kern = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        b.state_covariance()
        t_call.append((time.perf_counter() - t0) * 1e3)
        ms = b.last_covariance_ms()
        t_asm.append(ms["assembly"])
        t_kern.append(ms["kernel"])
    t_loop = []
    for _ in range(max(3, a.repeat // 6)):
        t0 = time.perf_counter()
        for w in range(a.windows):
            b.state_covariance(w0=w, n=1)
        t_loop.append((time.perf_counter() - t0) * 1e3)
    taps = [r["S0"] for r in b.state_covariance(want_S0=True)]
    rows = [np.r_[6 * 9:6 * 10, 60 + 9 * 9:60 + 9 * 10] for _ in taps]
    t_host = []
    for _ in range(5):
        t0 = time.perf_counter()
        for S, r in zip(taps, rows):
            scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), np.eye(S.shape[0])[:, r])[r]
        t_host.append((time.perf_counter() - t0) * 1e3)
    b.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    rec = dict(windows=a.windows, D=int(taps[0].shape[0]), call_ms=med(t_call), assembly_ms=med(t_asm), kernel_ms=med(t_kern),
               loop_of_single_calls_ms=med(t_loop), scipy_cholesky_one_core_ms=med(t_host))
    print(f"one call, {a.windows} windows (D = {rec['D']}): {rec['call_ms']:.3f} ms (assembly launches {rec['assembly_ms']:.3f} ms, "
          f"cov_kernel {rec['kernel_ms']:.3f} ms); loop of single calls {rec['loop_of_single_calls_ms']:.3f} ms; "
          f"scipy Cholesky of the taps on one core {rec['scipy_cholesky_one_core_ms']:.3f} ms")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
