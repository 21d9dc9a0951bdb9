#!/usr/bin/env python3
"""Timing of ONE okvis_ba_landmark_covariance call for 64 windows of BASELINE configs[1], every landmark of every window, next to
okvis_ba_state_covariance on the same batch in the same session and to a numpy / scipy evaluation of the same quantity on one core.

    python scripts/bench_landmark_covariance.py [--windows 64] [--repeat 30] [--optimize 5]

Prints the median of one call (host clock around the entry), its three HIP-event parts (okvis_ba_last_landmark_covariance_ms:
assembly launches, inverse stage = all Dp columns of S0^-1, landmark stage), the state covariance's call and parts, and the host
figure (scipy Cholesky inverse of every S0 tap, then V^-1 + G^T P G per landmark from the V / W taps); the last line is one JSON
record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from okvis_amd import solver, synthetic  # noqa: E402


def host_landmark_covariance(tap, pair_lm, pair_off):
    """the same quantity in fp64 on the host from one window's taps: [n_lm, 3, 3]"""
    import scipy.linalg
    S0, V6, W = tap["S0"], tap["V"], tap["W"].reshape(-1, 6, 3)
    Dp = tap["Spp"].shape[0]
    P = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S0, lower=True), np.eye(S0.shape[0])[:, :Dp])[:Dp]
    V = np.empty((V6.shape[0], 3, 3))
    V[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]] = V6
    V[:, [1, 2, 2], [0, 0, 1]] = V6[:, [1, 2, 4]]
    first = np.searchsorted(pair_lm, np.arange(V6.shape[0] + 1))
    out = np.full((V6.shape[0], 3, 3), np.nan)
    for l in range(V6.shape[0]):
        p0, p1 = first[l], first[l + 1]
        if p1 == p0:
            continue
        Vi = np.linalg.inv(V[l])
        rows = (pair_off[p0:p1, None] + np.arange(6)).reshape(-1)
        G = W[p0:p1].reshape(-1, 3) @ Vi
        out[l] = Vi + G.T @ (P[np.ix_(rows, rows)] @ G)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--optimize", type=int, default=5)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")   # (the host figure is one core's)
    wins = synthetic.config_batch(a.windows)
    b = solver.WindowBatch(wins)
    if a.optimize:
        b.optimize(a.optimize)
    b.landmark_covariance()                         # warm-up: scratch allocation, code objects
    b.state_covariance()
    t_call, parts = [], dict(assembly=[], inverse=[], landmark=[])
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        b.landmark_covariance()
        t_call.append((time.perf_counter() - t0) * 1e3)
        ms = b.last_landmark_covariance_ms()
        for k in parts:
            parts[k].append(ms[k])
    t_state, s_parts = [], dict(assembly=[], kernel=[])
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        b.state_covariance()
        t_state.append((time.perf_counter() - t0) * 1e3)
        ms = b.last_covariance_ms()
        for k in s_parts:
            s_parts[k].append(ms[k])
    taps = b.landmark_covariance(want_taps=True)
    lists = []
    for w in range(a.windows):
        pair_lm, pair_block = b.pairs(w)
        free = np.asarray(wins[w].pose_fixed).reshape(-1) == 0
        off = np.full(free.size, -1, np.int64)
        off[free] = 6 * np.arange(int(free.sum()))
        lists.append((pair_lm, off[pair_block]))
    b.close()
    t_host, worst = [], 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        host = [host_landmark_covariance(t, *pl) for t, pl in zip(taps, lists)]
        t_host.append((time.perf_counter() - t0) * 1e3)
    for t, h in zip(taps, host):
        ok = ~t["flags"]
        d = np.sqrt(np.einsum("lii->li", h[ok]))
        worst = max(worst, float((np.abs(t["cov"][ok] - h[ok]) / (d[:, :, None] * d[:, None, :])).max()))
    med = lambda v: float(np.median(v))  # noqa: E731
    n_lm = int(sum(t["cov"].shape[0] for t in taps))
    Dp = int(taps[0]["Spp"].shape[0])
    rec = dict(windows=a.windows, D=int(taps[0]["S0"].shape[0]), Dp=Dp, landmarks=n_lm, flagged=int(sum(t["flags"].sum() for t in taps)),
               call_ms=med(t_call), assembly_ms=med(parts["assembly"]), inverse_ms=med(parts["inverse"]), landmark_ms=med(parts["landmark"]),
               inverse_passes=-(-Dp // 15), state_call_ms=med(t_state), state_assembly_ms=med(s_parts["assembly"]),
               state_kernel_ms=med(s_parts["kernel"]), host_one_core_ms=med(t_host), device_vs_host_worst_e=worst)
    print(f"one call, {a.windows} windows (D = {rec['D']}, Dp = {Dp}), {n_lm} landmarks: {rec['call_ms']:.3f} ms (assembly launches "
          f"{rec['assembly_ms']:.3f} ms, inverse stage {rec['inverse_ms']:.3f} ms in {rec['inverse_passes']} passes of 15 columns, landmark stage "
          f"{rec['landmark_ms']:.3f} ms); state covariance of the newest state on the same batch {rec['state_call_ms']:.3f} ms (assembly "
          f"{rec['state_assembly_ms']:.3f} ms, cov_kernel {rec['state_kernel_ms']:.3f} ms, one pass); numpy / scipy on one core "
          f"{rec['host_one_core_ms']:.3f} ms; device against that host evaluation, worst e {worst:.3e}")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
