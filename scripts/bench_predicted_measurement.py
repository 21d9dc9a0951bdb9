#!/usr/bin/env python3
"""Timing of ONE okvis_ba_predicted_measurement call for 64 windows of BASELINE configs[1], every landmark of every window into both
cameras of the newest state, next to okvis_ba_landmark_covariance on the same batch in the same session and to a numpy / scipy
evaluation of the same quantity on one core.

    python scripts/bench_predicted_measurement.py [--windows 64] [--repeat 30] [--optimize 5]

Prints the median of one call (host clock around the entry), its three HIP-event parts (okvis_ba_last_predicted_measurement_ms:
assembly launches, inverse stage = all Dp columns of S0^-1, query stage), the landmark covariance's call and parts, and the host
figure (scipy Cholesky inverse of every S0 tap, then J_l V^-1 J_l^T + A P[R, R] A^T per query from the V / W / jac taps); the last
line is one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from okvis_amd import solver, synthetic  # noqa: E402


def host_predicted_covariance(tap, Q, pair_lm, pair_off, pose_off):
    """the same quantity in fp64 on the host from one window's taps: [n_q, 2, 2]"""
    import scipy.linalg
    S0, V6, W = tap["S0"], tap["V"], tap["W"].reshape(-1, 6, 3)
    Dp = tap["Spp"].shape[0]
    P = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S0, lower=True), np.eye(S0.shape[0])[:, :Dp])[:Dp]
    V = np.empty((V6.shape[0], 3, 3))
    V[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]] = V6
    V[:, [1, 2, 2], [0, 0, 1]] = V6[:, [1, 2, 4]]
    first = np.searchsorted(pair_lm, np.arange(V6.shape[0] + 1))
    out = np.full((len(Q), 2, 2), np.nan)
    for k, (l, p, e, _) in enumerate(Q):
        p0, p1 = first[l], first[l + 1]
        jac = tap["jac"][k]
        if p1 == p0 or not np.isfinite(jac[0]):
            continue
        Jl = jac[:6].reshape(2, 3)
        N = np.linalg.solve(V[l], Jl.T)
        A = np.zeros((2, Dp))
        rows = (pair_off[p0:p1, None] + np.arange(6)).reshape(-1)
        A[:, rows] = -(W[p0:p1].reshape(-1, 3) @ N).T
        for J, off in ((jac[6:18], pose_off[p]), (jac[18:30], pose_off[e])):
            if off >= 0:
                A[:, off:off + 6] += J.reshape(2, 6)
                rows = np.union1d(rows, off + np.arange(6))
        AR = A[:, rows]
        out[k] = Jl @ N + AR @ (P[np.ix_(rows, rows)] @ AR.T)
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
    Qs = [b.newest_state_queries(w) for w in range(a.windows)]
    b.predicted_measurement(Qs)                     # warm-up: scratch allocation, code objects
    b.landmark_covariance()
    t_call, parts = [], dict(assembly=[], inverse=[], query=[])
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        b.predicted_measurement(Qs)
        t_call.append((time.perf_counter() - t0) * 1e3)
        ms = b.last_predicted_measurement_ms()
        for k in parts:
            parts[k].append(ms[k])
    t_lm, l_parts = [], dict(assembly=[], inverse=[], landmark=[])
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        b.landmark_covariance()
        t_lm.append((time.perf_counter() - t0) * 1e3)
        ms = b.last_landmark_covariance_ms()
        for k in l_parts:
            l_parts[k].append(ms[k])
    taps = b.predicted_measurement(Qs, want_taps=True)
    lists = []
    for w in range(a.windows):
        pair_lm, pair_block = b.pairs(w)
        free = np.asarray(wins[w].pose_fixed).reshape(-1) == 0
        off = np.full(free.size, -1, np.int64)
        off[free] = 6 * np.arange(int(free.sum()))
        lists.append((pair_lm, off[pair_block], off))
    b.close()
    t_host, worst = [], 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        host = [host_predicted_covariance(t, Q, *pl) for t, Q, pl in zip(taps, Qs, lists)]
        t_host.append((time.perf_counter() - t0) * 1e3)
    for t, h in zip(taps, host):
        ok = t["flags"] == 0
        d = np.sqrt(np.einsum("lii->li", h[ok]))
        worst = max(worst, float((np.abs(t["cov"][ok] - h[ok]) / (d[:, :, None] * d[:, None, :])).max()))
    med = lambda v: float(np.median(v))  # noqa: E731
    n_q = int(sum(len(Q) for Q in Qs))
    Dp = int(taps[0]["Spp"].shape[0])
    sd = np.concatenate([np.sqrt(np.einsum("lii->li", t["cov"][t["flags"] == 0])).reshape(-1) for t in taps])
    rec = dict(windows=a.windows, D=int(taps[0]["S0"].shape[0]), Dp=Dp, queries=n_q, flagged=int(sum((t["flags"] != 0).sum() for t in taps)),
               call_ms=med(t_call), assembly_ms=med(parts["assembly"]), inverse_ms=med(parts["inverse"]), query_ms=med(parts["query"]),
               inverse_passes=-(-Dp // 15), lmcov_call_ms=med(t_lm), lmcov_assembly_ms=med(l_parts["assembly"]),
               lmcov_inverse_ms=med(l_parts["inverse"]), lmcov_landmark_ms=med(l_parts["landmark"]), host_one_core_ms=med(t_host),
               device_vs_host_worst_e=worst, sigma_px_median=float(np.median(sd)), sigma_px_max=float(sd.max()))
    print(f"one call, {a.windows} windows (D = {rec['D']}, Dp = {Dp}), {n_q} queries: {rec['call_ms']:.3f} ms (assembly launches "
          f"{rec['assembly_ms']:.3f} ms, inverse stage {rec['inverse_ms']:.3f} ms in {rec['inverse_passes']} passes of 15 columns, query stage "
          f"{rec['query_ms']:.3f} ms); landmark covariance of every landmark on the same batch {rec['lmcov_call_ms']:.3f} ms (assembly "
          f"{rec['lmcov_assembly_ms']:.3f} ms, inverse stage {rec['lmcov_inverse_ms']:.3f} ms, lmcov_kernel {rec['lmcov_landmark_ms']:.3f} ms); numpy / "
          f"scipy on one core {rec['host_one_core_ms']:.3f} ms; device against that host evaluation, worst e {worst:.3e}; predicted pixel "
          f"sigma median {rec['sigma_px_median']:.3f} max {rec['sigma_px_max']:.3f} px")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
