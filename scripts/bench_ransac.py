#!/usr/bin/env python3
"""Times a frame's RANSAC for 64 sequences as ONE okvis_fe_ransac call: per sequence two cameras with one rotation-only and one
relative job each (256 2D-2D problems) and one absolute problem over two cameras (64 3D-2D problems), n = 300 correspondences with
15 % of the second bearings swapped, 64 sample slots, max_iterations 50 -- the workloads of profiles/sac_solve_notes.md and
profiles/sac_abs_notes.md together.  Next to it, on the same inputs, the route a caller had before the entry: the samples drawn on
the host (numpy, vectorised), one okvis_fe_sac_solve call and one okvis_fe_sac_solve_absolute call that return every count and
validity flag, and the replay of the loop rule on the host (tests/ransac_statement.py, plain Python).  Host clock around each
part: median, p10, p90.  The kernels' own times come from a kernel-trace run of this script taken on its own, with no counters
(rocprofv3 --kernel-trace --stats -- python scripts/bench_ransac.py --calls 20 --no-parent).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_cases as RC  # noqa: E402
import ransac_statement as R  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

N, SLOTS = 300, 64


def frame_jobs(sequences=64, seed=0):
    jobs = []
    for q in range(sequences):
        for cam in range(2):
            for kind in (RC.ROTATION_ONLY, RC.RELATIVE):
                jobs.append(RC.ransac_job(kind, RC.exact_fields(kind, N, seed + 100 * q + 10 * cam + kind, outliers=0.15), n_slots=SLOTS,
                                          max_iterations=50, probability=0.99, threshold=9.0, seed=seed + 7919 * len(jobs)))
        jobs.append(RC.ransac_job(RC.ABSOLUTE, RC.exact_fields(RC.ABSOLUTE, N, seed + 100 * q + 5, outliers=0.15), n_slots=SLOTS,
                                  max_iterations=50, probability=0.99, threshold=9.0, seed=seed + 7919 * len(jobs)))
    return jobs


def stats_ms(f, calls):
    f()
    times = []
    for _ in range(calls):
        t = time.perf_counter()
        f()
        times.append(time.perf_counter() - t)
    p10, p50, p90 = np.percentile(1e3 * np.array(times), [10, 50, 90])
    return {"median_ms": float(p50), "p10_ms": float(p10), "p90_ms": float(p90)}


def host_draw(rng, jobs):
    """distinct indices per sample: the s smallest of n random keys (what replaces the device sampler on the host)"""
    return [np.argpartition(rng.random((SLOTS, N)), R.SAMPLE_SIZE[j["kind"]], axis=1)[:, :R.SAMPLE_SIZE[j["kind"]]].astype(np.int32) for j in jobs]


def array_bytes(jobs, one_call):
    """the arrays that cross the bus each way (without the job tables and the staging block's alignment)"""
    up = back = 0
    for j in jobs:
        s, width = R.SAMPLE_SIZE[j["kind"]], 9 if j["kind"] == RC.ROTATION_ONLY else 12
        up += 8 * N * 8 if j["kind"] != RC.ABSOLUTE else 8 * N * 7 + 4 * N + 2 * 12 * 8
        if one_call:
            back += 120 + 4 * N          # the record with the model, the inlier list
        else:
            up += 4 * SLOTS * s
            back += SLOTS * (1 + 4 + 8 * width) + 8 * SLOTS * ((N + 63) // 64)          # valid, counts, hypotheses, every ballot word
    return {"bytes_in": up, "bytes_back": back}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-parent", action="store_true")
    a = ap.parse_args()
    jobs = frame_jobs()
    fe = F.Frontend()
    table, keep, out = F.ransac_job_table(jobs)
    res = {"jobs": len(jobs), "n": N, "slots": SLOTS, "one_call": dict(stats_ms(lambda: fe._call("ransac", len(jobs), table), a.calls),
                                                                       **array_bytes(jobs, True))}
    got = [F.ransac_result(o) for o in out]
    res["stops"] = np.bincount([g["stop"] for g in got], minlength=5).tolist()
    res["median_iterations"] = float(np.median([g["iterations"] for g in got]))
    # the others return the true inliers and a swapped bearing or two that lie within the threshold of their epipolar plane by chance
    res["runs_with_exactly_the_true_inliers"] = int(sum(np.array_equal(g["inliers"], np.arange(N - 45)) for g in got))
    if not a.no_parent:
        rng = np.random.default_rng(1)
        rel = [j for j in jobs if j["kind"] != RC.ABSOLUTE]
        absolute = [j for j in jobs if j["kind"] == RC.ABSOLUTE]
        draw = host_draw(rng, rel + absolute)
        names2, names3 = ("kind", "bearing1", "bearing2", "sigma1", "sigma2", "threshold"), ("points", "bearing", "sigma", "cam_index",
                                                                                              "cam_offsets", "cam_rotations", "threshold")
        t2 = F.sac_solve_job_table([dict({k: j[k] for k in names2}, samples=q) for j, q in zip(rel, draw)])
        t3 = F.sac_absolute_job_table([dict({k: j[k] for k in names3}, samples=q) for j, q in zip(absolute, draw[len(rel):])])

        def two_calls():
            fe._call("sac_solve", len(rel), t2[0])
            fe._call("sac_solve_absolute", len(absolute), t3[0])

        def replay():
            return [R.loop(o["counts"], o["valid"], N, R.SAMPLE_SIZE[j["kind"]], 50, 0.99) for j, o in zip(rel + absolute, t2[2] + t3[2])]

        res["parent"] = {"host_draw": stats_ms(lambda: host_draw(rng, rel + absolute), a.calls),
                         "two_calls": dict(stats_ms(two_calls, a.calls), **array_bytes(jobs, False)),
                         "host_replay_python": stats_ms(replay, max(3, a.calls // 10))}
    fe.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
