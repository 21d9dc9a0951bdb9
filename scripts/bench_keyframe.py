"""Time ONE okvis_fe_keyframe_decision call that carries the keyframe decision of 64 sequences, next to the same definition as a plain
loop on one CPU core (kf_image_serial / kf_fold of okvis_amd/csrc/fe_keyframe.hpp, compiled for the host: tests/keyframe_probe.cpp).

Per sequence one multiframe of 2 cameras with 400 uniform keypoints each on 752 x 480 at 2^-4 pixel, about 35 % of them matched
inside a sub-rectangle: 64 jobs, 128 images, 51200 keypoints per call of the entry.

The host clock is around the C entry (tables and output arrays made beforehand), which returns after a stream synchronise: packing
into the pinned block, the copy in, the kernel, the copy back, the scatter to the caller's arrays and the per-job fold included.

    python scripts/bench_keyframe.py [--sequences 64] [--warmup 200] [--rounds 3] [--calls 2000] [--cpu-passes 50] [--profile]

--profile: warm-up and one round only, no CPU loop (for a run under rocprofv3 --kernel-trace --stats, which gives the kernel alone).
--worst-case: instead of the workload, ONE image of 8192 keypoints on y = x^2, all matched: every keypoint a vertex of both hulls,
8192^2 predicate evaluations per hull and for the inside test, all by one wave; 5 calls, the median.
Prints one JSON line."""
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
from okvis_amd import frontend as F  # noqa: E402


def workload(n_seq, n_kp=400, share=0.35):
    rng = np.random.default_rng(6400)
    jobs = []
    for _ in range(n_seq):
        images = []
        for _ in range(2):
            xy = rng.integers(0, [752 * 16, 480 * 16], (n_kp, 2)).astype(np.float32) / np.float32(16)
            box = np.nonzero((xy[:, 0] > 60) & (xy[:, 0] < 700) & (xy[:, 1] > 40) & (xy[:, 1] < 440))[0]
            m = np.zeros(n_kp, np.uint8)
            m[rng.permutation(box)[:int(share * n_kp)]] = 1
            images.append((np.concatenate([xy, np.full((n_kp, 1), 6, np.float32)], 1), m))
        jobs.append({"images": images, "num_frames": 5, "initialized": True})
    return jobs


def stats(x):
    x = np.asarray(x) * 1e6
    return {"median_us": float(np.median(x)), "p10_us": float(np.percentile(x, 10)), "p90_us": float(np.percentile(x, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--cpu-passes", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--worst-case", action="store_true")
    a = ap.parse_args()
    if a.worst_case:
        x = np.arange(F.KF_MAX_KEYPOINTS, dtype=np.float64) - F.KF_MAX_KEYPOINTS // 2
        job = {"images": [(np.stack([x, x * x], 1).astype(np.float32), np.ones(len(x), np.uint8))]}
        fe = F.Frontend()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = fe.keyframe_decision([job])[0]["images"][0]
            times.append(time.perf_counter() - t0)
        fe.close()
        assert r["hull_all_size"] == r["hull_matched_size"] == len(x) and r["n_inside"] == 0
        print(json.dumps({"worst_case_keypoints": len(x), "hull_vertices": r["hull_all_size"], "call_ms": float(np.median(times)) * 1e3}))
        return
    jobs = workload(a.sequences)
    kp, matched, images, table, counts = F.keyframe_job_table(jobs)
    n_im = len(counts)
    out_arrays = F.keyframe_outputs(len(jobs), n_im, sum(counts), False)
    fe = F.Frontend()
    args = (fe._ctx, len(matched), kp.ctypes.data, matched.ctypes.data, n_im, images, len(jobs), table,
            *[None if out_arrays[k] is None else out_arrays[k].ctypes.data for k in F.KF_OUTPUTS])
    entry = fe._L.okvis_fe_keyframe_decision

    def once():
        t0 = time.perf_counter()
        rc = entry(*args)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    for _ in range(a.warmup):
        once()
    out = {"sequences": a.sequences, "jobs": len(jobs), "images": n_im, "keypoints": int(len(matched)), "matched": int(matched.sum()),
           "hull_vertices_all": int(out_arrays["hull_all_size"].sum()), "hull_vertices_matched": int(out_arrays["hull_matched_size"].sum()),
           "new_keyframes": int(out_arrays["decision"].sum())}
    out["gpu_call"] = [stats([once() for _ in range(a.calls)]) for _ in range(1 if a.profile else a.rounds)]
    if not a.profile:
        # the same definition on one core: the header's plain loop, compiled for the host without contraction
        with tempfile.TemporaryDirectory() as tmp:
            so = os.path.join(tmp, "libkeyframe_probe.so")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                                   os.path.join(ROOT, "tests", "keyframe_probe.cpp"), "-o", so])
            probe = C.CDLL(so)
            begin = np.array([images[i].kp_begin for i in range(n_im)], np.int32)
            count = np.array(counts, np.int32)
            rec, ha, hm = np.zeros((n_im, 8)), np.zeros(len(matched), np.int32), np.zeros(len(matched), np.int32)
            dec, ov, ra = np.zeros(len(jobs), np.uint8), np.zeros(len(jobs)), np.zeros(len(jobs))
            vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
            probe.probe_kf_fold.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]

            def cpu_pass(fold):
                probe.probe_kf_images(n_im, vp(begin), vp(count), vp(kp), vp(matched), vp(rec), vp(ha), vp(hm))
                if fold:
                    for j in range(len(jobs)):
                        t = table[j]
                        dec[j] = probe.probe_kf_fold(t.n_cams, rec[t.im_begin:].ctypes.data, t.num_frames, t.initialized, t.overlap_threshold,
                                                     t.ratio_threshold, ov[j:].ctypes.data, ra[j:].ctypes.data)

            cpu_pass(True)
            per = []
            for _ in range(a.cpu_passes):      # the images only, one C call: the fold is 64 x a few operations, and Python's loop is not timed
                t0 = time.perf_counter()
                cpu_pass(False)
                per.append(time.perf_counter() - t0)
        out["cpu_loop_one_core"] = stats(per)
        out["cpu_loop_over_gpu_call"] = out["cpu_loop_one_core"]["median_us"] / float(np.median([r["median_us"] for r in out["gpu_call"]]))
        same = (rec[:, 0].tobytes() == out_arrays["area_all"].tobytes() and rec[:, 1].tobytes() == out_arrays["area_matched"].tobytes() and
                (rec[:, 5] == out_arrays["n_inside"]).all() and (rec[:, 3] == out_arrays["hull_all_size"]).all() and
                (dec == out_arrays["decision"]).all() and ov.tobytes() == out_arrays["overlap"].tobytes() and ra.tobytes() == out_arrays["ratio"].tobytes())
        out["gpu_equals_cpu_loop"] = bool(same)
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
