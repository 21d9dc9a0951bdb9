"""Time ONE okvis_fe_describe_keypoints call that carries the keypoint description of 64 sequences x 2 cameras with 400 keypoints
per image, ONE okvis_fe_detect_and_describe call against okvis_fe_detect_keypoints followed by okvis_fe_describe_keypoints on the
same images, and the same extraction as plain loops on one CPU core (describe_image_serial of okvis_amd/csrc/fe_describe.hpp,
compiled for the host with g++ -O2: tests/describe_probe.cpp).

Images: the seeded 752 x 480 scenes of scripts/bench_detect.py.  Keypoints of the describe call: 400 seeded positions per image,
all inside the margin; the angle stage runs (a radial-tangential camera, gravity 20 degrees off the image's y axis).  The chain
detects with min_dist = 12 so that the selection fills its 400 keypoints (asserted: at least 350 per image on average).

The host clock is around the C entries (tables and output arrays made beforehand), which return after a stream synchronise.

    python scripts/bench_describe.py [--sequences 64] [--warmup 5] [--rounds 3] [--calls 30] [--profile]

--profile: warm-up and one round of each call only, no CPU side (for a run under rocprofv3 --kernel-trace --memory-copy-trace
--stats).  Prints one JSON line."""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import describe_cases as BC  # noqa: E402
from bench_detect import H, W, image, stats  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

N_KP, THRESHOLD, MIN_DIST = 400, 10 ** 10, 12
INTR = [458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
DIRECTION = [np.sin(np.radians(20.0)) * np.cos(0.3), np.cos(np.radians(20.0)), np.sin(np.radians(20.0)) * np.sin(0.3)]


def keypoints(seed):
    rng = np.random.default_rng(9000 + seed)
    return np.stack([rng.uniform(11.5, W - 12.5, N_KP), rng.uniform(11.5, H - 12.5, N_KP), np.full(N_KP, 12.0)], axis=1).astype(np.float32)


def timed(entry, *call):
    def once():
        t0 = time.perf_counter()
        rc = entry(*call)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    n = 2 * a.sequences
    images = [image(k) for k in range(n)]
    kps = [keypoints(k) for k in range(n)]
    cam = F.camera(INTR, 1, W, H)
    fe = F.Frontend()
    L, ctx = fe._L, fe._ctx
    rounds = 1 if a.profile else a.rounds
    out = {"images": n, "width": W, "height": H, "keypoints_per_image": N_KP, "bytes_in_pixels": n * ((W * H + 15) & ~15)}

    # ---- describe alone: 400 given keypoints per image, the angle stage on
    table, keep, arrays = F.describe_job_table(images, kps, cam, DIRECTION, None, want=("rot", "angle"))
    once = timed(L.okvis_fe_describe_keypoints, ctx, n, table)
    for _ in range(a.warmup):
        once()
    out["describe_call"] = [stats([once() for _ in range(a.calls)]) for _ in range(rounds)]
    got = F.describe_results(table, arrays)
    assert all(g["n_valid"] == N_KP for g in got)
    out["bytes_back_describe"] = n * N_KP * (F.DESCRIBE_BYTES + 1 + 4 + 4)

    # ---- the chain against the two calls in sequence, on the keypoints the detector selects
    det, keep_d, arr_d = F.detect_job_table(images, THRESHOLD, MIN_DIST, N_KP, F.DETECT_MAX_CANDIDATES, F.DETECT_KP_SIZE)
    rows = [np.zeros((N_KP, 3), np.float32) for _ in images]
    chain, keep_c, arr_c = F.describe_job_table(images, rows, cam, DIRECTION, None, want=("rot", "angle"))
    once_chain = timed(L.okvis_fe_detect_and_describe, ctx, n, det, chain)
    for _ in range(a.warmup):
        once_chain()
    kept = np.array([det[j].n_keypoints for j in range(n)])
    assert kept.mean() >= 350, kept.mean()
    out["chain_keypoints_per_image"] = [int(kept.min()), float(kept.mean()), int(kept.max())]
    out["chain_call"] = [stats([once_chain() for _ in range(a.calls)]) for _ in range(rounds)]

    det2, keep_d2, arr_d2 = F.detect_job_table(images, THRESHOLD, MIN_DIST, N_KP, F.DETECT_MAX_CANDIDATES, F.DETECT_KP_SIZE)
    seq, keep_s, arr_s = F.describe_job_table(images, rows, cam, DIRECTION, None, want=("rot", "angle"))
    for j in range(n):
        seq[j].kp = arr_d2[j]["kp"].ctypes.data          # the describe call reads what the detect call wrote

    def two_calls():
        t0 = time.perf_counter()
        rc = L.okvis_fe_detect_keypoints(ctx, n, det2)
        for j in range(n):
            seq[j].n = det2[j].n_keypoints
        rc2 = L.okvis_fe_describe_keypoints(ctx, n, seq)
        dt = time.perf_counter() - t0
        assert rc == 0 and rc2 == 0, (rc, rc2)
        return dt

    for _ in range(a.warmup):
        two_calls()
    out["two_calls"] = [stats([two_calls() for _ in range(a.calls)]) for _ in range(rounds)]
    out["chain_equals_two_calls"] = all(arr_c[j][k][:kept[j]].tobytes() == arr_s[j][k][:kept[j]].tobytes() for j in range(n) for k in ("desc", "flags", "rot", "angle")) and \
        all(arr_d[j]["kp"][:kept[j]].tobytes() == arr_d2[j]["kp"][:kept[j]].tobytes() for j in range(n))
    med = lambda key: float(np.median([r["median_ms"] for r in out[key]]))
    out["two_calls_minus_chain_ms"] = med("two_calls") - med("chain_call")

    if not a.profile:
        jobs = [{"image": im, "kp": kp, "rot": g["rot"]} for im, kp, g in zip(images, kps, got)]
        with tempfile.TemporaryDirectory() as tmp:
            exe = BC.build_probe(tmp, sanitize=False, opt="-O2")
            BC.write_probe_input(os.path.join(tmp, "b.in"), jobs)
            per = []
            for _ in range(3):
                r = subprocess.run([exe, os.path.join(tmp, "b.in"), os.path.join(tmp, "b.out"), "--time"], check=True, capture_output=True)
                per.append(float(r.stdout.split()[-1]))
            out["cpu_loop_one_core"] = stats(per)
            cpu = BC.run_probe(exe, tmp, jobs, tag="b")
        out["gpu_equals_cpu_loop"] = all(g["desc"].tobytes() == c["desc"].tobytes() and (g["flags"] & 1).tobytes() == c["flags"].tobytes() for g, c in zip(got, cpu))
        out["cpu_loop_over_gpu_call"] = out["cpu_loop_one_core"]["median_ms"] / med("describe_call")
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
