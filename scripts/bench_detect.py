"""Time ONE okvis_fe_detect_keypoints call that carries the keypoint detection of 64 sequences x 2 cameras, next to the same
definition as plain loops on one CPU core (detect_image_serial of okvis_amd/csrc/fe_detect.hpp, compiled for the host with
g++ -O2: tests/detect_probe.cpp) and to the numpy statement (tests/detect_statement.py).

Per image a seeded synthetic 752 x 480 scene: rectangles of random grey on a textured background, +-2 grey levels of noise.
threshold is chosen so that 1000 to 4000 candidates arise per image (asserted); min_dist = 40, max_keypoints = 400.

The host clock is around the C entry (table and output arrays made beforehand), which returns after a stream synchronise: packing
the rows into the pinned block, the copy in, both kernels, the copy back and the scatter to the caller's arrays included.

    python scripts/bench_detect.py [--sequences 64] [--warmup 5] [--rounds 3] [--calls 30] [--profile]

--profile: warm-up and one round only, no CPU side (for a run under rocprofv3 --kernel-trace --memory-copy-trace --stats).
Prints one JSON line."""
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
import detect_cases as DC  # noqa: E402
import detect_statement as S  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

W, H = 752, 480
THRESHOLD, MIN_DIST, MAX_KEYPOINTS = 10 ** 10, 40, 400


def image(seed):
    rng = np.random.default_rng(8000 + seed)
    y, x = np.mgrid[0:H, 0:W]
    im = 110 + (8 + 32 * x / W) * np.sin(x / 2.5 + rng.uniform(0, 6)) * np.sin(y / 2.5 + rng.uniform(0, 6))       # texture, stronger to the right
    for _ in range(60):
        rw, rh = int(rng.integers(10, 120)), int(rng.integers(10, 90))
        x0, y0 = int(rng.integers(0, W - rw)), int(rng.integers(0, H - rh))
        im[y0:y0 + rh, x0:x0 + rw] = rng.integers(20, 236)
    im = im + rng.integers(-2, 3, im.shape)
    return np.clip(np.round(im), 0, 255).astype(np.uint8)


def stats(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": float(np.median(x)), "p10_ms": float(np.percentile(x, 10)), "p90_ms": float(np.percentile(x, 90))}


def corner_table():
    """S at an ideal right-angle corner of the given contrast: what a caller chooses `threshold` by"""
    out = {}
    for c in (10, 20, 50, 100):
        im = np.full((21, 21), 50, np.uint8)
        im[10:, 10:] = 50 + c
        out[str(c)] = int(S.score(im).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    images = [image(k) for k in range(2 * a.sequences)]
    table, keep, arrays = F.detect_job_table(images, THRESHOLD, MIN_DIST, MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES, F.DETECT_KP_SIZE,
                                             leave_out=("response", "pixel") if a.profile else ())
    fe = F.Frontend()
    entry, n = fe._L.okvis_fe_detect_keypoints, len(images)

    def once():
        t0 = time.perf_counter()
        rc = entry(fe._ctx, n, table)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    for _ in range(a.warmup):
        once()
    cand = np.array([table[j].n_candidates for j in range(n)])
    kept = np.array([table[j].n_keypoints for j in range(n)])
    assert cand.min() >= 1000 and cand.max() <= 4000, (cand.min(), cand.max())
    out = {"images": n, "width": W, "height": H, "threshold": THRESHOLD, "min_dist": MIN_DIST, "max_keypoints": MAX_KEYPOINTS,
           "candidates_per_image": [int(cand.min()), float(cand.mean()), int(cand.max())],
           "keypoints_per_image": [int(kept.min()), float(kept.mean()), int(kept.max())],
           "bytes_in_pixels": n * ((W * H + 15) & ~15), "bytes_back": n * 16 + n * MAX_KEYPOINTS * 24,
           "corner_score_by_contrast": corner_table()}
    out["gpu_call"] = [stats([once() for _ in range(a.calls)]) for _ in range(1 if a.profile else a.rounds)]
    if not a.profile:
        got = F.detect_results(table, arrays)
        # what the packing alone costs the host: the rows of every image into one block, as the entry does before its copy in
        block = np.zeros(out["bytes_in_pixels"], np.uint8)
        per = []
        for _ in range(10):
            t0 = time.perf_counter()
            at = 0
            for im in images:
                block[at:at + W * H] = im.reshape(-1)
                at += (W * H + 15) & ~15
            per.append(time.perf_counter() - t0)
        out["host_packing_numpy"] = stats(per)
        jobs = [DC.job(im, THRESHOLD, MIN_DIST, MAX_KEYPOINTS) for im in images]
        with tempfile.TemporaryDirectory() as tmp:
            exe = DC.build_probe(tmp, sanitize=False, opt="-O2")
            DC.write_probe_input(os.path.join(tmp, "b.in"), jobs)
            per = []
            for _ in range(3):
                r = subprocess.run([exe, os.path.join(tmp, "b.in"), os.path.join(tmp, "b.out"), "--time"], check=True, capture_output=True)
                per.append(float(r.stdout.split()[-1]))
            out["cpu_loop_one_core"] = stats(per)
            cpu = DC.run_probe(exe, tmp, jobs, tag="b")
        out["gpu_equals_cpu_loop"] = all(g[k].tobytes() == c[k].tobytes() for g, c in zip(got, cpu) for k in ("kp", "response", "pixel")) and \
            all(g["n_candidates"] == c["n_candidates"] and g["flags"] == c["flags"] for g, c in zip(got, cpu))
        per = []
        for k in range(2):
            t0 = time.perf_counter()
            st = DC.state(jobs[k])
            per.append(time.perf_counter() - t0)
            assert st["kp"].tobytes() == got[k]["kp"].tobytes()
        out["numpy_statement_per_image_ms"] = float(np.median(per)) * 1e3
        out["cpu_loop_over_gpu_call"] = out["cpu_loop_one_core"]["median_ms"] / float(np.median([r["median_ms"] for r in out["gpu_call"]]))
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
