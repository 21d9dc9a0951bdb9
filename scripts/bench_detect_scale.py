"""Time ONE okvis_fe_detect_keypoints_scaled call that carries the keypoint detection of 64 sequences x 2 cameras for octaves 0 to 4,
next to okvis_fe_detect_keypoints on the same images and to the same definition as plain loops on one CPU core
(detect_scaled_image_serial of okvis_amd/csrc/fe_detect_scale.hpp, compiled for the host with g++ -O2:
tests/detect_scale_probe.cpp).

Per image a seeded synthetic 752 x 480 scene whose content reaches the coarse layers: the rectangles and the texture of
scripts/bench_detect.py under a box mean whose side grows from left to right in four bands (1, 3, 5 and 9 pixels), +-2 grey levels
of noise on the sharp band only.  Plain noise would put every survivor on layer 0.  threshold, min_dist and max_keypoints are
bench_detect.py's; no job may overflow (asserted).

The host clock is around the C entry (table and output arrays made beforehand), which returns after a stream synchronise: packing
the rows into the pinned block, the copy in, the kernels, the copy back and the scatter to the caller's arrays included.

    python scripts/bench_detect_scale.py [--sequences 64] [--warmup 5] [--rounds 3] [--calls 30] [--profile --octaves N]

--profile: warm-up and one round of the scaled entry at --octaves only, no CPU side (for a run under rocprofv3 --kernel-trace
--memory-copy-trace --stats, which gives the per-kernel times).  Prints one JSON line."""
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
import bench_detect as BD  # noqa: E402
import detect_scale_cases as SC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

W, H = BD.W, BD.H
THRESHOLD, MIN_DIST, MAX_KEYPOINTS = BD.THRESHOLD, BD.MIN_DIST, BD.MAX_KEYPOINTS
BANDS = (1, 3, 5, 9)
CPU_IMAGES = 16          # the CPU loop is timed on the first 16 images and scaled to the batch


def box(im, k):
    src = np.pad(im.astype(np.int64), k // 2, mode="edge")
    acc = np.zeros(im.shape, np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += src[dy:dy + im.shape[0], dx:dx + im.shape[1]]
    return (acc + k * k // 2) // (k * k)


def image(seed):
    rng = np.random.default_rng(8000 + seed)
    y, x = np.mgrid[0:H, 0:W]
    im = 110 + (8 + 32 * x / W) * np.sin(x / 2.5 + rng.uniform(0, 6)) * np.sin(y / 2.5 + rng.uniform(0, 6))
    for _ in range(120):
        rw, rh = int(rng.integers(10, 120)), int(rng.integers(10, 90))
        x0, y0 = int(rng.integers(0, W - rw)), int(rng.integers(0, H - rh))
        im[y0:y0 + rh, x0:x0 + rw] = rng.integers(20, 236)
    im = np.clip(np.round(im), 0, 255).astype(np.int64)
    out = np.zeros((H, W), np.int64)
    for b, k in enumerate(BANDS):
        sl = slice(b * W // len(BANDS), (b + 1) * W // len(BANDS))
        out[:, sl] = box(im, k)[:, sl]
    out[:, :W // len(BANDS)] += rng.integers(-2, 3, (H, W // len(BANDS)))
    return np.clip(out, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--octaves", type=int, default=4)
    a = ap.parse_args()
    images = [image(k) for k in range(2 * a.sequences)]
    n = len(images)
    fe = F.Frontend()

    def timed(entry, table):
        def once():
            t0 = time.perf_counter()
            rc = entry(fe._ctx, n, table)
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            return dt
        return once

    out = {"images": n, "width": W, "height": H, "threshold": THRESHOLD, "min_dist": MIN_DIST, "max_keypoints": MAX_KEYPOINTS, "by_octaves": {}}
    got = {}
    for octaves in ([a.octaves] if a.profile else range(F.DETECT_MAX_OCTAVES + 1)):
        table, keep, arrays = F.detect_scale_job_table(images, THRESHOLD, octaves, MIN_DIST, MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES, F.DETECT_KP_SIZE,
                                                       leave_out=("response", "pixel") if a.profile else ())
        once = timed(fe._L.okvis_fe_detect_keypoints_scaled, table)
        for _ in range(a.warmup):
            once()
        assert not any(table[j].flags & F.DETECT_OVERFLOW for j in range(n))
        layers = np.array([list(table[j].n_layer_candidates) for j in range(n)])
        r = {"n_layers": int(table[0].n_layers), "layer_candidates_mean": [float(v) for v in layers.mean(axis=0)],
             "survivors_mean": float(np.mean([table[j].n_candidates for j in range(n)])),
             "keypoints_mean": float(np.mean([table[j].n_keypoints for j in range(n)])),
             "keypoints_by_layer": [int(sum((arrays[j]["layer"][:table[j].n_keypoints] == l).sum() for j in range(n))) for l in range(F.DETECT_MAX_LAYERS)],
             "pixels_in_layers": int(sum(w * h for w, h in F.detect_layers(W, H, octaves)))}
        r["gpu_call"] = [BD.stats([once() for _ in range(a.calls)]) for _ in range(1 if a.profile else a.rounds)]
        out["by_octaves"][str(octaves)] = r
        got[octaves] = (F.detect_scale_results(table, arrays), keep)
    if not a.profile:
        table, keep, arrays = F.detect_job_table(images, THRESHOLD, MIN_DIST, MAX_KEYPOINTS, F.DETECT_MAX_CANDIDATES, F.DETECT_KP_SIZE)
        once = timed(fe._L.okvis_fe_detect_keypoints, table)
        for _ in range(a.warmup):
            once()
        out["one_layer_entry"] = [BD.stats([once() for _ in range(a.calls)]) for _ in range(a.rounds)]
        old = F.detect_results(table, arrays)
        out["octaves_0_equals_one_layer_entry"] = all(g[k].tobytes() == o[k].tobytes() for g, o in zip(got[0][0], old) for k in ("kp", "response", "pixel"))
        jobs = [SC.job(im, F.DETECT_MAX_OCTAVES, THRESHOLD, MIN_DIST, MAX_KEYPOINTS) for im in images[:CPU_IMAGES]]   # the probe writes every score image
        with tempfile.TemporaryDirectory() as tmp:
            exe = SC.build_probe(tmp, sanitize=False, opt="-O2")
            cpu, per = None, []
            for _ in range(3):
                cpu, seconds = SC.run_probe(exe, tmp, jobs, tag="b", timed=True)
                per.append(seconds)
            out["cpu_loop_one_core_octaves_4"] = dict(BD.stats(np.array(per) * (n / len(jobs))), measured_on_images=len(jobs))
        out["gpu_equals_cpu_loop"] = all(g[k].tobytes() == c[k].tobytes() for g, c in zip(got[F.DETECT_MAX_OCTAVES][0], cpu) for k in ("kp", "response", "pixel", "layer")) and \
            all(g["n_candidates"] == c["n_candidates"] and g["flags"] == c["flags"] for g, c in zip(got[F.DETECT_MAX_OCTAVES][0], cpu))
        med = lambda rounds: float(np.median([r["median_ms"] for r in rounds]))
        out["octaves_4_over_one_layer_entry"] = med(out["by_octaves"]["4"]["gpu_call"]) / med(out["one_layer_entry"])
        out["cpu_loop_over_gpu_call"] = out["cpu_loop_one_core_octaves_4"]["median_ms"] / med(out["by_octaves"]["4"]["gpu_call"])
    fe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
