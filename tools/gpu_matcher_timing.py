"""measurement (not a test): the descriptor matcher on the device next to the host's double loop it replaces.

    python tools/gpu_matcher_timing.py [--out FILE]        every step below, each GPU step a child process under its own timeout
    python tools/gpu_matcher_timing.py --step match        12 jobs of 400 x 400 x 48 bytes in one okvis_fe_match_descriptors call
    python tools/gpu_matcher_timing.py --step candidates   one 4096 x 4096 x 48 bytes okvis_fe_hamming_candidates call
    python tools/gpu_matcher_timing.py --step host         tools/micro/host_hamming_loop.cpp (g++ -O2, one thread) on the same data

A call is timed with the host clock around the entry, which returns after a stream synchronise; warm-up calls first, then many
repeats, and the spread is printed with the median.  For kernel times run one step under rocprofv3 --kernel-trace --stats."""
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
THRESHOLD = 60.0


def image(rng, base, n):
    pick = np.where(rng.random(n) < 0.5, rng.integers(0, 8, n), rng.integers(0, len(base), n))
    out = base[pick].copy()
    for k in np.nonzero(rng.random(n) < 0.1)[0]:
        out[k] = rng.integers(0, 256, base.shape[1])
    flips = rng.integers(0, 5, n)
    for k in range(n):
        for _ in range(flips[k]):
            out[k, rng.integers(0, base.shape[1])] ^= np.uint8(1 << rng.integers(0, 8))
    return out


def scene(seed, n_a, n_b, n_base):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_base, 48)).astype(np.uint8)
    return image(rng, base, n_a), image(rng, base, n_b)


def match_jobs():
    return [scene(k, 400, 400, 300) for k in range(12)]


def candidate_job():
    return scene(99, 4096, 4096, 3000)


def spread(seconds):
    s = np.sort(np.asarray(seconds))
    return {"repeats": len(s), "min_s": float(s[0]), "median_s": float(s[len(s) // 2]), "p90_s": float(s[int(0.9 * (len(s) - 1))]),
            "max_s": float(s[-1])}


def step_match(warmup, repeats):
    from okvis_amd import frontend as F
    fe = F.Frontend()
    jobs = match_jobs()
    table = (F.MatchJobC * len(jobs))()
    keep = []
    for t, (a, b) in zip(table, jobs):
        out = np.zeros(len(b), np.int32), np.zeros(len(b), np.float32), np.zeros(len(b), np.uint8)
        keep.append(out)
        t.n_a, t.n_b, t.desc_a, t.desc_b = len(a), len(b), a.ctypes.data, b.ctypes.data
        t.pair_a, t.pair_dist, t.accepted = (o.ctypes.data for o in out)
    call = lambda: fe._call("match_descriptors", len(jobs), table, 48, THRESHOLD, 4, 0, 0.0)  # noqa: E731
    for _ in range(warmup):
        call()
    seconds = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        seconds.append(time.perf_counter() - t0)
    r = spread(seconds)
    r.update(step="match", jobs=len(jobs), shape=[400, 400, 48], num_best=4, accepted=int(sum(o[2].sum() for o in keep)))
    fe.close()
    return r


def step_candidates(warmup, repeats):
    from okvis_amd import frontend as F
    fe = F.Frontend()
    a, b = candidate_job()
    n = C.c_int32(0)
    args = (48, len(a), a.ctypes.data, None, len(b), b.ctypes.data, None, THRESHOLD)
    fe._call("hamming_candidates", *args, 0, None, None, C.byref(n))
    total = n.value
    pairs = np.zeros((total, 2), np.int32)
    out = {"step": "candidates", "shape": [4096, 4096, 48], "pairs": total}
    for name, cap, ptr in (("count_only", 0, None), ("fill", total, pairs.ctypes.data)):
        call = lambda: fe._call("hamming_candidates", *args, cap, ptr, None, C.byref(n))  # noqa: E731
        for _ in range(warmup):
            call()
        seconds = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            call()
            seconds.append(time.perf_counter() - t0)
        out[name] = spread(seconds)
    fe.close()
    return out


def step_host(repeats):
    work = tempfile.mkdtemp()
    exe = os.path.join(work, "host_hamming_loop")
    subprocess.check_call(["g++", "-O2", os.path.join(ROOT, "tools", "micro", "host_hamming_loop.cpp"), "-o", exe])
    out = {"step": "host"}
    for name, jobs, reps in (("match_12x400x400", match_jobs(), repeats), ("candidates_4096x4096", [candidate_job()], max(3, repeats // 10))):
        path = os.path.join(work, name + ".bin")
        with open(path, "wb") as f:
            np.array([len(jobs), 48], np.int32).tofile(f)
            np.array([THRESHOLD], np.float32).tofile(f)
            for a, b in jobs:
                np.array([len(a), len(b)], np.int32).tofile(f)
                a.tofile(f)
                b.tofile(f)
        out[name] = json.loads(subprocess.check_output(["taskset", "-c", "0", exe, path, str(reps)]).decode())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["match", "candidates", "host"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step == "match":
        print(json.dumps(step_match(args.warmup, args.repeats)))
        return
    if args.step == "candidates":
        print(json.dumps(step_candidates(args.warmup, max(10, args.repeats // 3))))
        return
    if args.step == "host":
        print(json.dumps(step_host(30)))
        return
    results = []
    for step, limit in (("host", 600), ("match", 180), ("candidates", 180), ("match", 180), ("candidates", 180)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--warmup", str(args.warmup),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                      # nothing more is started after a step that failed
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            sys.exit(p.returncode)
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
