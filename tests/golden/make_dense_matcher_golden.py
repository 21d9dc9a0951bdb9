"""Records tests/golden/dense_matcher.npz from the reference's own dense matcher.  Not run by any test.

    OKVIS_REFERENCE=<reference tree> python tests/golden/make_dense_matcher_golden.py [work directory]

needs the reference tree.  Compiles dense_matcher_recorder.cpp with the reference's
okvis_matcher/src/{DenseMatcher,MatchingAlgorithm,ThreadPool}.cpp, with the flags and stand-in headers oracle/ref/Makefile uses
for them, runs every case through okvis::DenseMatcher(1, num_best, use_ratio), and stores inputs and outputs.

Each case has to put the tie rules under test.  The matcher's lists are not visible from outside, so this is checked through
tests/matcher_statement.py once it has reproduced the reference's output of that case exactly: the run must contain a row whose
kept list holds equal distances, a candidate equal to a full list's last entry that was turned away, and a reassignment chain of
depth >= 2."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matcher_statement as S  # noqa: E402

# n_a, n_b, num_best, use_ratio, ratio, threshold, skipped fraction, seed
CASES = [(300, 280, 4, 0, 0.0, 60.0, 0.0, 1),
         (250, 300, 4, 1, 1.1, 60.0, 0.1, 2),
         (200, 200, 2, 0, 0.0, 40.0, 0.2, 3),
         (300, 300, 8, 1, 1.5, 60.0, 0.0, 4),
         (120, 260, 3, 1, 1.0, 50.0, 0.1, 5),
         (280, 150, 6, 0, 0.0, 20.5, 0.05, 6)]


def image(rng, base, n):
    """n descriptors: base descriptors with a few flipped bits (half of them from a few popular ones), exact duplicates, and some
    that look like nothing else"""
    out = np.zeros((n, 48), np.uint8)
    for k in range(n):
        u = rng.random()
        if u < 0.08:
            out[k] = rng.integers(0, 256, 48)
            continue
        if u < 0.2 and k > 0:
            out[k] = out[rng.integers(0, k)]               # an exact duplicate of an earlier keypoint
            continue
        j = rng.integers(0, 8) if rng.random() < 0.5 else rng.integers(0, len(base))
        d = base[j].copy()
        for _ in range(rng.integers(0, 5)):
            d[rng.integers(0, 48)] ^= np.uint8(1 << rng.integers(0, 8))
        out[k] = d
    return out


def build(work):
    ref = os.environ.get("OKVIS_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "okvis_matcher")):
        sys.exit("set OKVIS_REFERENCE to the reference tree (the directory that holds okvis_matcher/)")
    shim = os.path.join(ROOT, "oracle", "shim")
    exe = os.path.join(work, "dense_matcher_recorder")
    src = [os.path.join(ref, "okvis_matcher", "src", f) for f in ("DenseMatcher.cpp", "MatchingAlgorithm.cpp", "ThreadPool.cpp")]
    subprocess.check_call(["g++", "-std=gnu++14", "-O2", "-fPIC", "-w", "-DNDEBUG_SHIM_KEEP_ASSERTS", "-I" + shim,
                           "-I" + os.path.join(shim, "okvis_shadow"), "-I" + os.path.join(ref, "okvis_util", "include"),
                           "-I" + os.path.join(ref, "okvis_matcher", "include"), os.path.join(HERE, "dense_matcher_recorder.cpp"), *src,
                           "-o", exe, "-lpthread"])
    return exe


def main():
    work = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
    exe = build(work)
    out = {"n_cases": np.int32(len(CASES))}
    for i, (n_a, n_b, num_best, use_ratio, ratio, threshold, skipped, seed) in enumerate(CASES):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (40, 48)).astype(np.uint8)
        desc_a, desc_b = image(rng, base, n_a), image(rng, base, n_b)
        skip_a, skip_b = (rng.random(n_a) < skipped).astype(np.uint8), (rng.random(n_b) < skipped).astype(np.uint8)
        path = os.path.join(work, f"case{i}.bin")
        with open(path, "wb") as f:
            np.array([n_a, n_b, num_best, use_ratio], np.int32).tofile(f)
            np.array([threshold, ratio], np.float32).tofile(f)
            for a in (desc_a, desc_b, skip_a, skip_b):
                a.tofile(f)
        calls, pairs = [], []
        for line in subprocess.check_output([exe, path]).decode().split("\n"):
            w = line.split()
            if w:
                (calls if w[0] == "C" else pairs).append((int(w[1]), int(w[2]), float(w[3])))
        if not use_ratio:
            pairs = calls
        pair_a, pair_dist = np.full(n_b, -1, np.int32), np.full(n_b, S.FLT_MAX, np.float32)
        for a, b, d in pairs:
            assert pair_a[b] == -1
            pair_a[b], pair_dist[b] = a, d
        # the statement has to say the same before its view of the lists counts as the reference's
        ev = {}
        s_a, s_d, s_calls = S.match(desc_a, desc_b, threshold, num_best, bool(use_ratio), ratio, skip_a, skip_b, events=ev)
        assert (s_a == pair_a).all() and (s_d == pair_dist).all() and s_calls == calls, f"case {i}: the statement differs"
        assert ev["rows_with_equal_kept"] >= 1 and ev["equal_to_last_turned_away"] >= 1 and ev["max_chain_depth"] >= 2, (i, ev)
        print(f"case {i}: {n_a} x {n_b}, {len(pairs)} paired, {len(calls)} setBestMatch calls, {ev}")
        out.update({f"c{i}_desc_a": desc_a, f"c{i}_desc_b": desc_b, f"c{i}_skip_a": skip_a, f"c{i}_skip_b": skip_b,
                    f"c{i}_threshold": np.float32(threshold), f"c{i}_num_best": np.int32(num_best), f"c{i}_use_ratio": np.int32(use_ratio),
                    f"c{i}_ratio_threshold": np.float32(ratio), f"c{i}_pair_a": pair_a, f"c{i}_pair_dist": pair_dist,
                    f"c{i}_calls_ab": np.array([(a, b) for a, b, _ in calls], np.int32).reshape(-1, 2),
                    f"c{i}_calls_dist": np.array([d for _, _, d in calls], np.float64)})
    dst = os.path.join(HERE, "dense_matcher.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
