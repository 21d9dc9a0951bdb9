"""The sampler and the loop of okvis_fe_ransac as include/okvis_amd_frontend.h states them, in numpy integer and float64
arithmetic.  The referee of okvis_amd/csrc/fe_sac_loop.hpp: the probe (tests/ransac_probe.cpp) and the device are held to these
functions exactly.  Nothing here is pinned to OpenGV (its source is not part of the reference tree)."""
import math

import numpy as np

STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_EXHAUSTED, STOP_SKIPS, STOP_NO_SAMPLE = range(5)
SAMPLE_SIZE = {0: 4, 1: 2, 2: 8}          # by OKVIS_FE_SAC_* kind
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Q_LO, Q_HI = 2.0 ** -52, 1.0 - 2.0 ** -52
SKIP_FACTOR = 10


def philox(counter, key):
    """Philox4x32-10.  counter [..., 4], key [..., 2] (uint32 values) -> [..., 4] uint32.  Python integers and numpy uint64 alike."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    mask, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 bits: fits 64
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & mask, (p0 >> sh) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def draws(seed, m, s):
    """u_0 .. u_{s-1} of slot m as Python integers"""
    key = [seed & MASK, (seed >> 32) & MASK]
    u = [int(x) for x in philox([m, 0, 0, 0], key)]
    if s > 4:
        u += [int(x) for x in philox([m, 1, 0, 0], key)]
    return u[:s]


def sample(seed, m, n, s):
    """the sample of slot m: the sparse Fisher-Yates over A[i] = i, the touched entries in a dict"""
    assert 0 < s <= 8 and n >= s
    A, out = {}, []
    for k, u in enumerate(draws(int(seed), int(m), s)):
        j = k + ((u * (n - k)) >> 32)
        ak, aj = A.get(k, k), A.get(j, j)
        A[k], A[j] = aj, ak
        out.append(A[k])
    return out


def samples(seed, n_slots, n, s):
    """-> [n_slots][s] int32.  The generator vectorised over the slots, the draw slot by slot."""
    seed, n_slots = int(seed), int(n_slots)
    key = np.array([seed & MASK, (seed >> 32) & MASK], np.uint64)
    ctr = np.zeros((n_slots, 4), np.uint64)
    ctr[:, 0] = np.arange(n_slots)
    u = philox(ctr, np.broadcast_to(key, (n_slots, 2)))
    if s > 4:
        ctr[:, 1] = 1
        u = np.concatenate([u, philox(ctr, np.broadcast_to(key, (n_slots, 2)))], axis=1)
    out = np.zeros((n_slots, s), np.int32)
    for m in range(n_slots):
        A = {}
        for k in range(s):
            j = k + ((int(u[m, k]) * (n - k)) >> 32)
            ak, aj = A.get(k, k), A.get(j, j)
            A[k], A[j] = aj, ak
            out[m, k] = aj
    return out


def done(it, c, n, s, p):
    """the adaptive bound, multiplications only (Python floats are IEEE doubles, every operation rounded on its own)"""
    w = float(c) / float(n)
    ws = w
    for _ in range(s - 1):
        ws = ws * w
    q = min(max(1.0 - ws, Q_LO), Q_HI)
    r, b, e = 1.0, q, int(it)
    while e:
        if e & 1:
            r = r * b
        b = b * b
        e >>= 1
    return r <= 1.0 - p


def done_log(it, c, n, s, p):
    """the bound in its textbook form, for information: it >= log(1 - p) / log(1 - w^s)"""
    ws = (c / n) ** s
    if ws <= 0.0 or 1.0 - ws == 1.0:          # log(1) = 0: the bound is infinite
        return False
    if ws >= 1.0:
        return True
    return it >= math.log(1.0 - p) / math.log(1.0 - ws)


def loop(counts, valid, n, s, max_iterations=50, p=0.99):
    """the sequential rule over the slots in order -> dict(best, n_inliers, iterations, skipped, stop)"""
    it, skipped, best, best_count, stop = 0, 0, -1, -1, STOP_EXHAUSTED
    for m in range(len(counts)):
        if not valid[m]:
            skipped += 1
            if skipped >= SKIP_FACTOR * max_iterations:
                stop = STOP_SKIPS
                break
            continue
        if counts[m] > best_count:
            best, best_count = m, int(counts[m])
        it += 1
        if done(it, best_count, n, s, p):
            stop = STOP_CONVERGED
            break
        if it > max_iterations:
            stop = STOP_MAX_ITERATIONS
            break
    return {"best": best, "n_inliers": max(best_count, 0) if best >= 0 else 0, "iterations": it, "skipped": skipped, "stop": stop}


NO_SAMPLE = {"best": -1, "n_inliers": 0, "iterations": 0, "skipped": 0, "stop": STOP_NO_SAMPLE}
