"""The statement of okvis_fe_detect_keypoints (include/okvis_amd_frontend.h) in numpy int64 / float64, written from the header's
words: Sobel derivatives, the binomially weighted structure tensor, S = 16 (A C - B^2) - (A + C)^2, candidates under the total
order "larger S, then lower row-major index", the parabola's vertex per axis, greedy disc suppression.  Everything is exact:
integers in int64, one IEEE division and one addition per sub-pixel offset."""
import numpy as np

OVERFLOW, FULL = 1, 2
LOWEST = np.iinfo(np.int64).min


def score(image):
    """-> S [h][w] int64, 0 outside the score domain 2 <= x <= w-3, 2 <= y <= h-3"""
    I = np.asarray(image).astype(np.int64)
    h, w = I.shape
    assert h >= 5 and w >= 5
    Ix, Iy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    Ix[1:-1, 1:-1] = (I[:-2, 2:] + 2 * I[1:-1, 2:] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[1:-1, :-2] + I[2:, :-2])
    Iy[1:-1, 1:-1] = (I[2:, :-2] + 2 * I[2:, 1:-1] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[:-2, 1:-1] + I[:-2, 2:])
    assert np.abs(Ix).max() <= 1020 and np.abs(Iy).max() <= 1020

    def window(P):
        out = np.zeros((h, w), np.int64)
        for dy, ky in ((-1, 1), (0, 2), (1, 1)):
            for dx, kx in ((-1, 1), (0, 2), (1, 1)):
                out[2:h - 2, 2:w - 2] += ky * kx * P[2 + dy:h - 2 + dy, 2 + dx:w - 2 + dx]
        return out

    A, B, C = window(Ix * Ix), window(Ix * Iy), window(Iy * Iy)
    S = 16 * (A * C - B * B) - (A + C) * (A + C)
    assert np.abs(S).max() < 2 ** 53
    return S


def _offset(sm, s0, sp):
    num, den = np.int64(sm) - np.int64(sp), 2 * (np.int64(sm) - 2 * np.int64(s0) + np.int64(sp))
    if den == 0:
        return np.float64(0.0)
    d = np.float64(num) / np.float64(den)
    return min(max(d, np.float64(-0.5)), np.float64(0.5))


def candidates(image, threshold, S=None):
    """-> the candidates in beat order, strongest first: a list of (S, x, y, kp_x, kp_y) with kp_* float32"""
    S = score(image) if S is None else S
    h, w = S.shape
    pad = np.full((h + 2, w + 2), LOWEST, np.int64)              # outside the score domain: beaten
    pad[3:h - 1, 3:w - 1] = S[2:h - 2, 2:w - 2]
    centre = pad[1:-1, 1:-1]
    is_cand = np.zeros((h, w), bool)
    is_cand[2:h - 2, 2:w - 2] = S[2:h - 2, 2:w - 2] >= threshold
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
            earlier = dy < 0 or (dy == 0 and dx < 0)             # q has the lower index: p must be strictly larger
            is_cand &= (centre > q) if earlier else (centre >= q)
    ys, xs = np.nonzero(is_cand)
    order = sorted(range(len(xs)), key=lambda i: (-int(S[ys[i], xs[i]]), int(ys[i]) * w + int(xs[i])))
    out = []
    for i in order:
        x, y = int(xs[i]), int(ys[i])
        s0 = S[y, x]
        nb = lambda xx, yy: S[yy, xx] if 2 <= xx <= w - 3 and 2 <= yy <= h - 3 else s0
        fx = np.float32(np.float64(x) + _offset(nb(x - 1, y), s0, nb(x + 1, y)))
        fy = np.float32(np.float64(y) + _offset(nb(x, y - 1), s0, nb(x, y + 1)))
        out.append((int(s0), x, y, fx, fy))
    return out


def select(cands, min_dist, max_keypoints, cand_capacity, kp_size):
    """-> dict(kp [n][3] float32, response [n] float64, pixel [n][2] int32, n_candidates, flags)"""
    flags, acc = 0, []
    if len(cands) > cand_capacity:
        flags = OVERFLOW
    else:
        for c in cands:
            if all((c[1] - a[1]) ** 2 + (c[2] - a[2]) ** 2 >= min_dist * min_dist for a in acc):
                if len(acc) == max_keypoints:
                    flags |= FULL
                    break
                acc.append(c)
    return {"kp": np.array([[c[3], c[4], np.float32(kp_size)] for c in acc], np.float32).reshape(-1, 3),
            "response": np.array([np.float64(c[0]) for c in acc], np.float64), "pixel": np.array([[c[1], c[2]] for c in acc], np.int32).reshape(-1, 2),
            "n_candidates": len(cands), "flags": flags}


def detect(image, threshold, min_dist, max_keypoints, cand_capacity, kp_size):
    S = score(image)
    r = select(candidates(image, threshold, S), min_dist, max_keypoints, cand_capacity, kp_size)
    r["score"] = S
    return r
