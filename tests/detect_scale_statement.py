"""The statement of okvis_fe_detect_keypoints_scaled (include/okvis_amd_frontend.h) in numpy int64 / float64, written from the
header's words: the half-sampled pyramid, the one-layer detector (tests/detect_statement.py) on every layer, the cross-layer
test on raw scores, the piecewise linear scale, the full-resolution position, one greedy selection over the survivors of all
layers.  Everything is exact: integers in int64, the doubles a handful of IEEE operations."""
import numpy as np

import detect_statement as S

OVERFLOW, FULL = S.OVERFLOW, S.FULL
MAX_OCTAVES = 4


def pyramid(image, octaves):
    """-> [L_0, L_1, ...] uint8, the layers that exist"""
    layers = [np.ascontiguousarray(image)]
    while len(layers) <= octaves:
        L = layers[-1].astype(np.int64)
        h, w = L.shape[0] >> 1, L.shape[1] >> 1
        if w < 5 or h < 5:
            break
        L = L[:2 * h, :2 * w]                                                  # an odd last row or column is dropped
        layers.append(((L[0::2, 0::2] + L[0::2, 1::2] + L[1::2, 0::2] + L[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return layers


def _domain(Sc):
    h, w = Sc.shape
    return Sc[2:h - 2, 2:w - 2]


def below(Sf, x, y):
    """s_m: the maximum of S_{l-1}[2y+j][2x+i], i, j in -1..2; all 16 lie in the score domain"""
    h, w = Sf.shape
    assert 2 <= 2 * x - 1 and 2 * x + 2 <= w - 3 and 2 <= 2 * y - 1 and 2 * y + 2 <= h - 3
    return int(Sf[2 * y - 1:2 * y + 3, 2 * x - 1:2 * x + 3].max())


def above(Sc, x, y):
    """s_p: the maximum of S_{l+1}[(y>>1)+j][(x>>1)+i], i, j in -1..1, over those in the score domain; None when there is none"""
    h, w = Sc.shape
    xs = [xx for xx in range((x >> 1) - 1, (x >> 1) + 2) if 2 <= xx <= w - 3]
    ys = [yy for yy in range((y >> 1) - 1, (y >> 1) + 2) if 2 <= yy <= h - 3]
    if not xs or not ys:
        return None
    return int(Sc[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].max())


def _sub(Sc, x, y):
    """the sub-pixel offsets dx, dy of the one-layer statement, in double"""
    h, w = Sc.shape
    s0 = Sc[y, x]
    nb = lambda xx, yy: Sc[yy, xx] if 2 <= xx <= w - 3 and 2 <= yy <= h - 3 else s0
    return S._offset(nb(x - 1, y), s0, nb(x + 1, y)), S._offset(nb(x, y - 1), s0, nb(x, y + 1))


def survivors(layers, scores, threshold):
    """-> (the layers' candidate counts, the survivors of all layers in beat order): a survivor is a dict with S, layer, x, y (in
    its layer), kx, ky (float32, full resolution), scale (float64), d (float64), blocked_below / blocked_above for the rejected
    ones, which come in a second list"""
    counts, alive, dead = [], [], []
    for l, Sc in enumerate(scores):
        cands = S.candidates(layers[l], threshold, Sc)
        counts.append(len(cands))
        for s, x, y, fx, fy in cands:
            sm = below(scores[l - 1], x, y) if l >= 1 else None
            sp = above(scores[l + 1], x, y) if l + 1 < len(scores) else None
            ok_below, ok_above = sm is None or s > sm, sp is None or s >= sp
            if not (ok_below and ok_above):
                dead.append({"S": s, "layer": l, "x": x, "y": y, "blocked_below": not ok_below, "blocked_above": not ok_above})
                continue
            d = S._offset(sm, s, sp) if sm is not None and sp is not None else np.float64(0.0)
            t = np.float64(1.0) + d if d >= 0 else np.float64(1.0) + np.float64(0.5) * d
            scale = t * np.float64(2 ** l)
            if l == 0:
                kx, ky = fx, fy
            else:
                dx, dy = _sub(Sc, x, y)
                kx = np.float32((np.float64(x) + dx + np.float64(0.5)) * np.float64(2 ** l) - np.float64(0.5))
                ky = np.float32((np.float64(y) + dy + np.float64(0.5)) * np.float64(2 ** l) - np.float64(0.5))
            alive.append({"S": s, "layer": l, "x": x, "y": y, "kx": kx, "ky": ky, "scale": np.float64(scale), "d": np.float64(d),
                          "w": Sc.shape[1], "missing_above": sp is None and l + 1 < len(scores)})
    alive.sort(key=lambda c: (-c["S"], c["layer"], c["y"] * c["w"] + c["x"]))
    return counts, alive, dead


def centre(c):
    return ((2 * c["x"] + 1) << c["layer"]) - 1, ((2 * c["y"] + 1) << c["layer"]) - 1


def select(alive, min_dist, max_keypoints):
    """-> (accepted, flags, blockers): blockers[i] lists, for every survivor gone through and not accepted, the accepted keypoints
    closer than min_dist"""
    acc, flags, blockers = [], 0, []
    for c in alive:
        cx, cy = centre(c)
        close = [a for a in acc if (cx - centre(a)[0]) ** 2 + (cy - centre(a)[1]) ** 2 < 4 * min_dist * min_dist]
        if close:
            blockers.append((c, close))
            continue
        if len(acc) == max_keypoints:
            flags |= FULL
            break
        acc.append(c)
    return acc, flags, blockers


def detect(image, threshold, octaves, min_dist, max_keypoints, cand_capacity, kp_size):
    """-> dict(kp, response, pixel, layer, scale, n_candidates, flags, n_layers, n_layer_candidates, score [per layer], pyramid
    [layers 1..]) and, for the case builders, survivors / rejected / blockers"""
    layers = pyramid(image, octaves)
    scores = [S.score(L) for L in layers]
    counts, alive, dead = survivors(layers, scores, threshold)
    n_layer = np.zeros(MAX_OCTAVES + 1, np.int32)
    n_layer[:len(counts)] = counts
    acc, flags, blockers, n_cand = [], 0, [], len(alive)
    if any(c > cand_capacity for c in counts):                                  # the cross-layer test is not run
        flags, n_cand = OVERFLOW, (counts[0] if len(layers) == 1 else 0)          # one layer: every candidate survives
    elif len(alive) > cand_capacity:
        flags = OVERFLOW
    else:
        acc, flags, blockers = select(alive, min_dist, max_keypoints)
    size = lambda c: np.float32(np.float64(np.float32(kp_size)) * c["scale"])
    return {"kp": np.array([[c["kx"], c["ky"], size(c)] for c in acc], np.float32).reshape(-1, 3),
            "response": np.array([np.float64(c["S"]) for c in acc], np.float64), "pixel": np.array([[c["x"], c["y"]] for c in acc], np.int32).reshape(-1, 2),
            "layer": np.array([c["layer"] for c in acc], np.int32), "scale": np.array([c["scale"] for c in acc], np.float64),
            "n_candidates": n_cand, "flags": flags, "n_layers": len(layers), "n_layer_candidates": n_layer, "score": scores, "pyramid": layers[1:],
            "survivors": alive, "rejected": dead, "blockers": blockers, "accepted": acc}
