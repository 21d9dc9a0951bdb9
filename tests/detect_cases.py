"""Seeded cases of okvis_fe_detect_keypoints, shared by tests/test_detect_host.py and tests/test_gpu_detect.py.  Every family is
built once per process (cases) and stated once (stated: tests/detect_statement.py); where a case is there to show a property,
the builder asserts that the statement really shows it.

A case is a dict: image (2-D uint8, possibly a view with a pitch), threshold, min_dist, max_keypoints, cand_capacity, kp_size.

The largest magnitude: the issue asked for a 0/255 image on which the statement reaches 2^50.  No such image exists: S at a pixel
depends on its 5 x 5 neighbourhood only, and over all 2^25 neighbourhoods of 0/255 pixels the largest S is 665 425 170 360 000
(2^49.24, patch BEST_PATCH below) and the smallest -277 102 632 960 000 (period-four stripes); both were found by exhaustive search.
The binary case embeds both patches and asserts that the statement reaches exactly these two values."""
import functools
import os
import subprocess

import numpy as np

import detect_statement as S
from okvis_amd import frontend as F

HERE = os.path.dirname(os.path.abspath(__file__))
TX, TY = F.DETECT_TILE_X, F.DETECT_TILE_Y                 # the score kernel's tile
WAVE, GROUP = F.DETECT_WAVE, F.DETECT_SELECT_THREADS      # the selection kernel's widths
KP_SIZE = 12.0
BEST_PATCH, BEST_S = 0b0000000100011100111000000, 665425170360000       # bit 5 r + c of the number is pixel (r, c) of the 5 x 5 patch
WORST_S = -277102632960000
NAMES = ("shapes", "pitch", "values", "ties", "edges", "selection", "counts", "capacity", "mixed")


def job(image, threshold=1, min_dist=0, max_keypoints=64, cand_capacity=F.DETECT_MAX_CANDIDATES, kp_size=KP_SIZE):
    return {"image": image, "threshold": int(threshold), "min_dist": int(min_dist), "max_keypoints": int(max_keypoints),
            "cand_capacity": int(cand_capacity), "kp_size": float(kp_size)}


def state(j):
    return S.detect(np.ascontiguousarray(j["image"]), j["threshold"], j["min_dist"], j["max_keypoints"], j["cand_capacity"], j["kp_size"])


def with_pitch(img, extra, offset=0, seed=0):
    """the same pixels as a view of a larger buffer: rows `extra` bytes apart, starting `offset` bytes in; the rest is noise"""
    h, w = img.shape
    buf = np.random.default_rng(1000 + seed).integers(0, 256, h * (w + extra) + offset + 1, dtype=np.uint8)
    view = buf[offset:offset + h * (w + extra)].reshape(h, w + extra)[:, :w]
    view[...] = img
    assert view.strides == (w + extra, 1) and view.ctypes.data == buf.ctypes.data + offset
    return view


def uniform(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def dots(w, h, points, values=255, background=0):
    im = np.full((h, w), background, np.uint8)
    values = np.broadcast_to(values, len(points))
    for (x, y), v in zip(points, values):
        im[y, x] = v
    return im


def dot_grid(n, step=7, margin=4, values=None):
    """n single-pixel dots on a grid `step` apart: far enough for each to be one candidate at its own pixel (a dot reaches two
    pixels into the scores and three into the maximum search)"""
    cols = int(np.ceil(np.sqrt(n)))
    pts = [(margin + step * (i % cols), margin + step * (i // cols)) for i in range(n)]
    w, h = margin * 2 + step * (cols - 1) + 1, margin * 2 + step * ((n - 1) // cols) + 1
    vals = (150 + 15 * (np.arange(n) % 7)) if values is None else values        # seven brightnesses: many ties
    return dots(w, h, pts, vals.astype(np.uint8) if hasattr(vals, "astype") else vals), pts


def pixels(st):
    return [tuple(int(v) for v in p) for p in st["pixel"]]


# ---- the families ---------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 5), (5, 9), (9, 5), (7, 7)] + [(w, h) for w in (TX - 1, TX, TX + 1, 2 * TX + 3) for h in (TY - 1, TY, TY + 1, 2 * TY + 3)]   # (w, h)


def _shapes():
    out = []
    for i, (w, h) in enumerate(SHAPES):
        seed = 100 * i
        while (w, h) == (5, 5) and S.score(uniform(seed, w, h))[2, 2] < 1:       # the one score pixel is a candidate
            seed += 1
        out.append(job(uniform(seed, w, h), 1, 4, 100))
    assert state(out[0])["n_candidates"] == 1 and len(state(out[0])["kp"]) == 1
    return out


def _pitch():
    out = []
    for k, (w, h) in enumerate([(7, 7), (TX + 1, TY + 1), (2 * TX + 3, TY - 1)]):
        img = uniform(300 + k, w, h)
        for extra in (0, 1, 13):
            out.append(job(with_pitch(img, extra, 0, k), 1, 3, 100))
        out.append(job(with_pitch(img, 0, 1, k), 1, 3, 100))           # a view one byte into a larger buffer
        out.append(job(with_pitch(img, 13, 1, k), 1, 3, 100))
        want = state(out[-1])
        assert all(state(j)["kp"].tobytes() == want["kp"].tobytes() for j in out[-5:]) and len(want["kp"]) > 0
    return out


def patch_image(number, w=2 * TX + 3, h=2 * TY + 3, seed=7):
    """a 0/255 random image with the 5 x 5 patch `number` in its middle and period-four stripes at its left end"""
    im = (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)
    bits = np.array([(number >> i) & 1 for i in range(25)], np.uint8).reshape(5, 5) * 255
    im[h // 2 - 2:h // 2 + 3, w // 2 - 2:w // 2 + 3] = bits
    im[:8, :8] = (((np.arange(8) // 2) & 1) * 255).astype(np.uint8)[None, :]
    return im


def _values():
    w, h = 2 * TX + 3, 2 * TY + 3
    y, x = np.mgrid[0:h, 0:w]
    constant = job(np.full((h, w), 93, np.uint8), 1, 0, 100)
    checker = job((((x // 3 + y // 3) & 1) * 255).astype(np.uint8), 1, 0, 2048)
    binary = job(patch_image(BEST_PATCH), 1, 5, 200)
    ramp = job(np.round(100 + 40 * np.sin(x / 9.0) * np.cos(y / 7.0)).astype(np.uint8), 1, 0, 2048)
    st = state(constant)
    assert st["n_candidates"] == 0 and not st["score"].any()
    assert state(checker)["n_candidates"] > 100 and state(checker)["score"].max() > 2 ** 48
    sc = state(binary)["score"]
    assert sc.max() == sc[h // 2, w // 2] == BEST_S and sc.min() == WORST_S           # see the module's docstring
    sc = state(ramp)["score"]
    assert sc.min() < 0 < sc.max() < 2 ** 36 and state(ramp)["n_candidates"] > 0
    return [constant, checker, binary, ramp]


def _ties():
    w, h = 2 * TX + 3, 2 * TY + 3
    out = []
    for size in (2, 3):                                                   # a bright block: one candidate
        im = np.zeros((17, 18), np.uint8)
        im[7:7 + size, 6:6 + size] = 255
        out.append(job(im))
        st = state(out[-1])
        assert pixels(st) == [(6, 7) if size == 2 else (7, 8)] and st["n_candidates"] == 1
    sc = state(out[0])["score"]
    assert sc[7, 6] == sc[7, 7] == sc[8, 6] == sc[8, 7] == sc.max()       # a plateau of four: the lowest index is the candidate
    out.append(job(dots(w, h, [(100, 30), (9, 8), (60, 8)])))             # identical dots far apart: equal S, ordered by index
    st = state(out[-1])
    assert pixels(st) == [(9, 8), (60, 8), (100, 30)] and len(set(st["response"])) == 1
    # plateaus across the tile borders: two-pixel and four-pixel blocks on the border in x, in y and at the corner
    blocks = [((TX - 1, 5), (2, 1)), ((TX - 1, 25), (2, 2)), ((10, TY - 1), (1, 2)), ((30, TY - 1), (2, 2)), ((TX - 1, TY - 1), (2, 2)),
              ((2 * TX - 1, 2 * TY - 1), (2, 2)), ((2 * TX - 1, 6), (2, 1))]
    im = np.zeros((h, w), np.uint8)
    for (x0, y0), (bw, bh) in blocks:
        im[y0:y0 + bh, x0:x0 + bw] = 255
    out.append(job(im))
    st = state(out[-1])
    assert sorted(pixels(st)) == sorted(b[0] for b in blocks)             # each block: one candidate, its first pixel in index order
    for (x0, y0), (bw, bh) in blocks:
        assert len({int(v) for v in st["score"][y0:y0 + bh, x0:x0 + bw].ravel()}) == 1
    return out


def _edges():
    out = []
    for w, h in ((TX + 1, TY + 1), (33, 31)):
        on = [(2, 2), (w - 3, h - 3), (2, h - 3), (w - 3, 2), (10, 2), (10, h - 3)] + ([(2, h // 2)] if h > 24 else [])    # on the domain's edge
        off = [(18, 0), (18, h - 1)] + ([(w - 1, h // 2)] if h > 24 else [])                                             # beyond it
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 7 for i, p in enumerate(on + off) for q in (on + off)[:i])
        out.append(job(dots(w, h, on + off, 255 - 5 * np.arange(len(on + off)))))
        px = pixels(state(out[-1]))
        assert {2, w - 3} <= {p[0] for p in px} and {2, h - 3} <= {p[1] for p in px}
        assert all(p in px for p in on) and len(px) > len(on)             # the dots beyond the domain have their maxima on its edge
    return out


def _selection():
    out = [job(uniform(500, TX + 1, TY + 1), 1, 0, 2048)]                 # min_dist = 0 accepts every candidate
    st = state(out[0])
    assert st["n_candidates"] == len(st["kp"]) > 20 and st["flags"] == 0
    # P strongest, Q at squared distance 8^2 + 15^2 = 17^2 from it (accepted), R at 12^2 + 12^2 = 17^2 - 1 (suppressed)
    P, Q, R = (30, 30), (38, 45), (18, 18)
    im = dots(64, 64, [P, Q, R], [255, 230, 200])
    out.append(job(im, 1, 17))
    out.append(job(im, 1, 0))
    assert pixels(state(out[1])) == [P, Q] and pixels(state(out[2])) == [P, Q, R]
    assert (Q[0] - P[0]) ** 2 + (Q[1] - P[1]) ** 2 == 17 ** 2 and (R[0] - P[0]) ** 2 + (R[1] - P[1]) ** 2 == 17 ** 2 - 1
    assert (R[0] - Q[0]) ** 2 + (R[1] - Q[1]) ** 2 >= 17 ** 2            # R is suppressed by P alone
    img = uniform(501, 2 * TX + 3, 2 * TY + 3)
    n = len(state(job(img, 1, 6, 2048))["kp"])                            # what the rule can accept
    out += [job(img, 1, 6, 1), job(img, 1, 6, n), job(img, 1, 6, n - 1)]
    assert n > 10 and state(out[3])["flags"] == S.FULL and len(state(out[3])["kp"]) == 1
    assert state(out[4])["flags"] == 0 and len(state(out[4])["kp"]) == n
    assert state(out[5])["flags"] == S.FULL and len(state(out[5])["kp"]) == n - 1
    return out


COUNTS = (63, 64, 65, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1)


def _counts():
    out = []
    for n in sorted(set(COUNTS)):
        im, pts = dot_grid(n)
        out.append(job(im, 1, 0, 2048))
        st = state(out[-1])
        assert st["n_candidates"] == n == len(st["kp"]) and sorted(pixels(st)) == sorted(pts)
        if n in (WAVE + 1, GROUP + 1):
            out.append(job(im, 1, 10, 2048))                              # the grid's neighbours (7 apart) suppress each other
            assert 0 < len(state(out[-1])["kp"]) < n
    return out


def _capacity():
    im, _ = dot_grid(65)
    out = [job(im, 1, 0, 100, 65), job(im, 1, 0, 100, 64), job(im, 1, 0, 100, 1)]
    a, b, c = (state(j) for j in out)
    assert a["flags"] == 0 and len(a["kp"]) == 65
    assert b["flags"] == S.OVERFLOW and len(b["kp"]) == 0 and b["n_candidates"] == 65 and c["flags"] == S.OVERFLOW
    return out


def _mixed():
    rng = np.random.default_rng(77)
    out = []
    for j in range(130):
        w, h = int(rng.integers(5, 150)), int(rng.integers(5, 60))
        kind = j % 4
        if kind == 0:
            im = uniform(900 + j, w, h)
        elif kind == 1:
            im = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        elif kind == 2:
            im = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
            for _ in range(int(rng.integers(0, 12))):
                im[int(rng.integers(0, h)), int(rng.integers(0, w))] = int(rng.integers(0, 256))
        else:
            y, x = np.mgrid[0:h, 0:w]
            im = np.round(120 + 100 * np.sin(x / rng.uniform(1, 5)) * np.sin(y / rng.uniform(1, 5))).astype(np.uint8)
        im = with_pitch(im, int(rng.integers(0, 3)) * 5, j % 2, j)
        out.append(job(im, [1, 10 ** 9, 10 ** 12, 10 ** 14][j % 4 if j % 3 else 0], int(rng.integers(0, 21)), int(rng.integers(1, 51)),
                       [F.DETECT_MAX_CANDIDATES, 40, 5][j % 5 % 3], rng.uniform(1, 20)))
    st = [state(j) for j in out]
    assert {s["flags"] for s in st} == {0, S.OVERFLOW, S.FULL} and any(s["n_candidates"] == 0 for s in st)
    assert len({j["image"].shape for j in out}) > 100 and len({j["min_dist"] for j in out}) > 10
    return out


BUILDERS = {"shapes": _shapes, "pitch": _pitch, "values": _values, "ties": _ties, "edges": _edges, "selection": _selection,
            "counts": _counts, "capacity": _capacity, "mixed": _mixed}
assert tuple(BUILDERS) == NAMES


@functools.lru_cache(maxsize=None)
def cases(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def stated(name):
    return [state(j) for j in cases(name)]


# ---- translation ----------------------------------------------------------------------------------------------------------------
def translated(dx, dy, w=2 * TX + 3, h=3 * TY + 3, seed=11):
    """a 40 x 20 block of random bytes in a constant image, its first pixel at (20 + dx, 8 + dy)"""
    im = np.full((h, w), 128, np.uint8)
    im[8 + dy:28 + dy, 20 + dx:60 + dx] = uniform(seed, 40, 20)
    return job(im, 10 ** 9, 5, 30)


SHIFTS = [(0, 0), (1, 0), (0, 1), (TX - 20, 3), (37, TY - 8), (TX + 3, 6)]          # across the tile borders too


# ---- the end-to-end scene -------------------------------------------------------------------------------------------------------
SCENE_SEEDS = (1, 2, 3)
SCENE_THRESHOLD, SCENE_MIN_DIST = 10 ** 11, 8


@functools.lru_cache(maxsize=None)
def scene(seed, noise):
    """-> (job, corners): 160 x 120, axis-aligned rectangles of random grey (contrast at least 40 against the background of 110)
    whose corners lie at least 12 px from each other and from the border, with +-2 grey levels of noise when asked for.  A
    corner is the rectangle's own corner pixel."""
    rng = np.random.default_rng(4000 + seed)
    w, h, bg = 160, 120, 110
    im = np.full((h, w), bg, np.int64)
    rects = []
    while len(rects) < 5:
        rw, rh = int(rng.integers(13, 40)), int(rng.integers(13, 30))
        x0, y0 = int(rng.integers(12, w - 12 - rw)), int(rng.integers(12, h - 12 - rh))
        if all(x0 >= r[0] + r[2] + 12 or r[0] >= x0 + rw + 12 or y0 >= r[1] + r[3] + 12 or r[1] >= y0 + rh + 12 for r in rects):
            rects.append((x0, y0, rw, rh))
    corners = []
    for x0, y0, rw, rh in rects:
        g = int(rng.choice([int(rng.integers(5, bg - 40 + 1)), int(rng.integers(bg + 40, 251))]))
        assert abs(g - bg) >= 40
        im[y0:y0 + rh, x0:x0 + rw] = g
        corners += [(x0, y0), (x0 + rw - 1, y0), (x0, y0 + rh - 1), (x0 + rw - 1, y0 + rh - 1)]
    if noise:
        im = im + np.random.default_rng(5000 + seed).integers(-2, 3, im.shape)
    assert im.min() >= 0 and im.max() <= 255
    assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 12 for i, a in enumerate(corners) for b in corners[:i])
    return job(im.astype(np.uint8), SCENE_THRESHOLD, SCENE_MIN_DIST, 400), corners


def scene_holds(pixel_list, corners):
    """every corner has a keypoint within 1 px in each axis, and every keypoint lies within 1 px of a corner"""
    near = lambda p, q: abs(p[0] - q[0]) <= 1 and abs(p[1] - q[1]) <= 1
    return all(any(near(p, c) for p in pixel_list) for c in corners) and all(any(near(p, c) for c in corners) for p in pixel_list)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def check(got, want, where, with_score=True):
    """everything by bytes: nothing has a tolerance"""
    assert got["n_candidates"] == want["n_candidates"] and got["flags"] == want["flags"], (where, got["n_candidates"], want["n_candidates"], got["flags"], want["flags"])
    for k, dtype in (("pixel", np.int32), ("response", np.float64), ("kp", np.float32)):
        assert got[k].dtype == dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (where, k)
    if with_score:
        assert got["score"].dtype == np.int64 and np.array_equal(got["score"], want["score"]), (where, "score")


def check_shifted(got, base, dx, dy):
    """the image moved by (dx, dy) whole pixels: the same candidates and keypoints in the same order, moved by exactly that"""
    assert got["n_candidates"] == base["n_candidates"] and got["flags"] == base["flags"]
    assert np.array_equal(got["pixel"], base["pixel"] + np.array([dx, dy], np.int32)) and got["response"].tobytes() == base["response"].tobytes()
    # the sub-pixel offsets are unchanged: kp = (float)(pixel + d) with |d| <= 0.5, and pixel + d is exact in float here (x < 2^8, d a
    # double: the float rounding may differ after a shift), so the comparison is on the offsets recomputed in double from the scores
    off = lambda r: np.array([[_axis(r["score"], x, y, 1, 0), _axis(r["score"], x, y, 0, 1)] for x, y in r["pixel"]])
    assert off(got).tobytes() == off(base).tobytes()
    want = (got["pixel"].astype(np.float64) + off(got)).astype(np.float32)
    assert got["kp"][:, :2].tobytes() == want.tobytes() and got["kp"][:, 2].tobytes() == base["kp"][:, 2].tobytes()


def _axis(score, x, y, ax, ay):
    h, w = score.shape
    inside = lambda xx, yy: 2 <= xx <= w - 3 and 2 <= yy <= h - 3
    s0 = score[y, x]
    sm = score[y - ay, x - ax] if inside(x - ax, y - ay) else s0
    sp = score[y + ay, x + ax] if inside(x + ax, y + ay) else s0
    return float(S._offset(sm, s0, sp))


# ---- the host probe -------------------------------------------------------------------------------------------------------------
def build_probe(out_dir, sanitize=True, opt="-O1"):
    """tests/detect_probe.cpp with the sanitizers' runtimes linked statically (the CPU tests), or plain (the benchmark's yardstick)"""
    exe = os.path.join(str(out_dir), "detect_probe")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", opt, *flags, "-ffp-contract=off", os.path.join(HERE, "detect_probe.cpp"), "-o", exe], check=True)
    return exe


def write_probe_input(path, jobs):
    with open(path, "wb") as f:
        np.array([len(jobs)], np.int32).tofile(f)
        for j in jobs:
            im = j["image"]
            h, w = im.shape
            pitch = im.strides[0]
            np.array([w, h, pitch, j["min_dist"], j["max_keypoints"], j["cand_capacity"]], np.int32).tofile(f)
            np.array([j["threshold"]], np.int64).tofile(f)
            block = np.full((h, pitch), 0x3C, np.uint8)          # what lies between the rows is not the image's
            block[:, :w] = im
            block.reshape(-1)[:(h - 1) * pitch + w].tofile(f)


def run_probe(exe, out_dir, jobs, tag="p"):
    """-> per job the dict the statement gives (kp, response, pixel, n_candidates, flags, score)"""
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    write_probe_input(src, jobs)
    subprocess.run([exe, src, dst], check=True)
    raw, at, res = open(dst, "rb").read(), 0, []
    rec = np.dtype([("s", np.int64), ("x", np.int32), ("y", np.int32), ("fx", np.float32), ("fy", np.float32)])
    for j in jobs:
        h, w = j["image"].shape
        n, n_cand, flags, _ = np.frombuffer(raw, np.int32, 4, at)
        sel = np.frombuffer(raw, rec, n, at + 16)
        at += 16 + 24 * int(n)
        score = np.frombuffer(raw, np.int64, w * h, at).reshape(h, w)
        at += 8 * w * h
        kp = np.stack([sel["fx"], sel["fy"], np.full(n, j["kp_size"], np.float32)], axis=1).astype(np.float32).reshape(-1, 3)
        res.append({"kp": kp, "response": sel["s"].astype(np.float64), "pixel": np.stack([sel["x"], sel["y"]], axis=1).astype(np.int32).reshape(-1, 2),
                    "n_candidates": int(n_cand), "flags": int(flags), "score": score})
    assert at == len(raw)
    return res
