"""Seeded cases of okvis_fe_detect_keypoints_scaled, shared by tests/test_detect_scale_host.py and
tests/test_gpu_detect_scale.py.  Every family is built once per process (cases) and stated once (stated:
tests/detect_scale_statement.py); where a case is there to show a property, the builder asserts that the statement shows it.

A case is a detect_cases job (image, threshold, min_dist, max_keypoints, cand_capacity, kp_size) with octaves."""
import functools
import os
import subprocess

import numpy as np

import detect_cases as DC
import detect_scale_statement as SS
from okvis_amd import frontend as F

HERE = os.path.dirname(os.path.abspath(__file__))
TX, TY = DC.TX, DC.TY
NAMES = ("shapes", "long", "waves", "ties", "edges", "counts", "capacity", "across", "pitch", "mixed")
FIELDS = ("threshold", "octaves", "min_dist", "max_keypoints", "cand_capacity", "kp_size")


def job(image, octaves, threshold=1, min_dist=0, max_keypoints=64, cand_capacity=F.DETECT_MAX_CANDIDATES, kp_size=DC.KP_SIZE):
    return dict(DC.job(image, threshold, min_dist, max_keypoints, cand_capacity, kp_size), octaves=int(octaves))


def state(j):
    return SS.detect(np.ascontiguousarray(j["image"]), j["threshold"], j["octaves"], j["min_dist"], j["max_keypoints"], j["cand_capacity"], j["kp_size"])


def waves(w=384, h=96, periods=(6, 12, 24, 48, 96)):
    """five vertical bands, w // 5 wide, of 128 + 100 sin(2 pi x / p) sin(2 pi y / p), p = 6, 12, 24, 48, 96: structure for every
    layer; the columns left over are 0.  (384 x 96, threshold 1e9, octaves 4: layer candidates 1936 / 602 / 134 / 18 / 1, survivors
    767 / 173 / 42 / 7 / 1.)"""
    y, x = np.mgrid[0:h, 0:w]
    im, bw = np.zeros((h, w)), w // len(periods)
    for b, p in enumerate(periods):
        sl = slice(b * bw, (b + 1) * bw)
        im[:, sl] = 128 + 100 * np.sin(2 * np.pi * x[:, sl] / p) * np.sin(2 * np.pi * y[:, sl] / p)
    return np.round(im).astype(np.uint8)


def blurred(seed, w, h, k):
    """uniform noise under a k x k box mean: the larger k, the coarser the layer its corners are found on"""
    src = np.random.default_rng(seed).integers(0, 256, (h + k - 1, w + k - 1)).astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += src[dy:dy + h, dx:dx + w]
    return (acc // (k * k)).astype(np.uint8)


def layer_counts(st, key="survivors"):
    return [sum(1 for c in st[key] if c["layer"] == l) for l in range(SS.MAX_OCTAVES + 1)]


# ---- the families ---------------------------------------------------------------------------------------------------------------
SMALL = [(5, 5), (9, 9), (10, 10), (11, 23), (19, 10), (20, 9)]
TILE_EDGE = [(w, h) for w in range(2 * TX - 1, 2 * TX + 4) for h in range(2 * TY - 1, 2 * TY + 4)]     # layer 1 meets the score tile's edges
N_LAYERS = {(5, 5): 1, (9, 9): 1, (10, 10): 2, (11, 23): 2, (19, 10): 2, (20, 9): 1}


def _shapes():
    out = [job(DC.uniform(40 + i, w, h), 4, 1, 3, 200) for i, (w, h) in enumerate(SMALL)]
    out += [job(blurred(60 + i, w, h, 2 + i % 4), 4, 1, 3, 400) for i, (w, h) in enumerate(TILE_EDGE)]
    for j, (w, h) in zip(out, SMALL):
        assert state(j)["n_layers"] == N_LAYERS[(w, h)]
    assert [L.shape for L in SS.pyramid(out[2]["image"], 4)] == [(10, 10), (5, 5)]
    st = [state(j) for j in out[len(SMALL):]]
    assert all(s["n_layers"] == 3 and s["flags"] in (0, SS.FULL) for s in st) and sum(len(set(s["layer"])) >= 2 for s in st) > 5
    return out


def _long():
    """8192 x 80: five layers, the last 512 x 5; 8192 x 5 and 5 x 8192: one layer"""
    wide = np.tile(waves(512, 80, (24, 48, 96, 48, 24)), (1, 16))                 # the short periods alone would pass cand_capacity
    wide[:, -64:] = DC.uniform(72, 64, 80)                                        # and fine structure at the far end
    out = [job(wide, 4, 10 ** 11, 9, F.DETECT_MAX_KEYPOINTS), job(DC.uniform(70, F.DETECT_MAX_DIM, 5), 4, 1, 9, F.DETECT_MAX_KEYPOINTS),
           job(DC.uniform(71, 5, F.DETECT_MAX_DIM), 4, 1, 9, F.DETECT_MAX_KEYPOINTS)]
    st = state(out[0])
    assert st["n_layers"] == 5 and st["pyramid"][-1].shape == (5, 512) and st["flags"] in (0, SS.FULL) and st["kp"][:, 0].max() > 8180
    assert len(set(st["layer"])) >= 4 and st["n_layer_candidates"].min() > 0
    assert all(state(j)["n_layers"] == 1 and state(j)["n_candidates"] > 500 for j in out[1:])
    return out


def _waves():
    out = [job(waves(), o, 10 ** 9, 0, F.DETECT_MAX_KEYPOINTS) for o in range(5)]
    st = state(out[4])
    # rejections in both directions, selected keypoints on all five layers, d != 0 on more than 200
    assert sum(d["blocked_below"] for d in st["rejected"]) > 0 and sum(d["blocked_above"] for d in st["rejected"]) > 0
    assert set(int(l) for l in st["layer"]) == {0, 1, 2, 3, 4} and sum(1 for c in st["accepted"] if c["d"] != 0) > 200
    assert all(a > b > 0 for a, b in zip(st["n_layer_candidates"], st["n_layer_candidates"][1:]))
    assert [state(j)["n_layers"] for j in out] == [1, 2, 3, 4, 5]
    return out


def _ties():
    """a sharp rectangle on even coordinates: the scores tie across layers, and the finer layer wins"""
    im = np.full((128, 128), 110, np.uint8)
    im[32:96, 32:96] = 200
    out = [job(im, 4, 10 ** 9, 5, 64)]
    st = state(out[0])
    assert len(st["kp"]) == 4 and set(int(l) for l in st["layer"]) == {0} and st["n_layers"] == 5
    tied = [d for d in st["rejected"] if d["blocked_below"] and d["layer"] == 1 and d["S"] == SS.below(st["score"][0], d["x"], d["y"])]
    assert tied, "a layer-1 candidate whose score equals the largest below it"
    return out


def _edges():
    """odd w_l and h_l with a survivor on the last domain column and one on the last domain row of a layer that has a layer above
    it: all nine pixels above lie beyond the domain there, and that side counts as missing"""
    out, found = [], set()
    for seed in range(200):
        j = job(blurred(300 + seed, 47, 39, 1 + seed % 3), 4, 1, 0, 400)        # 47 x 39, 23 x 19, 11 x 9, 5 x 4 (does not exist)
        st = state(j)
        assert st["n_layers"] == 3
        here = set()
        for c in st["accepted"]:
            w, h = st["score"][c["layer"]].shape[1], st["score"][c["layer"]].shape[0]
            if c["missing_above"] and c["layer"] < 2:
                assert c["x"] == w - 3 or c["y"] == h - 3
                here.add((c["layer"], "x" if c["x"] == w - 3 else "y"))
        if here - found:
            out.append(j)
            found |= here
        if len(found) == 4:
            break
    assert found == {(0, "x"), (0, "y"), (1, "x"), (1, "y")}, found
    return out


COUNTS = (63, 64, 65, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def _counts_base():
    # a few grey levels of noise on the waves: the bands' symmetry alone leaves survivors with equal scores
    im = np.clip(waves(384, 192).astype(np.int64) + np.random.default_rng(5).integers(-3, 4, (192, 384)), 0, 255).astype(np.uint8)
    st = state(job(im, 4, 10 ** 9, 0, F.DETECT_MAX_KEYPOINTS))
    return im, st


def _counts():
    """threshold = the score of the k-th strongest survivor: survival does not depend on the threshold, so exactly k survive"""
    im, base = _counts_base()
    ranked = base["survivors"]
    assert len(ranked) > max(COUNTS) + 1
    out = []
    for k in COUNTS:
        assert ranked[k - 1]["S"] > ranked[k]["S"], "the k-th strongest survivor is alone with its score"
        out.append(job(im, 4, ranked[k - 1]["S"], 0, F.DETECT_MAX_KEYPOINTS))
        st = state(out[-1])
        assert st["n_candidates"] == k == len(st["kp"]) and st["flags"] == 0
    return out


def _capacity():
    """cand_capacity at the survivor count, at the largest layer's count, and one less of each; max_keypoints at what the rule can
    accept and one less.  The limit holds for every layer's list and for the pooled list, whichever is longer."""
    im, base = _counts_base()
    n, top = base["n_candidates"], int(base["n_layer_candidates"].max())
    assert 0 < n < top, "here a layer's list is the longest"
    out = [job(im, 4, 10 ** 9, 0, 2048, c) for c in (top, top - 1, n, n - 1, 1)]
    a, b = state(out[0]), state(out[1])
    assert a["flags"] in (0, SS.FULL) and a["n_candidates"] == n and len(a["kp"]) > 0
    assert all(s["flags"] == SS.OVERFLOW and s["n_candidates"] == 0 and len(s["kp"]) == 0 and int(s["n_layer_candidates"].max()) == top
               for s in (state(j) for j in out[1:]))
    # an image whose survivors are more than any layer's candidates: smooth blobs, too faint for the threshold on layer 0
    im2 = blurred(9, 200, 120, 8)
    thr = state(job(im2, 3, 1, 0, 2048))["survivors"][134]["S"]
    st = state(job(im2, 3, thr, 0, 2048))
    n2, top2 = st["n_candidates"], int(st["n_layer_candidates"].max())
    assert n2 > top2 > 0 and len(set(st["layer"])) == 3, "here the pooled list is the longest"
    out += [job(im2, 3, thr, 0, 2048, c) for c in (n2, n2 - 1, top2, top2 - 1)]
    d, e, f, g = (state(j) for j in out[-4:])
    assert d["flags"] == 0 and len(d["kp"]) == n2
    assert e["flags"] == f["flags"] == SS.OVERFLOW and e["n_candidates"] == f["n_candidates"] == n2 and len(e["kp"]) == len(f["kp"]) == 0
    assert g["flags"] == SS.OVERFLOW and g["n_candidates"] == 0
    # FULL: max_keypoints at what the rule can accept, and one less
    acc = len(state(job(im, 4, 10 ** 9, 12, 2048))["kp"])
    out += [job(im, 4, 10 ** 9, 12, acc), job(im, 4, 10 ** 9, 12, acc - 1)]
    f, g = state(out[-2]), state(out[-1])
    assert 10 < acc < n and f["flags"] == 0 and len(f["kp"]) == acc and g["flags"] == SS.FULL and len(g["kp"]) == acc - 1
    return out


def _across():
    """min_dist values at which a rejected survivor's only blocker lies on another layer"""
    out = []
    for md in range(1, 41):
        j = job(waves(), 4, 10 ** 9, md, F.DETECT_MAX_KEYPOINTS)
        st = state(j)
        if any(len(close) == 1 and close[0]["layer"] != c["layer"] for c, close in st["blockers"]):
            out.append(j)
        if len(out) == 3:
            break
    assert out, "no min_dist in 1..40 has a survivor blocked from another layer alone"
    return out


def _pitch():
    out = []
    for k, (w, h) in enumerate([(23, 21), (2 * TX + 1, 2 * TY + 1)]):
        img = blurred(700 + k, w, h, 2)
        for extra, offset in ((0, 0), (1, 0), (13, 0), (0, 1), (13, 1)):
            out.append(job(DC.with_pitch(img, extra, offset, k), 4, 1, 3, 100))
        want = state(out[-1])
        assert all(state(j)["kp"].tobytes() == want["kp"].tobytes() for j in out[-5:]) and len(want["kp"]) > 0 and want["n_layers"] > 1
    return out


def _mixed():
    rng = np.random.default_rng(78)
    out = []
    for j in range(130):
        w, h = int(rng.integers(5, 150)), int(rng.integers(5, 60))
        kind = j % 4
        if kind == 0:
            im = DC.uniform(1900 + j, w, h)
        elif kind == 1:
            im = blurred(1900 + j, w, h, int(rng.integers(2, 6)))
        elif kind == 2:
            im = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
            for _ in range(int(rng.integers(0, 12))):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                im[y0:y0 + int(rng.integers(1, 5)), x0:x0 + int(rng.integers(1, 5))] = int(rng.integers(0, 256))
        else:
            y, x = np.mgrid[0:h, 0:w]
            im = np.round(120 + 100 * np.sin(x / rng.uniform(1, 9)) * np.sin(y / rng.uniform(1, 9))).astype(np.uint8)
        im = DC.with_pitch(im, int(rng.integers(0, 3)) * 5, j % 2, j)
        out.append(job(im, j % 5, [1, 10 ** 9, 10 ** 12, 10 ** 14][j % 4 if j % 3 else 0], int(rng.integers(0, 21)), int(rng.integers(1, 51)),
                       [F.DETECT_MAX_CANDIDATES, 40, 5][j % 7 % 3], rng.uniform(1, 20)))
    st = [state(j) for j in out]
    assert {s["flags"] for s in st} == {0, SS.OVERFLOW, SS.FULL} and any(s["n_candidates"] == 0 and s["flags"] == 0 for s in st)
    assert {s["n_layers"] for s in st} == {1, 2, 3, 4} and {int(l) for s in st for l in s["layer"]} >= {0, 1}
    assert any(s["flags"] == SS.OVERFLOW and s["n_candidates"] > 0 for s in st) and any(s["flags"] == SS.OVERFLOW and s["n_candidates"] == 0 for s in st)
    return out


BUILDERS = {"shapes": _shapes, "long": _long, "waves": _waves, "ties": _ties, "edges": _edges, "counts": _counts, "capacity": _capacity,
            "across": _across, "pitch": _pitch, "mixed": _mixed}
assert tuple(BUILDERS) == NAMES


@functools.lru_cache(maxsize=None)
def cases(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def stated(name):
    return [state(j) for j in cases(name)]


def as_scaled(j, octaves=0):
    """a detect_cases job for the new entry"""
    return dict(j, octaves=octaves)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def check(got, want, where, with_referee=True):
    """everything by bytes: nothing has a tolerance"""
    for k in ("n_candidates", "flags", "n_layers"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert np.array_equal(got["n_layer_candidates"], want["n_layer_candidates"]), (where, got["n_layer_candidates"], want["n_layer_candidates"])
    names = (("pixel", np.int32), ("layer", np.int32), ("response", np.float64), ("kp", np.float32)) + ((("scale", np.float64),) if with_referee else ())
    for k, dtype in names:
        assert got[k].dtype == dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (where, k)
    if with_referee:
        for k, dtype in (("score", np.int64), ("pyramid", np.uint8)):
            assert len(got[k]) == len(want[k]), (where, k)
            for l, (a, b) in enumerate(zip(got[k], want[k])):
                assert a.dtype == dtype and a.shape == b.shape and np.array_equal(a, b), (where, k, l)


# ---- the host probe -------------------------------------------------------------------------------------------------------------
def build_probe(out_dir, sanitize=True, opt="-O1"):
    """tests/detect_scale_probe.cpp with the sanitizers' runtimes linked statically (the CPU tests), or plain (the benchmark's yardstick)"""
    exe = os.path.join(str(out_dir), "detect_scale_probe")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", opt, *flags, "-ffp-contract=off", os.path.join(HERE, "detect_scale_probe.cpp"), "-o", exe], check=True)
    return exe


def write_probe_input(path, jobs):
    with open(path, "wb") as f:
        np.array([len(jobs)], np.int32).tofile(f)
        for j in jobs:
            im = j["image"]
            h, w = im.shape
            pitch = im.strides[0]
            np.array([w, h, pitch, j["min_dist"], j["max_keypoints"], j["cand_capacity"], j["octaves"]], np.int32).tofile(f)
            np.array([j["kp_size"]], np.float32).tofile(f)
            np.array([j["threshold"]], np.int64).tofile(f)
            block = np.full((h, pitch), 0x3C, np.uint8)          # what lies between the rows is not the image's
            block[:, :w] = im
            block.reshape(-1)[:(h - 1) * pitch + w].tofile(f)


def run_probe(exe, out_dir, jobs, tag="p", timed=False):
    """-> per job the dict the statement gives (without the builders' extras); with timed, also the seconds inside the driver"""
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    write_probe_input(src, jobs)
    done = subprocess.run([exe, src, dst] + (["--time"] if timed else []), check=True, capture_output=True, text=True)
    raw, at, res = open(dst, "rb").read(), 0, []
    rec = np.dtype([("s", np.int64), ("x", np.int32), ("y", np.int32), ("fx", np.float32), ("fy", np.float32)])
    ext = np.dtype([("scale", np.float64), ("size", np.float32), ("layer", np.int32)])
    for j in jobs:
        h, w = j["image"].shape
        head = np.frombuffer(raw, np.int32, 10, at)
        n, n_cand, flags, n_layers, counts = int(head[0]), int(head[1]), int(head[2]), int(head[4]), head[5:10].copy()
        at += 40
        sel = np.frombuffer(raw, rec, n, at)
        at += 24 * n
        sx = np.frombuffer(raw, ext, n, at)
        at += 16 * n
        layers = F.detect_layers(w, h, j["octaves"])
        assert len(layers) == n_layers
        score, pyr = [], []
        for lw, lh in layers:
            score.append(np.frombuffer(raw, np.int64, lw * lh, at).reshape(lh, lw))
            at += 8 * lw * lh
        for lw, lh in layers[1:]:
            pyr.append(np.frombuffer(raw, np.uint8, lw * lh, at).reshape(lh, lw))
            at += lw * lh
        res.append({"kp": np.stack([sel["fx"], sel["fy"], sx["size"]], axis=1).astype(np.float32).reshape(-1, 3), "response": sel["s"].astype(np.float64),
                    "pixel": np.stack([sel["x"], sel["y"]], axis=1).astype(np.int32).reshape(-1, 2), "layer": sx["layer"].astype(np.int32),
                    "scale": sx["scale"].astype(np.float64), "n_candidates": n_cand, "flags": flags, "n_layers": n_layers,
                    "n_layer_candidates": counts.astype(np.int32), "score": score, "pyramid": pyr})
    assert at == len(raw)
    return (res, float(done.stdout.split()[-1])) if timed else res
