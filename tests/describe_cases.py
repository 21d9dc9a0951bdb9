"""Seeded cases of okvis_fe_describe_keypoints and okvis_fe_detect_and_describe, shared by tests/test_describe_host.py and
tests/test_gpu_describe.py.  Every family is built once per process (cases) and stated once (stated: tests/describe_statement.py);
where a case is there to show a property, the builder asserts that the statement really shows it.

A case with given rotations is a dict: image (2-D uint8, possibly a view with a pitch), kp [n][3] float32, rot [n] int32.
An angle case is a dict: cam (tri_statement.camera), kp, direction; its image is ANGLE_IMAGE (the angle does not read it).

The bound on angle64, per keypoint: |angle64 - statement| <= 4 max(e64, e_in) degrees, with e64 the distance of the float64 numpy
evaluation from the long double statement and e_in the largest distance between the statement and itself with every input (kp,
intrinsics, direction) moved by one rounding in the direction that hurts most: the sum, over the inputs, of the distance the
statement moves when that input alone is scaled by 1 + 2^-53 (first order, the worst case over the 2^k sign patterns; a handful of
random patterns, as the solvers' cases draw them, finds less than that)."""
import functools
import os
import subprocess

import numpy as np

import describe_statement as S
import tri_statement as T
from detect_cases import uniform, with_pitch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("edge", "rot", "phase", "values", "pitch", "mixed")
HI = lambda size: 16 * (size - 1) - S.MARGIN          # the largest valid q along a side of `size` pixels
BOUND_FACTOR = 4.0
V_MAX = 255 * 3600


def job(image, kp, rot):
    kp = np.asarray(kp, np.float64).reshape(-1, 2 if np.ndim(kp) == 2 and np.shape(kp)[1] == 2 else 3)
    if kp.shape[1] == 2:
        kp = np.concatenate([kp, np.full((len(kp), 1), 12.0)], axis=1)
    return {"image": image, "kp": np.ascontiguousarray(kp, np.float32), "rot": np.ascontiguousarray(np.broadcast_to(rot, len(kp)), np.int32)}


def state(j):
    desc, flags, V = S.describe(np.ascontiguousarray(j["image"]), j["kp"], j["rot"])
    return {"desc": desc, "flags": flags, "rot": j["rot"].copy(), "n_valid": int((flags & S.VALID).sum()), "V": V}


def q_to_kp(q):
    """a coordinate whose q is exactly this: q / 16 is exact in float for q < 2^20"""
    return np.asarray(q, np.float64) / 16.0


def textured(seed, w, h):
    """smooth structure plus noise: neighbouring boxes differ, few exact ties"""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    im = 120 + 60 * np.sin(x / 3.1 + rng.uniform(0, 6)) * np.cos(y / 4.3 + rng.uniform(0, 6)) + 40 * np.sin((x + 2 * y) / 7.0) + rng.integers(-20, 21, (h, w))
    return np.clip(np.round(im), 0, 255).astype(np.uint8)


# ---- the families ---------------------------------------------------------------------------------------------------------------
def _edge():
    out = [job(uniform(1, 23, 23), [[11.0, 11.0]], 5)]                       # 23 x 23: the one valid position
    st = state(out[0])
    assert HI(23) == S.MARGIN and st["n_valid"] == 1 and st["desc"].any()
    for (w, h) in ((23, 23), (23, 40), (40, 23), (37, 41)):
        qs_x, qs_y = [S.MARGIN - 1, S.MARGIN, HI(w), HI(w) + 1], [S.MARGIN - 1, S.MARGIN, HI(h), HI(h) + 1]
        pts = [(qx, qy) for qx in qs_x for qy in qs_y]                       # all four sides and corners, one step in and one out
        kp = q_to_kp(pts)
        out.append(job(textured(10 + w + h, w, h), kp, (np.arange(len(kp)) * 67) % S.N_ROT))
        st = state(out[-1])
        want = np.array([S.MARGIN <= qx <= HI(w) and S.MARGIN <= qy <= HI(h) for qx, qy in pts])
        assert np.array_equal(st["flags"] == S.VALID, want) and want.sum() == 4 and not st["desc"][~want].any()
    # kp * 16 + 0.5 an integer: q = that integer (floor leaves it), from both sides of the margin; and just below
    w, h = 40, 30
    halves = np.array([S.MARGIN - 0.5, S.MARGIN + 0.5, HI(w) - 0.5, HI(w) + 0.5]) / 16.0
    below = np.nextafter(halves.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    kp = [[x, 14.0] for x in np.concatenate([halves, below])]
    out.append(job(textured(3, w, h), kp, 300))
    qx, _, valid = S.position(out[-1]["kp"], w, h)
    assert valid.tolist() == [True, True, True, False, False, True, True, True] and qx[:3].tolist() == [S.MARGIN, S.MARGIN + 1, HI(w)]
    bad = [[-3.0, 14.0], [14.0, -1e30], [np.nan, 14.0], [14.0, np.nan], [np.inf, 14.0], [14.0, -np.inf], [1e30, 1e30], [-0.03125, 14.0], [14.0, 14.0]]
    out.append(job(textured(4, w, h), bad, 77))
    st = state(out[-1])
    assert st["flags"].tolist() == [0] * 8 + [S.VALID]
    out.append(job(textured(5, w, h), np.zeros((0, 3)), 0))                  # n = 0
    return out


def _rot():
    out = [job(textured(20, 64, 64), [[31.3125, 32.6875]] * S.N_ROT, np.arange(S.N_ROT))]
    st = state(out[0])
    d = st["desc"]
    step = np.unpackbits(d ^ np.roll(d, -1, axis=0), axis=1).sum(axis=1)
    assert st["n_valid"] == S.N_ROT and step.max() < 40 and len({r.tobytes() for r in d}) > 512      # neighbouring indices are close, the turn is not idle
    return out


def _phase():
    kp = [[30 + i / 16.0, 29 + j / 16.0] for j in range(16) for i in range(16)]
    out = [job(textured(21, 64, 60), kp, (np.arange(256) * 4 + 1) % S.N_ROT)]
    qx, qy, valid = S.position(out[0]["kp"], 64, 60)
    assert valid.all() and len({(int(a) % 16, int(b) % 16) for a, b in zip(qx, qy)}) == 256
    return out


def _values():
    w, h = 48, 44
    y, x = np.mgrid[0:h, 0:w]
    kp = [[15.0 + 0.4375 * i, 14.5 + 0.3125 * (i % 7)] for i in range(40)]
    rot = (np.arange(40) * 101) % S.N_ROT
    constant = job(np.full((h, w), 93, np.uint8), kp, rot)
    st = state(constant)
    assert st["n_valid"] == 40 and not st["desc"].any()                       # equal means: no bit, VALID all the same
    white = job(np.full((h, w), 255, np.uint8), kp, rot)
    assert state(white)["V"].max() == V_MAX and not state(white)["desc"].any()
    checker = job((((x // 8 + y // 8) & 1) * 255).astype(np.uint8), kp, rot)
    st = state(checker)
    assert st["V"].max() == V_MAX and st["V"].min() == 0 and st["desc"].any()  # the largest V against the smallest: the largest cross products
    fine = job((((x + y) & 1) * 255).astype(np.uint8), kp, rot)
    assert state(fine)["desc"].any()
    return [constant, white, checker, fine]


def _pitch():
    out = []
    img = textured(30, 41, 37)
    kp = [[12.0 + 1.3 * i, 11.5 + 0.9 * i] for i in range(12)]
    rot = (np.arange(12) * 89) % S.N_ROT
    for extra, offset in ((0, 0), (1, 0), (13, 0), (0, 1), (13, 1), (7, 3), (2, 2)):
        out.append(job(with_pitch(img, extra, offset, extra), kp, rot))
    want = state(out[0])
    assert want["n_valid"] == 12 and all(state(j)["desc"].tobytes() == want["desc"].tobytes() for j in out)
    assert {j["image"].ctypes.data % 4 for j in out} >= {1, 2, 3} and {j["image"].strides[0] % 2 for j in out} == {0, 1}
    return out


def _mixed():
    rng = np.random.default_rng(78)
    out = []
    for j in range(130):
        w, h = int(rng.integers(23, 90)), int(rng.integers(23, 70))
        im = [uniform(800 + j, w, h), textured(800 + j, w, h), (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)][j % 3]
        im = with_pitch(im, int(rng.integers(0, 3)) * 5, j % 2, j)
        n = int(rng.integers(0, 13)) if j % 10 else 0
        kp = np.stack([rng.uniform(8, w - 8, n), rng.uniform(8, h - 8, n)], axis=1).reshape(-1, 2)
        out.append(job(im, kp, rng.integers(0, S.N_ROT, n)))
    st = [state(j) for j in out]
    assert sum(s["n_valid"] for s in st) > 200 and sum(len(s["flags"]) - s["n_valid"] for s in st) > 100 and sum(len(j["kp"]) == 0 for j in out) >= 13
    return out


BUILDERS = {"edge": _edge, "rot": _rot, "phase": _phase, "values": _values, "pitch": _pitch, "mixed": _mixed}
assert tuple(BUILDERS) == NAMES


@functools.lru_cache(maxsize=None)
def cases(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def stated(name):
    return [state(j) for j in cases(name)]


def check(got, want, where):
    """everything by bytes: nothing has a tolerance"""
    assert got["n_valid"] == want["n_valid"], (where, got["n_valid"], want["n_valid"])
    for k, dtype in (("desc", np.uint8), ("flags", np.uint8), ("rot", np.int32)):
        if k in got:
            assert got[k].dtype == dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (where, k)


# ---- shifts and turns -----------------------------------------------------------------------------------------------------------
SHIFTS = [(0, 0), (1, 0), (0, 1), (5, 3), (16, 9)]


@functools.lru_cache(maxsize=None)
def shifted(dx, dy, w=80, h=70):
    """a textured 40 x 36 block in a textured frame moved by whole pixels, and the keypoints with it"""
    big = textured(40, w + 32, h + 32)
    im = np.ascontiguousarray(big[16 - dy:16 - dy + h, 16 - dx:16 - dx + w])
    rng = np.random.default_rng(41)
    kp = np.stack([rng.integers(13 * 16, 40 * 16, 30) / 16.0 + dx, rng.integers(13 * 16, 36 * 16, 30) / 16.0 + dy], axis=1)
    return job(im, kp, rng.integers(0, S.N_ROT, 30))


@functools.lru_cache(maxsize=None)
def quarter_turn(seed=50, w=61, h=47, n=40):
    """-> (job on I, job on rot90(I, -1)): the keypoint (qx, qy) at rot goes to (16 (h - 1) - qy, qx) at rot + 256"""
    im = textured(seed, w, h)
    rng = np.random.default_rng(seed)
    qx, qy = rng.integers(S.MARGIN, HI(w) + 1, n), rng.integers(S.MARGIN, HI(h) + 1, n)
    rot = rng.integers(0, S.N_ROT, n)
    a = job(im, np.stack([q_to_kp(qx), q_to_kp(qy)], axis=1), rot)
    b = job(np.ascontiguousarray(np.rot90(im, -1)), np.stack([q_to_kp(16 * (h - 1) - qy), q_to_kp(qx)], axis=1), (rot + 256) % S.N_ROT)
    return a, b


# ---- the scene ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(n=400, w=752, h=480):
    """one stereo pair of the reference's image size with n keypoints each, some of them in the margin"""
    out = []
    for cam in range(2):
        rng = np.random.default_rng(60 + cam)
        kp = np.stack([rng.uniform(5, w - 5, n), rng.uniform(5, h - 5, n)], axis=1)
        out.append(job(textured(60 + cam, w, h), kp, rng.integers(0, S.N_ROT, n)))
    return out


# ---- the angle stage ------------------------------------------------------------------------------------------------------------
CAMERAS = {
    "none": T.camera([458.6, 457.3, 367.2, 248.4], T.DIST_NONE),
    "radtan": T.camera([458.6, 457.3, 367.2, 248.4, -0.2834, 0.0739, 0.00019, 1.76e-05], 1),
    "equi": T.camera([461.6, 460.3, 362.7, 248.1, -0.0027, 0.0241, -0.0430, 0.0311], T.DIST_EQUI),
    "radtan8": T.camera([458.6, 457.3, 367.2, 248.4, -0.2834, 0.0739, 0.00019, 1.76e-05, 0.01, 0.02, -0.01, 0.005], T.DIST_RADTAN8),
}
ANGLE_IMAGE_SHAPE = (480, 752)
FLOAT_SLACK = 360.0 * 2.0 ** -23          # two float ulps at 180 degrees


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _angle_cases():
    out = []
    for m, (name, cam) in enumerate(CAMERAS.items()):
        rng = np.random.default_rng(90 + m)
        kp = np.stack([rng.uniform(12, 740, 200), rng.uniform(12, 468, 200), np.full(200, 12.0)], axis=1).astype(np.float32)
        far = kp.copy()
        far[:3, :2] = [[30000.0, 20000.0], [-9000.0, 14000.0], [5000.0, -7000.0]]      # where backProject's iteration has nothing to converge to
        axis_near = _unit([7e-7 * np.cos(m), 7e-7 * np.sin(m), -1.0])                  # gravity within 1e-6 rad of the optical axis
        ray = np.asarray(T.back_project(T.Ctx(), cam, kp[:1], "c_", np.ones(1, bool))[0][0], np.float64)
        for tag, d, k in (("generic", _unit([0.12, 0.95, 0.28]), kp), ("sideways", _unit([-0.9, 0.1, 0.42]), kp), ("axis", axis_near, kp),
                          ("along_ray", ray, kp), ("far", _unit([0.12, 0.95, 0.28]), far)):
            out.append({"name": f"{name}/{tag}", "cam": cam, "kp": k, "direction": np.asarray(d, np.float64)})
    return out


@functools.lru_cache(maxsize=None)
def angle_cases():
    return _angle_cases()


def _state_angle(c):
    a_ld, defined = S.angle(c["cam"], c["kp"], c["direction"], T.LD)
    a_np, defined_np = S.angle(c["cam"], c["kp"], c["direction"], np.float64)
    with np.errstate(invalid="ignore"):
        e64 = np.abs(np.asarray(T.LD(a_np) - a_ld, np.float64))
    # one rounding of every input, in the direction that hurts: the moves of the angle under each input alone (x of every keypoint
    # at once, y likewise, each intrinsic, each component of the direction) moved by 2^-53 of itself, summed
    e_in = np.zeros(len(a_ld))
    kp64, intr, direction = c["kp"].astype(np.float64), np.asarray(c["cam"]["intr"], np.float64), np.asarray(c["direction"], np.float64)
    up = T.LD(1) + T.LD(2) ** -53          # not a double: 1 + 2^-53 rounds to 1 there

    def moved(kp=kp64, intr=intr, direction=direction):
        a, _d = S.angle(dict(c["cam"], intr=intr), T.LD(kp), T.LD(direction), T.LD)
        with np.errstate(invalid="ignore"):
            return np.abs(np.asarray(a - a_ld, np.float64))

    def scaled(a, index):
        a = T.LD(a).copy()
        a[index] = a[index] * up
        return a

    for col in (0, 1):
        e_in += moved(kp=scaled(kp64, (slice(None), col)))
    for i in np.flatnonzero(intr):
        e_in += moved(intr=scaled(intr, i))
    for i in np.flatnonzero(direction):
        e_in += moved(direction=scaled(direction, i))
    bound = BOUND_FACTOR * np.maximum(e64, e_in)
    stated_rot = S.rot_of_angle(np.asarray(a_ld, np.float64).astype(np.float32))
    near = S.bin_distance(np.asarray(a_ld, np.float64)) <= FLOAT_SLACK + bound        # left out of the comparison of rot alone
    return {"angle": a_ld, "defined": defined & defined_np, "angle_np": a_np, "e64": e64, "e_in": e_in, "bound": bound, "rot": stated_rot,
            "near_boundary": near}


@functools.lru_cache(maxsize=None)
def stated_angles():
    return [_state_angle(c) for c in angle_cases()]


# ---- the host probe -------------------------------------------------------------------------------------------------------------
def build_probe(out_dir, sanitize=True, opt="-O1"):
    """tests/describe_probe.cpp with the sanitizers' runtimes linked statically (the CPU tests), or plain (the benchmark's yardstick)"""
    exe = os.path.join(str(out_dir), "describe_probe")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", opt, *flags, "-ffp-contract=off", os.path.join(HERE, "describe_probe.cpp"), "-o", exe], check=True)
    return exe


def write_probe_input(path, jobs):
    with open(path, "wb") as f:
        np.array([len(jobs)], np.int32).tofile(f)
        for j in jobs:
            im = j["image"]
            h, w = im.shape
            pitch = im.strides[0]
            np.array([w, h, pitch, len(j["kp"])], np.int32).tofile(f)
            block = np.full((h, pitch), 0x3C, np.uint8)          # what lies between the rows is not the image's
            block[:, :w] = im
            block.reshape(-1)[:(h - 1) * pitch + w].tofile(f)
            j["kp"].tofile(f)
            j["rot"].tofile(f)


def run_probe(exe, out_dir, jobs, tag="p", timed=False):
    """-> per job the dict the statement gives (desc, flags, n_valid); with timed, also the seconds inside describe_image_serial"""
    src, dst = os.path.join(str(out_dir), tag + ".in"), os.path.join(str(out_dir), tag + ".out")
    write_probe_input(src, jobs)
    done = subprocess.run([exe, src, dst] + (["--time"] if timed else []), check=True, capture_output=True, text=True)
    raw, at, res = open(dst, "rb").read(), 0, []
    for j in jobs:
        n = len(j["kp"])
        n_valid = int(np.frombuffer(raw, np.int32, 1, at)[0])
        desc = np.frombuffer(raw, np.uint8, 48 * n, at + 4).reshape(n, 48)
        flags = np.frombuffer(raw, np.uint8, n, at + 4 + 48 * n)
        at += 4 + 49 * n
        res.append({"desc": desc, "flags": flags, "n_valid": n_valid})
    assert at == len(raw)
    return (res, float(done.stdout)) if timed else res


def run_angle_probe(exe, out_dir, y, x):
    """dsc_angle_degrees of the header on the pairs (y, x) -> degrees [n] float64"""
    src, dst = os.path.join(str(out_dir), "angle.in"), os.path.join(str(out_dir), "angle.out")
    with open(src, "wb") as f:
        np.array([len(y)], np.int32).tofile(f)
        np.stack([y, x], axis=1).astype(np.float64).tofile(f)
    subprocess.run([exe, "--angle", src, dst], check=True)
    return np.fromfile(dst, np.float64)

