"""An independent statement of okvis_fe_describe_keypoints (include/okvis_amd_frontend.h): the gravity-aligned binary descriptor,
in numpy int64, and its angle stage in numpy's long double.  TEST INFRASTRUCTURE ONLY: imports nothing from the product and does
not read okvis_amd/csrc/fe_describe_tables.inc; the tables are built here from a 60-digit mpmath evaluation.

  tables()        cs [1024][2], base [60][2], ring [60], half [5], pairs [383][2]
  position        qx = floor((double)kp.x * 16 + 0.5), VALID iff finite and 176 <= qx <= 16 (w - 1) - 176 (the same in y)
  centres         (qx, qy) + R(rotated Q16 offsets), R = Q46 -> Q4, half away from zero
  samples         V_k = sum I[y][x] wy(y) wx(x), the area-weighted box of side 2 h around the centre, in sixteenths of a pixel
  describe        bit b = V_i A_k > V_k A_i for pair b = (i, k), byte b >> 3, bit b & 7; an invalid keypoint has a zero row, flag 0
  angle           Frame::describe (okvis_cv/include/okvis/implementation/Frame.hpp:139-150) with the long double backProject /
                  project of tests/tri_statement.py: any dtype through tri_statement.Ctx
  rot_of_angle    ((int)floor((double)angle * 1024 / 360 + 0.5)) mod 1024 of the float angle"""
import functools

import mpmath as mp
import numpy as np

import tri_statement as T

VALID, ANGLE_UNDEFINED = 1, 2
N_RING = (1, 10, 14, 15, 20)
RADII = ("0", "2.9", "4.9", "7.4", "10.8")
HALF = (10, 16, 19, 27, 30)
MARGIN = 176
N_POINTS, N_PAIRS, N_ROT, DESC_BYTES = 60, 383, 1024, 48


def _round(z):
    """to nearest, half away from zero"""
    return int(mp.sign(z)) * int(mp.floor(abs(z) + mp.mpf(1) / 2))


@functools.lru_cache(maxsize=None)
def tables():
    with mp.workdps(60):
        pts, ring = [], []
        for m, n in enumerate(N_RING):
            r = mp.mpf("0.85") * mp.mpf(RADII[m])
            for a in range(n):
                t = 2 * mp.pi * a / n
                pts.append((r * mp.cos(t), r * mp.sin(t)))
                ring.append(m)
        base = np.array([[_round(65536 * x), _round(65536 * y)] for x, y in pts], np.int64)
        cs = np.array([[_round(2 ** 30 * mp.cos(2 * mp.pi * j / N_ROT)), _round(2 ** 30 * mp.sin(2 * mp.pi * j / N_ROT))] for j in range(N_ROT)],
                      np.int64)
        dist = lambda i, k: mp.sqrt((pts[i][0] - pts[k][0]) ** 2 + (pts[i][1] - pts[k][1]) ** 2)
        pairs = np.array([(i, k) for i in range(N_POINTS) for k in range(i + 1, N_POINTS) if dist(i, k) < mp.mpf("5.1")], np.int64)
        # the box half widths are the stated integers; they are 1.3 r_m sin(pi / N_m) in sixteenths, 0.65 px for the centre
        want_half = [_round(16 * mp.mpf("0.65"))] + [_round(16 * mp.mpf("1.3") * mp.mpf("0.85") * mp.mpf(RADII[m]) * mp.sin(mp.pi / N_RING[m]))
                                                     for m in range(1, 5)]
        assert tuple(want_half) == HALF
    return {"cs": cs, "base": base, "ring": np.array(ring, np.int64), "half": np.array(HALF, np.int64), "pairs": pairs}


def reduce_q46(z):
    """R(z) = sign(z) ((|z| + 2^41) >> 42) on int64 arrays"""
    return np.sign(z) * ((np.abs(z) + (1 << 41)) >> 42)


def offsets(rot):
    """rot [n] -> dx, dy [n][60] in sixteenths of a pixel"""
    t = tables()
    c, s = t["cs"][rot, 0][:, None], t["cs"][rot, 1][:, None]
    bx, by = t["base"][:, 0][None, :], t["base"][:, 1][None, :]
    return reduce_q46(c * bx - s * by), reduce_q46(s * bx + c * by)


def position(kp, w, h):
    """kp [n][>=2] float32 -> qx, qy [n] int64 (0 where not finite), valid [n]"""
    xy = np.asarray(kp, np.float32).reshape(len(kp), -1)[:, :2].astype(np.float64)
    fin = np.isfinite(xy).all(axis=1)
    with np.errstate(all="ignore"):
        q = np.floor(np.where(fin[:, None], xy, 0.0) * 16.0 + 0.5)
    inside = (q[:, 0] >= MARGIN) & (q[:, 0] <= 16 * (w - 1) - MARGIN) & (q[:, 1] >= MARGIN) & (q[:, 1] <= 16 * (h - 1) - MARGIN)
    valid = fin & inside
    q = np.where(valid[:, None], q, 0.0).astype(np.int64)
    return q[:, 0], q[:, 1], valid


def _weights(c, hw, limit):
    """the five pixels from the one that holds c - hw, and the length each shares with [c - hw, c + hw) -> index [5][n], weight [5][n]"""
    first = (c - hw + 8) >> 4
    idx = first[None, :] + np.arange(5)[:, None]
    wt = np.maximum(0, np.minimum(16 * idx + 8, (c + hw)[None, :]) - np.maximum(16 * idx - 8, (c - hw)[None, :]))
    assert (wt.sum(axis=0) == 2 * hw).all() and (wt[(idx < 0) | (idx > limit)] == 0).all()      # no box leaves the image
    return np.clip(idx, 0, limit), wt


def samples(image, qx, qy, rot):
    """-> V [n][60] int64 for valid positions"""
    t = tables()
    im = np.asarray(image).astype(np.int64)
    h, w = im.shape
    dx, dy = offsets(np.asarray(rot, np.int64))
    V = np.zeros((len(qx), N_POINTS), np.int64)
    for k in range(N_POINTS):
        hw = np.full(len(qx), t["half"][t["ring"][k]], np.int64)
        ix, wx = _weights(qx + dx[:, k], hw, w - 1)
        iy, wy = _weights(qy + dy[:, k], hw, h - 1)
        for j in range(5):
            for i in range(5):
                V[:, k] += im[iy[j], ix[i]] * wy[j] * wx[i]
    return V


def describe(image, kp, rot):
    """-> desc [n][48] uint8, flags [n] uint8 (VALID or 0), V [n][60] (zero rows where invalid)"""
    t = tables()
    h, w = np.asarray(image).shape
    n = len(kp)
    desc, flags, V = np.zeros((n, DESC_BYTES), np.uint8), np.zeros(n, np.uint8), np.zeros((n, N_POINTS), np.int64)
    if n == 0:
        return desc, flags, V
    rot = np.asarray(rot, np.int64).reshape(n)
    assert ((rot >= 0) & (rot < N_ROT)).all()
    qx, qy, valid = position(kp, w, h)
    if valid.any():
        V[valid] = samples(image, qx[valid], qy[valid], rot[valid])
        A = (2 * t["half"][t["ring"]]) ** 2
        i, k = t["pairs"][:, 0], t["pairs"][:, 1]
        bits = np.zeros((n, 8 * DESC_BYTES), np.uint8)
        bits[:, :N_PAIRS] = V[:, i] * A[k][None, :] > V[:, k] * A[i][None, :]
        desc[valid] = np.packbits(bits, axis=1, bitorder="little")[valid]
        flags[valid] = VALID
    return desc, flags, V


# ---- the angle stage ------------------------------------------------------------------------------------------------------------
def angle(cam, kp, direction, dtype=T.LD, order=0):
    """Frame.hpp:139-150 per keypoint -> angle in degrees [n] (dtype), defined [n]: backProject succeeded, the projection's
    distortion is defined and eg is finite"""
    cx = T.Ctx(dtype, order=order)
    kp = np.asarray(kp).reshape(-1, 3)          # float32 as the entry takes them; the sensitivity draws pass perturbed doubles
    n = len(kp)
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        ep, ok = T.back_project(cx, cam, kp, "d_", active)
        status, uv, J = T.project(cx, cam, ep, np.ones(n), "d_", active, want_jacobian=True)
        d = cx.c(direction)
        eg0 = cx.sum([J[:, 0, c] * d[c] for c in range(3)])
        eg1 = cx.sum([J[:, 1, c] * d[c] for c in range(3)])
        a = np.arctan2(eg1, eg0) / cx.c(np.float64(np.pi)) * cx.c(180)     # M_PI is the double nearest to pi: the reference divides by it
    defined = ok & np.isfinite(np.asarray(eg0, np.float64)) & np.isfinite(np.asarray(eg1, np.float64)) & _distortion_defined(cam, ep)
    return a, defined


def _distortion_defined(cam, ep):
    if cam["model"] != T.DIST_RADTAN8:
        return np.ones(len(ep), bool)
    x, y = np.asarray(ep[:, 0], np.float64), np.asarray(ep[:, 1], np.float64)
    with np.errstate(all="ignore"):
        return ~(x * x + y * y > 9.0)


def rot_of_angle(a32):
    """the float angle -> 0..1023"""
    a = np.asarray(a32, np.float32).astype(np.float64)
    a = np.where(np.isfinite(a), a, 0.0)          # an undefined angle has no index: the callers leave those keypoints out
    return (np.floor(a * 1024.0 / 360.0 + 0.5).astype(np.int64)) % N_ROT


def bin_distance(a):
    """degrees between an angle and the nearest boundary between two rotation indices"""
    t = np.asarray(a, np.float64) * 1024.0 / 360.0 + 0.5
    return np.abs(t - np.round(t)) * 360.0 / 1024.0
