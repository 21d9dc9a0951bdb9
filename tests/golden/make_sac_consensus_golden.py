"""Records tests/golden/sac_consensus.npz from the reference's own RANSAC adapters and sample-consensus problems.  Not run by any test.

    OKVIS_REFERENCE=<reference tree> python tests/golden/make_sac_consensus_golden.py [work directory]

needs the reference tree and oracle/_ref/obj (the reference's estimator, built by oracle/ref/Makefile).  Compiles
sac_consensus_recorder.cpp with the reference's okvis_frontend/src/{FrameNoncentralAbsoluteAdapter,FrameRelativeAdapter}.cpp, with the
flags and stand-in headers oracle/ref/Makefile uses plus oracle/shim/callers, links the reference objects, and runs every case:
a scene of two multi-frames with two cameras (different T_SC, rotation included), keypoints of varying size, landmarks, and 50
hypotheses per problem from the true pose to far off.  Stored: the keypoints, what the adapters hold, every score the reference
returns, and countWithinDistance / selectWithinDistance.

The relative-pose problem calls opengv::triangulation::triangulate2, which is OpenGV's and not in the reference tree; the recorder
defines it (two-view midpoint method).  Those scores pin everything except that function: c{i}_rel_pinned = 0.

Asserted here and again by tests/test_sac_consensus_host.py: each kind has a case where two hypotheses tie for the largest count, a
hypothesis without inliers and one with all; no recorded score lies within the comparison band of the threshold.  Prints how far
the reference's double scores lie from the long double statement (tests/sac_statement.py): the figure the tolerances come from."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sac_statement as S  # noqa: E402

THRESHOLD = 9.0
K = 50
BAND_FACTOR = 10.0   # the comparison band of a kind = this times the largest distance measured for the kind (the tests' tolerance)
# product model (OKVIS_BA_DIST_*) -> NCameraSystem::DistortionType
REF_TYPE = {S.DIST_RADTAN: 1, S.DIST_EQUI: 0, S.DIST_RADTAN8: 3}
INTR = {S.DIST_RADTAN: [458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05],
        S.DIST_EQUI: [350.0, 360.0, 378.0, 238.0, -0.021, 0.014, 0.0006, 0.0003],
        S.DIST_RADTAN8: [420.0, 418.0, 370.0, 243.0, -0.25, 0.06, 0.0002, -0.0001, 0.004, 0.03, -0.01, 0.002]}
# model, landmarks, pixel noise, fraction of wrong associations, translation between the frames [m], seed
CASES = [(S.DIST_RADTAN, 60, 0.15, 0.0, 0.35, 1),
         (S.DIST_EQUI, 60, 0.4, 0.2, 0.35, 2),
         (S.DIST_RADTAN8, 60, 0.4, 0.15, 0.5, 3),
         (S.DIST_RADTAN, 125, 0.5, 0.25, 0.25, 4),
         (S.DIST_EQUI, 60, 0.1, 0.0, 0.004, 5)]      # next to no translation: the rotation-only problem explains everything


def rot(axis, angle):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def quat_xyzw(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def rot_of_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def project(intr, model, p_C):
    x, y = p_C[:, 0] / p_C[:, 2], p_C[:, 1] / p_C[:, 2]
    xd, yd, _ = S._distort(model, np.asarray(intr[4:], float), x, y)
    return np.stack([intr[0] * xd + intr[2], intr[1] * yd + intr[3]], axis=1)


def perturbed(rng, R, t, magnitude):
    return rot(rng.normal(size=3), magnitude * rng.uniform(0.5, 1.0)) @ R, t + magnitude * rng.uniform(0.5, 1.0) * rng.normal(size=3) / np.sqrt(3)


def hypotheses(rng, R, t, with_translation):
    """K hypotheses around (R, t): the exact one twice (a tie for the largest count, neither of them first), perturbations from 1e-9
    to 1 in rotation [rad] and translation [m], and two that are far off"""
    mags = 10.0 ** rng.uniform(-9, 0, K - 4)
    models = [perturbed(rng, R, t, m) for m in mags]
    models += [(R, t), (R, t), (rot([1, 0, 0], np.pi) @ R, t + 5.0), (rot([0.3, 1, 0.2], 2.0) @ R, -t - 3.0)]
    order = rng.permutation(K)
    while min(order.tolist().index(K - 4), order.tolist().index(K - 3)) < 5:
        order = rng.permutation(K)
    models = [models[i] for i in order]
    if with_translation:
        return np.array([np.concatenate([Rm, tm[:, None]], axis=1) for Rm, tm in models])
    return np.array([Rm for Rm, _ in models])


def scene(model, n_lm, noise, wrong, baseline, seed):
    rng = np.random.default_rng(seed)
    intr = np.zeros(12)
    intr[:len(INTR[model])] = INTR[model]
    R_SC = [rot([0.2, -1.0, 0.4], 0.03), rot([1.0, 0.3, -0.2], 0.08)]
    r_SC = [np.array([0.02, -0.05, 0.01]), np.array([0.025, 0.06, -0.004])]
    R_WS = [rot(rng.normal(size=3), 0.4)]
    r_WS = [rng.normal(size=3)]
    R_WS.append(R_WS[0] @ rot(rng.normal(size=3), 0.06))
    d = rng.normal(size=3)
    r_WS.append(r_WS[0] + R_WS[0] @ (baseline * d / np.linalg.norm(d)))
    # points in front of camera 0 of frame A; some of the homogeneous points are not normalised
    z = rng.uniform(2.0, 12.0, n_lm)
    p_C = np.stack([0.5 * z * rng.uniform(-1, 1, n_lm), 0.32 * z * rng.uniform(-1, 1, n_lm), z], axis=1)
    p_W = (R_WS[0] @ (R_SC[0] @ p_C.T + r_SC[0][:, None]) + r_WS[0][:, None]).T
    w = rng.choice([1.0, 1.0, 0.5, 2.5, -1.0], n_lm)
    hp = np.concatenate([p_W * w[:, None], w[:, None]], axis=1)
    kps, lms = [], []
    for f in range(2):
        for c in range(2):
            R_WC, r_WC = R_WS[f] @ R_SC[c], R_WS[f] @ r_SC[c] + r_WS[f]
            q = (p_W - r_WC) @ R_WC                   # R_WC^T (p - r)
            uv = project(intr, model, q)
            seen = (q[:, 2] > 0.3) & (uv[:, 0] > 5) & (uv[:, 0] < 747) & (uv[:, 1] > 5) & (uv[:, 1] < 475) & (rng.random(n_lm) < 0.93)
            idx = np.nonzero(seen)[0]
            kp = np.zeros((len(idx), 3), np.float32)
            kp[:, :2] = uv[idx] + noise * rng.normal(size=(len(idx), 2))
            bad = rng.random(len(idx)) < wrong        # a wrong association: the keypoint is somewhere else in the image
            kp[bad, 0], kp[bad, 1] = rng.uniform(20, 730, bad.sum()), rng.uniform(20, 460, bad.sum())
            kp[:, 2] = rng.uniform(5.0, 20.0, len(idx))
            # distractors without a landmark, and a shuffle
            n_free = 12
            free = np.stack([rng.uniform(20, 730, n_free), rng.uniform(20, 460, n_free), rng.uniform(5, 20, n_free)], axis=1).astype(np.float32)
            kp, lm = np.concatenate([kp, free]), np.concatenate([idx, np.full(n_free, -1)]).astype(np.int32)
            order = rng.permutation(len(kp))
            kps.append(np.ascontiguousarray(kp[order]))
            lms.append(np.ascontiguousarray(lm[order]))
    # (a landmark seen by one keypoint only stays out of the absolute adapter, which wants two observations: the adapter's business)
    T_SC = np.array([np.concatenate([r_SC[c], quat_xyzw(R_SC[c])]) for c in range(2)])
    R_SC_used = [rot_of_quat(T_SC[c][3:]) for c in range(2)]     # what the reference makes of the quaternion
    models_abs = hypotheses(rng, R_WS[1], r_WS[1], True)
    models_rot, models_rel = [], []
    for c in range(2):
        Ra, ra = R_WS[0] @ R_SC_used[c], R_WS[0] @ r_SC[c] + r_WS[0]
        Rb, rb = R_WS[1] @ R_SC_used[c], R_WS[1] @ r_SC[c] + r_WS[1]
        R12, t12 = Ra.T @ Rb, Ra.T @ (rb - ra)
        models_rot.append(hypotheses(rng, R12, t12, False))
        models_rel.append(hypotheses(rng, R12, t12, True))
    return dict(model=model, intr=intr, T_SC=T_SC, kps=kps, lms=lms, hp=hp, models_abs=models_abs, models_rot=models_rot, models_rel=models_rel)


def build(work):
    ref = os.environ.get("OKVIS_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "okvis_frontend")):
        sys.exit("set OKVIS_REFERENCE to the reference tree (the directory that holds okvis_frontend/)")
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    if not os.path.exists(os.path.join(obj, "Estimator.o")):
        sys.exit("oracle/_ref/obj is missing: make -C oracle/ref REF=<reference tree> first")
    shim = os.path.join(ROOT, "oracle", "shim")
    inc = [os.path.join(shim, "callers"), shim, os.path.join(shim, "okvis_shadow")] + \
          [os.path.join(ref, d, "include") for d in ("okvis_ceres", "okvis_kinematics", "okvis_cv", "okvis_common", "okvis_time", "okvis_util",
                                                      "okvis_frontend")] + [os.path.join(ROOT, "include")]
    objects = [os.path.join(obj, f) for f in sorted(os.listdir(obj))
               if f.endswith(".o") and not f.startswith("matcher_") and not f.startswith("own_ref")]
    exe = os.path.join(work, "sac_consensus_recorder")
    src = [os.path.join(ref, "okvis_frontend", "src", f) for f in ("FrameNoncentralAbsoluteAdapter.cpp", "FrameRelativeAdapter.cpp")]
    subprocess.check_call(["g++", "-std=gnu++14", "-O2", "-fPIC", "-w", "-DNDEBUG_SHIM_KEEP_ASSERTS", *["-I" + d for d in inc],
                           os.path.join(HERE, "sac_consensus_recorder.cpp"), *src, *objects, "-o", exe, "-lpthread"])
    return exe


class Reader:
    def __init__(self, path):
        self.b, self.o = open(path, "rb").read(), 0

    def take(self, dtype, *shape):
        n = int(np.prod(shape)) if shape else 1
        a = np.frombuffer(self.b, dtype, n, self.o).copy()
        self.o += a.nbytes
        return a.reshape(shape) if shape else a[0]

    def problem(self, k, n):
        scores, counts = self.take(np.float64, k, n), self.take(np.int32, k)
        best, ni = int(self.take(np.int32)), int(self.take(np.int32))
        return scores, counts, best, self.take(np.int32, ni)


def run_case(exe, work, i, sc):
    path, out = os.path.join(work, f"sac_case{i}.bin"), os.path.join(work, f"sac_case{i}.out")
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", REF_TYPE[sc["model"]], *[len(k) for k in sc["kps"]], len(sc["hp"]), K, K, K))
        f.write(struct.pack("<d", THRESHOLD))
        sc["intr"].astype(np.float64).tofile(f)
        sc["T_SC"].astype(np.float64).tofile(f)
        for kp, lm in zip(sc["kps"], sc["lms"]):
            kp.astype(np.float32).tofile(f)
            lm.astype(np.int32).tofile(f)
        sc["hp"].astype(np.float64).tofile(f)
        sc["models_abs"].astype(np.float64).tofile(f)
        for c in range(2):
            sc["models_rot"][c].astype(np.float64).tofile(f)
            sc["models_rel"][c].astype(np.float64).tofile(f)
    subprocess.check_call([exe, path, out])
    r = Reader(out)
    rec = {}
    n = int(r.take(np.int32))
    per = np.frombuffer(r.b, np.dtype([("bearing", "<f8", 3), ("point", "<f8", 3), ("sigma", "<f8"), ("cam", "<i4"), ("kp", "<i4")]), n, r.o)
    r.o += per.nbytes
    rec["abs"] = dict(bearing=per["bearing"].copy(), points=per["point"].copy(), sigma=per["sigma"].copy(), cam_index=per["cam"].copy(),
                      kp_index=per["kp"].copy(), cam_offsets=r.take(np.float64, 2, 3), cam_rotations=r.take(np.float64, 2, 3, 3),
                      models=sc["models_abs"])
    rec["abs"]["scores"], rec["abs"]["counts"], rec["abs"]["best"], rec["abs"]["inliers"] = r.problem(K, n)
    for c in range(2):
        n = int(r.take(np.int32))
        per = np.frombuffer(r.b, np.dtype([("a", "<i4"), ("b", "<i4"), ("f1", "<f8", 3), ("f2", "<f8", 3), ("s1", "<f8"), ("s2", "<f8")]), n, r.o)
        r.o += per.nbytes
        common = dict(idx_a=per["a"].copy(), idx_b=per["b"].copy(), bearing1=per["f1"].copy(), bearing2=per["f2"].copy(),
                      sigma1=per["s1"].copy(), sigma2=per["s2"].copy())
        for kind, models in (("rot", sc["models_rot"][c]), ("rel", sc["models_rel"][c])):
            p = dict(common, models=models)
            p["scores"], p["counts"], p["best"], p["inliers"] = r.problem(K, n)
            rec[f"{kind}{c}"] = p
    assert r.o == len(r.b)
    return rec


def job_of(name, p):
    kind = {"abs": S.ABSOLUTE, "rot": S.ROTATION_ONLY, "rel": S.RELATIVE}[name[:3]]
    return dict(p, kind=kind, threshold=THRESHOLD)


def main():
    work = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
    exe = build(work)
    out = {"n_cases": np.int32(len(CASES)), "threshold": np.float64(THRESHOLD)}
    worst = {"abs": 0.0, "rot": 0.0, "rel": 0.0, "bearing": 0.0, "sigma": 0.0}
    closest = {"abs": np.inf, "rot": np.inf, "rel": np.inf}
    seen = {k: {"tie": False, "none": False, "all": False} for k in ("abs", "rot", "rel")}
    for i, case in enumerate(CASES):
        sc = scene(*case)
        rec = run_case(exe, work, i, sc)
        pre = f"c{i}_"
        out[pre + "model"], out[pre + "intr"], out[pre + "T_SC"] = np.int32(sc["model"]), sc["intr"], sc["T_SC"]
        for j, name in enumerate(("kp_a0", "kp_a1", "kp_b0", "kp_b1")):
            out[pre + name] = sc["kps"][j]
        # the adapters' bearing vectors and sigma angles against the statement, by keypoint
        stated = [S.bearing_vectors(sc["intr"], sc["model"], kp) for kp in sc["kps"]]
        a = rec["abs"]
        for c in range(2):
            m = a["cam_index"] == c
            b, s, ok, _ = stated[2 + c]
            assert ok[a["kp_index"][m]].all()
            worst["bearing"] = max(worst["bearing"], float(np.abs(a["bearing"][m] - b[a["kp_index"][m]]).max()))
            worst["sigma"] = max(worst["sigma"], float(np.abs(a["sigma"][m] / s[a["kp_index"][m]] - 1).max()))
            p = rec[f"rot{c}"]
            for f, (idx, bk, sk) in enumerate((("idx_a", "bearing1", "sigma1"), ("idx_b", "bearing2", "sigma2"))):
                b, s, ok, _ = stated[2 * f + c]
                worst["bearing"] = max(worst["bearing"], float(np.abs(p[bk] - b[p[idx]]).max()))
                worst["sigma"] = max(worst["sigma"], float(np.abs(p[sk] / s[p[idx]] - 1).max()))
        for name, p in rec.items():
            kind = name[:3]
            want = S.scores(job_of(name, p))
            dist = float(S.distance(p["scores"], want).max())
            worst[kind] = max(worst[kind], dist)
            counts, best, inliers = S.consensus(want, THRESHOLD)
            assert (counts == p["counts"]).all() and best == p["best"] and (inliers == p["inliers"]).all(), (i, name)
            closest[kind] = min(closest[kind], float(S.distance(THRESHOLD, p["scores"]).min()))
            n = p["scores"].shape[1]
            seen[kind]["tie"] |= bool((counts == counts.max()).sum() >= 2 and counts.max() > 0 and best > 0)
            seen[kind]["none"] |= bool((counts == 0).any())
            seen[kind]["all"] |= bool((counts == n).any())
            print(f"case {i} {name}: n = {n}, counts {counts.min()}..{counts.max()} (best {best}, {(counts == counts.max()).sum()} at the top), "
                  f"reference vs statement {dist:.2e}")
            for key, v in p.items():
                if kind == "rel" and key in ("idx_a", "idx_b", "bearing1", "bearing2", "sigma1", "sigma2"):
                    continue   # the same adapter as the rotation-only problem of this camera
                out[f"{pre}{name}_{key}"] = np.asarray(v)
            out[f"{pre}{name}_pinned"] = np.int32(0 if kind == "rel" else 1)
    assert all(all(v.values()) for v in seen.values()), seen
    print("largest distance of the reference's double results from the long double statement:", {k: f"{v:.3e}" for k, v in worst.items()})
    for kind in closest:   # the inlier decision of every recorded cell is unambiguous
        print(f"{kind}: the score closest to the threshold is {closest[kind]:.3e} away, the comparison band is {BAND_FACTOR * worst[kind]:.3e}")
        assert closest[kind] > BAND_FACTOR * worst[kind], kind
    dst = os.path.join(HERE, "sac_consensus.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1 << 20


if __name__ == "__main__":
    main()
