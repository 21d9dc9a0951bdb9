#!/usr/bin/env python3
"""Digest of the frontend entries (include/okvis_amd_frontend.h) over the scenes of the existing tests: needs a GPU.

Every okvis_fe_* entry (the nineteen of the header, the table query aside; create and destroy by way of the context) is called through okvis_amd.frontend;
every output array of every case is hashed (SHA-256).  OUT.json holds one record per group of cases (the part of a case's name
in front of the slash): how many cases and arrays, and the SHA-256 over their (case, array, hash) lines in sorted order.  Two trees
whose files are equal computed the same bytes for every case; two runs on one tree show that the digest is repeatable.  Where a
group differs, --cases FILE writes the hash of every array of every case (some 18 000 lines: to be compared, not to be kept).

    python tools/fe_digest.py OUT.json [--root TREE] [--cases FILE]   (TREE: the checkout whose okvis_amd is used, default this one)

The scenes (tests/vmatch_scene.py, the generator of tests/test_gpu_descriptor_matcher.py, tests/sac_cases.py,
tests/sac_solve_cases.py, tests/sac_abs_cases.py, tests/ransac_cases.py, tests/imu_propagate_cases.py, tests/keyframe_cases.py, tests/detect_cases.py, tests/describe_cases.py, tests/detect_scale_cases.py, tests/golden/) are those of the checkout the tool
itself is in; nothing outside it is read.
  verified matching   the eight shapes of tests/test_gpu_vmatch.py x both kinds x both camera models x the five (num_best, use_ratio)
                      settings x with and without skip masks, every case alone, and all of them as one mixed batch per setting
  stand-alone pieces  the same scenes through project_landmarks (and the two camera models the scenes lack), gate_3d2d,
                      hamming_candidates (also with a capacity under the total) and stereo_triangulate (with and without sigma_ray,
                      want_uncertainty 0 and 1, the _gn variant)
  descriptor matcher  widths 16 / 32 / 48 / 64 through both matchers, alone and as a batch; the recorded cases of dense_matcher.npz
  RANSAC              the recorded problems of sac_consensus.npz with and without scores, alone and as a batch; bearing_vectors for
                      the four camera models
  RANSAC solvers      sac_solve over n in {1, 63, 64, 65, 257} correspondences x K in {1, 8, 9} (relative) / {1, 64, 65} (rotation
                      only) hypotheses x solve only / with consensus / with scores / with essentials, every job alone, all of
                      them (scored next to unscored, both kinds) as one batch per output setting, and two scored jobs whose
                      hypotheses stay on the device (models null)
  RANSAC absolute solver  sac_solve_absolute over n in {4, 63, 64, 65, 257} correspondences x K in {1, 3, 4, 5, 9} samples (the four
                      samples of a wave, the eight hypotheses of a consensus tile) x 1, 2 and 8 cameras x solve only / with consensus /
                      with scores / with candidates, every job alone, all of them (scored next to unscored) as one batch per output
                      setting, and a scored job whose hypotheses stay on the device (models null)
  RANSAC loop         ransac over n in {s-1, s, 63, 64, 65, 257} correspondences x {1, 5, 8, 9, 64, 65} sample slots x the three
                      kinds on scenes with a third of the second bearings swapped, with and without the referee outputs, every
                      job alone and all of them as one mixed batch; the three end-to-end scenes.  Left out where the tree under
                      --root is from before the entry
  propagation         imu_propagate_cases.batch() as one call; every spec alone under flags 0, IMU_COV, IMU_JAC and both
  keyframe            every family of keyframe_cases.NAMES with and without the hull lists, every job alone and the family as
                      one call
  detect              every family of detect_cases.NAMES with and without the score image, every job alone and the family as one
                      call; the end-to-end scenes and the shifted images.  Left out where the tree under --root is from before
                      the entry
  describe            every family of describe_cases.NAMES, the stereo pair, the shifted and the turned images with given
                      rotations, every job alone and the family as one call; the angle cases of the four camera models; the
                      chain on detect families.  Left out where the tree under --root is from before the entries
  detect_scaled       every family of detect_scale_cases.NAMES with and without the referee outputs (scale, the layers' score
                      images and pixels), every job alone (detect_scaled) and the family as one call (detect_scaled_batch);
                      detect_scaled_and_describe on the capacity and edges families and twenty mixed jobs with every output
                      (detect_scaled_chain).  Left out where the tree under --root is from before the entries
"""
import argparse
import ctypes as C
import functools
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--cases")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402

import imu_propagate_cases as IC  # noqa: E402
import keyframe_cases as KC  # noqa: E402
import ransac_cases as RC  # noqa: E402
import sac_abs_cases as SAC  # noqa: E402
import sac_cases  # noqa: E402
import sac_solve_cases as SSC  # noqa: E402
import test_gpu_descriptor_matcher as DM  # noqa: E402  (its scene generator and the golden cases)
import vmatch_scene as SC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402
from okvis_amd.window import DIST_EQUIDISTANT, DIST_RADTAN  # noqa: E402

assert os.path.abspath(F.__file__).startswith(os.path.abspath(args.root) + os.sep), F.__file__

SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (257, 513), (400, 400)]
KINDS = [F.MATCH_3D2D, F.MATCH_2D2D]
MODELS = [DIST_RADTAN, DIST_EQUIDISTANT]
SETTINGS = [(1, False), (4, False), (8, False), (4, True), (8, True)]
RATIO = 1.2
OTHER_INTR = {0: [455.0, 452.0, 370.0, 245.0],                                                    # DIST_NONE
              3: [420.0, 418.0, 370.0, 243.0, -0.25, 0.06, 0.0002, -0.0001, 0.004, 0.03, -0.01, 0.002]}   # DIST_RADTAN8
BEARING_INTR = dict(OTHER_INTR)
BEARING_INTR.update({int(m): SC.INTR[m] for m in MODELS})

out = {}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(name, **arrays):
    assert name not in out, name
    out[name] = {k: sha(v) for k, v in arrays.items()}


@functools.lru_cache(maxsize=None)
def scene(model, k, skipped=0.0):
    return SC.scene(model, 1000 + 10 * k + model, *SHAPES[k], skipped)


def vjob(kind, s):
    cam = F.camera(s["intr"], s["model"])
    j = {"kind": kind, "desc_a": s["desc_a"], "desc_b": s["desc_b"], "kp_a": s["kp_a"], "kp_b": s["kp_b"], "cam_a": cam, "cam_b": cam,
         "skip_a": s["skip_a"], "skip_b": s["skip_b"]}
    if kind == F.MATCH_3D2D:
        j.update(hp_W=s["hp_W"], T_CbW=s["T_CbW"], P3=s["P3"])
    else:
        j.update(T_AB=s["T_AB"], UOplus=s["UOplus"])
    return j


fe = F.Frontend()

# ---------------------------------------------------------------- verified matching
cases = [(kind, model, k, skipped) for kind in KINDS for model in MODELS for k in range(len(SHAPES)) for skipped in (0.0, 0.15)]
for num_best, use_ratio in SETTINGS:
    tag = f"nb{num_best}_ratio{int(use_ratio)}"
    for kind, model, k, skipped in cases:
        got, = fe.match_verified([vjob(kind, scene(model, k, skipped))], SC.THRESHOLD, num_best, use_ratio, RATIO)
        record(f"vmatch/kind{kind}_model{model}_shape{k}_skip{int(skipped > 0)}_{tag}", **got)
    batch = fe.match_verified([vjob(kind, scene(model, k, skipped)) for kind, model, k, skipped in cases], SC.THRESHOLD, num_best, use_ratio,
                              RATIO)
    for j, got in enumerate(batch):
        record(f"vmatch_batch/{tag}_job{j}", **got)

# ---------------------------------------------------------------- stand-alone pieces
for model in MODELS:
    for k in range(len(SHAPES)):
        s = scene(model, k)
        name = f"model{model}_shape{k}"
        cam = F.camera(s["intr"], model)
        uv, U, st = fe.project_landmarks(cam, s["T_CbW"], s["P3"], s["hp_W"])
        record(f"project_landmarks/{name}", uv=uv, U=U, status=st)
        pairs, dist = fe.hamming_candidates(s["desc_a"], s["desc_b"], SC.THRESHOLD)
        record(f"hamming_candidates/{name}", pairs=pairs, dist=dist)
        sk = scene(model, k, 0.15)
        pairs_s, dist_s = fe.hamming_candidates(sk["desc_a"], sk["desc_b"], SC.THRESHOLD, sk["skip_a"], sk["skip_b"])
        record(f"hamming_candidates/{name}_skip", pairs=pairs_s, dist=dist_s)
        if len(pairs) > 1:       # a capacity under the total: the prefix comes back, the rest stays as it was
            cap, n = len(pairs) // 2, C.c_int32(-1)
            p2, d2 = np.full((cap + 1, 2), -7, np.int32), np.full(cap + 1, -7.0, np.float32)
            fe._call("hamming_candidates", SC.WIDTH, len(s["desc_a"]), s["desc_a"].ctypes.data, None, len(s["desc_b"]), s["desc_b"].ctypes.data,
                     None, SC.THRESHOLD, cap, p2.ctypes.data, d2.ctypes.data, C.byref(n))
            record(f"hamming_candidates/{name}_capacity", pairs=p2, dist=d2, total=np.int32(n.value))
        chi2, flags = fe.gate_3d2d(uv, U, s["kp_b"], pairs) if len(uv) else (np.zeros(0), np.zeros(0, np.uint8))
        record(f"gate_3d2d/{name}", chi2=chi2, flags=flags)
        tri = (cam, cam, s["T_AB"], s["UOplus"], s["kp_a"], s["kp_b"], pairs)
        sig = SC.pair_sigmas(s, pairs)
        for sname, sigma in (("sigma", sig), ("nosigma", None)):
            for want in (0, 1):
                hp, cov, fl = fe.stereo_triangulate(*tri, sigma, want_uncertainty=bool(want))
                record(f"stereo_triangulate/{name}_{sname}_unc{want}", hp=hp, cov=cov, flags=fl)
            hp, cov, fl, gn = fe.stereo_triangulate_gn(*tri, sigma)
            record(f"stereo_triangulate_gn/{name}_{sname}", hp=hp, cov=cov, flags=fl, gn=gn)
for model, intr in OTHER_INTR.items():     # the camera models the scenes do not have: the landmarks of the largest scenes
    for k in (6, 7):
        s = scene(DIST_RADTAN, k)
        uv, U, st = fe.project_landmarks(F.camera(intr, model), s["T_CbW"], s["P3"], s["hp_W"])
        record(f"project_landmarks/model{model}_shape{k}", uv=uv, U=U, status=st)

# ---------------------------------------------------------------- descriptor matcher
for width in (16, 32, 48, 64):
    jobs = []
    for k, (n_a, n_b) in enumerate(DM.SIZES):
        for skips in (False, True):
            a, b, sa, sb = DM.scene(100 * width + k, n_a, n_b, width, 0.25 if skips else 0.0)
            jobs.append((a, b, sa, sb))
            name = f"w{width}_size{k}_skip{int(skips)}"
            pairs, dist = fe.hamming_candidates(a, b, width * 8 * 0.12, sa, sb)
            record(f"hamming_candidates/{name}", pairs=pairs, dist=dist)
            for num_best, use_ratio in ((1, False), (4, False), (4, True), (8, True)):
                (pa, pd, acc), = fe.match_descriptors([(a, b, sa, sb)], width * 8 * 0.15, num_best, use_ratio, RATIO)
                record(f"match_descriptors/{name}_nb{num_best}_ratio{int(use_ratio)}", pair_a=pa, pair_dist=pd, accepted=acc)
    for num_best, use_ratio in ((4, False), (4, True)):
        for j, (pa, pd, acc) in enumerate(fe.match_descriptors(jobs, width * 8 * 0.15, num_best, use_ratio, RATIO)):
            record(f"match_descriptors_batch/w{width}_nb{num_best}_ratio{int(use_ratio)}_job{j}", pair_a=pa, pair_dist=pd, accepted=acc)
golden = DM.golden_cases()
assert len(golden) == 6
for i, c in enumerate(golden):
    (pa, pd, acc), = fe.match_descriptors([(c["desc_a"], c["desc_b"], c["skip_a"], c["skip_b"])], float(c["threshold"]), int(c["num_best"]),
                                          bool(c["use_ratio"]), float(c["ratio_threshold"]))
    record(f"match_descriptors/golden{i}", pair_a=pa, pair_dist=pd, accepted=acc)

# ---------------------------------------------------------------- RANSAC
sac = sac_cases.golden_jobs()
for want_scores in (False, True):
    tag = f"scores{int(want_scores)}"
    for i, name, job in sac:
        r, = fe.sac_consensus([job], want_scores)
        record(f"sac_consensus/case{i}_{name}_{tag}", **{k: np.asarray(v) for k, v in r.items()})
    for (i, name, _), r in zip(sac, fe.sac_consensus([job for _, _, job in sac], want_scores)):
        record(f"sac_consensus_batch/case{i}_{name}_{tag}", **{k: np.asarray(v) for k, v in r.items()})
rng = np.random.default_rng(40)
for model, intr in sorted(BEARING_INTR.items()):
    for n in (1, 257, 5000):
        kp = np.stack([rng.uniform(5, 747, n), rng.uniform(5, 475, n), rng.uniform(4, 30, n)], axis=1).astype(np.float32)
        b, s, ok = fe.bearing_vectors(F.camera(intr, model), kp)
        record(f"bearing_vectors/model{model}_n{n}", bearing=b, sigma=s, ok=ok)


def arrays(r):
    return {k: np.asarray(v) for k, v in r.items()}


# sac_solve: n at the ballot-word edges and the edge of a 256-lane tile; K at the SAC_MODEL_TILE edge (relative) and at the 64
# samples of a wave (rotation only).  sac_solve_cases.case draws samples without repetition, which needs n >= 8: the n = 1 scene
# is sac_solve_cases.scene with every sample index 0 (hypotheses invalid by rule, the consensus stage still runs over them).
def solve_case(n, k):
    if n >= 8:
        return SSC.case(300 + n, n, k)
    rng = np.random.default_rng(300 + n)
    _, _, b1, b2 = SSC.scene(rng, n)
    return {"bearing1": b1, "bearing2": b2, "sigma1": rng.uniform(0.5e-6, 2e-6, n), "sigma2": rng.uniform(0.5e-6, 2e-6, n),
            "samples5": np.zeros((k, 8), np.int32), "samples2": np.zeros((k, 2), np.int32), "n": n}


SOLVE_N = (1, 63, 64, 65, 257)
SOLVE_K = {F.SAC_RELATIVE: (1, 8, 9), F.SAC_ROTATION_ONLY: (1, 64, 65)}
SOLVE_MODES = {"solve_only": (False, False, False), "consensus": (True, False, False), "scores": (True, True, False),
               "essentials": (True, False, True)}       # (consensus, want_scores, want_essentials)


def solve_job(kind, n, k, consensus):
    make = SSC.relative_job if kind == F.SAC_RELATIVE else SSC.rotation_job
    return make(solve_case(n, k), consensus=consensus)


solve_shapes = [(kind, n, k) for kind in (F.SAC_RELATIVE, F.SAC_ROTATION_ONLY) for n in SOLVE_N for k in SOLVE_K[kind]]
for mode, (consensus, want_scores, want_essentials) in SOLVE_MODES.items():
    for kind, n, k in solve_shapes:
        r, = fe.sac_solve([solve_job(kind, n, k, consensus)], want_scores, want_essentials)
        record(f"sac_solve/kind{kind}_n{n}_k{k}_{mode}", **arrays(r))
mixed = [(kind, n, k, consensus) for kind, n, k in solve_shapes for consensus in (False, True)]      # scored next to unscored
for tag, want_scores, want_essentials in (("plain", False, False), ("scores", True, False), ("essentials", False, True)):
    for (kind, n, k, consensus), r in zip(mixed, fe.sac_solve([solve_job(*m) for m in mixed], want_scores, want_essentials)):
        record(f"sac_solve_batch/{tag}_kind{kind}_n{n}_k{k}_consensus{int(consensus)}", **arrays(r))
for kind, n, k in ((F.SAC_RELATIVE, 65, 9), (F.SAC_ROTATION_ONLY, 257, 65)):     # models null on a scored job: they stay on the device
    table, keep, (o,) = F.sac_solve_job_table([solve_job(kind, n, k, True)], want_scores=True, want_essentials=True)
    models = o.pop("models")
    table[0].models = None
    fe._call("sac_solve", 1, table)
    assert not models.any()
    record(f"sac_solve/kind{kind}_n{n}_k{k}_device_only_models", **o)

# ---------------------------------------------------------------- RANSAC absolute solver
# sac_solve_absolute: n at the ballot-word edges and the edge of a 256-lane tile (4: the least a sample needs); K at the four
# samples of a wave and at the SAC_MODEL_TILE edge; the central problem, two cameras, and eight with the outer two in use
ABS_N = (4, 63, 64, 65, 257)
ABS_K = (1, 3, 4, 5, 9)
ABS_CAMS = ((1, None), (2, None), (8, (0, 7)))
ABS_MODES = {"solve_only": (False, False, False), "consensus": (True, False, False), "scores": (True, True, False),
             "candidates": (True, False, True)}       # (consensus, want_scores, want_candidates)


def abs_job(n, k, cams, consensus):
    c = SAC.case(500 + n, n, 130, cams[0], False, cams[1])
    q = c["samples"][:k] if n > 4 else np.repeat(c["samples"], k, axis=0)
    return SAC.job(c, q, consensus=consensus)


abs_shapes = [(n, k, cams) for n in ABS_N for k in ABS_K for cams in ABS_CAMS]
for mode, (consensus, want_scores, want_candidates) in ABS_MODES.items():
    for n, k, cams in abs_shapes:
        r, = fe.sac_solve_absolute([abs_job(n, k, cams, consensus)], want_scores, want_candidates)
        record(f"sac_solve_absolute/cams{cams[0]}_n{n}_k{k}_{mode}", **arrays(r))
mixed = [(n, k, cams, consensus) for n, k, cams in abs_shapes for consensus in (False, True)]      # scored next to unscored
for tag, want_scores, want_candidates in (("plain", False, False), ("scores", True, False), ("candidates", False, True)):
    for (n, k, cams, consensus), r in zip(mixed, fe.sac_solve_absolute([abs_job(*m) for m in mixed], want_scores, want_candidates)):
        record(f"sac_solve_absolute_batch/{tag}_cams{cams[0]}_n{n}_k{k}_consensus{int(consensus)}", **arrays(r))
table, keep, (o,) = F.sac_absolute_job_table([abs_job(257, 9, ABS_CAMS[1], True)], want_scores=True, want_candidates=True)
models = o.pop("models")      # models null on a scored job: they stay on the device
table[0].models = None
fe._call("sac_solve_absolute", 1, table)
assert not models.any()
record("sac_solve_absolute/cams2_n257_k9_device_only_models", **o)

# ---------------------------------------------------------------- RANSAC loop
# ransac: n below the sample size, at it, at the ballot-word edges and the edge of a 256-lane tile; slots at the consensus tile,
# the four samples of a three-point wave and the 64 lanes of the loop's wave; scenes with a third of the second bearings swapped
RANSAC_N = (-1, 0, 63, 64, 65, 257)          # offsets from the sample size below 63
RANSAC_SLOTS = (1, 5, 8, 9, 64, 65)
if hasattr(fe, "ransac"):          # a tree from before the entry has every other group
    def ransac_digest_job(kind, dn, slots):
        n = F.SAC_SAMPLE_SIZE[kind] + dn if dn <= 0 else dn
        return RC.ransac_job(kind, RC.exact_fields(kind, n, 700 + 10 * n + kind, outliers=0.34), n_slots=slots, max_iterations=50,
                             probability=0.99, threshold=9.0, seed=0x9E3779B97F4A7C15 ^ (n * 1024 + slots))

    ransac_shapes = [(kind, dn, slots) for kind in RC.KINDS for dn in RANSAC_N for slots in RANSAC_SLOTS]
    for referee in (False, True):
        tag = f"referee{int(referee)}"
        for kind, dn, slots in ransac_shapes:
            r, = fe.ransac([ransac_digest_job(kind, dn, slots)], referee)
            record(f"ransac/kind{kind}_n{dn}_slots{slots}_{tag}", **arrays(r))
        for (kind, dn, slots), r in zip(ransac_shapes, fe.ransac([ransac_digest_job(*s) for s in ransac_shapes], referee)):
            record(f"ransac_batch/kind{kind}_n{dn}_slots{slots}_{tag}", **arrays(r))
        for kind in RC.KINDS:
            r, = fe.ransac([RC.end_to_end(kind)[0]], referee)
            record(f"ransac/end_to_end_kind{kind}_{tag}", **arrays(r))

# ---------------------------------------------------------------- propagation
PROP = ("T_WS", "sb", "count", "cov", "jac")


def propagate(spec_list):
    s_t, s_gyr, s_acc, ends, jobs = IC.pool(spec_list)
    return dict(zip(PROP, fe.imu_propagate(IC.PARAMS, s_t, s_gyr, s_acc, jobs, ends)))


record("imu_propagate/batch", **propagate(IC.batch()))
for spec in IC.specs():
    for flags in (0, F.IMU_COV, F.IMU_JAC, F.IMU_COV | F.IMU_JAC):
        record(f"imu_propagate/{spec['name']}_flags{flags}", **propagate([dict(spec, flags=flags)]))


# ---------------------------------------------------------------- keyframe decision
def kf_arrays(r):
    ims = r["images"]
    a = {k: np.array([im[k] for im in ims]) for k in ("n_matched", "hull_all_size", "hull_matched_size", "area_all", "area_matched", "n_inside", "flags")}
    for k in ("hull_all", "hull_matched"):
        if k in ims[0]:
            a[k] = np.concatenate([np.asarray(im[k], np.int32) for im in ims])
    return dict(a, decision=np.uint8(r["decision"]), overlap=np.float64(r["overlap"]), ratio=np.float64(r["ratio"]))


for name in KC.NAMES:
    jobs = KC.cases(name)
    for want_hulls in (False, True):
        tag = f"{name}_hulls{int(want_hulls)}"
        for j, job in enumerate(jobs):
            r, = fe.keyframe_decision([job], want_hulls)
            record(f"keyframe/{tag}_job{j}", **kf_arrays(r))
        for j, r in enumerate(fe.keyframe_decision(jobs, want_hulls)):
            record(f"keyframe_batch/{tag}_job{j}", **kf_arrays(r))

# ---------------------------------------------------------------- keypoint detection
if hasattr(fe, "detect_keypoints"):          # a tree from before the entry has every other group
    import detect_cases as DC  # noqa: E402  (it reads the tile shape from the tree's okvis_amd.frontend)

    def detect(jobs, want_score):
        return fe.detect_keypoints([j["image"] for j in jobs], *[[j[k] for j in jobs] for k in ("threshold", "min_dist", "max_keypoints",
                                                                                               "cand_capacity", "kp_size")], want_score=want_score)

    def det_arrays(r):
        return {k: np.asarray(v) for k, v in r.items()}

    families = {name: DC.cases(name) for name in DC.NAMES}
    families["scenes"] = [DC.scene(seed, noise)[0] for seed in DC.SCENE_SEEDS for noise in (False, True)]
    families["shifts"] = [DC.translated(dx, dy) for dx, dy in DC.SHIFTS]
    for name, jobs in families.items():
        for want_score in (False, True):
            tag = f"{name}_score{int(want_score)}"
            for j, job in enumerate(jobs):
                r, = detect([job], want_score)
                record(f"detect/{tag}_job{j}", **det_arrays(r))
            for j, r in enumerate(detect(jobs, want_score)):
                record(f"detect_batch/{tag}_job{j}", **det_arrays(r))

# ---------------------------------------------------------------- keypoint description
if hasattr(fe, "describe_keypoints"):        # a tree from before the entries has every other group
    import describe_cases as BC  # noqa: E402

    ALL = ("rot", "angle", "angle64")

    def describe(jobs):
        return fe.describe_keypoints([j["image"] for j in jobs], [j["kp"] for j in jobs], rot=[j["rot"] for j in jobs], want=ALL)

    families = {name: BC.cases(name) for name in BC.NAMES}
    families["scene"] = BC.scene()
    families["shifts"] = [BC.shifted(dx, dy) for dx, dy in BC.SHIFTS]
    families["turn"] = list(BC.quarter_turn())
    for name, jobs in families.items():
        for j, job in enumerate(jobs):
            r, = describe([job])
            record(f"describe/{name}_job{j}", **det_arrays(r))
        for j, r in enumerate(describe(jobs)):
            record(f"describe_batch/{name}_job{j}", **det_arrays(r))
    angle_image = BC.textured(70, BC.ANGLE_IMAGE_SHAPE[1], BC.ANGLE_IMAGE_SHAPE[0])
    for c in BC.angle_cases():
        r, = fe.describe_keypoints([angle_image], [c["kp"]], F.camera(c["cam"]["intr"], c["cam"]["model"]), c["direction"], want=ALL)
        record(f"describe_angle/{c['name'].replace('/', '_')}", **det_arrays(r))
    chain = DC.cases("selection") + DC.cases("capacity") + DC.cases("mixed")[:20]
    cam = F.camera(BC.CAMERAS["equi"]["intr"], 2, 160, 120)
    fields = [[j[k] for j in chain] for k in ("threshold", "min_dist", "max_keypoints", "cand_capacity", "kp_size")]
    for j, r in enumerate(fe.detect_and_describe([j["image"] for j in chain], fields[0], cam, [0.2, 0.9, 0.38], *fields[1:], want=ALL)):
        record(f"describe_chain/job{j}", **det_arrays(r))

# ---------------------------------------------------------------- keypoint detection over a scale space
if hasattr(fe, "detect_keypoints_scaled"):   # a tree from before the entries has every other group
    import detect_scale_cases as DSC  # noqa: E402

    def scaled_args(jobs):
        return [[j["image"] for j in jobs]] + [[j[k] for j in jobs] for k in DSC.FIELDS]

    def detect_scaled(jobs, referee):
        return fe.detect_keypoints_scaled(*scaled_args(jobs), want_score=referee, want_pyramid=referee, want_scale=referee)

    def scaled_arrays(r):    # score and pyramid are lists of layers of different shapes: their bytes one behind the other
        return {k: np.frombuffer(b"".join(np.ascontiguousarray(a).tobytes() for a in v), np.uint8) if isinstance(v, list) else np.asarray(v)
                for k, v in r.items()}

    for name in DSC.NAMES:
        jobs = DSC.cases(name)
        for referee in (False, True):
            tag = f"{name}_referee{int(referee)}"
            for j, job in enumerate(jobs):
                r, = detect_scaled([job], referee)
                record(f"detect_scaled/{tag}_job{j}", **scaled_arrays(r))
            for j, r in enumerate(detect_scaled(jobs, referee)):
                record(f"detect_scaled_batch/{tag}_job{j}", **scaled_arrays(r))
    chain = DSC.cases("capacity") + DSC.cases("edges") + DSC.cases("mixed")[:20]
    cam = F.camera(BC.CAMERAS["equi"]["intr"], 2, 160, 120)
    images, threshold, octaves, *rest = scaled_args(chain)
    for j, r in enumerate(fe.detect_scaled_and_describe(images, threshold, octaves, cam, [0.2, 0.9, 0.38], *rest, want_score=True, want_pyramid=True,
                                                        want_scale=True, want=ALL)):
        record(f"detect_scaled_chain/job{j}", **scaled_arrays(r))
fe.close()

if args.cases:
    json.dump(out, open(args.cases, "w"), indent=1, sort_keys=True)
groups = {}
for name in sorted(out):
    g = groups.setdefault(name.split("/")[0], {"cases": 0, "arrays": 0, "sha256": hashlib.sha256()})
    g["cases"] += 1
    for k in sorted(out[name]):
        g["arrays"] += 1
        g["sha256"].update(f"{name} {k} {out[name][k]}\n".encode())
for g in groups.values():
    g["sha256"] = g["sha256"].hexdigest()
json.dump(groups, open(args.out, "w"), indent=1, sort_keys=True)
print(f"{len(out)} cases in {len(groups)} groups -> {args.out}: sha256 {hashlib.sha256(open(args.out, 'rb').read()).hexdigest()}")
