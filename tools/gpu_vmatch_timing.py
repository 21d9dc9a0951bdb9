"""measurement (not a test): whole verified matching steps in one okvis_fe_match_verified call next to the route the same work took
before it: per step okvis_fe_project_landmarks, okvis_fe_hamming_candidates (count, then fill) and okvis_fe_gate_3d2d /
okvis_fe_stereo_triangulate(want_uncertainty = 0), each a synchronous call (the call sequence of
okvis_amd/csrc/host/okvis_matching_batched.hpp).  The host's DenseMatcher loop that follows those calls there is NOT part of the timed
route: the figure for the earlier route is a lower bound.

    python tools/gpu_vmatch_timing.py [--out FILE]        every step below, each GPU step a child process under its own timeout
    python tools/gpu_vmatch_timing.py --step fused        12 steps of 400 x 400 x 48 bytes, 6 of each kind, in one call
    python tools/gpu_vmatch_timing.py --step pieces       the same 12 steps through the separate entries, one after the other
    python tools/gpu_vmatch_timing.py --step occupancy    lanes busy per verification pass, derived from the scene and the lists

A call is timed with the host clock around the entry, which returns after a stream synchronise; warm-up calls first, then many
repeats; minimum, median and p90 are printed.  For kernel times run one step under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, JOBS = 400, 12


def scenes():
    import vmatch_scene as SC
    from okvis_amd.window import DIST_EQUIDISTANT, DIST_RADTAN
    return [(SC.KIND_3D2D if k % 2 else SC.KIND_2D2D, SC.scene(DIST_RADTAN if k % 4 < 2 else DIST_EQUIDISTANT, 7000 + k, N, N))
            for k in range(JOBS)]


def spec(F, kind, s):
    cam = F.camera(s["intr"], s["model"])
    j = {"kind": kind, "desc_a": s["desc_a"], "desc_b": s["desc_b"], "kp_a": s["kp_a"], "kp_b": s["kp_b"], "cam_a": cam, "cam_b": cam}
    if kind == F.MATCH_3D2D:
        j.update(hp_W=s["hp_W"], T_CbW=s["T_CbW"], P3=s["P3"])
    else:
        j.update(T_AB=s["T_AB"], UOplus=s["UOplus"])
    return j


def spread(seconds):
    s = np.sort(np.asarray(seconds))
    return {"repeats": len(s), "min_s": float(s[0]), "median_s": float(s[len(s) // 2]), "p90_s": float(s[int(0.9 * (len(s) - 1))]),
            "max_s": float(s[-1])}


def timed(call, warmup, repeats):
    for _ in range(warmup):
        call()
    seconds = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        seconds.append(time.perf_counter() - t0)
    return spread(seconds)


def step_fused(warmup, repeats):
    import vmatch_scene as SC
    from okvis_amd import frontend as F
    fe = F.Frontend()
    table, keep, out = F.vmatch_job_table([spec(F, kind, s) for kind, s in scenes()])
    r = timed(lambda: fe._call("match_verified", JOBS, table, SC.WIDTH, SC.THRESHOLD, SC.NUM_BEST, 0, 0.0), warmup, repeats)
    r.update(step="fused", jobs=JOBS, shape=[N, N, SC.WIDTH], num_best=SC.NUM_BEST, accepted=int(sum(o["accepted"].sum() for o in out)))
    fe.close()
    return r


def step_pieces(warmup, repeats):
    """the separate entries with every buffer allocated beforehand, so that the clock sees the calls and not numpy"""
    import vmatch_scene as SC
    from okvis_amd import frontend as F
    fe = F.Frontend()
    calls, keep, verified = [], [], []
    for kind, s in scenes():
        cam = F.camera(s["intr"], s["model"])
        pairs, _ = fe.hamming_candidates(s["desc_a"], s["desc_b"], SC.THRESHOLD)
        n, total = C.c_int32(0), len(pairs)
        buf = np.zeros((total, 2), np.int32)
        cand = (SC.WIDTH, N, s["desc_a"].ctypes.data, None, N, s["desc_b"].ctypes.data, None, SC.THRESHOLD)
        calls.append(("hamming_candidates", cand + (0, None, None, C.byref(n))))
        calls.append(("hamming_candidates", cand + (total, buf.ctypes.data, None, C.byref(n))))
        flags = np.zeros(total, np.uint8)
        if kind == F.MATCH_3D2D:
            uv, U, st = np.zeros((N, 2)), np.zeros((N, 4)), np.zeros(N, np.uint8)
            T, P3 = np.ascontiguousarray(s["T_CbW"]), np.ascontiguousarray(s["P3"])
            calls.insert(len(calls) - 2, ("project_landmarks", (C.byref(cam), T.ctypes.data, P3.ctypes.data, N, s["hp_W"].ctypes.data,
                                                                 uv.ctypes.data, U.ctypes.data, st.ctypes.data)))
            chi2 = np.zeros(total)
            # (the binding gates the candidates of the rows whose projection succeeded; all of them here: an upper bound on the work
            # of this call, by the few rows that project outside the image)
            calls.append(("gate_3d2d", (N, uv.ctypes.data, U.ctypes.data, N, s["kp_b"].ctypes.data, total, buf.ctypes.data, chi2.ctypes.data,
                                        flags.ctypes.data)))
            keep.append((cam, n, buf, flags, uv, U, st, T, P3, chi2))
        else:
            T, UO, sig = np.ascontiguousarray(s["T_AB"]), np.ascontiguousarray(s["UOplus"]), SC.pair_sigmas(s, pairs)
            calls.append(("stereo_triangulate", (C.byref(cam), C.byref(cam), T.ctypes.data, UO.ctypes.data, N, s["kp_a"].ctypes.data, N,
                                                 s["kp_b"].ctypes.data, total, buf.ctypes.data, sig.ctypes.data, 0, None, None,
                                                 flags.ctypes.data)))
            keep.append((cam, n, buf, flags, T, UO, sig))
        verified.append(flags)

    def run():
        for name, args in calls:
            fe._call(name, *args)

    r = timed(run, warmup, repeats)
    r.update(step="pieces", jobs=JOBS, calls=len(calls), candidates=int(sum(len(f) for f in verified)),
             verified=int(sum((f & 1 != 0).sum() for f in verified)))
    fe.close()
    return r


def step_occupancy():
    """the verification passes of verified_lists_kernel replayed on the host: per (row, tile of 256) the pairs in play with d < threshold
    and d < the list's last entry at the start of the tile are verified 64 at a time; next to it what the same pairs would occupy under
    the 64-lane mask of the distance loop"""
    import matcher_statement as S0
    import vmatch_scene as SC
    from okvis_amd import frontend as F
    fe = F.Frontend()
    asked = passes = blocks = 0
    for kind, s in scenes():
        cam = F.camera(s["intr"], s["model"])
        pairs, _ = fe.hamming_candidates(s["desc_a"], s["desc_b"], SC.THRESHOLD)
        if kind == F.MATCH_3D2D:
            uv, U, st = fe.project_landmarks(cam, s["T_CbW"], s["P3"], s["hp_W"])
            ok = (fe.gate_3d2d(uv, U, s["kp_b"], pairs)[1] & F.GATE_VERIFIED != 0) & (st[pairs[:, 0]] == F.PROJ_SUCCESSFUL)
        else:
            ok = fe.stereo_triangulate(cam, cam, s["T_AB"], s["UOplus"], s["kp_a"], s["kp_b"], pairs, SC.pair_sigmas(s, pairs),
                                       want_uncertainty=False)[2] & F.TRI_VALID != 0
        ham = S0.hamming_matrix(s["desc_a"], s["desc_b"]).astype(np.float32)
        good = np.zeros(ham.shape, bool)
        good[pairs[:, 0], pairs[:, 1]] = ok
        for a in range(N):
            if kind == F.MATCH_3D2D and st[a] != F.PROJ_SUCCESSFUL:
                continue
            lst = [SC.THRESHOLD] * SC.NUM_BEST
            for b0 in range(0, N, 256):
                d = ham[a, b0:b0 + 256]
                cand = np.flatnonzero(d < lst[-1])            # (the list starts at the threshold)
                asked += len(cand)
                passes += (len(cand) + 63) // 64
                blocks += len(set(cand // 64))
                for t in cand:
                    if good[a, b0 + t] and d[t] < lst[-1]:
                        lst = sorted(lst[:-1] + [float(d[t])])
    fe.close()
    return {"step": "occupancy", "verifications": asked, "gathered_passes": passes, "lanes_per_gathered_pass": asked / max(1, passes),
            "blocks_of_64_with_a_candidate": blocks, "lanes_per_block_under_the_distance_mask": asked / max(1, blocks)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["fused", "pieces", "occupancy"])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step == "fused":
        print(json.dumps(step_fused(args.warmup, args.repeats)))
        return
    if args.step == "pieces":
        print(json.dumps(step_pieces(args.warmup, args.repeats)))
        return
    if args.step == "occupancy":
        print(json.dumps(step_occupancy()))
        return
    results = []
    for step, limit in (("pieces", 180), ("fused", 180), ("pieces", 180), ("fused", 180), ("occupancy", 180)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--warmup", str(args.warmup),
               "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                      # nothing more is started after a step that failed
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            sys.exit(p.returncode)
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
