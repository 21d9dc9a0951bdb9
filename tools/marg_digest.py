#!/usr/bin/env python3
"""Digest of okvis_ba_marginalize / okvis_ba_marginalize_batch over a fixed list of cases, one per route of the dense tail at its
smallest shape (the shapes of tests/test_gpu_marginalization.py and tests/test_gpu_marginalize_batch.py): needs the GPU.

For every case, every way of calling (single calls, one batched call, batched calls of one window) and every window: dim, rank,
sweeps, the block lists and the SHA-256 of the bytes of H, b0, J and e0.  Two trees whose digests are equal compute the same bits on
every route the list reaches.  Each case runs in a process of its own under a time limit; the first one that fails ends the run.

    python tools/marg_digest.py out.json [--root TREE]      (TREE: the built checkout whose okvis_amd is used, default this one)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--case", help="(internal) run this case alone and write its record to `out`")
args = ap.parse_args()
CASES = ("mixed_six", "tiled", "tiled_gauge_deficient", "hbm_workspace", "prior_291_rows", "tiled_switched_off")
CASE_SECONDS = 180

if not args.case:   # the driver: never opens the GPU itself
    out = {}
    for name in CASES:
        part = f"{args.out}.{name}.part"
        subprocess.run([sys.executable, os.path.abspath(__file__), part, "--root", args.root, "--case", name], check=True, timeout=CASE_SECONDS)
        out[name] = json.load(open(part))
        os.unlink(part)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print(f"{len(out)} cases -> {args.out}: sha256 {hashlib.sha256(open(args.out, 'rb').read()).hexdigest()}")
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402

from okvis_amd import solver, synthetic  # noqa: E402
from okvis_amd.window import TUNE_NO_MARG_TILES, default_options, set_options  # noqa: E402
from tests import oracle_lib  # noqa: E402  (the previous priors of two cases are the oracle's results, as in the tests)
from tests.test_gpu_marginalization import flags  # noqa: E402
from tests.test_gpu_marginalize_batch import mixed_six, observation_free  # noqa: E402


def record(r):
    d = dict(dim=int(r["dim"]), rank=int(r["rank"]), sweeps=[int(x) for x in r["sweeps"]])
    for k in ("block_type", "block_idx", "block_off"):
        d[k] = [int(x) for x in r[k]]
    for k in ("H", "b0", "J", "e0"):
        d[k + "_sha256"] = hashlib.sha256(np.ascontiguousarray(r[k], np.float64).tobytes()).hexdigest()
    return d


def every_way(ws, jobs, options=None):
    """windows ws in one solver: single calls, one batched call over all of them, batched calls of one"""
    b = solver.WindowBatch(ws, options=options or default_options())
    n = len(ws)
    out = dict(single_calls=[record(b.marginalize(i, *jobs[i])) for i in range(n)],
               one_batch=[record(r) for r in b.marginalize_batch(0, jobs)],
               batches_of_one=[record(b.marginalize_batch(i, [jobs[i]])[0]) for i in range(n)])
    b.close()
    return out


def alone_and_between(w, job, options=None):
    """w as the only window of a solver, and between two windows on the LDS route (windows 0 and 4 of the mixed six)"""
    ws, jobs = mixed_six(oracle_lib)
    return dict(alone=every_way([w], [job], options), between=every_way([ws[0], w, ws[4]], [jobs[0], job, jobs[4]], options))


def tiled_window(first_pose_prior=True):
    w = synthetic.small_window(seed=61, K=8, L=30)   # D = 120 <= 174, 105 kept rows > 96: the tiled tail
    if not first_pose_prior:   # the kept block is singular along the gauge directions: no proof of full rank, the fall-back
        w.pprior_pose = np.zeros(0, np.int32); w.pprior_meas = np.zeros((0, 7)); w.pprior_sqrtinfo = np.zeros((0, 36))
    return w, flags(w, [0], [0]) + (None,)


oracle_lib.lib()
if args.case == "mixed_six":
    rec = every_way(*mixed_six(oracle_lib))
elif args.case == "tiled":
    rec = alone_and_between(*tiled_window())
    assert rec["alone"]["single_calls"][0]["dim"] == 105
elif args.case == "tiled_gauge_deficient":
    rec = alone_and_between(*tiled_window(first_pose_prior=False))
    r = rec["alone"]["single_calls"][0]
    assert r["dim"] == 105 and r["rank"] < r["dim"], r     # (the tiled route only ends with full rank: the fall-back ran)
elif args.case == "hbm_workspace":
    w = synthetic.make_window(20, 30, 1.0, 2, frame_dt=0.1)   # D = 300: system assembled in HBM, the large instantiation
    rec = alone_and_between(w, flags(w, [0, 1], [0, 1]) + (None,))
elif args.case == "prior_291_rows":   # the second stage of test_previous_prior_of_more_than_192_rows
    w = synthetic.make_window(20, 30, 1.0, 3, frame_dt=0.1)
    r1 = oracle_lib.OracleWindow(w).marginalize(*flags(w, [], [0]))
    assert r1["dim"] == 291
    w2 = observation_free(w)
    rec = alone_and_between(w2, flags(w2, [0], []) + (dict(block_type=r1["block_type"], block_idx=r1["block_idx"], H=r1["H"], b0=r1["b0"]),))
elif args.case == "tiled_switched_off":
    w, job = tiled_window()
    rec = dict(alone=every_way([w], [job], set_options(default_options(), tuning_flags=TUNE_NO_MARG_TILES)))
else:
    raise KeyError(args.case)
json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
