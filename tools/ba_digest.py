#!/usr/bin/env python3
"""Digest of the solver's own C-ABI entries (okvis_amd/csrc/ba_capi.hip, capi_upload.inc, capi_queries.inc): needs the GPU.

Cases: the small synthetic window on a one-window solver, the covariance referee's windows A and D (tests/cov_cases.py), a
three-window batch of different shapes, and the same batch on two sub-batch streams (n_streams = 2).  Every solver is patchable.
Each case runs a fixed sequence - upload, optimize, every fetch, every okvis_ba_download array (the diagnostic ones that are plain
data included; not the clock stamps), pairs, launch_route, algorithmic_bytes, set_state, a second optimize, a value patch,
optimize_timed without a limit - and records every status and summary and the SHA-256 of every returned array; behind every step
but the first optimize the fetches alone are taken again (the file stays small enough to read).  No timings.  Two
trees whose digests are equal hand out the same bits on every path the list reaches.  Each case runs in a process of its own under
a time limit; the first one that fails ends the run.

    python tools/ba_digest.py out.json [--root TREE]      (TREE: the built checkout whose okvis_amd is used, default this one)
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
CASES = ("small", "cov_A", "cov_D", "three", "three_two_streams")
CASE_SECONDS = 120
ITERS = 3

if not args.case:   # the driver: never opens the GPU itself
    out = {}
    for name in CASES:
        part = f"{args.out}.{name}.part"
        subprocess.run([sys.executable, os.path.abspath(__file__), part, "--root", args.root, "--case", name], check=True, timeout=CASE_SECONDS)
        out[name] = json.load(open(part))
        os.unlink(part)
    with open(args.out, "w") as f:   # one line per case and step
        f.write("{\n" + ",\n".join(f' "{c}": {{\n' + ",\n".join(f'  "{k}": {json.dumps(v, sort_keys=True)}' for k, v in sorted(out[c].items())) + "\n }"
                                  for c in sorted(out)) + "\n}\n")
    json.load(open(args.out))
    print(f"{len(out)} cases -> {args.out}: sha256 {hashlib.sha256(open(args.out, 'rb').read()).hexdigest()}")
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.root))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

from okvis_amd import solver, synthetic  # noqa: E402
from okvis_amd.window import Patch, default_options  # noqa: E402
from tests import cov_cases as cc  # noqa: E402

NO_DIGEST = ("PROF",)   # clock stamps


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def arrays(b, w):
    """every array of okvis_ba_array_size / okvis_ba_download: [status of the size call, doubles, status of the download, SHA-256]"""
    rec = {}
    dp = C.POINTER(C.c_double)
    for name, which in sorted(solver.ARR.items()):
        if name in NO_DIGEST:
            continue
        n = C.c_int64(-1)
        r = [b._L.okvis_ba_array_size(b._h, w, which, C.byref(n)), n.value]
        if r[0] == 0:
            out = np.zeros(max(n.value, 0))
            r += [b._L.okvis_ba_download(b._h, w, which, out.ctypes.data_as(dp), n.value), sha(out)]
        rec[name] = r
    return rec


def fetches(b):
    return [dict(get_state=[sha(a) for a in b.get_state(w)], fetch_results={k: sha(v) for k, v in b.fetch_results(w).items()},
                 fetch_imu_caches=sha(b.fetch_imu_caches(w))) for w in range(len(b))]


def everything(b):
    rec = dict(launch_route=b.launch_route(), algorithmic_bytes=b.algorithmic_bytes(), windows=fetches(b))
    for w in range(len(b)):
        rec["windows"][w].update(reduced_dim=b.reduced_dim(w), pairs=[sha(a) for a in b.pairs(w)], arrays=arrays(b, w))
    return rec


opt = default_options()
if args.case == "small":
    windows = [synthetic.small_window(seed=1, K=4, L=40)]
elif args.case in ("cov_A", "cov_D"):
    windows = [cc.window(args.case[-1])]
else:
    windows = [synthetic.small_window(seed=1, K=4, L=40), cc.window("A"), synthetic.small_window(seed=2, K=3, L=25)]
    if args.case == "three_two_streams":
        opt.n_streams = 2
b = solver.WindowBatch(windows, options=opt, patchable=True)
rec = dict(uploaded=fetches(b))
assert (b.launch_route()["sub_batches"] > 1) == (args.case == "three_two_streams")
rec["optimize"] = b.optimize(ITERS)
rec["optimized"] = everything(b)
w = len(b) - 1
pose, sb, lm = (a.copy() for a in b.get_state(w))
pose[:, :3] += 0.01
lm[:, :3] += 0.02
b.set_state(w, pose, sb + 0.001, lm)
rec["set_state"] = fetches(b)
rec["second_optimize"] = b.optimize(ITERS)
rec["optimized_again"] = fetches(b)
b.patch(0, Patch(set_lm_idx=np.array([0], np.int32), set_lm=b.get_state(0)[2][:1] + 0.03))
rec["patched"] = fetches(b)
rec["optimize_timed"] = b.optimize_timed(ITERS, 1, -1.0)
rec["timed"] = fetches(b)
b.close()
json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
