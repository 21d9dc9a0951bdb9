#!/usr/bin/env python3
"""Digest of okvis_ba_state_covariance / okvis_ba_landmark_covariance / okvis_ba_predicted_measurement over the referee's cases
(tests/cov_cases.py, tests/lmcov_cases.py, tests/predcov_cases.py): needs the GPU.

State covariance on A-F at the uploaded state and after optimize(OPT_ITERS): the default selection, the same with the S0 tap, one
permuted block list.  Landmark covariance on A-F, H, U with taps: every landmark, and a selection with a repeat.  Predicted
measurement on the same eight with the case's query list and taps.  One mixed range and the singular window of every entry (the
results of its BackendError).  Per window: dim / n, info and the SHA-256 of the bytes of min_pivot and of every returned array.
Two trees whose digests are equal compute the same bits on every path the list reaches.  Each case runs in a process of its own
under a time limit; the first one that fails ends the run.

    python tools/cov_digest.py out.json [--root TREE]      (TREE: the built checkout whose okvis_amd is used, default this one)
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
STATE, LANDMARK = ("A", "B", "C", "D", "E", "F"), ("A", "B", "C", "D", "E", "F", "H", "U")   # cov_cases.CASES, lmcov_cases.CASES
CASES = tuple(f"state_{n}" for n in STATE) + tuple(f"landmark_{n}" for n in LANDMARK) + tuple(f"predicted_{n}" for n in LANDMARK) + \
    ("state_mixed", "landmark_mixed", "predicted_mixed", "state_singular", "landmark_singular", "predicted_singular")
CASE_SECONDS = 120

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

from okvis_amd import _lib, solver  # noqa: E402
from tests import cov_cases as cc  # noqa: E402
from tests import lmcov_cases as lc  # noqa: E402
from tests import predcov_cases as pc  # noqa: E402

assert STATE == tuple(cc.CASES) and LANDMARK == tuple(lc.CASES) == tuple(pc.CASES)


def record(r):
    """a window's result dict: the integers as they are, min_pivot and every array as the SHA-256 of its bytes"""
    d = {}
    for k, v in r.items():
        if k in ("dim", "info"):
            d[k] = int(v)
        elif k == "min_pivot":
            d[k + "_sha256"] = hashlib.sha256(np.float64(v).tobytes()).hexdigest()
        else:
            a = np.ascontiguousarray(v)
            d[k] = dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())
    if "dim" not in d:
        d["n"] = int(r["cov"].shape[0])
    return d


def records(rs):
    return [record(r) for r in rs]


def with_results_of_the_error(call):
    try:
        call()
    except _lib.BackendError as err:
        assert err.status == -5, err.status   # OKVIS_BA_ERR_NUMERIC
        return records(err.results)
    raise AssertionError("the singular window went through")


kind, name = args.case.split("_")
if kind == "state" and name in STATE:
    rec = {}
    for state in ("uploaded", "optimized"):
        b = solver.WindowBatch([cc.window(name)])
        if state == "optimized":
            b.optimize(cc.OPT_ITERS)
        rec[state] = dict(default=records(b.state_covariance()), with_S0=records(b.state_covariance(want_S0=True)),
                          permuted=records(b.state_covariance(cc.selections(name)["newest+first"])))
        b.close()
elif kind == "landmark" and name in LANDMARK:
    b = solver.WindowBatch([lc.window(name)])
    rec = dict(every=records(b.landmark_covariance(want_taps=True)), selection=records(b.landmark_covariance([7, 3, 3, 0], want_taps=True)))
    b.close()
elif kind == "predicted" and name in LANDMARK:
    w, Q, _ = pc.queries(name)
    b = solver.WindowBatch([w])
    rec = dict(queries=records(b.predicted_measurement([Q], want_taps=True)))
    b.close()
elif name == "mixed":   # the windows of each entry's test_a_mixed_range_has_the_bits_of_the_single_calls
    if kind == "state":
        names, sels = ("A", "C", "D"), ("newest", "first+newest", "sb")
        blocks = [cc.selections(n)[s] for n, s in zip(names, sels)]
        b = solver.WindowBatch([cc.window(n) for n in names])
        rec = dict(whole=records(b.state_covariance(blocks, want_S0=True)), tail=records(b.state_covariance(blocks[1:], w0=1, n=2)))
    elif kind == "landmark":
        b = solver.WindowBatch([lc.window(n) for n in ("A", "C", "H", "U", "F")])
        rec = dict(whole=records(b.landmark_covariance(want_taps=True)), middle=records(b.landmark_covariance(w0=1, n=3)),
                   selections=records(b.landmark_covariance([[1, 0], None, [29, 29], [lc.NO_PAIRS, 6], [59]])))
    else:
        cases = [pc.queries(n) for n in ("A", "C", "H", "U", "F")]
        Qs = [c[1] for c in cases]
        b = solver.WindowBatch([c[0] for c in cases])
        rec = dict(whole=records(b.predicted_measurement(Qs, want_taps=True)), middle=records(b.predicted_measurement(Qs[1:4], w0=1, n=3)))
    b.close()
elif name == "singular":   # each entry's test_a_singular_window_fails_alone
    if kind == "state":
        blocks = [cc.selections("A")["newest"], [(cc.POSE, 3), (cc.SB, 3)], cc.selections("B")["newest"]]
        b = solver.WindowBatch([cc.window("A"), cc.singular_window(), cc.window("B")])
        rec = dict(results=with_results_of_the_error(lambda: b.state_covariance(blocks, want_S0=True)))
    elif kind == "landmark":
        b = solver.WindowBatch([cc.window("A"), cc.singular_window(), cc.window("B")])
        rec = dict(results=with_results_of_the_error(lambda: b.landmark_covariance(want_taps=True)))
    else:
        (wA, QA, _), (wB, QB, _) = pc.queries("A"), pc.queries("B")
        Qs = np.array([[l, 3, 4 + l % 2, l % 2] for l in range(40)], np.int32)
        b = solver.WindowBatch([wA, cc.singular_window(), wB])
        rec = dict(results=with_results_of_the_error(lambda: b.predicted_measurement([QA, Qs, QB], want_taps=True)))
    b.close()
else:
    raise KeyError(args.case)
json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
