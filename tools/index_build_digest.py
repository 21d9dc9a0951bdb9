#!/usr/bin/env python3
"""Digest of the index build (okvis_amd/csrc/capi_index_build.inc) over a fixed list of windows x option sets: host only.

For every case the SHA-256 of the arena okvis_ba_check_window builds (OKVIS_BA_DEBUG=arena=<file>: the arena's bytes and the WinPtrs
record behind them) and of every list okvis_ba_check_window_lists hands out, for the window alone and as one of 64.  Two trees
whose digests are equal build the same bytes for every branch the list reaches; each case asserts, through the statistics and the
PIECE_PATH / CHAIN / LDL_COMP lists, that it takes the branch it is there for.

    python tools/index_build_digest.py out.json [--root TREE]      (TREE: the checkout whose okvis_amd is used, default this one)
"""
import argparse
import copy
import hashlib
import json
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
dump = tempfile.NamedTemporaryFile(suffix=".arena", delete=False).name
os.environ["OKVIS_BA_DEBUG"] = "arena=" + dump     # (read once, when the library is loaded)
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402

from okvis_amd import solver, synthetic  # noqa: E402
from okvis_amd.window import (SOLVE_CHAIN, SOLVE_DENSE, STRATEGY_LM, TUNE_H0_ON_HOST, TUNE_LDL_COMP_ALL, TUNE_NO_LDL_COMP,  # noqa: E402
                              default_options, set_options)


def repeat_observations(w, times):
    """Every observation `times` times, every fifth and seventh dropped again (tests/test_index_build.py): runs of every length"""
    keep = None
    for n in ("obs_lm", "obs_pose", "obs_ext", "obs_cam", "obs_uv", "obs_sqrtw"):
        a = np.repeat(np.asarray(getattr(w, n)), times, axis=0)
        if keep is None:
            keep = (np.arange(len(a)) % 5 != 3) & (np.arange(len(a)) % 7 != 2)
        setattr(w, n, a[keep])
    return w


def with_prior(w, blocks, seed):
    """A dense marginalisation prior over blocks [(type, index)] (0 pose, 1 speed/bias), upper triangular J"""
    rng = np.random.default_rng(seed)
    dims = [6 if t == 0 else 9 for t, _ in blocks]
    Dm = sum(dims)
    w.marg_J = np.triu(rng.standard_normal((Dm, Dm))) * 3.0
    w.marg_e0 = rng.standard_normal(Dm) * 0.1
    w.marg_block_type = np.array([t for t, _ in blocks], np.int32)
    w.marg_block_idx = np.array([i for _, i in blocks], np.int32)
    w.marg_block_off = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(np.int32)
    lin = np.zeros((len(blocks), 9))
    for k, (t, i) in enumerate(blocks):
        lin[k, :7 if t == 0 else 9] = w.pose[i] if t == 0 else w.sb[i]
    w.marg_lin = lin
    return w


def long_track():
    """Landmarks with more than LIN2_PIECES (128) pieces and at most 256 observations: 80 frames, all but six blocks fixed"""
    w = synthetic.make_window(80, 12, 1.0, 5, frame_dt=0.05)
    w.pose_fixed = np.array([0] * 6 + [1] * (w.n_pose - 6), np.uint8)
    w.sb_fixed = np.array([0] * 6 + [1] * (w.n_sb - 6), np.uint8)
    return repeat_observations(w, 2)


def no_priors():
    w = synthetic.small_window(seed=41, K=5, L=60)
    w.pprior_pose, w.pprior_meas, w.pprior_sqrtinfo = np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros((0, 36))
    w.sbprior_sb, w.sbprior_meas, w.sbprior_sqrtinfo = np.zeros(0, np.int32), np.zeros((0, 9)), np.zeros((0, 81))
    return w


A = synthetic.config_A
frame = lambda: synthetic.make_window(8, 430, 0.5, seed=20240924)   # noqa: E731  (bench.py's frame_host: the replay's size)
small = lambda: synthetic.small_window(seed=41, K=5, L=60)          # noqa: E731
large = lambda: synthetic.make_window(20, 30, 1.0, 2, frame_dt=0.1)  # noqa: E731  (D = 300 > MAX_D_LDS)
prior30 = lambda: with_prior(synthetic.small_window(seed=6, K=5, L=70), [(0, 0), (1, 0), (0, 1), (1, 1)], 6)   # noqa: E731
prior150 = lambda: with_prior(A(), [(0, i) for i in range(10)] + [(1, i) for i in range(10)], 7)              # noqa: E731
opt = lambda strategy=None, **kw: set_options(default_options(strategy), **kw)                                   # noqa: E731

# name -> (window, options, what the single-window build must show: keys of check())
CASES = {
    "A": (A, opt(), dict(piece_path=1, chain=10)),
    "frame": (frame, opt(), dict(piece_path=1)),
    "sparse": (lambda: A(visibility=0.35, seed=3), opt(), dict(piece_path=1)),
    "shared_ext": (lambda: synthetic.small_window(seed=11, K=5, L=80, estimate_extrinsics="shared"), opt(), dict(piece_path=0)),
    "perframe_ext": (lambda: synthetic.small_window(seed=12, K=5, L=80, estimate_extrinsics="perframe"), opt(), dict(piece_path=0)),
    "long_track": (long_track, opt(), dict(piece_path=0, max_track_over=128)),
    "repeated_obs": (lambda: repeat_observations(synthetic.small_window(seed=8, K=6, L=50, visibility=0.6), 3), opt(), dict(piece_path=1)),
    "A_chain": (A, opt(tuning_solve_mode=SOLVE_CHAIN), dict(chain=10)),
    "A_dense": (A, opt(tuning_solve_mode=SOLVE_DENSE), dict(chain=0, ldl_comp=1 << 5)),
    "small_auto": (small, opt(), dict(chain=0)),
    "small_chain": (small, opt(tuning_solve_mode=SOLVE_CHAIN), dict(chain=5, ldl_comp=1)),
    "small_dense": (small, opt(tuning_solve_mode=SOLVE_DENSE), dict(chain=0, ldl_comp=0b1100)),
    "large": (large, opt(), dict(D=300, chain=0, ldl_comp=0, Dp_over=96)),
    "prior30": (prior30, opt(tuning_solve_mode=SOLVE_CHAIN), dict(chain=5)),
    "prior30_h0_host": (prior30, opt(tuning_solve_mode=SOLVE_CHAIN, tuning_flags=TUNE_H0_ON_HOST), dict(same_arena_as="prior30")),
    "prior150": (prior150, opt(), dict(chain=0)),
    "prior150_h0_host": (prior150, opt(tuning_flags=TUNE_H0_ON_HOST), dict(other_arena_than="prior150")),
    "no_imu": (lambda: synthetic.small_window(seed=5, K=5, L=60, with_imu=False), opt(), dict(n_imu=0)),
    "no_priors": (no_priors, opt(tuning_solve_mode=SOLVE_DENSE), dict(ldl_comp=0)),
    "fp32": (A, opt(fp32_linearize=1), dict(piece_path=1)),
    "lm_strategy": (A, opt(STRATEGY_LM), dict(other_arena_than="A")),
    "reserved0_bit2": (A, opt(reserved0=4), dict(piece_path=1, other_arena_than="A")),
    "reserved0_bit3": (A, opt(reserved0=8), dict(piece_path=0)),
    "reserved0_bits23": (A, opt(reserved0=12), dict(piece_path=0)),
    "debug_arrays_1": (A, opt(debug_arrays=1), dict(arena_over="A")),
    "debug_arrays_2": (A, opt(debug_arrays=2), dict(arena_over="A")),
    "group_lm_64": (frame, opt(tuning_group_lm=64), dict(groups_under="frame")),
    "group_lm_8": (frame, opt(tuning_group_lm=8), dict(groups_over="frame")),
    "group_work_250": (A, opt(tuning_group_work=250), dict(groups_over="A")),
    "schur_lm_24": (A, opt(schur_lm_per_block=24), dict(chunks_under_groups=True)),
    "split_small_1": (A, opt(tuning_split_small_min=1), dict(piece_path=1)),
    "no_ldl_comp": (A, opt(tuning_flags=TUNE_NO_LDL_COMP), dict(ldl_comp=0)),
    "ldl_comp_all": (A, opt(tuning_flags=TUNE_LDL_COMP_ALL), dict(ldl_comp=0xFFFFFFFF)),
}


def sha(b):
    return hashlib.sha256(b).hexdigest()


out = {}
for name, (make, o, want) in CASES.items():
    w = make()
    st = solver.check_window(copy.deepcopy(w), o)
    rec = dict(stats={k: int(v) for k, v in st.items()}, arena_sha256=sha(open(dump, "rb").read()), lists={})
    for n_windows in (1, 64):
        L = solver.index_lists(w, o, n_windows)
        rec["lists"][str(n_windows)] = {k: (sha(np.ascontiguousarray(v, np.int32).tobytes()) if isinstance(v, np.ndarray) else int(v))
                                        for k, v in L.items()}
        if n_windows == 1:
            L1 = L
    out[name] = rec
    # ---- the case takes the branch it is there for ----
    for k, v in want.items():
        if k in ("piece_path", "chain", "ldl_comp"):
            assert L1[k] == v, (name, k, L1[k], v)
        elif k == "D":
            assert st["D"] == v, (name, st)
        elif k == "Dp_over":
            assert st["Dp"] > v, (name, st)   # several Schur tiles
        elif k == "n_imu":
            assert w.n_imu == v
        elif k == "max_track_over":   # no free extrinsics, yet not the piece path: a landmark with too many pieces
            assert not np.any(np.asarray(w.pose_fixed)[np.asarray(w.obs_ext)] == 0) and np.bincount(w.obs_lm).max() > v
        elif k == "same_arena_as":
            assert rec["arena_sha256"] == out[v]["arena_sha256"], (name, v)
        elif k == "other_arena_than":
            assert rec["arena_sha256"] != out[v]["arena_sha256"], (name, v)
        elif k == "arena_over":
            assert st["arena_bytes"] > out[v]["stats"]["arena_bytes"], (name, v)
        elif k == "groups_under":
            assert st["n_group"] < out[v]["stats"]["n_group"], (name, v)
        elif k == "groups_over":
            assert st["n_group"] > out[v]["stats"]["n_group"], (name, v)
        elif k == "chunks_under_groups":
            assert st["n_chunk"] < st["n_group"], (name, st)
        else:
            raise KeyError(k)
os.unlink(dump)
json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
print(f"{len(out)} cases -> {args.out}: sha256 {sha(open(args.out, 'rb').read())}")
