"""The windows and selections of the state-covariance referee — TEST INFRASTRUCTURE, host only.  tests/test_state_covariance_host.py
proves on the CPU that these inputs can tell the right definition from wrong ones; tests/test_gpu_state_covariance.py compares
the kernel on them.

    A  small_window(seed=1, K=4, L=40)                                   D = 60
    B  small_window(seed=3, K=4, L=60, estimate_extrinsics="shared")     D = 72
    C  small_window(seed=4, K=3, L=60, estimate_extrinsics="perframe")   D = 81, not a multiple of 2 or 16
    D  make_window(10, 120, 1.0, seed=5)                                 D = 150
    E  A with the marginalisation prior of test_gpu_parity.py::test_marginalisation_prior_evaluation   D = 60
    F  12 keyframes with the first pose fixed                            D = 174, the limit
    G  12 keyframes, nothing fixed                                       D = 180, one block over (OKVIS_BA_ERR_UNSUPPORTED)

Selections (lists of (block type, index), 0 = pose-type, 1 = speed/bias): the newest state (15 rows), one pose (6), one
speed/bias block (9), first and newest state together (30), the same two states newest first, and for B and C an extrinsics block
together with a pose.  References are computed once per process and shared (reference())."""
from __future__ import annotations

import copy

import numpy as np

from okvis_amd import synthetic

from . import cov_statement as cs

POSE, SB = 0, 1
BOUND_FACTOR = 4.0          # the project's margin over an independent fp64 evaluation
E_REF_MAX = 1e-4            # condition on the inputs: no bound ever exceeds BOUND_FACTOR x this
MUTATION_MARGIN = 100.0     # a wrong definition moves Sigma by more than this x e_ref
OPT_ITERS = 5


def _prior(w, seed=32):
    """the synthetic dense prior of test_gpu_parity.py::test_marginalisation_prior_evaluation over pose 0, speed/bias 0, pose 1"""
    rng = np.random.default_rng(seed)
    Dm = 6 + 9 + 6
    A = rng.standard_normal((Dm, Dm))
    w.marg_J = np.triu(A) * 3.0
    w.marg_e0 = rng.standard_normal(Dm) * 0.1
    w.marg_block_type = np.array([0, 1, 0], np.int32)
    w.marg_block_idx = np.array([0, 0, 1], np.int32)
    w.marg_block_off = np.array([0, 6, 15], np.int32)
    lin = np.zeros((3, 9))
    lin[0, :7] = synthetic.pose_oplus(w.pose[0], rng.normal(0, 0.02, 6))
    lin[1] = w.sb[0] + rng.normal(0, 0.01, 9)
    lin[2, :7] = synthetic.pose_oplus(w.pose[1], rng.normal(0, 0.02, 6))
    w.marg_lin = lin
    return w


def _twelve(fix_first):
    w = synthetic.make_window(12, 60, 0.7, seed=6)
    if fix_first:
        w.pose_fixed = np.asarray(w.pose_fixed).copy()
        w.pose_fixed[0] = 1
    return w


def no_prior(w):
    """w without its marginalisation prior (a mutation)"""
    w = copy.deepcopy(w)
    w.marg_J, w.marg_e0, w.marg_lin = np.zeros((0, 0)), np.zeros(0), np.zeros((0, 9))
    w.marg_block_type = w.marg_block_idx = w.marg_block_off = np.zeros(0, np.int32)
    return w


def singular_window():
    """no IMU terms and no speed/bias prior: the speed/bias rows of S0 are exactly zero"""
    w = synthetic.make_window(4, 40, 0.7, seed=1, with_imu=False)
    w.sbprior_sb, w.sbprior_meas, w.sbprior_sqrtinfo = np.zeros(0, np.int32), np.zeros((0, 9)), np.zeros((0, 81))
    return w


MAKE = {
    "A": lambda: synthetic.small_window(seed=1, K=4, L=40),
    "B": lambda: synthetic.small_window(seed=3, K=4, L=60, estimate_extrinsics="shared"),
    "C": lambda: synthetic.small_window(seed=4, K=3, L=60, estimate_extrinsics="perframe"),
    "D": lambda: synthetic.make_window(10, 120, 1.0, seed=5),
    "E": lambda: _prior(synthetic.small_window(seed=1, K=4, L=40)),
    "F": lambda: _twelve(True),
    "G": lambda: _twelve(False),
}
DIM = dict(A=60, B=72, C=81, D=150, E=60, F=174, G=180)
KEYFRAMES = dict(A=4, B=4, C=3, D=10, E=4, F=12, G=12)
CASES = ("A", "B", "C", "D", "E", "F")      # the windows the kernel serves


def window(name):
    return MAKE[name]()


def selections(name):
    K = KEYFRAMES[name]
    first = 1 if name == "F" else 0          # (F: pose 0 is fixed)
    sel = {
        "newest": [(POSE, K - 1), (SB, K - 1)],
        "pose": [(POSE, 1)],
        "sb": [(SB, K - 2)],
        "first+newest": [(POSE, first), (SB, first), (POSE, K - 1), (SB, K - 1)],
        "newest+first": [(POSE, K - 1), (SB, K - 1), (POSE, first), (SB, first)],
    }
    if name in ("B", "C"):
        sel["ext+pose"] = [(POSE, K), (POSE, 1)]     # (the pose-type blocks behind the K body poses are the extrinsics)
    return sel


def columns(name, w):
    """C: the union of the rows any selection of the case names, ascending"""
    rows = set()
    for blocks in selections(name).values():
        rows |= set(int(r) for r in cs.rows_of(w, blocks))
    return np.array(sorted(rows), np.int64)


class Inverse:
    """the block C x C of the inverse of one matrix: by mpmath (X), by the two fp64 host routes, and their distances from X"""

    def __init__(self, S, cols, host=True):
        self.cols = np.asarray(cols)
        self.X = cs.inverse_block_mp(S, cols)
        if host:
            self.chol, self.lu = cs.host_inverses(np.asarray(S, np.float64), cols)
            self.e_chol, self.e_lu = cs.e(self.chol, self.X), cs.e(self.lu, self.X)
            self.e_ref = max(self.e_chol, self.e_lu)

    def block(self, rows):
        """rows x rows of X (rows a subset of C, any order)"""
        at = np.searchsorted(self.cols, rows)
        assert np.array_equal(self.cols[at], rows)
        return self.X[np.ix_(at, at)]

    def cut(self, Y, rows):
        at = np.searchsorted(self.cols, rows)
        return np.asarray(Y)[np.ix_(at, at)]


_cache = {}


def reference(oracle, name, optimized=False, extended=False):
    """(window, columns C, S0 in long double, Inverse of it) of the oracle's statement for a case — the fp64 build's arrays, at the
    uploaded state or after optimize(OPT_ITERS), or (extended) the long double build's at the uploaded state"""
    key = (name, bool(optimized), bool(extended))
    if key not in _cache:
        assert not (optimized and extended), "the long double oracle re-preintegrates through set_state: another linearisation rule"
        w = window(name)
        lin = cs.linearized(oracle, w, extended=extended, optimize=OPT_ITERS if optimized else 0)
        S0 = cs.S0_of(w, lin)
        C = columns(name, w)
        _cache[key] = (w, C, S0, Inverse(S0, C), lin)
    return _cache[key]
