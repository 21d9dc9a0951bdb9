"""The windows of the landmark-covariance referee — TEST INFRASTRUCTURE, host only.  tests/test_landmark_covariance_host.py proves
on the CPU that these inputs can tell the right definition from wrong ones; tests/test_gpu_landmark_covariance.py compares the
kernels on them.  The windows A to F of tests/cov_cases.py, and

    H  small_window(seed=7, K=4, L=30, estimate_extrinsics="perframe", visibility=1.0)   D = 108, Dp = 72: every landmark touches
       12 blocks = 72 rows, more than a wave has lanes
    U  A with the observations of landmark 5 removed: one landmark without pairs

References are computed once per process and shared (reference())."""
from __future__ import annotations

import numpy as np

from okvis_amd import synthetic

from . import cov_cases as cc
from . import cov_statement as cs
from . import fp32_cases
from . import lmcov_statement as ls

NO_PAIRS = 5      # the landmark of U without observations


def _unobserved():
    w = cc.window("A")
    return fp32_cases._keep(w, np.asarray(w.obs_lm) != NO_PAIRS)


MAKE = dict(cc.MAKE)
MAKE["H"] = lambda: synthetic.small_window(seed=7, K=4, L=30, estimate_extrinsics="perframe", visibility=1.0)
MAKE["U"] = _unobserved
DIM = dict(cc.DIM, H=108, U=60)
POSE_DIM = dict(A=24, B=36, C=54, D=60, E=24, F=66, H=72, U=24)
CASES = cc.CASES + ("H", "U")            # the windows the entry serves
FULL = ("A", "B", "C", "E", "H", "U")    # the cases whose whole P is formed at 60 digits on the GPU machine (D, F: close to a minute each)


def window(name):
    return MAKE[name]()


class Reference:
    """the statement of one case on one set of arrays: terms, S0, P at 60 digits (Inverse over 0 .. Dp-1, with the fp64 host
    routes), X* [n_lm, 3, 3], and the fp64 host evaluation's distance from it, per landmark"""

    def __init__(self, w, lin):
        self.w, self.lin = w, lin
        self.Dp = ls.pose_dim(w)
        self.S0 = cs.S0_of(w, lin)
        self.inv = cc.Inverse(self.S0, np.arange(self.Dp))
        self.terms = ls.landmark_terms(w, lin["LM_V"], lin["PAIR_W"], lin["pairs"])
        self.X = ls.sigma_all(self.terms, self.inv.X)
        self.X_chol = ls.sigma_all(self.terms, self.inv.chol, "np")
        self.X_lu = ls.sigma_all(self.terms, self.inv.lu, "np")
        self.e_ref = np.maximum(ls.e(self.X_chol, self.X), ls.e(self.X_lu, self.X))      # per landmark
        self.observed = np.array([t[0].size > 0 for t in self.terms])


_cache = {}


def reference(oracle, name, optimized=False, extended=False):
    """Reference of a case on the oracle's arrays — the fp64 build's, at the uploaded state or after optimize(OPT_ITERS), or
    (extended) the long double build's at the uploaded state"""
    key = (name, bool(optimized), bool(extended))
    if key not in _cache:
        assert not (optimized and extended)
        w = window(name)
        _cache[key] = Reference(w, cs.linearized(oracle, w, extended=extended, optimize=cc.OPT_ITERS if optimized else 0))
    return _cache[key]
