"""GPU: okvis_fe_imu_propagate against the long double referee, call by call (cases and limits: tests/imu_propagate_cases.py).

Every call of a chain is judged on its own: the referee gets the DEVICE's carried state of the previous end, and each requested
array has to lie within 4 * max(e_oracle, n_steps * 2^-52) of it (error = max-abs difference over max-abs of the referee's array).
The counts are the compiled reference's, recorded in tests/golden/imu_propagation.npz."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_propagate_cases as IC  # noqa: E402
import sac_cases  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402

pytestmark = pytest.mark.gpu
OUT = ("T_WS", "sb", "count", "cov", "jac")
ERR_ARG = -1


def run(spec_list, fe=None):
    """one call for the jobs of spec_list -> per job a list (one entry per end) of dict(T_WS, sb, count, cov, jac); rows nobody
    wrote hold NaN"""
    own = fe is None
    fe = F.Frontend() if own else fe
    s_t, s_gyr, s_acc, ends, jobs = IC.pool(spec_list)
    res = fe.imu_propagate(IC.PARAMS, s_t, s_gyr, s_acc, jobs, ends)
    if own:
        fe.close()
    return [[dict(zip(OUT, (a[j["e_begin"] + k] for a in res))) for k in range(j["e_count"])] for j in jobs]


@functools.lru_cache(maxsize=None)
def batch_result():
    return run(IC.batch())


def same(x, y):
    return all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in OUT)


def unwritten(a):
    return bool(np.isnan(a).all())


def check_job(spec, got):
    """every covered call of one job against the referee, from the device's own carried state; -> the number of calls judged"""
    rec = IC.golden_chain(spec)
    T, sb, n = spec["T_WS"], spec["sb"], 0
    for k, t0, t1 in IC.calls(spec):
        g = got[k]
        assert g["count"] == rec[k]["count"], (spec["name"], k)
        if IC.covered(spec, t1):
            ref, limit = IC.judge(spec, T, sb, t0, t1)
            assert g["count"] == ref["count"]
            wanted = ["T_WS", "sb"] + (["cov"] if spec["flags"] & IC.COV else []) + (["jac"] if spec["flags"] & IC.JAC else [])
            for a in wanted:
                e = IC.error(g[a], ref[a])
                print(f"{spec['name']}[{k}] {a}: device {e:.2e} limit {limit[a]:.2e}")
                assert e <= limit[a], (spec["name"], k, a, e, limit[a])
            if spec["flags"] & IC.JAC:
                assert jac_structure(g["jac"]), (spec["name"], k)
            n += 1
        ran = g["count"] >= 0 and spec["s_count"] >= 2     # the call got past the early returns
        assert unwritten(g["cov"]) == (not (spec["flags"] & IC.COV and ran)), (spec["name"], k)
        assert unwritten(g["jac"]) == (not (spec["flags"] & IC.JAC and ran)), (spec["name"], k)
        T, sb = g["T_WS"], g["sb"]
    return n


def jac_structure(jac):
    """the entries of F that setIdentity() sets and no block assignment overwrites (ImuError.cpp:480-491) are exactly 0 and 1"""
    written = np.zeros((15, 15), bool)
    for r, c in ((0, 3), (0, 6), (0, 9), (0, 12), (3, 9), (6, 3), (6, 9), (6, 12)):
        written[r:r + 3, c:c + 3] = True
    return np.array_equal(jac[~written], np.eye(15)[~written])


def test_cases_1_to_6_meet_the_limit_call_by_call():
    specs = [s for s in IC.specs() if s["case"] <= 6]
    got = run(specs)
    assert sum(check_job(s, g) for s, g in zip(specs, got)) == 5 + 3 + 10 + 10 + 1 + 1


def test_mixed_batch_meets_the_limit_call_by_call():
    specs, got = IC.batch(), batch_result()
    assert len(specs) == 130 and {s["flags"] for s in specs} == {0, 1, 2, 3} and {s["prm"] for s in specs} == {0, 1}
    assert {s["case"] for s in specs} == set(range(1, 9))
    assert sum(check_job(s, g) for s, g in zip(specs, got)) > 250


def test_whole_chain_stays_with_the_referees():
    """the state after the ten calls of case 3, against the referee's own chain: 10 x the single-call limit"""
    s = IC.by_name("chain")
    got, = run([s])
    ref = IC.chain(IC.oracle_lib.lib_ld().orc_imu_propagation, s)
    e_oracle = 0.0
    T, sb = s["T_WS"], s["sb"]
    for (k, t0, t1), r in zip(IC.calls(s), ref):
        _, limit = IC.judge(s, T, sb, t0, t1)
        e_oracle = max(e_oracle, limit["T_WS"], limit["sb"])
        T, sb = r["T_WS"], r["sb"]
    for a in ("T_WS", "sb"):
        e = IC.error(got[-1][a], ref[-1][a])
        print(f"chain end {a}: device {e:.2e} limit {10 * e_oracle:.2e}")
        assert e <= 10 * e_oracle, (a, e, e_oracle)


def test_edge_counts_leave_the_state_alone():
    unc, one = IC.by_name("uncovered"), IC.by_name("one_sample")
    (a, b, c), (d, e) = run([unc, one])
    assert [a["count"], b["count"], c["count"]] == [5, -1, -1] and [d["count"], e["count"]] == [0, 0]
    for x in (b, c):       # the chain goes on from the unchanged state
        assert x["T_WS"].tobytes() == a["T_WS"].tobytes() and x["sb"].tobytes() == a["sb"].tobytes()
        assert unwritten(x["cov"]) and unwritten(x["jac"])
    assert check_job(unc, [a, b, c]) == 1
    for x in (d, e):
        assert x["T_WS"].tobytes() == one["T_WS"].tobytes() and x["sb"].tobytes() == one["sb"].tobytes()
        assert unwritten(x["cov"]) and unwritten(x["jac"])


def test_optional_outputs():
    base = [IC.by_name(n) for n in ("steps11", "chain_between", "steps101", "same_interval")]
    full = run([dict(s, flags=3) for s in base])
    for flags in (0, 1, 2):
        part = run([dict(s, flags=flags) for s in base])
        for f, p in zip(full, part):
            for x, y in zip(f, p):
                assert all(x[k].tobytes() == y[k].tobytes() for k in ("T_WS", "sb", "count"))
                assert x["cov"].tobytes() == y["cov"].tobytes() if flags & 1 else unwritten(y["cov"])
                assert x["jac"].tobytes() == y["jac"].tobytes() if flags & 2 else unwritten(y["jac"])
    # a job asks for what the call has no array for
    s_t, s_gyr, s_acc, ends, jobs = IC.pool([dict(base[0], flags=3)])
    for without in ("cov", "jac"):
        rc, arrays = raw_call(s_t, s_gyr, s_acc, ends, jobs, without=without)
        assert rc == ERR_ARG and all(untouched(a) for a in arrays.values())
    rc, arrays = raw_call(s_t, s_gyr, s_acc, ends, [dict(jobs[0], flags=0)], without="cov")   # not asked for: fine without
    assert rc == 0 and arrays["T_WS"].tobytes() == full[0][0]["T_WS"].tobytes()


def test_batch_invariance():
    specs, got = IC.batch(), batch_result()
    rev = run(specs[::-1])[::-1]
    fe = F.Frontend()
    for s, g, r in zip(specs, got, rev):
        alone, = run([s], fe)
        assert len(g) == len(r) == len(alone)
        for x, y, z in zip(g, r, alone):
            assert same(x, y) and same(x, z), s["name"]
    fe.close()


# ------------------------------------------------------------------------------------------------ argument errors

def raw_call(s_t, s_gyr, s_acc, ends, jobs, fe=None, without=None, n_params=None, n_samples=None, n_ends=None, null=()):
    """the entry through ctypes, the outputs prefilled with the byte 0x5A -> (status, the output arrays)"""
    own = fe is None
    fe = F.Frontend() if own else fe
    prm, s_t, s_gyr, s_acc, ends = F.imu_pools(IC.PARAMS, s_t, s_gyr, s_acc, ends)
    table = F.imu_job_table(jobs)
    m = len(ends)
    arrays = {"T_WS": np.empty((m, 7)), "sb": np.empty((m, 9)), "cov": np.empty((m, 225)), "jac": np.empty((m, 225)),
              "count": np.empty(m, np.int32)}
    for a in arrays.values():
        a.view(np.uint8)[...] = 0x5A
    p = {k: (None if k == without or k in null else a.ctypes.data) for k, a in arrays.items()}
    ins = {"params": C.addressof(prm), "s_t": s_t.ctypes.data, "s_gyr": s_gyr.ctypes.data, "s_acc": s_acc.ctypes.data, "ends": ends.ctypes.data}
    ins = {k: (None if k in null else v) for k, v in ins.items()}
    rc = fe._L.okvis_fe_imu_propagate(None if "ctx" in null else fe._ctx, len(IC.PARAMS) if n_params is None else n_params, ins["params"],
                                      len(s_t) if n_samples is None else n_samples, ins["s_t"], ins["s_gyr"], ins["s_acc"],
                                      m if n_ends is None else n_ends, ins["ends"], len(jobs), None if "jobs" in null else table,
                                      p["T_WS"], p["sb"], p["cov"], p["jac"], p["count"])
    if own:
        fe.close()
    return rc, arrays


def untouched(a):
    return bool((a.view(np.uint8) == 0x5A).all())


def test_argument_errors_write_nothing_and_leave_the_context_usable():
    good = [dict(IC.by_name("steps11")), dict(IC.by_name("chain_between"))]
    want = run(good)
    s_t, s_gyr, s_acc, ends, jobs = IC.pool(good)
    fe = F.Frontend()

    def rejected(what, **kw):
        a = dict(s_t=s_t, s_gyr=s_gyr, s_acc=s_acc, ends=ends, jobs=jobs)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        rc, arrays = raw_call(a["s_t"], a["s_gyr"], a["s_acc"], a["ends"], a["jobs"], fe=fe, **kw)
        assert rc == ERR_ARG, (what, rc)
        assert all(untouched(x) for x in arrays.values()), what

    def job(j, **kw):
        return [dict(x, **kw) if i == j else x for i, x in enumerate(jobs)]

    n_s, n_e = len(s_t), len(ends)
    rejected("samples outside the pool", jobs=job(1, s_count=jobs[1]["s_count"] + 1))
    rejected("negative sample range", jobs=job(0, s_begin=-1))
    rejected("pool smaller than said", n_samples=n_s - 1)
    rejected("ends outside the pool", jobs=job(1, e_count=jobs[1]["e_count"] + 1))
    rejected("negative end range", jobs=job(0, e_begin=-1))
    rejected("no ends", jobs=job(0, e_count=0))
    rejected("end pool smaller than said", n_ends=n_e - 1)
    rejected("prm out of range", jobs=job(0, prm=len(IC.PARAMS)))
    rejected("prm negative", jobs=job(0, prm=-1))
    rejected("no parameter sets", n_params=0)
    rejected("unknown flag", jobs=job(0, flags=4))
    t_bad = s_t.copy()
    t_bad[5] = t_bad[4]
    rejected("stamps not ascending", s_t=t_bad)
    e_bad = ends.copy()
    e_bad[3], e_bad[4] = ends[4], ends[3]
    rejected("ends not ascending", ends=e_bad)
    rejected("end before the start", jobs=job(0, t_start=int(ends[0]) + 1))
    rejected("deque starts after the start", jobs=job(0, t_start=int(s_t[0]) - 1))
    for name in ("ctx", "jobs", "params", "s_t", "s_gyr", "s_acc", "ends", "T_WS", "sb", "count", "cov", "jac"):
        rejected("NULL " + name, null=(name,))
    rc, arrays = raw_call(s_t, s_gyr, s_acc, ends, [], fe=fe)      # an empty call is valid and writes nothing
    assert rc == 0 and all(untouched(x) for x in arrays.values())
    after = run(good, fe)
    fe.close()
    for w, a in zip(want, after):
        for x, y in zip(w, a):
            assert same(x, y)
    assert check_job(good[0], after[0]) == 1 and check_job(good[1], after[1]) == 10


# ------------------------------------------------------------------------------------------------ next to the other entries

def test_mixed_with_sac_consensus_on_one_context():
    g = sac_cases.golden()
    sac = [sac_cases.golden_job(g, 0, name) for name in sac_cases.PROBLEMS][:2]
    small, large = [IC.by_name("steps2")], IC.batch()[:40]

    def consensus(fe):
        return [{k: np.asarray(v) for k, v in r.items()} for r in fe.sac_consensus(sac, want_scores=True)]

    steps = [lambda fe: run(small, fe), consensus, lambda fe: run(large, fe), consensus, lambda fe: run(small, fe)]
    fe = F.Frontend()                       # its staging block starts empty and moves when the large batch comes
    mixed = [step(fe) for step in steps]
    fe.close()
    for i, (step, got) in enumerate(zip(steps, mixed)):
        own = F.Frontend()
        want = step(own)
        own.close()
        if i in (1, 3):
            assert all(x.keys() == y.keys() and all(x[k].tobytes() == y[k].tobytes() for k in x) for x, y in zip(got, want)), i
        else:
            assert all(same(x, y) for gj, wj in zip(got, want) for x, y in zip(gj, wj)), i
    assert mixed[0][0][0]["count"] == 2 and int(mixed[1][0]["n_inliers"]) > 0
