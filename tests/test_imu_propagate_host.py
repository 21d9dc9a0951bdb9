"""CPU: the yardstick, the fixture and the statement of okvis_fe_imu_propagate (cases and limits: tests/imu_propagate_cases.py).

  - the yardstick holds: on every covered call of the cases the COMPILED REFERENCE (oracle/_ref, where it is built) lies within
    4 * max(e_oracle, n_steps * 2^-52) of the long double referee, array by array, and oracle, referee and reference return the
    same count; the oracle and the referee are checked against the recorded reference where oracle/_ref is absent;
  - tests/golden/imu_propagation.npz holds the cases' inputs as the generator makes them today, and the reference's outputs as
    the reference computes them today (where oracle/_ref is built);
  - case 5 pins the reference's saturation quirk (x100 on the accelerometer's variance, x10^4 on the gyroscope's) against the
    reference's output;
  - the step functions the kernel is made of (okvis_amd/csrc/fe_propagate.hpp), compiled for the host without contraction and driven
    lane by lane (tests/propagate_probe.cpp), meet the limit the device is held to;
  - the header declares the entry and the built library exports it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_propagate_cases as IC  # noqa: E402
import ref_lib  # noqa: E402

HAVE_REF = ref_lib.available()


def covered_calls():
    """(spec, k, start, end, the recorded reference's inputs T, sb) of every covered call of cases 1-8"""
    for s in IC.specs():
        rec = IC.golden_chain(s)
        T, sb = s["T_WS"], s["sb"]
        for k, t0, t1 in IC.calls(s):
            if IC.covered(s, t1):
                yield s, k, t0, t1, T, sb
            T, sb = rec[k]["T_WS"], rec[k]["sb"]


def test_the_reference_lies_within_the_yardstick():
    n = 0
    for s, k, t0, t1, T, sb in covered_calls():
        ref, limit = IC.judge(s, T, sb, t0, t1)
        got = IC.call(ref_lib.lib().ref_imu_propagation, s, T, sb, t0, t1) if HAVE_REF else IC.golden_chain(s)[k]
        assert got["count"] == ref["count"], (s["name"], k)
        for a in IC.ARRAYS:
            e = IC.error(got[a], ref[a])
            print(f"{s['name']}[{k}] {a}: reference {e:.2e} limit {limit[a]:.2e}")
            assert e <= limit[a], (s["name"], k, a, e, limit[a])
        n += 1
    assert n == 5 + 3 + 10 + 10 + 1 + 1 + 1


def test_edge_counts_of_oracle_referee_and_reference():
    s = IC.by_name("uncovered")
    rec = IC.golden_chain(s)
    assert [r["count"] for r in rec] == [5, -1, -1]
    for fn in (IC.referee, IC.oracle):
        r = fn(s, rec[0]["T_WS"], rec[0]["sb"], s["ends"][0], s["ends"][1])
        assert r["count"] == -1 and r["T_WS"].tobytes() == rec[0]["T_WS"].tobytes() and r["sb"].tobytes() == rec[0]["sb"].tobytes()
    assert rec[1]["T_WS"].tobytes() == rec[0]["T_WS"].tobytes() == rec[2]["T_WS"].tobytes()
    assert [r["count"] for r in IC.golden_chain(IC.by_name("one_sample"))] == [0, 0]


def test_fixture_inputs_are_the_generators():
    g = IC.golden()
    for name, (t, gyr, acc) in IC.streams().items():
        assert np.array_equal(g[f"stream/{name}/t"], t) and g[f"stream/{name}/gyr"].tobytes() == gyr.tobytes()
        assert g[f"stream/{name}/acc"].tobytes() == acc.tobytes()
    assert np.array_equal(g["params"], [[p.sigma_g_c, p.sigma_a_c, p.sigma_gw_c, p.sigma_aw_c, p.g, p.g_max, p.a_max] for p in IC.PARAMS])
    for s in IC.specs():
        n = s["name"]
        assert list(g[f"{n}/deque"]) == [s["s_begin"], s["s_count"], s["flags"], s["prm"], s["case"]]
        assert list(g[f"{n}/times"]) == [s["t_start"]] + s["ends"]
        assert g[f"{n}/T_WS0"].tobytes() == s["T_WS"].tobytes() and g[f"{n}/sb0"].tobytes() == s["sb"].tobytes()
    assert os.path.getsize(IC.GOLDEN) < 1 << 20


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref is not built and the reference tree is not here")
def test_fixture_outputs_are_what_the_reference_computes():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_imu_propagation_golden as M
    now, g = M.record(), IC.golden()
    assert now.keys() == g.keys()
    for k in g:
        assert np.asarray(now[k]).shape == g[k].shape and np.asarray(now[k]).tobytes() == g[k].tobytes(), k


def test_saturation_quirk_is_the_references():
    """A saturated step multiplies the LOCAL sigma by 100 (ImuError.cpp:369-389).  The gyroscope's variance takes the local sigma
    twice (x 10^4, :434), the speed's takes it once and the parameter's once (x 100, :438).  The restatement with the quirk meets
    the reference's recorded covariance within the yardstick; and the size of the quirk is read off that record: against the same
    call with one sensor's limit lifted (same F_delta in every step, so the difference obeys D <- F D F^T + dQ, and F_delta leaves
    the alpha-alpha and v-v blocks of such a D alone) the block's trace grows by exactly the noise the saturated steps add."""
    import dataclasses
    s = IC.by_name("saturated")
    sat = IC.golden_chain(s)[0]
    ref, limit = IC.judge(s, s["T_WS"], s["sb"], s["t_start"], s["ends"][0])
    assert sat["count"] == ref["count"] == 11
    assert IC.error(sat["cov"], ref["cov"]) <= limit["cov"]
    p, dt = IC.PARAMS[0], IC.DT * 1e-9
    args = (s["T_WS"], s["sb"], s["t_start"], s["ends"][0])
    no_g = IC.referee(dict(s, params=dataclasses.replace(p, g_max=1e3)), *args)["cov"]
    no_a = IC.referee(dict(s, params=dataclasses.replace(p, a_max=1e3)), *args)["cov"]
    # samples 45 and 47 each sit in two steps (as the second sample and as the first): two saturated steps per sensor
    d_alpha = np.trace((sat["cov"] - no_g)[3:6, 3:6])
    d_v = np.trace((sat["cov"] - no_a)[6:9, 6:9])
    assert np.isclose(d_alpha, 3 * 2 * dt * p.sigma_g_c ** 2 * (100.0 ** 2 - 1), rtol=1e-9, atol=0)
    assert np.isclose(d_v, 3 * 2 * dt * p.sigma_a_c ** 2 * (100.0 - 1), rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("probe") / "libpropagate_probe.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "propagate_probe.cpp"),
                           "-o", so])
    return C.CDLL(so).probe_imu_propagation


def test_the_step_functions_meet_the_device_limit_on_the_host(probe):
    n = 0
    for s, k, t0, t1, T, sb in covered_calls():
        ref, limit = IC.judge(s, T, sb, t0, t1)
        got = IC.call(probe, s, T, sb, t0, t1)
        assert got["count"] == ref["count"] == IC.golden_chain(s)[k]["count"]
        for a in IC.ARRAYS:
            e = IC.error(got[a], ref[a])
            print(f"{s['name']}[{k}] {a}: probe {e:.2e} limit {limit[a]:.2e}")
            assert e <= limit[a], (s["name"], k, a, e, limit[a])
        assert jac_structure(got["jac"])
        n += 1
    assert n == 31


def jac_structure(jac):
    """the entries of F that setIdentity() sets and no block assignment overwrites (ImuError.cpp:480-491) are exactly 0 and 1"""
    written = np.zeros((15, 15), bool)
    for r, c in ((0, 3), (0, 6), (0, 9), (0, 12), (3, 9), (6, 3), (6, 9), (6, 12)):
        written[r:r + 3, c:c + 3] = True
    return np.array_equal(jac[~written], np.eye(15)[~written])


def test_header_declares_and_library_exports_the_entry():
    text = open(os.path.join(ROOT, "include", "okvis_amd_frontend.h")).read()
    assert "int okvis_fe_imu_propagate(okvis_fe_context* ctx" in text and "typedef struct okvis_fe_imu_job" in text
    from okvis_amd import _lib, frontend
    assert "okvis_fe_imu_propagate" in frontend.SYMBOLS
    assert hasattr(_lib.lib(), "okvis_fe_imu_propagate")
    assert C.sizeof(frontend.ImuJobC) == 160
