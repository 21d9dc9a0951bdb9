"""Record tests/golden/imu_propagation.npz: the inputs of the cases of tests/imu_propagate_cases.py (the three sample streams and,
per spec, its deque, times, start state, flags and parameter set) and what the COMPILED REFERENCE (oracle/_ref, ImuError::propagation
itself) returns for every call of every chain, each call from the state the call before it returned.  Data only.

    python tests/golden/make_imu_propagation_golden.py          (needs oracle/_ref, i.e. the reference tree at build time)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_propagate_cases as IC  # noqa: E402
import ref_lib  # noqa: E402


def record():
    out = {}
    for name, (t, g, a) in IC.streams().items():
        out[f"stream/{name}/t"], out[f"stream/{name}/gyr"], out[f"stream/{name}/acc"] = t, g, a
    out["params"] = np.array([[p.sigma_g_c, p.sigma_a_c, p.sigma_gw_c, p.sigma_aw_c, p.g, p.g_max, p.a_max] for p in IC.PARAMS])
    fn = ref_lib.lib().ref_imu_propagation
    for s in IC.specs():
        n = s["name"]
        out[f"{n}/deque"] = np.array([s["s_begin"], s["s_count"], s["flags"], s["prm"], s["case"]], np.int64)
        out[f"{n}/times"] = np.array([s["t_start"]] + s["ends"], np.int64)
        out[f"{n}/T_WS0"], out[f"{n}/sb0"] = s["T_WS"], s["sb"]
        chain = IC.chain(fn, s)
        out[f"{n}/count"] = np.array([r["count"] for r in chain], np.int32)
        for a in IC.ARRAYS:
            out[f"{n}/{a}"] = np.stack([r[a] for r in chain])
    return out


if __name__ == "__main__":
    assert ref_lib.available(), "oracle/_ref is not built and the reference tree is not here"
    np.savez_compressed(IC.GOLDEN, **record())
    print(IC.GOLDEN, os.path.getsize(IC.GOLDEN), "bytes")
