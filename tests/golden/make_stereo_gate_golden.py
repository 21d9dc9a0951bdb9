"""Records tests/golden/stereo_gate.npz: for the cases of tests/tri_cases.py that the reference build can run (in_golden), the inputs
and what the reference's own ProbabilisticStereoTriangulator and camera classes return for them (ref_fe_* of oracle/_ref through
tests/ref_lib.py).  Data only; run on a machine with the reference build:  python tests/golden/make_stereo_gate_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_lib as R  # noqa: E402
import tri_cases as TC  # noqa: E402
from okvis_amd import frontend as F  # noqa: E402


def main():
    ref = F.Frontend(api=(R.lib(), "ref_fe_"))
    out = {}
    for name, case in TC.cases().items():
        if not TC.in_golden(case):
            continue
        for k, v in TC.arrays(case).items():
            out[f"{name}/in/{k}"] = v
        for k, v in TC.call(ref, F.camera, case, gn=False).items():
            out[f"{name}/ref/{k}"] = v
    path = os.path.join(ROOT, "tests", "golden", "stereo_gate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len({k.split("/")[0] for k in out}), "cases")


if __name__ == "__main__":
    main()
