"""Phase stamps of Schur workgroup 0 of window 0 (SSTAMP 16..23, ba_schur2.hpp) under the load of bench.py's batch: 64 bench windows,
Gauss-Newton, eager launches, debug_arrays = 2; median / min / max over 25 launches.

    python tools/gpu_schur_stamps_64.py [TREE [TUNING_FLAGS]]     (TREE: the checkout whose okvis_amd is used, default this one;
                                                                    0x200 = OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from okvis_amd import solver, synthetic
from okvis_amd.window import default_options
opt = default_options(); opt.gauss_newton = 1
opt.function_tolerance = opt.gradient_tolerance = opt.parameter_tolerance = 0.0
opt.use_graph = 0; opt.debug_arrays = 2
opt.tuning.flags = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0
b = solver.WindowBatch([synthetic.make_window(10, 400, 1.0, 20240923 + i) for i in range(64)], options=opt)
print(sys.argv[1] if len(sys.argv) > 1 else "this tree", "route", b.launch_route())
b.begin(); b.iterate(6); b.synchronize()
rows = []
for _ in range(25):
    b.iterate(1); b.synchronize()
    p = np.array(b.array("PROF"))
    rows.append([(p[k] - p[k - 1]) / 2100.0 for k in range(17, 24)] + [(p[23] - p[16]) / 2100.0])
rows = np.array(rows)
names = ["head", "V^-1 (first data)", "first fill + list sums", "first products", "rest of the chunk", "accumulators -> LDS", "partial stores", "total"]
for j, n in enumerate(names):
    print(f"  {n:26s} median {np.median(rows[:, j]):6.2f}  min {rows[:, j].min():6.2f}  max {rows[:, j].max():6.2f} us")
b.finish(); b.close()
