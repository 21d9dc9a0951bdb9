"""Diagnostic (not a test): clock64() phase stamps of linearise group 0 of window 0, alone and under load.
usage: python tools/gpu_lin_stamps.py [n_windows] [reserved0] [tuning flags] [launches] [split_small_min]
  reserved0 bit 3 = staged kernel, bit 2 = no fused launch; tuning flags e.g. 0x400 = OKVIS_BA_TUNE_LIN_NO_RECORDS
  split_small_min = 1 gives a small batch the factors' own launch, and with it linearize2_rec_kernel (default: from 40 windows on)
Both kernels stamp their first instruction (slot 38, kept in a register until the end).  linearize2_rec_kernel (lin_records 1)
also keeps stamp 40 — every operand has been requested — in a register; in linearize2_kernel stamp 40 stands between its requests
and 41 behind the last of them.  "launch -> all requests issued" is 38 -> 40 resp. 38 -> 41."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from okvis_amd import solver, synthetic
from okvis_amd.window import default_options
opt = default_options(); opt.gauss_newton = 1; opt.function_tolerance = 0; opt.gradient_tolerance = 0; opt.parameter_tolerance = 0; opt.use_graph = 0; opt.debug_arrays = 2
NW = int(sys.argv[1]) if len(sys.argv) > 1 else 1
opt.reserved0 = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0
opt.tuning.flags = int(sys.argv[3], 0) if len(sys.argv) > 3 else 0
N = int(sys.argv[4]) if len(sys.argv) > 4 else 25
if len(sys.argv) > 5: opt.tuning.split_small_min = int(sys.argv[5])
b = solver.WindowBatch([synthetic.config_A(seed=20240923 + i) for i in range(NW)], options=opt)
route = b.launch_route()
b.begin(); b.iterate(3); b.synchronize()
P = []
for _ in range(N):   # one launch per sample: the stamps are those of the last launch
    b.iterate(1); b.synchronize()
    P.append(np.array(b.array("PROF"), dtype=float)[:64])
P = np.array(P)
ln = {41: "entry: records + index lists requested", 42: "phase A (back-substitution) + park", 43: "phase B residual/Jacobian/products",
      44: "merge + piece records | stage + barrier", 45: "C(a) per landmark", 46: "C(b) per pair", 47: "C(c) per block", 48: "barrier", 49: "-",
      50: "fused reduction", 51: "scalars"}
med = lambda a: float(np.median(a))
print(f"linearise phases of group 0 (thread 0), {NW} windows, reserved0 {opt.reserved0}, flags {opt.tuning.flags:#x}, "
      f"lin_records {route.get('lin_records')}, median of {N} launches:")
if (P[:, 38] > 0).all():
    d = P[:, 40 if route.get("lin_records") else 41] - P[:, 38]; print(f"  {'launch -> all requests issued':44s} {med(d):10.0f} cyc {med(d)/2100:8.2f} us")
    d = P[:, 42] - P[:, 38]; print(f"  {'launch -> first barrier passed':44s} {med(d):10.0f} cyc {med(d)/2100:8.2f} us")
for k in range(41, 52):
    d = P[:, k] - P[:, k - 1]; print(f"  {ln[k]:44s} {med(d):10.0f} cyc {med(d)/2100:8.2f} us")
print("  total from stamp 40", med(P[:, 51] - P[:, 40]) / 2100, "us")
if (P[:, 38] > 0).all():
    print("  total from launch  ", med(P[:, 51] - P[:, 38]) / 2100, "us")
