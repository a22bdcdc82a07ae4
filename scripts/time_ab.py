"""One process of the alternated A/B protocol of profiles/uniform_class_ab.txt and profiles/ew2_fine_ab.txt: roofline workload, Ar
probe; fused, VdW and Coulomb builds, 3 warm-up + 10 timed launches each (HIP events), plan-creation time of the process's first and
second plan.    python scripts/time_ab.py LABEL
The library comes from CEG_HIP_LIB (an older one may lack entry points of include/ceg_hip.h: they are left unbound); the switches
CEG_HIP_UNIFORM_CLASS / CEG_HIP_EW2_FINE are read at plan creation.  Run the configurations in turn, several processes each, and
compare the per-run minima."""
import os, sys, time
here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..')]
import ctypes as C
import torch
from ceg_hip import _abi
probe = C.CDLL(os.environ.get("CEG_HIP_LIB", str(_abi.LIB_PATH)))
for name in list(_abi.PROTOTYPES):            # an older library lacks the newer entry points
    if not hasattr(probe, name):
        del _abi.PROTOTYPES[name]
from ceg_hip import workloads as W
from ceg_hip.plan import GridPlan
label = sys.argv[1]
dev = torch.device("cuda", 0)
w = W.roofline_workload("Ar", 255)
nx, ny, nz = w.cset.npoints
v = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev); c = torch.empty_like(v)
torch.cuda.synchronize()
t0 = time.perf_counter()
plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
t1 = time.perf_counter()
plan2 = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)          # memoised fit, cached image list
t2 = time.perf_counter()
plan2.close()
fine = plan._lib.ceg_plan_ew2_fine(plan._h) if "ceg_plan_ew2_fine" in _abi.PROTOTYPES else -1
print(f"{label} plan  first {1e3*(t1-t0):.2f} ms  second {1e3*(t2-t1):.2f} ms  class {plan.uniform_class} fine {fine}", flush=True)
s = torch.cuda.current_stream().cuda_stream
for mode in ("fused", "vdw", "coulomb"):
    def launch():
        if mode == "fused": plan.build_fused(v.data_ptr(), c.data_ptr(), nx * ny * nz, 0, nx, 0, 0, s)
        elif mode == "vdw": plan.build_vdw(v.data_ptr(), nx * ny * nz, 0, nx, 0, 0, s)
        else: plan.build_coulomb(c.data_ptr(), nx * ny * nz, 0, nx, 0, 0, s)
    for _ in range(3): launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(f"{label} {mode} min {min(ts):.4f} mean {sum(ts)/len(ts):.4f} all {' '.join('%.4f' % t for t in ts)}", flush=True)
plan.close()
