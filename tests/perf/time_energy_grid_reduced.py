"""Timing of ``ceg_energy_grid_reduced`` (energy_grid collapsed over its rotation axis on the device) against the route it replaces:
``ceg_energy_grid`` into a host array followed by ``mean_boltzmann`` + ``min`` in NumPy.

Workload of profiles/energy_grid.txt: CO2 in CHA_1.4_3b4eeb96, step 0.3 A (95^3 lattice points), 50 rotations from
``rotation_matrices`` on 10 fixed unit vectors, no block file.  One warm-up of every route, then ``--repeats`` rounds in which the
routes follow each other (a, b, c, d, a, b, ...); median and range per route:

  (a) ceg_energy_grid, host output (timed), then mean_boltzmann at 300 K + min on the host (timed separately)
  (b) ceg_energy_grid_reduced, host outputs, 300 K + min
  (c) the same with 8 temperatures
  (d) device outputs, 300 K + min (ends in a device synchronise)

and the worst error of (b) against (a) in units of the bound of tests/test_gpu_energy_grid_reduced.py.

``--baseline-lib PATH``: only the ceg_energy_grid part of (a), through another build of libceg_hip.so (the parent commit's, which
does not export the new entry) -- a process of its own, run before and after the main one for the spread between processes.
``--trace-only``: one warm-up and one call of (b) and of (c), for a kernel trace.  A session, every step under its own time limit:

    timeout -k 10 300 python tests/perf/time_energy_grid_reduced.py --baseline-lib PARENT/libceg_hip.so --out base1.txt &&
    timeout -k 10 400 python tests/perf/time_energy_grid_reduced.py --out new.txt &&
    timeout -k 10 300 python tests/perf/time_energy_grid_reduced.py --baseline-lib PARENT/libceg_hip.so --out base2.txt &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d trace -- python tests/perf/time_energy_grid_reduced.py --trace-only
"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

EIGHT = (77.0, 150.0, 200.0, 250.0, 300.0, 400.0, 600.0, 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    from ceg_hip import _abi
    if args.baseline_lib:
        os.environ["CEG_HIP_LIB"] = str(Path(args.baseline_lib).resolve())
        _abi.PROTOTYPES.pop("ceg_energy_grid_reduced")               # the parent's library does not export it
    import torch
    import ceg_hip as ceg
    from ceg_hip.energy import GpuEnergySetup
    from ceg_hip.hostmirror.lebedev import rotation_matrices
    from ceg_hip.hostmirror.utils import mean_boltzmann

    golden = ROOT / "tests" / "golden" / "raspa"
    with tempfile.TemporaryDirectory() as tmp:
        raspa = Path(tmp) / "raspa"
        raspa.mkdir()
        for sub in ("forcefield", "molecules", "structures"):
            os.symlink(golden / sub, raspa / sub)
        ceg.setdir_RASPA(raspa)
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021", "CO2", "TraPPE", blockfile=False)
    rng = np.random.default_rng(50)
    u = rng.normal(size=(10, 3))
    rots = rotation_matrices(u / np.linalg.norm(u, axis=1)[:, None], False)
    nrot = len(rots)
    mat = setup.framework.mat
    num = [int(math.floor(np.linalg.norm(mat[:, a]) / args.step)) + 1 for a in range(3)]
    points = num[0] * num[1] * num[2]
    say(f"CO2 in CHA_1.4_3b4eeb96, step {args.step} A: lattice {num[0]} x {num[1]} x {num[2]}, {nrot} rotations, {nrot * points} elements "
        f"({8 * nrot * points / 1e6:.0f} MB), {8 * points / 1e6:.1f} MB per reduced output; device {torch.cuda.get_device_name(0)}; "
        f"library {_abi.load_library()._name}")
    gs = GpuEnergySetup(setup)
    res = {}

    def route_a():
        t0 = time.perf_counter()
        full = gs.energy_grid_rotations(args.step, rots)
        t1 = time.perf_counter()
        res["a"] = (mean_boltzmann(full, 300.0), full.min(axis=0))
        res["full"] = full
        return t1 - t0, time.perf_counter() - t1

    if args.baseline_lib:
        route_a()
        ts = [route_a() for _ in range(args.repeats)]
        g = [t[0] for t in ts]
        say(f"baseline ceg_energy_grid, host output: median {statistics.median(g) * 1e3:8.1f} ms   ({', '.join(f'{t * 1e3:.1f}' for t in g)})")
        gs.close()
        return

    def route_b():
        t0 = time.perf_counter()
        res["b"] = gs.energy_grid_reduced(args.step, rots, (300.0,))
        return time.perf_counter() - t0

    def route_c():
        t0 = time.perf_counter()
        res["c"] = gs.energy_grid_reduced(args.step, rots, EIGHT)
        return time.perf_counter() - t0

    d_mean = torch.empty(points, dtype=torch.float64, device="cuda:0")
    d_min = torch.empty(points, dtype=torch.float64, device="cuda:0")

    def route_d():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gs.energy_grid_reduced(args.step, rots, (300.0,), out_device_ptrs=(d_mean.data_ptr(), d_min.data_ptr(), None))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.trace_only:
        for fn in (route_b, route_c, route_b, route_c):
            fn()
        say("trace: two calls of route (b) and two of route (c), two slabs each = 4 lattices per variant of k_egrid_reduce")
        gs.close()
        return

    for fn in (route_a, route_b, route_c, route_d):                  # warm-up of every route
        fn()
    t = {k: [] for k in "abcd"}
    t_np = []
    for _ in range(args.repeats):
        g, r = route_a()
        t["a"].append(g)
        t_np.append(r)
        t["b"].append(route_b())
        t["c"].append(route_c())
        t["d"].append(route_d())

    def row(name, ts):
        say(f"{name:<62s} median {statistics.median(ts) * 1e3:8.1f} ms   ({', '.join(f'{x * 1e3:.1f}' for x in ts)})")
    row("(a) ceg_energy_grid, host output", t["a"])
    row("    + mean_boltzmann(300 K) + min in NumPy", t_np)
    row("(b) ceg_energy_grid_reduced, host outputs, 300 K + min", t["b"])
    row("(c) ceg_energy_grid_reduced, host outputs, 8 temperatures + min", t["c"])
    row("(d) ceg_energy_grid_reduced, device outputs, 300 K + min", t["d"])
    ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
    say(f"(b) / (a) = {mb / ma:.3f} of the ceg_energy_grid part alone, {mb / (ma + statistics.median(t_np)):.4f} with the host reduction; "
        f"(c) / (b) = {statistics.median(t['c']) / mb:.3f}")
    # (b) against (a): min bit for bit, mean in units of 1e-12 sum(f |x|)/sum(f)
    full, (ref, mn) = res["full"], res["a"]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        m = mn - 30.0 * 300.0
        f = np.exp((m[None] - full) / 300.0)
        bound = 1e-12 * (f * np.abs(full)).sum(axis=0) / f.sum(axis=0)
    ok = ref < 1e90
    ratio = np.where(ok, np.abs(res["b"].mean[0] - ref) / bound, 0.0)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    say(f"min of (b) == min of (a) bit for bit: {np.array_equal(res['b'].min, mn)}; {ok.sum()} accessible points, worst |mean(b) - mean(a)| = "
        f"{ratio[i]:.3g} of the bound 1e-12 sum(f|x|)/sum(f) at point {i} (device {res['b'].mean[0][i]!r}, mirror {ref[i]!r}); "
        f"inaccessible points agree: {bool(np.all(res['b'].mean[0][~ok] >= 1e90))}; 300 K of (c) == (b) bit for bit: "
        f"{np.array_equal(res['c'].mean[4], res['b'].mean[0])}")
    gs.close()


if __name__ == "__main__":
    main()
