"""Timing of ``ceg_grid_basins`` at 95^3 (the energy lattice of the README) and 189^3, on the smooth FP64 field with noise of
``tests/perf/time_basins.py`` (same seed), the starts being all its local minima (``ceg_grid_local_minima`` with a negative tolerance,
the list left in device memory).

Three routes in alternated windows (dev, host, numpy, dev, host, numpy, ...), median and range of the per-call time of the windows:

  dev    ``ceg_grid_basins`` on the device-resident field and list, every output on the device; ends in a synchronise
  host   ``ceg_hip.basins.local_basins`` on a host array and a host list (upload, call, results back)
  numpy  what a user does without the entry point: the read-back of the field and of the list plus ``local_basins_host``

Then the shape of the result (levels, covered points, multi-owner points, the largest owner list, pairs) and a comparison of every
integer of the device result with the NumPy form.

``--trace-only``: one warm-up and one ``dev`` call at 189^3, for ``rocprofv3 --kernel-trace --stats``.  A session:

    timeout -k 10 900 python tests/perf/time_basin_flow.py --out basin_flow.txt &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d trace -- python tests/perf/time_basin_flow.py --trace-only
"""
import argparse
import ctypes as C
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_basins import inputs      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[95, 189])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tolerance", type=float, default=-1.0)
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

    import torch
    from ceg_hip import _abi, basins as B
    lib = _abi.load_library()
    if lib.ceg_device_count() < 1:
        raise SystemExit("time_basin_flow: no HIP device visible")
    null = C.c_void_p(0)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    for n in ([189] if args.trace_only else args.sizes):
        field = inputs(n)[0]
        dims = (n, n, n)
        d32 = _abi.i32ptr(np.asarray(dims, dtype=np.int32))
        npts = n ** 3
        dfield = torch.from_numpy(np.ascontiguousarray(field.ravel(order="F"))).cuda()
        count, pairs = C.c_int64(0), C.c_int64(0)
        cap = 1 << 20
        dijk = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _abi.check(lib, lib.ceg_grid_local_minima(0, ptr(dfield), 1, d32, 0, args.tolerance, ptr(dijk), 1, cap, C.byref(count), None, null))
        ns = int(count.value)
        assert ns <= cap
        dlevel, downer = torch.empty(npts, dtype=torch.int32, device="cuda"), torch.empty(npts, dtype=torch.int32, device="cuda")
        dnown = torch.empty(npts, dtype=torch.uint8, device="cuda")
        dshared = torch.empty((npts, 2), dtype=torch.int32, device="cuda")
        dsize = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def dev():
            _abi.check(lib, lib.ceg_grid_basins(0, ptr(dfield), 1, d32, ptr(dijk), 1, ns, 0, math.inf, 0, ptr(dlevel), ptr(downer), ptr(dnown), 1,
                                                ptr(dshared), npts, C.byref(pairs), ptr(dsize), 1, null))
            torch.cuda.synchronize()

        hmins = dijk[:ns].cpu().numpy()

        def host():
            return B.local_basins(field, hmins)

        def numpy_route():
            return B.local_basins_host(dfield.cpu().numpy().reshape(dims, order="F"), dijk[:ns].cpu().numpy())

        if args.trace_only:
            dev()
            dev()
            say(f"trace-only: two dev calls at {n}^3, {ns} starts")
            return
        say(f"== {n}^3 = {npts} points, {ns} starts (all local minima); {args.repeats} alternated windows per route; median [min .. max] in ms")
        routes = {"dev": [dev, 1], "host": [host, 1], "numpy": [numpy_route, 1]}
        times = {k: [] for k in routes}
        for k, r in routes.items():
            if k != "numpy":                                         # NumPy has nothing to warm up, and its calls take seconds
                r[0]()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r[0]()
                torch.cuda.synchronize()
                r[1] = int(min(max(0.25 / max(time.perf_counter() - t0, 1e-6), 3), 2000))      # a window of about 0.25 s
        ref = None
        for w in range(args.repeats):
            for k, (f, calls) in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _c in range(calls):
                    out = f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / calls * 1e3)
                if k == "numpy":
                    ref = out
        parts = [f"{k} {statistics.median(v):10.3f} [{min(v):10.3f} .. {max(v):10.3f}]" for k, v in times.items()]
        say(f"{'ceg_grid_basins':18s} " + "   ".join(parts))
        say(f"{'':18s} dev is {statistics.median(times['numpy']) / statistics.median(times['dev']):.0f} x the numpy route, "
            f"host {statistics.median(times['numpy']) / statistics.median(times['host']):.0f} x")
        dev()
        level = dlevel.cpu().numpy()
        nown = dnown.cpu().numpy()
        levels = int(level.max()) + 1
        covered, multi = int((nown > 0).sum()), int((nown > 1).sum())
        batches = (levels - 1) // 16 + 1                             # level launches come 16 at a time, then the counts are read
        say(f"{'':18s} {levels} levels ({2 + 16 * batches + (levels - 1) + 5} launches, {batches + 1} synchronisations); covered {covered} points "
            f"({100.0 * covered / npts:.1f} %), multi-owner {multi} ({100.0 * multi / max(covered, 1):.1f} % of covered), "
            f"largest owner list {int(nown.max())}, pairs {pairs.value}")
        k = int(pairs.value)
        same = (np.array_equal(level.reshape(dims, order="F"), ref.level) and np.array_equal(downer.cpu().numpy().reshape(dims, order="F"), ref.owner)
                and np.array_equal(nown.reshape(dims, order="F"), ref.nowners) and np.array_equal(dshared[:k].cpu().numpy(), ref.shared)
                and np.array_equal(dsize[:ns].cpu().numpy(), ref.size))
        assert same, "the device result differs from the NumPy form"
        say(f"{'':18s} device result equals the NumPy form (level, owner, nowners, shared, size)")


if __name__ == "__main__":
    main()
