"""Timing of the grid analysis entry points (``ceg_grid_local_minima``, ``ceg_grid_components``, ``ceg_grid_site_proximity``,
``ceg_grid_site_density``) at 95^3 (the energy lattice of the README) and 189^3 (its density map), on synthetic inputs made from a
seed: a smooth FP64 field with noise (minima, band components), an int64 density map of Gaussian clouds around 100 sites (non-zero
components, site sums), 100 random sites in a 24.6 A cubic cell with maxdist 1 A (proximity map).

Per entry point three routes, in alternated windows (dev, host, numpy, dev, host, numpy, ...) of about 0.25 s each
(one call and three windows for numpy), median and range of the per-call time of the windows:

  dev    the device call on a device-resident input (outputs on the device where the entry point has them); ends in a synchronise
  host   the binding of ceg_hip/basins.py on a host array (upload, call, results back)
  numpy  what a user does without these entry points: the read-back of the device array plus the ``*_host`` NumPy form.  The proximity
         map in NumPy takes all 27 offsets per site and is timed with 1 site only (said in its line); it is linear in the sites.

``--trace-only``: one warm-up and one ``dev`` call of everything at 189^3, for ``rocprofv3 --kernel-trace --stats``.  A session:

    timeout -k 10 900 python tests/perf/time_basins.py --out basins.txt &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d trace -- python tests/perf/time_basins.py --trace-only
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12      # B/s, the streaming figure of the MI355X


def inputs(n, nsites=100, seed=1):
    r = np.random.default_rng([seed, n])
    ax = np.arange(n) / n
    i, j, k = np.meshgrid(ax, ax, ax, indexing="ij")
    field = -800.0 + 600.0 * (np.sin(6 * np.pi * i) * np.cos(4 * np.pi * j) + np.sin(2 * np.pi * (k + i)) * np.cos(8 * np.pi * k)) \
        + 5.0 * r.normal(size=(n, n, n))
    sites = r.random((nsites, 3))
    bins = np.zeros((n, n, n), dtype=np.int64)
    w = max(int(0.03 * n), 2)
    for s in sites:                                          # a cloud of counts around every site, most of the map empty
        c = np.rint(s * n).astype(int)
        idx = [np.arange(c[q] - 2 * w, c[q] + 2 * w + 1) for q in range(3)]
        d2 = ((idx[0][:, None, None] - s[0] * n) ** 2 + (idx[1][None, :, None] - s[1] * n) ** 2 + (idx[2][None, None, :] - s[2] * n) ** 2)
        cloud = r.poisson(400.0 * np.exp(-d2 / (2.0 * (w / 2.0) ** 2)))
        bins[np.ix_(idx[0] % n, idx[1] % n, idx[2] % n)] += cloud
    return np.asfortranarray(field), np.asfortranarray(bins), sites, np.eye(3) * 24.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[95, 189])
    ap.add_argument("--repeats", type=int, default=5)
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
        raise SystemExit("time_basins: no HIP device visible")
    null = C.c_void_p(0)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a.ravel(order="F"))).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    for n in ([189] if args.trace_only else args.sizes):
        field, bins, sites, mat = inputs(n)
        dims = (n, n, n)
        d32 = _abi.i32ptr(np.asarray(dims, dtype=np.int32))
        npts = n ** 3
        dfield, dbins = dev(field), dev(bins)
        lo, hi = -1000.0, -700.0
        cap = 1 << 20
        dijk = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
        dlab = torch.empty(npts, dtype=torch.int32, device="cuda")
        dseed, dsize = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
        dsum = torch.empty(cap, dtype=torch.int64, device="cuda")
        dsite, doff = torch.empty(npts, dtype=torch.int32, device="cuda"), torch.empty((npts, 3), dtype=torch.int8, device="cuda")
        ns = len(sites)
        drho, dmom = torch.empty(ns + 1, dtype=torch.int64, device="cuda"), torch.empty((ns + 1, 3), dtype=torch.int64, device="cuda")
        count, ext = C.c_int64(0), C.c_double(0.0)
        kept, _ = B.snap_sites(sites, dims)
        assert len(kept) == ns
        flat, m9 = np.ascontiguousarray(kept).ravel(), np.ascontiguousarray(mat.T).ravel()

        def minima_dev():
            _abi.check(lib, lib.ceg_grid_local_minima(0, ptr(dfield), 1, d32, 0, 0.01, ptr(dijk), 1, cap, C.byref(count), C.byref(ext), null))

        def comps_dev(grid, i64, mode):
            _abi.check(lib, lib.ceg_grid_components(0, ptr(grid), i64, 1, d32, mode, lo, hi, ptr(dlab), 1, ptr(dseed), ptr(dsize),
                                                    ptr(dsum) if i64 else null, 1, cap, C.byref(count), null))

        def prox_dev():
            _abi.check(lib, lib.ceg_grid_site_proximity(0, d32, _abi.dptr(m9), _abi.dptr(flat), ns, 1.0, ptr(dsite), ptr(doff), 1, null))

        def dens_dev():
            _abi.check(lib, lib.ceg_grid_site_density(0, ptr(dbins), 1, ptr(dsite), ptr(doff), 1, d32, ns, ptr(drho), ptr(dmom), 1, null))
            torch.cuda.synchronize()

        prox_dev()
        hsite = dsite.cpu().numpy().reshape(dims, order="F")
        hoff = np.moveaxis(doff.cpu().numpy().T.reshape((3,) + dims, order="F"), 0, -1)
        few = 1
        entries = [
            ("local_minima tol 0.01", minima_dev, lambda: B.local_minima(field, 0.01),
             lambda: B.local_minima_host(dfield.cpu().numpy().reshape(dims, order="F"), 0.01), ""),
            ("components nonzero int64", lambda: comps_dev(dbins, 1, 0), lambda: B.grid_components(bins),
             lambda: B.grid_components_host(dbins.cpu().numpy().reshape(dims, order="F")), ""),
            ("components band fp64", lambda: comps_dev(dfield, 0, 1), lambda: B.compute_levels(field, lo, hi),
             lambda: B.compute_levels_host(dfield.cpu().numpy().reshape(dims, order="F"), lo, hi), ""),
            (f"site_proximity {ns} sites", prox_dev, lambda: B.site_proximity_map(sites, dims, mat, 1.0),
             lambda: B.site_proximity_map_host(sites[:few], dims, mat, 1.0), f" (numpy: {few} sites only)"),
            (f"site_density {ns} sites", dens_dev, lambda: B.site_density(bins, hsite, hoff, ns),
             lambda: B.site_density_host(dbins.cpu().numpy().reshape(dims, order="F"), dsite.cpu().numpy().reshape(dims, order="F"),
                                         np.moveaxis(doff.cpu().numpy().T.reshape((3,) + dims, order="F"), 0, -1), ns), ""),
        ]
        if args.trace_only:
            for name, fdev, *_ in entries:
                fdev(); torch.cuda.synchronize()
                fdev(); torch.cuda.synchronize()
            say(f"trace-only: two dev calls of every entry point at {n}^3")
            return
        say(f"== {n}^3 = {npts} points; {args.repeats} alternated windows per route; median [min .. max] in ms")
        for name, fdev, fhost, fnumpy, note in entries:
            routes = {"dev": [fdev, 1], "host": [fhost, 1], "numpy": [fnumpy, 1]}
            times = {k: [] for k in routes}
            for k, r in routes.items():
                if k != "numpy":                                 # NumPy has nothing to warm up, and its calls take seconds
                    r[0]()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r[0]()
                    torch.cuda.synchronize()
                    r[1] = int(min(max(0.25 / max(time.perf_counter() - t0, 1e-6), 5), 2000))      # a window of about 0.25 s
            for w in range(args.repeats):
                for k, (f, calls) in routes.items():
                    if k == "numpy" and w >= 3:
                        continue
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _c in range(calls):
                        f()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / calls * 1e3)
            parts = [f"{k} {statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]" for k, v in times.items()]
            say(f"{name:28s} " + "   ".join(parts) + note)
            if name.startswith("local_minima"):
                t = statistics.median(times["dev"]) * 1e-3
                say(f"{'':28s} count {count.value}; whole dev call (4 launches, a scan, 2 synchronisations): {8 * npts / t / 1e9:.1f} GB/s of the "
                    f"8*a*b*c bytes = {100 * 8 * npts / t / HBM_ACHIEVABLE:.1f} % of 6.3 TB/s; the single pass alone: see the kernel trace")
            elif name.startswith("components"):
                say(f"{'':28s} count {count.value}")
        # the device results against the NumPy forms, once per size
        minima_dev()
        want = B.local_minima_host(field, 0.01)
        assert count.value == len(want) and np.array_equal(dijk[:len(want)].cpu().numpy(), want)
        comps_dev(dbins, 1, 0)
        hc = B.grid_components_host(bins)
        assert count.value == len(hc.seed) and np.array_equal(dlab.cpu().numpy().reshape(dims, order="F"), hc.labels)
        assert np.array_equal(dsum[:count.value].cpu().numpy(), hc.sum)
        dens_dev()
        hr, hm = B.site_density_host(bins, hsite, hoff, ns)
        assert np.array_equal(drho.cpu().numpy(), hr) and np.array_equal(dmom.cpu().numpy(), hm)
        say("device results equal the NumPy forms (minima, int64 components with sums, site sums)")


if __name__ == "__main__":
    main()
