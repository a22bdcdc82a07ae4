"""Timing of the site extraction (``ceg_grid_smooth``, ``ceg_grid_ranked``, ``ceg_grid_site_nearest``, the host greedy pass and the whole
``average_clusters`` call) on the Poisson-cloud density map of ``tests/perf/time_basins.py`` at 95^3 and 189^3 with 100 sites.

Per device entry point two routes, in alternated windows (dev, numpy, dev, numpy, ...), median and range of the per-call time:

  dev    the device call on a device-resident input with device outputs; ends in a synchronise
  numpy  what a user does without the entry point: the read-back of the device array plus the ``*_host`` NumPy form (one call per
         window, three windows; the nearest-site form is timed with 10 sites and said so: it is linear in the sites)

The smoothing is also timed pass by pass: calls with the real taps on one axis and the single tap 1.0 on the two others, minus the call
with 1.0 on all three, give what the real taps add to that pass; the kernel trace (``--trace-only`` under ``rocprofv3 --kernel-trace``)
gives the passes themselves.  A pass reads and writes 8 bytes per voxel: 16*a*b*c bytes against the 6.3 TB/s streaming figure.

Then, once per size: the host greedy pass alone and the whole device-backed ``average_clusters`` call, at the default ``atol`` (0.0)
and at ``atol = 0.1``, with the number of voxels that survive the crop.
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT), str(ROOT / "tests" / "perf")):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_basins import HBM_ACHIEVABLE, inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[95, 189])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
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
        raise SystemExit("time_site_extraction: no HIP device visible")
    null = C.c_void_p(0)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a.ravel(order="F"))).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def windows(routes):
        """routes: name -> (callable, windowed).  -> name -> list of per-call ms"""
        calls = {}
        for k, (f, windowed) in routes.items():
            calls[k] = 1
            if windowed:
                f()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                calls[k] = int(min(max(0.25 / max(time.perf_counter() - t0, 1e-6), 5), 2000))
        times = {k: [] for k in routes}
        for w in range(args.repeats):
            for k, (f, windowed) in routes.items():
                if not windowed and w >= 3:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _c in range(calls[k]):
                    f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / calls[k] * 1e3)
        return times

    def fmt(times):
        return "   ".join(f"{k} {statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]" for k, v in times.items())

    for n in ([189] if args.trace_only else args.sizes):
        _, bins, sites, mat = inputs(n)
        dims = (n, n, n)
        d32 = _abi.i32ptr(np.asarray(dims, dtype=np.int32))
        npts = n ** 3
        counter = float(bins.sum()) / (0.5 * len(sites))                          # half an atom per site and frame
        scale = 1.0 / counter
        taps = [B.gaussian_taps(s) for s in B.smoothing_sigmas(dims, mat)]
        one = np.ones(1)
        dbins = dev(bins)
        dsm = torch.empty(npts, dtype=torch.float64, device="cuda")
        didx = torch.empty(npts, dtype=torch.int32, device="cuda")
        dval = torch.empty(npts, dtype=torch.float64, device="cuda")
        dlin, dsite = torch.empty(npts, dtype=torch.int32, device="cuda"), torch.empty(npts, dtype=torch.int32, device="cuda")
        dofs, ddist = torch.empty((npts, 3), dtype=torch.int8, device="cuda"), torch.empty(npts, dtype=torch.float64, device="cuda")
        count = C.c_int64(0)
        kept, _ = B.snap_sites(sites, dims)
        flat, m9 = np.ascontiguousarray(kept).ravel(), np.ascontiguousarray(mat.T).ravel()
        ortho, safemin = B._periodic_setup(mat)
        crop = 0.1 * float(bins.max()) * scale / 100

        def smooth_dev(t=taps):
            _abi.check(lib, lib.ceg_grid_smooth(0, ptr(dbins), 1, 1, scale, d32, _abi.dptr(t[0]), len(t[0]), _abi.dptr(t[1]), len(t[1]),
                                                _abi.dptr(t[2]), len(t[2]), ptr(dsm), 1, null))

        def ranked_dev():
            _abi.check(lib, lib.ceg_grid_ranked(0, ptr(dsm), 1, d32, crop, ptr(didx), ptr(dval), 1, npts, C.byref(count), null))

        def nearest_dev():
            _abi.check(lib, lib.ceg_grid_site_nearest(0, d32, _abi.dptr(m9), int(ortho), safemin, _abi.dptr(flat), len(kept), 0, ptr(dbins), 1,
                                                      ptr(dlin), ptr(dsite), ptr(dofs), ptr(ddist), 1, npts, C.byref(count), null))

        if args.trace_only:
            for f in (smooth_dev, ranked_dev, nearest_dev):
                f(); torch.cuda.synchronize()
                f(); torch.cuda.synchronize()
            say(f"trace-only: two dev calls of every entry point at {n}^3, taps {[len(t) for t in taps]}")
            return
        say(f"== {n}^3 = {npts} points, {len(kept)} sites, taps {[len(t) for t in taps]}; {args.repeats} alternated windows; "
            "median [min .. max] in ms")
        few = 10

        def host_bins():
            return dbins.cpu().numpy().reshape(dims, order="F")

        def host_smoothed():
            return dsm.cpu().numpy().reshape(dims, order="F")

        smooth_dev()
        t = windows({"dev": (smooth_dev, True), "numpy": (lambda: B.smooth_grid_host(host_bins(), taps, scale=scale), False)})
        say(f"{'smooth (3 passes)':28s} " + fmt(t))
        base = statistics.median(windows({"dev": (lambda: smooth_dev((one, one, one)), True)})["dev"])
        say(f"{'':28s} one tap per axis (three copies through LDS, allocation, upload of the taps, synchronise): {base:.3f} ms")
        for axis in range(3):
            tt = [taps[q] if q == axis else one for q in range(3)]
            ms = statistics.median(windows({"dev": (lambda tt=tt: smooth_dev(tt), True)})["dev"])
            extra = max(ms - base, 1e-6) + base / 3
            say(f"{'':28s} axis {axis} with {len(taps[axis])} taps: call {ms:.3f} ms; that pass about {extra:.3f} ms = "
                f"{16 * npts / (extra * 1e-3) / 1e12:.2f} TB/s of its 16*a*b*c bytes ({100 * 16 * npts / (extra * 1e-3) / HBM_ACHIEVABLE:.0f} % of 6.3 TB/s)")
        smooth_dev()                                                              # the per-axis calls left their own result in dsm
        ranked_dev()
        nranked = count.value
        t = windows({"dev": (ranked_dev, True), "numpy": (lambda: B.ranked_above_host(host_smoothed(), crop), False)})
        say(f"{'ranked above the crop':28s} " + fmt(t) + f"   ({nranked} voxels above crop {crop:.3g})")
        nearest_dev()
        nactive = count.value
        t = windows({"dev": (nearest_dev, True),
                     "numpy": (lambda: B.site_nearest_host(kept[:few], dims, mat, bins=host_bins(), origin=0), False)})
        say(f"{'site_nearest':28s} " + fmt(t) + f"   ({nactive} active voxels; numpy: {few} sites only)")
        # the device results against the NumPy forms, once per size
        hs = B.smooth_grid_host(bins, taps, scale=scale)
        ds = host_smoothed()
        assert np.allclose(ds, hs, rtol=1e-13, atol=0)
        hi, hv = B.ranked_above_host(ds, crop)
        ranked_dev()
        assert count.value == len(hi) and np.array_equal(didx[:len(hi)].cpu().numpy(), hi) and np.array_equal(dval[:len(hi)].cpu().numpy(), hv)
        nearest_dev()
        hl, hsi, ho, hd = B.site_nearest_host(kept, dims, mat, bins=bins, origin=0)
        k = len(hl)
        assert count.value == k and np.array_equal(dlin[:k].cpu().numpy(), hl) and np.array_equal(dsite[:k].cpu().numpy(), hsi)
        assert np.array_equal(dofs[:k].cpu().numpy(), ho) and np.array_equal(ddist[:k].cpu().numpy(), hd)
        say("device results equal the NumPy forms (ranking, nearest site with distances; smoothing to 1e-13)")
        if args.no_pipeline:
            continue
        values = bins.ravel(order="F").astype(np.float64) * scale
        for atol in (0.0, 0.1):
            c = atol * float(values.max()) / 100
            smooth_dev()
            lin, smv = B.ranked_above((dsm.data_ptr(), dims), c)
            t0 = time.perf_counter()
            ret = B.coalesce_ranked(lin, smv, values[lin], dims, mat, 1.0, atol)
            tg = time.perf_counter() - t0
            say(f"atol {atol}: crop {c:.3g}, {len(lin)} of {npts} voxels ranked ({100 * len(lin) / npts:.1f} %); host greedy pass "
                f"{tg * 1e3:.1f} ms -> {len(ret)} basins")
            t0 = time.perf_counter()
            try:
                out = B.average_clusters((dbins.data_ptr(), dims, np.int64), 1.0, mat, counter=counter, atol=atol)
                tw = time.perf_counter() - t0
                say(f"atol {atol}: average_clusters, device-resident bins: {tw * 1e3:.1f} ms -> {len(out)} sites; the greedy pass is "
                    f"{100 * tg / tw:.0f} % of the call")
            except (_abi.CegError, ValueError) as e:
                say(f"atol {atol}: average_clusters stopped after {(time.perf_counter() - t0) * 1e3:.1f} ms: {e}")


if __name__ == "__main__":
    main()
