"""Timing of the sequential part of the site extraction once it runs in the library: ``ceg_grid_coalesce`` (the greedy pass on the
device), ``ceg_grid_site_partition`` and ``ceg_cluster_closer_than``, and the whole ``average_clusters`` call, on the maps of
``tests/perf/time_site_extraction.py`` (the Poisson-cloud density map at 95^3 and 189^3, 100 sites) at ``atol`` 0.1 and 0.

Per size and ``atol``, in alternated windows (dev, host, dev, host, ...), one call per window, median and range:

  greedy     dev: ``ceg_grid_coalesce`` on the device-resident ranking and bins, the basins back to the host
             host: ``ceg_coalesce_ranked`` on the same ranking in host memory (the values gathered beforehand)
  partition  dev: ``ceg_grid_site_partition`` on the device-resident bins, the sites being the centres the greedy pass left
             host: ``site_nearest`` (device) plus the Python ``_accumulate_closest``; with more sites than ``site_nearest`` takes only
             the device route is timed
  cluster    lib: ``ceg_cluster_closer_than`` on the list of a first round; python: ``cluster_closer_than_host`` on the same list (on its
             first ``--python-entries`` entries where the list is longer, said in the line: the loop is quadratic)

and once: that the device greedy output equals the host's, and the whole ``average_clusters`` call with its number of sites.

``--host-check N`` needs no device: it runs the first refinement round of the host composition at ``atol = 0`` and says how many sites
it leaves without a voxel.  Every (size, atol) runs in a child process of its own under a time limit; the first one that fails ends the run.

    timeout -k 10 1100 python tests/perf/time_site_coalesce.py --out profiles/site_coalesce.txt
"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT), str(ROOT / "tests" / "perf")):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_basins import inputs  # noqa: E402


def fmt(v):
    return f"{statistics.median(v):10.2f} [{min(v):10.2f} .. {max(v):10.2f}]"


def child(n, atol, windows, vpl, python_entries):
    import torch
    from ceg_hip import _abi, basins as B
    lib = _abi.load_library()
    if lib.ceg_device_count() < 1:
        raise SystemExit("time_site_coalesce: no HIP device visible")
    null = C.c_void_p(0)
    _, bins, sites, mat = inputs(n)
    dims = (n, n, n)
    d32 = _abi.i32ptr(np.asarray(dims, dtype=np.int32))
    npts = n ** 3
    counter = float(bins.sum()) / (0.5 * len(sites))                              # half an atom per site and frame
    scale = 1.0 / counter
    taps = [B.gaussian_taps(s) for s in B.smoothing_sigmas(dims, mat)]
    dbins = torch.from_numpy(np.ascontiguousarray(bins.ravel(order="F"))).cuda()
    dsm = torch.empty(npts, dtype=torch.float64, device="cuda")
    didx = torch.empty(npts, dtype=torch.int32, device="cuda")
    dval = torch.empty(npts, dtype=torch.float64, device="cuda")
    count = C.c_int64(0)
    values = bins.ravel(order="F").astype(np.float64) * scale
    crop = atol * float(values.max()) / 100
    dmap = (dbins.data_ptr(), dims, np.int64)
    B.smooth_grid(dmap, taps, scale=scale, out_ptr=dsm.data_ptr())
    _abi.check(lib, lib.ceg_grid_ranked(0, C.c_void_p(dsm.data_ptr()), 1, d32, crop, C.c_void_p(didx.data_ptr()), C.c_void_p(dval.data_ptr()), 1,
                                        npts, C.byref(count), null))
    nr = int(count.value)
    lin, smv = didx[:nr].cpu().numpy(), dval[:nr].cpu().numpy()
    gathered = values[lin]
    print(f"== {n}^3, atol {atol}: crop {crop:.3g}, {nr} of {npts} voxels ranked; {windows} alternated windows, one call each; "
          "median [min .. max] in ms", flush=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def greedy_dev():
        return B.grid_coalesce(didx.data_ptr(), dval.data_ptr(), dmap, mat, 1.0, atol, counter=counter, nranked=nr, voxels_per_launch=vpl)

    def greedy_host():
        return B.coalesce_ranked(lin, smv, gathered, dims, mat, 1.0, atol)

    greedy_dev()                                                                  # warm-up: module load
    td, th = [], []
    for _ in range(windows):
        ms, got = timed(greedy_dev)
        td.append(ms)
        ms, want = timed(greedy_host)
        th.append(ms)
    same = len(got) == len(want) and all(v == rv and np.array_equal(p, rp) for (v, p), (rv, rp) in zip(got, want))
    nvox = vpl if vpl else 32768
    launches = (nr + nvox - 1) // nvox
    print(f"greedy     dev {fmt(td)}   host {fmt(th)}   -> {len(want)} basins; the device output "
          f"{'equals' if same else 'DIFFERS FROM'} the host's; host min / dev median {min(th) / statistics.median(td):.1f}; "
          f"{statistics.median(td) * 1e3 / max(nr, 1):.2f} us per voxel, {launches} launches of at most {nvox} voxels, "
          f"about {statistics.median(td) / max(launches, 1):.0f} ms each", flush=True)
    if not same:
        raise SystemExit(1)
    if not want:
        return
    pts = np.asarray([p for _, p in want]).reshape(-1, 3)
    kept, deleted = B.snap_sites(pts, dims)

    def part_dev():
        return B.site_partition(dmap, kept, mat, counter=counter)

    def part_host():
        l, s, o, _ = B.site_nearest(kept, dims, mat, bins=(dbins.data_ptr(), dims), origin=0, want_dist=False)
        return B._accumulate_closest(values, dims, len(kept), l, s, o, deleted)

    part_dev()
    host_ok = len(kept) <= _abi.SITE_PROXIMITY_MAX_SITES
    td, th = [], []
    for _ in range(windows):
        ms, part = timed(part_dev)
        td.append(ms)
        if host_ok:
            ms, ref = timed(part_host)
            th.append(ms)
    line = f"partition  dev {fmt(td)}   "
    if host_ok:
        ok = np.array_equal(part.sums, ref.sums) and np.array_equal(part.centres, ref.centres, equal_nan=True) and part.cap_bound == ref.cap_bound
        line += f"host {fmt(th)}   {'equal' if ok else 'DIFFERENT'} results; "
    else:
        line += f"host: site_nearest takes at most {_abi.SITE_PROXIMITY_MAX_SITES} sites; "
    print(line + f"{len(kept)} sites, {part.count} active voxels", flush=True)
    live = part.sums != 0
    ret = [(float(s), c) for s, c in zip(part.sums[live], part.centres[live])]
    cut = ret[:python_entries]
    tl, tp, tc = [], [], []
    for _ in range(windows):
        ms, a = timed(lambda: B.cluster_closer_than(ret, mat, 1.0))
        tl.append(ms)
        ms, b = timed(lambda: B.cluster_closer_than(cut, mat, 1.0))
        tc.append(ms)
        ms, c = timed(lambda: B.cluster_closer_than_host(cut, mat, 1.0))
        tp.append(ms)
    ok = len(b) == len(c) and all(v == rv and np.array_equal(p, rp) for (v, p), (rv, rp) in zip(b, c))
    print(f"cluster    lib {fmt(tl)} on {len(ret)} entries -> {len(a)};   on the first {len(cut)}: lib {fmt(tc)}   python {fmt(tp)}   "
          f"{'equal' if ok else 'DIFFERENT'} results", flush=True)
    t0 = time.perf_counter()
    try:
        ms, out = timed(lambda: B.average_clusters(dmap, 1.0, mat, counter=counter, atol=atol))
        print(f"average_clusters, device-resident bins: {ms:.1f} ms -> {len(out)} sites", flush=True)
    except (_abi.CegError, ValueError) as e:                                      # the reference's own error for a site without a voxel
        print(f"average_clusters, device-resident bins: stopped after {(time.perf_counter() - t0) * 1e3:.1f} ms: {e}", flush=True)


def host_check(n):
    """no device: the first refinement round of the host composition at ``atol = 0`` on the same map, from the NumPy smoothing and ranking,
    the library's host greedy pass, ``site_nearest_host`` and ``_accumulate_closest`` -- how many sites it leaves without a voxel"""
    from ceg_hip import basins as B
    _, bins, sites, mat = inputs(n)
    dims = (n, n, n)
    values = bins.ravel(order="F").astype(np.float64) * (1.0 / (float(bins.sum()) / (0.5 * len(sites))))
    taps = [B.gaussian_taps(s) for s in B.smoothing_sigmas(dims, mat)]
    lin, smv = B.ranked_above_host(B.smooth_grid_host(values.reshape(dims, order="F"), taps), 0.0)
    ret = B.coalesce_ranked(lin, smv, values[lin], dims, mat, 1.0, 0.0)
    kept, deleted = B.snap_sites(np.asarray([p for _, p in ret]), dims)
    l, s, o, _ = B.site_nearest_host(kept, dims, mat, bins=(values != 0).reshape(dims, order="F"), origin=0, want_dist=False)
    hc = B._accumulate_closest(values, dims, len(kept), l, s, o, deleted)
    line = f"host composition at {n}^3, atol 0: {len(lin)} voxels ranked, {len(ret)} basins, {int((hc.sums == 0).sum())} of {len(kept)} sites without a voxel"
    try:
        B.updated_sites_with_closest(hc)
        print(line + "; updated_sites_with_closest passes", flush=True)
    except ValueError as e:
        print(line + f"; updated_sites_with_closest raises: {e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[95, 189])
    ap.add_argument("--atols", type=float, nargs="+", default=[0.1, 0.0])
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--voxels-per-launch", type=int, default=0)
    ap.add_argument("--python-entries", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=420, help="seconds for one (size, atol)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    ap.add_argument("--host-check", type=int, default=None, help="no device: the host composition's first round at atol 0 at this size")
    args = ap.parse_args()
    if args.host_check:
        host_check(args.host_check)
        return
    if args.child:
        child(int(args.child[0]), float(args.child[1]), args.windows, args.voxels_per_launch, args.python_entries)
        return
    lines = []
    for n in args.sizes:
        for atol in args.atols:
            cmd = [sys.executable, __file__, "--child", str(n), str(atol), "--windows", str(args.windows), "--voxels-per-launch",
                   str(args.voxels_per_launch), "--python-entries", str(args.python_entries)]
            try:
                res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
                text, rc = res.stdout, res.returncode
            except subprocess.TimeoutExpired as e:
                text, rc = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
            print(text, end="", flush=True)
            lines.append(text)
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text("".join(lines))
            if rc != 0:
                raise SystemExit(f"time_site_coalesce: {n}^3 at atol {atol} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
