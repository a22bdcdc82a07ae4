"""Grid analysis of the reference's ``src/basins.jl`` on the device: ``local_minima`` (:40-99), ``local_components`` (:279-313),
``compute_levels`` (:842-869), ``site_proximity_map!`` (:466-578), ``closest_from_proximity`` (:580-597), ``proximal_map`` (:607-610), ``local_basins`` (:195-264), ``decompose_basins`` (:765-797),
on top of ``ceg_grid_local_minima`` / ``ceg_grid_components`` / ``ceg_grid_site_proximity`` / ``ceg_grid_site_density`` /
``ceg_grid_basins``.

Everything is 0-based.  A grid argument is a NumPy array ``g[i, j, k]`` (any memory order; it is handed over in Julia's, first axis
fastest) or ``(device_ptr, (a, b, c))`` -- ``(device_ptr, (a, b, c), dtype)`` where both int64 and float64 are legal -- for an array that
is already in device memory in that order (a lattice of ``ceg_energy_grid_reduced``, the bins of the MC sampler).

The ``*_host`` functions are vectorised NumPy restatements of the same definitions, for where no device is wanted; they never touch
the library.  The last section goes from a density map to the list of sites: ``average_clusters``, ``coalescing_basins``,
``closest_to_sites`` (see there).  Not covered: ``energy_levels``, ``output_sites``, the unwrapped coordinates of the reference's component lists and basin sets (a point is its wrapped index here).

The basins follow the definition (``x`` belongs to basin ``i`` iff no start reaches ``x`` at an earlier breadth-first level than
``i`` does); the reference as written departs from it at the sole last-level point of a basin (basins.jl:153), see
``ceg_grid_basins`` in the header.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from . import _abi

__all__ = ["local_minima", "grid_components", "local_components", "compute_levels", "site_proximity_map", "site_density",
           "closest_from_proximity", "proximal_map", "snap_sites", "check_maxdist", "Components",
           "local_minima_host", "grid_components_host", "local_components_host", "compute_levels_host", "site_proximity_map_host",
           "site_density_host", "closest_from_proximity_host", "proximal_map_host",
           "Basins", "local_basins", "basin_points", "decompose_basins", "local_basins_host", "decompose_basins_host",
           "circular_distance",
           "ClosestSites", "gaussian_taps", "smoothing_sigmas", "smooth_grid", "ranked_above", "site_nearest", "coalesce_ranked",
           "grid_coalesce", "site_partition", "SitePartition", "cluster_closer_than", "closest_to_sites", "updated_sites_with_closest", "coalescing_basins", "average_clusters",
           "smooth_grid_host", "ranked_above_host", "site_nearest_host", "coalesce_ranked_host", "cluster_closer_than_host",
           "closest_to_sites_host", "updated_sites_with_closest_host", "coalescing_basins_host", "average_clusters_host"]


class Components(NamedTuple):
    """``labels[i, j, k]``: -1 for an inactive point, else the rank of its component in the order of discovery of the reference's
    ``k, j, i`` scan (= by smallest linear index).  ``label[n]``, ``seed[n]`` (smallest linear index ``i + a*(j + b*k)``), ``size[n]``,
    ``sum[n]``: the n-th component kept, in the order the function documents."""
    labels: np.ndarray
    label: np.ndarray
    seed: np.ndarray
    size: np.ndarray
    sum: np.ndarray


# ---------------------------------------------------------------------------------------------------------------- arguments
def _grid_arg(grid, dtypes):
    """-> (address, on_device, dims, dtype, keepalive)"""
    if isinstance(grid, tuple):
        ptr, dims = int(grid[0]), tuple(int(d) for d in grid[1])
        dt = np.dtype(grid[2]) if len(grid) > 2 else np.dtype(dtypes[0])
        if dt not in [np.dtype(d) for d in dtypes]:
            raise TypeError(f"a device grid of {dt} is not accepted here")
        arr = None
    else:
        arr = np.asarray(grid)
        if arr.ndim != 3:
            raise ValueError("a grid has three axes")
        dt = arr.dtype if arr.dtype in [np.dtype(d) for d in dtypes] else np.dtype(dtypes[0])
        if arr.dtype != dt and not np.can_cast(arr.dtype, dt, "safe"):
            raise TypeError(f"a grid of {arr.dtype} is not accepted here")
        arr = np.asfortranarray(arr, dtype=dt)
        ptr, dims = arr.ctypes.data, arr.shape
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError("dims must be three positive numbers")
    if dims[0] * dims[1] * dims[2] > 2**31 - 1:
        raise ValueError("a*b*c does not fit int32")
    return C.c_void_p(ptr), int(arr is None), dims, dt, arr


def _dims_arg(dims):
    return np.ascontiguousarray(dims, dtype=np.int32)


def _stream(stream):
    return C.c_void_p(int(stream) if stream else 0)


# ---------------------------------------------------------------------------------------------------------------- local_minima
def local_minima(grid, tolerance=1e-2, *, maxima=False, device=0, capacity=4096, stream=None, return_extremum=False):
    """``local_minima(grid, tolerance; lt)``: the (n, 3) int32 array of the 0-based (i, j, k) of the local minima (``maxima``:
    ``lt = >``), sorted as Julia sorts CartesianIndex (last axis slowest).  ``tolerance < 0``: all of them.  An ``extremum >= 0``
    with ``tolerance >= 0`` (the reference's ``@assert``) raises ``CegError``; no extremum at all is an empty array.
    ``capacity`` is the first guess of the room; a larger count calls again."""
    lib = _abi.load_library()
    ptr, on_dev, dims, _, keep = _grid_arg(grid, (np.float64,))
    count, ext = C.c_int64(0), C.c_double(0.0)
    cap = max(int(capacity), 0)
    while True:
        ijk = np.empty((max(cap, 1), 3), dtype=np.int32)
        _abi.check(lib, lib.ceg_grid_local_minima(device, ptr, on_dev, _abi.i32ptr(_dims_arg(dims)), int(bool(maxima)), float(tolerance),
                                                  C.c_void_p(ijk.ctypes.data), 0, cap, C.byref(count), C.byref(ext), _stream(stream)))
        if count.value <= cap:
            break
        cap = int(count.value)
    out = ijk[:count.value].copy()
    return (out, ext.value) if return_extremum else out


def local_minima_host(grid, tolerance=1e-2, *, maxima=False, return_extremum=False):
    """The same in NumPy: 26 rolled comparisons."""
    g = np.asarray(grid, dtype=np.float64)
    keep = np.ones(g.shape, dtype=bool)
    for d0 in (-1, 0, 1):
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                if d0 == d1 == d2 == 0:
                    continue
                n = np.roll(g, (d0, d1, d2), axis=(0, 1, 2))
                with np.errstate(invalid="ignore"):
                    keep &= (g > n) if maxima else (g < n)
    lin = np.flatnonzero(keep.ravel(order="F"))
    vals = g.ravel(order="F")[lin]
    ext = float(vals.min()) if lin.size else math.inf
    if lin.size and tolerance >= 0:
        if not ext < 0:
            raise ValueError("tolerance >= 0 needs a negative extremum (basins.jl:91)")
        thr = ext + abs(ext * tolerance)
        lin = lin[~(vals > thr)]
    a, b, _ = g.shape
    out = np.stack([lin % a, (lin // a) % b, lin // (a * b)], axis=1).astype(np.int32)
    return (out, ext) if return_extremum else out


# ---------------------------------------------------------------------------------------------------------------- components
def grid_components(grid, mode=_abi.COMPONENTS_NONZERO, lo=0.0, hi=0.0, *, want_labels=True, device=0, capacity=4096, stream=None,
                    labels_ptr=None) -> Components:
    """``ceg_grid_components`` as it stands: every component, in the order of discovery.  ``sum`` is exact for an int64 grid and
    empty for an FP64 one.  ``labels_ptr``: a device address for the labels instead of a host array (``labels`` is then ``None``)."""
    lib = _abi.load_library()
    ptr, on_dev, dims, dt, keep = _grid_arg(grid, (np.float64, np.int64) if mode == _abi.COMPONENTS_NONZERO else (np.float64,))
    is_i64 = int(dt == np.int64)
    n = dims[0] * dims[1] * dims[2]
    labels = np.empty(n, dtype=np.int32) if (want_labels and labels_ptr is None) else None
    lab_arg = C.c_void_p(int(labels_ptr)) if labels_ptr is not None else C.c_void_p(labels.ctypes.data if labels is not None else 0)
    count = C.c_int64(0)
    cap = max(int(capacity), 0)
    while True:
        seed, size = np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
        ssum = np.zeros(max(cap, 1), dtype=np.int64)
        _abi.check(lib, lib.ceg_grid_components(device, ptr, is_i64, on_dev, _abi.i32ptr(_dims_arg(dims)), int(mode), float(lo), float(hi),
                                                lab_arg, int(labels_ptr is not None), C.c_void_p(seed.ctypes.data), C.c_void_p(size.ctypes.data),
                                                C.c_void_p(ssum.ctypes.data if is_i64 else 0), 0, cap, C.byref(count), _stream(stream)))
        if count.value <= cap:
            break
        cap = int(count.value)
    k = int(count.value)
    return Components(None if labels is None else labels.reshape(dims, order="F"), np.arange(k, dtype=np.int32), seed[:k].copy(),
                      size[:k].copy(), ssum[:k].copy() if is_i64 else np.empty(0, dtype=np.int64))


def grid_components_host(grid, mode=_abi.COMPONENTS_NONZERO, lo=0.0, hi=0.0) -> Components:
    """The same in NumPy: every active point starts with its linear index as its label, takes the smallest label among its six
    periodic neighbours, and then its label's label (twice): labels are indices of points of the same component, so the jump
    shortens the chains.  Repeated until nothing changes; every component then carries its smallest index."""
    g = np.asarray(grid)
    if mode == _abi.COMPONENTS_NONZERO:
        active = g != 0
    else:
        with np.errstate(invalid="ignore"):
            active = (g > lo) & (g < hi)
    a, b, c = g.shape
    n = a * b * c
    big = np.int64(n)
    index = np.arange(n, dtype=np.int64).reshape(g.shape, order="F")
    lab = np.where(active, index, big)
    while True:
        new = lab
        for axis in range(3):
            for s in (1, -1):
                new = np.minimum(new, np.roll(lab, s, axis=axis))
        new = np.where(active, new, big)
        table = np.append(new.ravel(order="F"), big)                 # label of the point with that index; `big` stays `big`
        for _ in range(2):
            table = table[table]
        new = table[:n].reshape(g.shape, order="F")
        if np.array_equal(new, lab):
            break
        lab = new
    flat = lab.ravel(order="F")
    act = flat < big
    seeds, inv, sizes = np.unique(flat[act], return_inverse=True, return_counts=True)
    labels = np.full(n, -1, dtype=np.int32)
    labels[act] = inv.astype(np.int32)
    if g.dtype == np.int64:
        sums = np.zeros(seeds.size, dtype=np.int64)
        np.add.at(sums, inv, g.ravel(order="F")[act])
    else:
        sums = np.empty(0, dtype=np.int64)
    return Components(labels.reshape(g.shape, order="F"), np.arange(seeds.size, dtype=np.int32), seeds.astype(np.int32),
                      sizes.astype(np.int32), sums)


def _cut_components(comp: Components, values, total, atol, rtol, ntol) -> Components:
    """:300-311 from (seed, size, sum): drop sums below atol, sort by decreasing sum (stable, as ``sort!(...; rev=true)``), cut at
    ntol entries and where the running sum passes rtol of the grid's total"""
    sums = np.asarray(values)
    kept = np.flatnonzero(~(sums < atol))
    order = kept[np.argsort(-sums[kept], kind="stable")]
    max_tot = total * rtol if rtol < 1 else math.inf
    run, stop = 0.0, len(order)
    for pos, idx in enumerate(order):
        run += float(sums[idx])
        if pos + 1 > ntol or run > max_tot:
            stop = pos
            break
    order = order[:stop]
    return Components(comp.labels, comp.label[order], comp.seed[order], comp.size[order], sums[order])


def _float_sums(grid, labels, k):
    """per-component FP64 sums by label, in linear-index order (the reference adds in the order of its queue: last bits may differ)"""
    g = np.asarray(grid, dtype=np.float64).ravel(order="F")
    lab = labels.ravel(order="F")
    act = lab >= 0
    return np.bincount(lab[act], weights=g[act], minlength=k)


def local_components(grid, *, atol=0.0, rtol=1.0, ntol=math.inf, device=0, stream=None) -> Components:
    """``local_components(grid; atol, rtol, ntol)``: the connected components of the non-zero points, sorted by decreasing sum,
    those with a sum below ``atol`` dropped, cut at ``ntol`` entries and at the fraction ``rtol`` of the grid's total.  An int64
    grid (host or device) is summed exactly on the device; an FP64 grid must be a host array and is summed here by label."""
    comp = grid_components(grid, _abi.COMPONENTS_NONZERO, device=device, stream=stream)
    if comp.sum.size or not comp.seed.size:
        if isinstance(grid, tuple):
            total = float(comp.sum.sum())
        else:
            total = float(np.asarray(grid).sum())
        return _cut_components(comp, comp.sum, total, atol, rtol, ntol)
    if isinstance(grid, tuple):
        raise TypeError("FP64 sums per component are not computed on the device: pass the host array")
    return _cut_components(comp, _float_sums(grid, comp.labels, comp.seed.size), float(np.asarray(grid).sum()), atol, rtol, ntol)


def local_components_host(grid, *, atol=0.0, rtol=1.0, ntol=math.inf) -> Components:
    comp = grid_components_host(grid, _abi.COMPONENTS_NONZERO)
    g = np.asarray(grid)
    sums = comp.sum if g.dtype == np.int64 else _float_sums(g, comp.labels, comp.seed.size)
    return _cut_components(comp, sums, float(g.sum()), atol, rtol, ntol)


def compute_levels(grid, mine, maxe, *, device=0, stream=None) -> Components:
    """``compute_levels`` on a mean lattice (``ceg_energy_grid_reduced``): the components of ``mine < value < maxe``, in the order of
    discovery.  Strict on both sides (the reference admits ``==`` for the point a scan starts from)."""
    return grid_components(grid, _abi.COMPONENTS_BAND, mine, maxe, device=device, stream=stream)


def compute_levels_host(grid, mine, maxe) -> Components:
    return grid_components_host(np.asarray(grid, dtype=np.float64), _abi.COMPONENTS_BAND, mine, maxe)


# ---------------------------------------------------------------------------------------------------------------- sites
def snap_sites(sites, dims):
    """:471-484: the sites that snap to the voxel ``1 + round(dims*x)`` of an earlier site are deleted.  -> (kept sites, deleted
    0-based indices)"""
    s = np.asarray(sites, dtype=np.float64).reshape(-1, 3)
    vox = np.rint(s * np.asarray(dims, dtype=np.float64)).astype(np.int64)          # Julia's round: half to even
    seen, deleted = set(), []
    for idx, v in enumerate(map(tuple, vox)):
        if v in seen:
            deleted.append(idx)
        else:
            seen.add(v)
    keep = np.ones(len(s), dtype=bool)
    keep[deleted] = False
    return s[keep], np.asarray(deleted, dtype=np.int64)


def check_maxdist(dims, mat, maxdist):
    """the refusal of ``ceg_grid_site_proximity``: a ball of ``maxdist`` plus the skin must not meet its own image"""
    m = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    if not (maxdist > 0 and math.isfinite(maxdist)):
        raise ValueError("maxdist must be a positive number")
    det = abs(np.linalg.det(m))
    widths = [det / np.linalg.norm(np.cross(m[:, (q + 1) % 3], m[:, (q + 2) % 3])) for q in range(3)] if det > 0 else [0.0]
    protoskin = np.linalg.norm(m @ (1.0 / np.asarray(dims, dtype=np.float64)))
    if not 2.0 * (maxdist + protoskin) < min(widths):
        raise ValueError("maxdist: 2*(maxdist + voxel diagonal) must stay below the smallest width of the cell")


def site_proximity_map(sites, dims, mat, maxdist=2.0, *, device=0, stream=None, out_ptrs=None):
    """``site_proximity_map!(sites, dims, mat, maxdist)``.  ``sites``: (n, 3) fractional; ``mat``: the cell, columns = cell vectors.
    -> ``(site, offset, deleted)``: ``site[i, j, k]`` int32, 0 = none, else the 1-based index into the KEPT sites; ``offset[i, j, k, :]``
    int8; ``deleted`` the 0-based indices of the input sites that snapped to the voxel of an earlier one (the reference deletes them
    from ``sites``).  ``out_ptrs = (site_ptr, offset_ptr)``: write the map to device memory instead (``site`` / ``offset`` are ``None``)."""
    lib = _abi.load_library()
    dims = tuple(int(d) for d in dims)
    kept, deleted = snap_sites(sites, dims)
    m = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).reshape(3, 3).T).ravel()      # column-major
    n = dims[0] * dims[1] * dims[2]
    flat = np.ascontiguousarray(kept).ravel()
    if out_ptrs is None:
        site, off = np.empty(n, dtype=np.int32), np.empty((n, 3), dtype=np.int8)
        sp, op, on_dev = site.ctypes.data, off.ctypes.data, 0
    else:
        site = off = None
        sp, op, on_dev = int(out_ptrs[0]), int(out_ptrs[1]), 1
    _abi.check(lib, lib.ceg_grid_site_proximity(device, _abi.i32ptr(_dims_arg(dims)), _abi.dptr(m), _abi.dptr(flat) if len(kept) else None,
                                                len(kept), float(maxdist), C.c_void_p(sp), C.c_void_p(op), on_dev, _stream(stream)))
    if site is None:
        return None, None, deleted
    return site.reshape(dims, order="F"), np.moveaxis(off.T.reshape((3,) + dims, order="F"), 0, -1), deleted


def site_proximity_map_host(sites, dims, mat, maxdist=2.0):
    """The definition in NumPy, all 27 cell offsets per site: the nearest (site, offset) of every point, lowest site first among
    equals, assigned iff ``d2 < maxdist^2``."""
    dims = tuple(int(d) for d in dims)
    check_maxdist(dims, mat, maxdist)
    kept, deleted = snap_sites(sites, dims)
    m = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    a, b, c = dims
    w = np.stack(np.meshgrid(np.arange(a), np.arange(b), np.arange(c), indexing="ij"), axis=-1)      # (a, b, c, 3)
    best = np.full(dims, np.inf)
    site = np.zeros(dims, dtype=np.int32)
    off = np.zeros(dims + (3,), dtype=np.int8)
    dd = np.asarray(dims, dtype=np.float64)
    for s, x in enumerate(kept):
        sbest = np.full(dims, np.inf)
        soff = np.zeros(dims + (3,), dtype=np.int8)
        for o0 in (-1, 0, 1):
            for o1 in (-1, 0, 1):
                for o2 in (-1, 0, 1):
                    o = np.array([o0, o1, o2])
                    v = x - (w + o * np.asarray(dims)) / dd
                    d = v[..., 0, None] * m[:, 0] + v[..., 1, None] * m[:, 1] + v[..., 2, None] * m[:, 2]
                    d2 = (d * d).sum(axis=-1)
                    better = d2 < sbest
                    sbest = np.where(better, d2, sbest)
                    soff[better] = o
        better = sbest < best
        best = np.where(better, sbest, best)
        site[better] = s + 1
        off[better] = soff[better]
    out = best < maxdist * maxdist
    site[~out] = 0
    off[~out] = 0
    return site, off, deleted


def _map_arg(a, dtype, shape_tail=()):
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a)), 1, None
    arr = np.asarray(a, dtype=dtype)
    if shape_tail:                                   # offset[i, j, k, :] -> [x][3] with x in Julia's order
        arr = np.ascontiguousarray(np.moveaxis(arr, -1, 0).reshape(3, -1, order="F").T)
    else:
        arr = np.asfortranarray(arr)
    return C.c_void_p(arr.ctypes.data), 0, arr


def site_density(bins, site, offset, nsites, *, device=0, stream=None):
    """``ceg_grid_site_density``: ``(rho[nsites+1], moment[nsites+1, 3])`` int64, exact; the last entry is the unattributed rest.
    ``bins``: an int64 grid (host array or ``(device_ptr, dims)``); ``site`` / ``offset``: the map of ``site_proximity_map`` as arrays, or
    two device addresses."""
    lib = _abi.load_library()
    ptr, on_dev, dims, _, keep = _grid_arg(bins, (np.int64,))
    sp, s_dev, keep_s = _map_arg(site, np.int32)
    op, o_dev, keep_o = _map_arg(offset, np.int8, (3,))
    if s_dev != o_dev:
        raise ValueError("site and offset live in the same memory")
    if keep_s is not None and (keep_s.shape != tuple(dims) or keep_o.shape != (dims[0] * dims[1] * dims[2], 3)):
        raise ValueError("the proximity map and the bins differ in shape")
    rho, mom = np.zeros(nsites + 1, dtype=np.int64), np.zeros((nsites + 1, 3), dtype=np.int64)
    _abi.check(lib, lib.ceg_grid_site_density(device, ptr, on_dev, sp, op, s_dev, _abi.i32ptr(_dims_arg(dims)), int(nsites),
                                              C.c_void_p(rho.ctypes.data), C.c_void_p(mom.ctypes.data), 0, _stream(stream)))
    return rho, mom


def site_density_host(bins, site, offset, nsites):
    g = np.asarray(bins, dtype=np.int64)
    s = np.asarray(site)
    o = np.asarray(offset).astype(np.int64)
    a, b, c = g.shape
    nz = np.nonzero((g != 0) & (s >= 0) & (s <= nsites))
    lab = np.where(s[nz] == 0, nsites, s[nz] - 1)
    val = g[nz]
    rho, mom = np.zeros(nsites + 1, dtype=np.int64), np.zeros((nsites + 1, 3), dtype=np.int64)
    np.add.at(rho, lab, val)
    for q, (w, d) in enumerate(zip(nz, (a, b, c))):
        np.add.at(mom[:, q], lab, val * (o[nz][:, q] * d + w))
    return rho, mom


def _centres(rho, mom, dims):
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = mom.astype(np.float64) / (np.asarray(dims, dtype=np.float64)[None, :] * rho.astype(np.float64)[:, None])
    return [(float(r), p) for r, p in zip(rho, pos)]


def closest_from_proximity(bins, site, offset, nsites, *, device=0, stream=None):
    """``closest_from_proximity(grid, proximity, numsites)``: the list of ``(rho, pos)``, ``pos`` the fractional barycentre (NaN where
    ``rho`` is 0, as the reference's 0/0); entry ``nsites`` is the unattributed rest.  Divide ``rho`` by the number of frames times the
    atoms per frame for probabilities."""
    rho, mom = site_density(bins, site, offset, nsites, device=device, stream=stream)
    dims = bins[1] if isinstance(bins, tuple) else np.asarray(bins).shape
    return _centres(rho, mom, dims)


def closest_from_proximity_host(bins, site, offset, nsites):
    rho, mom = site_density_host(bins, site, offset, nsites)
    return _centres(rho, mom, np.asarray(bins).shape)


def proximal_map(bins, sites, mat, maxdist=2.0, *, device=0, stream=None):
    """``proximal_map(grid, sites, mat, maxdist)``: the density closest to each kept site and within ``maxdist``; the last entry is
    the rest.  -> ``(rho, deleted)``"""
    dims = bins[1] if isinstance(bins, tuple) else np.asarray(bins).shape
    site, off, deleted = site_proximity_map(sites, dims, mat, maxdist, device=device, stream=stream)
    nk = len(np.asarray(sites).reshape(-1, 3)) - len(deleted)
    rho, _ = site_density(bins, site, off, nk, device=device, stream=stream)
    return rho.astype(np.float64), deleted


def proximal_map_host(bins, sites, mat, maxdist=2.0):
    site, off, deleted = site_proximity_map_host(sites, np.asarray(bins).shape, mat, maxdist)
    nk = len(np.asarray(sites).reshape(-1, 3)) - len(deleted)
    rho, _ = site_density_host(bins, site, off, nk)
    return rho.astype(np.float64), deleted


# ---------------------------------------------------------------------------------------------------------------- basins
class Basins(NamedTuple):
    """``level[i, j, k]``: the breadth-first level at which the nearest start reaches the point, -1 where none does.  ``owner[i, j, k]``:
    the smallest index (into the list of starts) of a basin the point belongs to, -1 for none; ``nowners[i, j, k]`` (uint8): how many
    basins it belongs to.  ``shared`` (m, 2) int32: ``(linear index i + a*(j + b*k), owner)`` for every owner of every point with more
    than one, sorted by index then owner.  ``size[n]``: the points of each basin (0 for a start that was skipped or merged away by
    ``cluster``).  ``kept``: the indices of the starts that have a basin, ascending -- the reference's ``basinsets`` is
    ``[basin_points(b, i) for i in b.kept]``.  The start of basin ``i`` is its one point of level 0."""
    level: np.ndarray
    owner: np.ndarray
    nowners: np.ndarray
    shared: np.ndarray
    size: np.ndarray
    kept: np.ndarray


def circular_distance(a, m, n):
    """:108-113 as written, on 1-based coordinates: the wrapped distance is taken only when ``min(m, n) < a // 2 < max(m, n)``"""
    b = a // 2
    i, j = (m, n) if m <= n else (n, m)
    if i < b < j:
        return min(j - i, i - j + a)
    return j - i


def _cluster_reps(minima, cluster, dims):
    """``clean_cluster!`` (:116-128) over a list of 0-based minima -> ``unions`` (0-based positions in that list)"""
    m = np.asarray(minima, dtype=np.int64).reshape(-1, 3) + 1                    # the reference's coordinates are 1-based
    unions = np.arange(len(m))
    if not cluster > 0:
        return unions
    half = [d // 2 for d in dims]
    for i1 in range(len(m) - 1):
        dist = np.zeros(len(m) - i1 - 1, dtype=np.int64)
        for q in range(3):
            lo, hi = np.minimum(m[i1, q], m[i1 + 1:, q]), np.maximum(m[i1, q], m[i1 + 1:, q])
            dist += np.where((lo < half[q]) & (half[q] < hi), np.minimum(hi - lo, lo - hi + dims[q]), hi - lo)
        unions[i1 + 1:][dist <= cluster] = unions[i1]
    return unions


def _basins_from_pairs(level, pt, ow, nstarts, kept, dims):
    """the maps and lists from the (point, owner) pairs, duplicates allowed"""
    n = dims[0] * dims[1] * dims[2]
    key = np.unique(pt.astype(np.int64) * max(nstarts, 1) + ow.astype(np.int64))
    pt, ow = key // max(nstarts, 1), key % max(nstarts, 1)
    cnt = np.bincount(pt, minlength=n)
    if cnt.size and cnt.max(initial=0) > 255:
        raise ValueError("a point with more than 255 owners")
    owner = np.full(n, -1, dtype=np.int32)
    first = np.ones(pt.size, dtype=bool)
    first[1:] = pt[1:] != pt[:-1]
    owner[pt[first]] = ow[first]
    multi = cnt[pt] > 1
    shared = np.stack([pt[multi], ow[multi]], axis=1).astype(np.int32).reshape(-1, 2)
    size = np.bincount(ow, minlength=nstarts).astype(np.int32)
    return Basins(np.asarray(level, dtype=np.int32).reshape(dims, order="F"), owner.reshape(dims, order="F"),
                  cnt.astype(np.uint8).reshape(dims, order="F"), shared, size, np.asarray(kept, dtype=np.int64))


def _pairs(b: Basins):
    own, cnt = b.owner.ravel(order="F"), b.nowners.ravel(order="F")
    single = np.flatnonzero(cnt == 1)
    return np.concatenate([single, b.shared[:, 0].astype(np.int64)]), np.concatenate([own[single].astype(np.int64), b.shared[:, 1].astype(np.int64)])


def _apply_cluster(b: Basins, minima, cluster) -> Basins:
    """:250 over the kept minima: the owners relabelled to the basin they are merged into, duplicates removed"""
    if not cluster > 0 or not len(b.kept):
        return b
    dims = b.level.shape
    unions = _cluster_reps(np.asarray(minima).reshape(-1, 3)[b.kept], cluster, dims)
    rep = np.arange(len(b.size), dtype=np.int64)
    rep[b.kept] = b.kept[unions]
    pt, ow = _pairs(b)
    return _basins_from_pairs(b.level.ravel(order="F"), pt, rep[ow], len(b.size), np.unique(rep[b.kept]), dims)


def _starts_arg(minima):
    m = np.ascontiguousarray(np.asarray(minima, dtype=np.int64).reshape(-1, 3))
    if m.size and (m.min() < -2**31 or m.max() > 2**31 - 1):
        raise ValueError("a start does not fit int32")
    return m.astype(np.int32)


def local_basins(grid, minima=None, tolerance=-math.inf, *, maxima=False, cluster=0, skip_above=math.inf, maxdist=0, device=0,
                 stream=None) -> Basins:
    """``local_basins(grid, minima; lt, cluster, skip, maxdist)`` / ``local_basins(grid, tolerance; ...)`` on the device.  ``minima``:
    (n, 3) 0-based starts (distinct, inside the grid; they need not be minima), or ``None``: ``local_minima(grid, tolerance)`` runs
    first, on the device, and its list goes from device memory into ``ceg_grid_basins`` (this route allocates through torch).
    ``skip_above``: the reference's ``skip`` as ``v -> v > skip_above``.  ``cluster`` is applied on the host, over the list of kept
    minima.  A point with more than ``_abi.BASINS_MAX_OWNERS`` owners raises ``CegError`` (code -5)."""
    lib = _abi.load_library()
    ptr, on_dev, dims, _, keep = _grid_arg(grid, (np.float64,))
    n = dims[0] * dims[1] * dims[2]
    d32 = _dims_arg(dims)
    hold = []
    if minima is None:
        import torch
        dev = torch.device("cuda", device)
        if not on_dev:
            tg = torch.from_numpy(keep.ravel(order="F")).to(dev)
            torch.cuda.synchronize(dev)
            hold.append(tg)
            ptr, on_dev = C.c_void_p(tg.data_ptr()), 1
        count, cap = C.c_int64(0), 4096
        while True:
            tm = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            _abi.check(lib, lib.ceg_grid_local_minima(device, ptr, on_dev, _abi.i32ptr(d32), int(bool(maxima)), float(tolerance),
                                                      C.c_void_p(tm.data_ptr()), 1, cap, C.byref(count), None, _stream(stream)))
            if count.value <= cap:
                break
            cap = int(count.value)
        hold.append(tm)
        ns, sptr, s_dev = int(count.value), C.c_void_p(tm.data_ptr()), 1
        starts = None
    else:
        starts = _starts_arg(minima)
        ns, sptr, s_dev = len(starts), C.c_void_p(starts.ctypes.data if len(starts) else 0), 0
    level, owner = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    nown, size = np.empty(n, dtype=np.uint8), np.zeros(max(ns, 1), dtype=np.int32)
    count = C.c_int64(0)
    cap = n // 2 + 4096
    shared = np.empty((cap, 2), dtype=np.int32)

    def call(maps, cap, shared):
        _abi.check(lib, lib.ceg_grid_basins(device, ptr, on_dev, _abi.i32ptr(d32), sptr, s_dev, ns, int(bool(maxima)), float(skip_above),
                                            int(maxdist), C.c_void_p(level.ctypes.data if maps else 0), C.c_void_p(owner.ctypes.data if maps else 0),
                                            C.c_void_p(nown.ctypes.data if maps else 0), 0, C.c_void_p(shared.ctypes.data), cap, C.byref(count),
                                            C.c_void_p(size.ctypes.data if maps else 0), 0, _stream(stream)))

    call(True, cap, shared)
    if count.value > cap:                                            # the pairs alone, with the room they need
        cap = int(count.value)
        shared = np.empty((cap, 2), dtype=np.int32)
        call(False, cap, shared)
    size = size[:ns]
    b = Basins(level.reshape(dims, order="F"), owner.reshape(dims, order="F"), nown.reshape(dims, order="F"), shared[:count.value].copy(),
               size, np.flatnonzero(size > 0))
    if cluster > 0:
        if starts is None:
            starts = hold[-1][:ns].cpu().numpy()
        b = _apply_cluster(b, starts, cluster)
    return b


def basin_points(b: Basins, i):
    """the wrapped 0-based points (m, 3) of basin ``i`` (an index into the list of starts), in linear-index order"""
    a, bb, _ = b.level.shape
    lin = np.flatnonzero((b.owner.ravel(order="F") == i) & (b.nowners.ravel(order="F") == 1))
    lin = np.sort(np.concatenate([lin, b.shared[b.shared[:, 1] == i, 0].astype(np.int64)]))
    return np.stack([lin % a, (lin // a) % bb, lin // (a * bb)], axis=1).astype(np.int32)


def _decompose(b: Basins):
    a, bb, _ = b.level.shape
    pt, ow = _pairs(b)
    order = np.lexsort((ow, pt))
    pt, ow = pt[order], ow[order]
    lin, counts = np.unique(pt, return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    points = np.stack([lin % a, (lin // a) % bb, lin // (a * bb)], axis=1).astype(np.int32)
    return points, offsets, np.searchsorted(b.kept, ow).astype(np.int32)


def decompose_basins(grid, minima=None, tolerance=-math.inf, **kw):
    """``decompose_basins(grid, basinsets)`` / ``decompose_basins(grid, tolerance; ...)`` (:765-797) -> ``(points, offsets, owners)``:
    ``points`` (m, 3) the 0-based points that belong to a basin, sorted as :790 sorts them (k, then j, then i); the reference's
    ``nodes[points[p]]`` is ``owners[offsets[p]:offsets[p + 1]]``, ascending 0-based positions in the list of kept basins (``Basins.kept``).
    ``grid`` may be a ``Basins`` already computed; otherwise the arguments are those of ``local_basins``."""
    return _decompose(grid if isinstance(grid, Basins) else local_basins(grid, minima, tolerance, **kw))


def _lin_neighbour(lin, q, dims):
    a, b, c = dims
    i, j, k = lin % a, (lin // a) % b, lin // (a * b)
    step = 1 if q % 2 == 0 else -1
    if q // 2 == 0:
        i = (i + step) % a
    elif q // 2 == 1:
        j = (j + step) % b
    else:
        k = (k + step) % c
    return i + a * (j + b * k)


def local_basins_host(grid, minima=None, tolerance=-math.inf, *, maxima=False, cluster=0, skip_above=math.inf, maxdist=0) -> Basins:
    """The definition in NumPy, level by level over (point, owner) pairs: the pairs of level L + 1 are the pairs of level L moved
    along every edge to a point that no earlier level reached, duplicates removed."""
    g = np.asarray(grid, dtype=np.float64)
    if g.ndim != 3:
        raise ValueError("a grid has three axes")
    dims = g.shape
    a, b, c = dims
    n = a * b * c
    gf = g.ravel(order="F")
    starts = local_minima_host(g, tolerance, maxima=maxima) if minima is None else _starts_arg(minima)
    ns = len(starts)
    s64 = starts.astype(np.int64).reshape(-1, 3)
    if ns and (s64.min() < 0 or np.any(s64 >= np.asarray(dims))):
        raise ValueError("a start is outside the grid")
    lin0 = s64[:, 0] + a * (s64[:, 1] + b * s64[:, 2])
    if len(np.unique(lin0)) != ns:
        raise ValueError("a start repeats an earlier start")
    alive = ~(gf[lin0] > skip_above)
    level = np.full(n, -1, dtype=np.int32)
    pt, ow = lin0[alive], np.flatnonzero(alive)
    level[pt] = 0
    all_pt, all_ow = [pt], [ow]
    L = 0
    while pt.size and (maxdist == 0 or L + 1 <= maxdist - 1):
        cv, co = [], []
        for q in range(6):
            v = _lin_neighbour(pt, q, dims)
            with np.errstate(invalid="ignore"):
                edge = ((gf[pt] > gf[v]) if maxima else (gf[pt] < gf[v])) & ~(gf[v] > skip_above) & (level[v] < 0)
            cv.append(v[edge])
            co.append(ow[edge])
        key = np.unique(np.concatenate(cv) * max(ns, 1) + np.concatenate(co))
        pt, ow = key // max(ns, 1), key % max(ns, 1)
        L += 1
        level[pt] = L
        all_pt.append(pt)
        all_ow.append(ow)
    out = _basins_from_pairs(level, np.concatenate(all_pt), np.concatenate(all_ow), ns, np.flatnonzero(alive), dims)
    return _apply_cluster(out, starts, cluster)


def decompose_basins_host(grid, minima=None, tolerance=-math.inf, **kw):
    return _decompose(grid if isinstance(grid, Basins) else local_basins_host(grid, minima, tolerance, **kw))


# ---------------------------------------------------------------------------------------------------------------- site extraction
# From a density map to the list of sites: average_clusters (averageclusters.jl:280-294), coalescing_basins (basins.jl:661-731),
# closest_to_sites (:324-437), updated_sites_with_closest (:447-456), cluster_closer_than! (:613-642), on top of ceg_grid_smooth /
# ceg_grid_ranked / ceg_grid_coalesce / ceg_grid_site_partition (device) and ceg_cluster_closer_than (host, in the library);
# ceg_grid_site_nearest and ceg_coalesce_ranked are the stages on their own.
#
# A density map is an FP64 grid, or the sampler's int64 bins with the number of frames ``counter``: its values are then
# ``bins * (1.0 / counter)`` -- one multiplication per voxel, the form the device applies; the reference's ``bins ./ counter`` can differ
# from it in the last bit.
class ClosestSites(NamedTuple):
    """``sums[s]``: the density attributed to kept site ``s``; ``centres[s]``: the value-weighted centre of its voxels, fractional, with the
    cell offsets applied (NaN where ``sums`` is 0); ``deleted``: the 0-based indices of the input sites that snapped to the voxel of an
    earlier one; ``cap_bound``: whether the cap ``s + rho > 1`` (basins.jl:430) skipped a voxel."""
    sums: np.ndarray
    centres: np.ndarray
    deleted: np.ndarray
    cap_bound: bool


def _mat_arg(mat):
    m = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    return m, np.ascontiguousarray(m.T).ravel()                                  # column-major for the library


def _periodic_setup(m):
    from .hostmirror.utils import prepare_periodic_distance_computations
    ortho, safemin = prepare_periodic_distance_computations(m)
    return bool(ortho), float(safemin)


def _as_density(grid):
    """a host array of any integer dtype is a map of counts: handed on as int64 (the library's bins); everything else as it is"""
    if isinstance(grid, tuple):
        return grid
    arr = np.asarray(grid)
    if arr.dtype.kind in "iu" and arr.dtype != np.int64:
        if arr.dtype == np.uint64 and arr.size and arr.max() >= 2**63:
            raise ValueError("a bin does not fit int64")
        arr = arr.astype(np.int64)
    return arr


def _is_bins(grid, counter):
    if isinstance(grid, tuple):
        return np.dtype(grid[2] if len(grid) > 2 else (np.int64 if counter is not None else np.float64)) == np.int64
    return np.asarray(grid).dtype.kind in "iu"


def _density_values(grid, counter, device=0, stream=None):
    """-> (flat FP64 values in Julia's order, dims).  A map in device memory comes back through ``ceg_grid_smooth`` with the one tap
    1.0 per axis: ``fma(1.0, x, 0.0)`` is ``x``, and int64 bins arrive scaled as every other stage sees them."""
    grid = _as_density(grid)
    bins = _is_bins(grid, counter)
    if bins and counter is None:
        raise ValueError("integer bins need their counter")
    scale = 1.0 / float(counter) if bins else 1.0
    if isinstance(grid, tuple):
        dims = tuple(int(d) for d in grid[1])
        one = np.ones(1)
        src = (grid[0], dims, np.int64 if bins else np.float64)
        return smooth_grid(src, (one, one, one), scale=scale, device=device, stream=stream).ravel(order="F"), dims
    flat = grid.ravel(order="F")
    if bins:
        if flat.size and np.abs(flat).max() >= 2**53:
            raise ValueError("a bin with |value| >= 2^53")
        return flat.astype(np.float64) * scale, tuple(grid.shape)
    return np.ascontiguousarray(flat, dtype=np.float64), tuple(grid.shape)


def _device_map(grid, counter, values, dims, device):
    """the map as the device stages of one pipeline call take it: where it already lies in device memory, else uploaded once (bins as
    bins, an FP64 map as it is).  -> (grid argument, FP64 view in device memory or None, keepalive)"""
    grid, bins, _ = _map_scale(grid, counter)
    if isinstance(grid, tuple):
        return grid, (None if bins else grid), None
    import torch
    dev = torch.device("cuda", device)
    t = torch.from_numpy(np.ascontiguousarray(grid.ravel(order="F")) if bins else values).to(dev)
    torch.cuda.synchronize(dev)
    arg = (t.data_ptr(), dims, np.int64 if bins else np.float64)
    return arg, (None if bins else arg), t


def gaussian_taps(sigma):
    """The taps of one axis: ``[1.0]`` for ``sigma == 0``, else ``w = 2*ceil(sigma)`` and ``g[x] = exp(-x^2/(2 sigma^2))`` for
    ``x = -w..w`` divided by their sum.  This definition is this package's (what ImageFiltering's ``KernelFactors.gaussian`` computes
    as far as its documentation goes; the package was not at hand to compare)."""
    sigma = float(sigma)
    if not (sigma >= 0 and math.isfinite(sigma)):
        raise ValueError("sigma must be a finite number >= 0")
    if sigma == 0:
        return np.ones(1)
    w = 2 * int(math.ceil(sigma))
    x = np.arange(-w, w + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def smoothing_sigmas(dims, mat, smooth=None):
    """:667-668: ``sigma_c = smooth * dims[c] / |column c of mat|``; ``smooth=None`` is the voxel diagonal ``|mat * (1 ./ dims)|``"""
    m = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    d = np.asarray(dims, dtype=np.float64)
    if smooth is None:
        smooth = float(np.linalg.norm(m @ (1.0 / d)))
    return tuple(float(smooth) * d[c] / float(np.linalg.norm(m[:, c])) for c in range(3))


def _taps_arg(taps):
    if len(taps) != 3:
        raise ValueError("three tap arrays, one per axis")
    return [np.ascontiguousarray(t, dtype=np.float64).ravel() for t in taps]


def smooth_grid(grid, taps, *, scale=1.0, device=0, stream=None, out_ptr=None):
    """``ceg_grid_smooth``: the circular separable filter of ``grid`` (FP64, or int64 bins times ``scale``) with ``taps = (t0, t1, t2)``,
    one odd-length array per axis (``gaussian_taps``).  ``y[p] = sum_t taps[t + w] * x[(p + t) mod n]`` with ``t`` ascending and one fma per
    tap, along axis 0, then 1, then 2.  -> the FP64 array, or ``None`` with ``out_ptr`` (a device address that receives it)."""
    lib = _abi.load_library()
    ptr, on_dev, dims, dt, keep = _grid_arg(_as_density(grid), (np.float64, np.int64))
    t0, t1, t2 = _taps_arg(taps)
    out = None if out_ptr is not None else np.empty(dims[0] * dims[1] * dims[2], dtype=np.float64)
    _abi.check(lib, lib.ceg_grid_smooth(device, ptr, int(dt == np.int64), on_dev, float(scale), _abi.i32ptr(_dims_arg(dims)), _abi.dptr(t0),
                                        len(t0), _abi.dptr(t1), len(t1), _abi.dptr(t2), len(t2),
                                        C.c_void_p(int(out_ptr) if out_ptr is not None else out.ctypes.data), int(out_ptr is not None),
                                        _stream(stream)))
    return None if out is None else out.reshape(dims, order="F")


def smooth_grid_host(grid, taps, *, scale=1.0, dtype=np.float64):
    """The same three passes in NumPy, in ``dtype`` (``np.longdouble`` for a reference).  A multiplication and an addition per tap where
    the device has one fma: the two agree to within the bound of the rounding analysis, not to the bit."""
    g = np.asarray(grid)
    x = g.astype(np.float64) * np.float64(scale) if g.dtype.kind in "iu" else g.astype(np.float64)
    x = x.astype(dtype)
    for axis, t in enumerate(_taps_arg(taps)):
        w = len(t) // 2
        acc = np.zeros_like(x)
        for q in range(len(t)):
            acc = acc + t[q].astype(dtype) * np.roll(x, -(q - w), axis=axis)
        x = acc
    return x


def ranked_above(grid, crop, *, device=0, stream=None, capacity=None):
    """``ceg_grid_ranked``: ``(lin, values)`` -- the 0-based linear indices (``i + a*(j + b*k)``) of the voxels with a value ``> crop``,
    by decreasing value, equal values by ascending index (``sortperm(vec(grid), rev=true)`` cut at ``<= crop``), and those values.
    A NaN is dropped (the reference would visit it first); ``crop >= 0``."""
    lib = _abi.load_library()
    ptr, on_dev, dims, _, keep = _grid_arg(grid, (np.float64,))
    n = dims[0] * dims[1] * dims[2]
    cap = n if capacity is None else max(int(capacity), 0)
    count = C.c_int64(0)
    while True:
        idx, val = np.empty(max(cap, 1), dtype=np.int32), np.empty(max(cap, 1), dtype=np.float64)
        _abi.check(lib, lib.ceg_grid_ranked(device, ptr, on_dev, _abi.i32ptr(_dims_arg(dims)), float(crop), C.c_void_p(idx.ctypes.data),
                                            C.c_void_p(val.ctypes.data), 0, cap, C.byref(count), _stream(stream)))
        if count.value <= cap:
            break
        cap = int(count.value)
    return idx[:count.value].copy(), val[:count.value].copy()


def ranked_above_host(grid, crop):
    if not crop >= 0:
        raise ValueError("crop must be a number >= 0")
    flat = np.asarray(grid, dtype=np.float64).ravel(order="F")
    with np.errstate(invalid="ignore"):
        sel = np.flatnonzero(flat > crop)
    order = sel[np.argsort(-flat[sel], kind="stable")]
    return order.astype(np.int32), flat[order]


def _sites_arg(sites):
    s = np.ascontiguousarray(np.asarray(sites, dtype=np.float64).reshape(-1, 3))
    if not len(s):
        raise ValueError("at least one site")
    if not np.all(np.abs(s) <= 64.0):
        raise ValueError("fractional site coordinates must be finite with |x| <= 64")
    return s


def site_nearest(sites, dims, mat, *, bins=None, origin=0, device=0, stream=None, capacity=None, want_dist=True):
    """``ceg_grid_site_nearest``: for every active voxel (``bins != 0``; every voxel without ``bins``) the site at the smallest
    ``periodic_distance_with_ofs!`` of ``site - (w + origin) ./ dims``, the lowest index among equals, at any distance (phase 2 of
    ``closest_to_sites``).  ``bins``: an int64 grid, host array or ``(device_ptr, dims)``.  -> ``(lin, site, offset, dist)`` in
    linear-index order: int32 0-based linear indices, int32 0-based sites, int8 (n, 3) cell offsets, FP64 distances (``None``
    without ``want_dist``)."""
    lib = _abi.load_library()
    dims = tuple(int(d) for d in dims)
    m, mcol = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    s = _sites_arg(sites)
    n = dims[0] * dims[1] * dims[2]
    if bins is None:
        bptr, b_dev, keep = C.c_void_p(0), 0, None
    else:
        bptr, b_dev, bdims, _, keep = _grid_arg(bins, (np.int64,))
        if tuple(bdims) != dims:
            raise ValueError("bins and dims differ")
    cap = n if capacity is None else max(int(capacity), 0)
    count = C.c_int64(0)
    while True:
        k = max(cap, 1)
        lin, site, off = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32), np.empty((k, 3), dtype=np.int8)
        dist = np.empty(k, dtype=np.float64) if want_dist else None
        _abi.check(lib, lib.ceg_grid_site_nearest(device, _abi.i32ptr(_dims_arg(dims)), _abi.dptr(mcol), int(ortho), safemin, _abi.dptr(s.ravel()),
                                                  len(s), int(origin), bptr, b_dev, C.c_void_p(lin.ctypes.data), C.c_void_p(site.ctypes.data),
                                                  C.c_void_p(off.ctypes.data), C.c_void_p(dist.ctypes.data if want_dist else 0), 0, cap,
                                                  C.byref(count), _stream(stream)))
        if count.value <= cap:
            break
        cap = int(count.value)
    k = int(count.value)
    return lin[:k].copy(), site[:k].copy(), off[:k].copy(), (dist[:k].copy() if want_dist else None)


def _pdwo_many(m, ortho, safemin, buf):
    """``periodic_distance_with_ofs!`` (utils.jl:257-280) over the rows of ``buf`` (n, 3), vectorised, operation by operation
    -> (d, ofs int64 (n, 3))"""
    def norm(v):
        x = m[0, 0] * v[:, 0] + m[0, 1] * v[:, 1] + m[0, 2] * v[:, 2]
        y = m[1, 0] * v[:, 0] + m[1, 1] * v[:, 1] + m[1, 2] * v[:, 2]
        z = m[2, 0] * v[:, 0] + m[2, 1] * v[:, 1] + m[2, 2] * v[:, 2]
        return np.sqrt(x * x + y * y + z * z)

    diff = buf + 0.5
    fl = np.floor(diff)
    ofs = fl.astype(np.int64)
    v = diff - fl - 0.5
    d = norm(v)
    if ortho:
        return d, ofs
    ref = d.copy()
    live = ~(ref <= safemin)                                  # rows still in the search
    for q in range(3):
        v[:, q] = v[:, q] + 1
        nn = norm(v)
        hit = live & (nn < ref)
        d[hit], ofs[hit, q], live = nn[hit], ofs[hit, q] - 1, live & ~hit
        v[:, q] = v[:, q] - 2
        nn = norm(v)
        hit = live & (nn < ref)
        d[hit], ofs[hit, q], live = nn[hit], ofs[hit, q] + 1, live & ~hit
        v[:, q] = v[:, q] + 1
    return d, ofs


def site_nearest_host(sites, dims, mat, *, bins=None, origin=0, want_dist=True):
    """The same in NumPy, one site at a time over all the active voxels."""
    dims = tuple(int(d) for d in dims)
    if origin not in (0, 1):
        raise ValueError("origin is 0 or 1")
    m, _ = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    s = _sites_arg(sites)
    a, b, c = dims
    if bins is None:
        lin = np.arange(a * b * c, dtype=np.int64)
    else:
        lin = np.flatnonzero(np.asarray(bins).ravel(order="F") != 0)
    w = np.stack([lin % a, (lin // a) % b, lin // (a * b)], axis=1) + origin
    frac = w.astype(np.float64) / np.asarray(dims, dtype=np.float64)
    best = np.full(len(lin), np.inf)
    site = np.zeros(len(lin), dtype=np.int32)
    off = np.zeros((len(lin), 3), dtype=np.int8)
    for idx, x in enumerate(s):
        d, o = _pdwo_many(m, ortho, safemin, x[None, :] - frac)
        better = d < best
        best = np.where(better, d, best)
        site[better] = idx
        off[better] = o[better]
    return lin.astype(np.int32), site, off, (best if want_dist else None)


def _pdwo_one(m, ortho, safemin, buf):
    """``periodic_distance_with_ofs!`` on one difference, plain floats -> (d, ofs list of float)"""
    def norm(v):
        x = m[0][0] * v[0] + m[0][1] * v[1] + m[0][2] * v[2]
        y = m[1][0] * v[0] + m[1][1] * v[1] + m[1][2] * v[2]
        z = m[2][0] * v[0] + m[2][1] * v[1] + m[2][2] * v[2]
        return math.sqrt(x * x + y * y + z * z)

    v, ofs = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for q in range(3):
        diff = buf[q] + 0.5
        ofs[q] = float(math.floor(diff))
        v[q] = diff - ofs[q] - 0.5
    ref = norm(v)
    if ortho or ref <= safemin:
        return ref, ofs
    for q in range(3):
        v[q] += 1
        nn = norm(v)
        if nn < ref:
            ofs[q] -= 1
            return nn, ofs
        v[q] -= 2
        nn = norm(v)
        if nn < ref:
            ofs[q] += 1
            return nn, ofs
        v[q] += 1
    return ref, ofs


def coalesce_ranked(lin, smoothed, values, dims, mat, maxdist, atol=0.1, maxbasins=math.inf):
    """``ceg_coalesce_ranked``: the greedy pass of ``coalescing_basins`` (:677-719) over a ranking already cut at the crop, in the
    library (host code, no device).  ``lin`` / ``smoothed``: what ``ranked_above`` returns; ``values``: the unsmoothed map at ``lin``.
    -> list of ``(value, centre)``, ``centre`` a length-3 array."""
    lib = _abi.load_library()
    lin = np.ascontiguousarray(lin, dtype=np.int32)
    sm = np.ascontiguousarray(smoothed, dtype=np.float64)
    va = np.ascontiguousarray(values, dtype=np.float64)
    if not (len(lin) == len(sm) == len(va)):
        raise ValueError("lin, smoothed and values differ in length")
    m, mcol = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    cap, count = max(len(lin), 1), C.c_int64(0)
    val, cen = np.empty(cap, dtype=np.float64), np.empty((cap, 3), dtype=np.float64)
    _abi.check(lib, lib.ceg_coalesce_ranked(_abi.i32ptr(lin), _abi.dptr(sm), _abi.dptr(va), len(lin), _abi.i32ptr(_dims_arg(dims)),
                                            _abi.dptr(mcol), int(ortho), safemin, float(maxdist), float(atol), float(maxbasins),
                                            _abi.dptr(val), _abi.dptr(cen.ravel()), cap, C.byref(count)))
    return [(float(val[q]), cen[q].copy()) for q in range(int(count.value))]


def coalesce_ranked_host(lin, smoothed, values, dims, mat, maxdist, atol=0.1, maxbasins=math.inf):
    """The same loop in plain Python floats: the same IEEE operations in the same order, so the same bits."""
    m, _ = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    ml = m.tolist()
    a, b, c = (int(d) for d in dims)
    ret = []
    for x, smval, val in zip(np.asarray(lin).tolist(), np.asarray(smoothed, dtype=np.float64).tolist(),
                             np.asarray(values, dtype=np.float64).tolist()):
        i, j, k = x % a + 1, (x // a) % b + 1, x // (a * b) + 1
        pos = [i / a, j / b, k / c]
        in_distance = []
        for idx, (_, center) in enumerate(ret):
            d, ofs = _pdwo_one(ml, ortho, safemin, [pos[q] - center[q] for q in range(3)])
            if d > maxdist:
                continue
            in_distance.append((idx, ofs, d))
        if not in_distance and smval >= atol:
            ret.append((val, pos))
            if len(ret) >= maxbasins:
                break
            continue
        if len(in_distance) > 1:
            in_distance.sort(key=lambda e: (math.isnan(e[2]), e[2]))
            submid = 1 if val < atol else next((q + 1 for q, e in enumerate(in_distance) if e[2] < maxdist / 2), 1)
            del in_distance[submid:]
        newcenter = [pos[q] * val for q in range(3)]
        newval = val
        for j2, o2, _ in in_distance:
            val2, center2 = ret[j2]
            for q in range(3):
                newcenter[q] += (center2[q] + o2[q]) * val2
            newval += val2
        if newval == 0:
            continue
        newcenter = [x / newval for x in newcenter]
        if len(in_distance) == 1:
            ret[in_distance[0][0]] = (newval, newcenter)
        else:
            for j2 in sorted((e[0] for e in in_distance), reverse=True):
                del ret[j2]
            ret.append((newval, newcenter))
    return [(float(v), np.asarray(p, dtype=np.float64)) for v, p in ret]


def _map_scale(grid, counter):
    """-> (grid as the library takes it, is bins, scale)"""
    grid = _as_density(grid)
    bins = _is_bins(grid, counter)
    if bins and counter is None:
        raise ValueError("integer bins need their counter")
    if isinstance(grid, tuple):
        grid = (grid[0], tuple(int(d) for d in grid[1]), np.int64 if bins else np.float64)
    return grid, bins, (1.0 / float(counter)) if bins else 1.0


def grid_coalesce(lin, smoothed, grid, mat, maxdist, atol=0.1, maxbasins=math.inf, *, counter=None, nranked=None, voxels_per_launch=0,
                  device=0, stream=None, out_ptrs=None, capacity=None):
    """``ceg_grid_coalesce``: the greedy pass of ``coalescing_basins`` on the device, the bytes of ``coalesce_ranked``.  ``lin`` /
    ``smoothed``: the ranking as ``ranked_above`` returns it, or two device addresses with ``nranked``.  ``grid``: the unsmoothed map, FP64
    or int64 bins with ``counter``, host array or ``(device_ptr, dims[, dtype])``; the kernel gathers the values itself.
    ``voxels_per_launch``: the cut of the run into launches (0: the default); the result does not depend on it.
    -> list of ``(value, centre)``; with ``out_ptrs = (value_ptr, centre_ptr)`` and ``capacity`` the basins go to device memory and the
    full count is returned."""
    lib = _abi.load_library()
    grid, bins, scale = _map_scale(grid, counter)
    gptr, g_dev, dims, dt, keep = _grid_arg(grid, (np.float64, np.int64))
    if isinstance(lin, (int, np.integer)):
        if nranked is None:
            raise ValueError("a ranking in device memory needs nranked")
        nr, lptr, sptr, r_dev = int(nranked), C.c_void_p(int(lin)), C.c_void_p(int(smoothed)), 1
    else:
        lin = np.ascontiguousarray(lin, dtype=np.int32)
        sm = np.ascontiguousarray(smoothed, dtype=np.float64)
        if len(lin) != len(sm):
            raise ValueError("lin and smoothed differ in length")
        nr, lptr, sptr, r_dev = len(lin), C.c_void_p(lin.ctypes.data), C.c_void_p(sm.ctypes.data), 0
    m, mcol = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    count = C.c_int64(0)
    if out_ptrs is None:
        cap = max(nr, 1) if capacity is None else max(int(capacity), 0)
        val, cen = np.empty(max(cap, 1), dtype=np.float64), np.empty((max(cap, 1), 3), dtype=np.float64)
        vptr, cptr, o_dev = C.c_void_p(val.ctypes.data), C.c_void_p(cen.ctypes.data), 0
    else:
        if capacity is None:
            raise ValueError("device outputs need their capacity")
        cap, vptr, cptr, o_dev = max(int(capacity), 0), C.c_void_p(int(out_ptrs[0])), C.c_void_p(int(out_ptrs[1])), 1
    _abi.check(lib, lib.ceg_grid_coalesce(device, lptr, sptr, r_dev, nr, gptr, int(dt == np.int64), g_dev, scale, _abi.i32ptr(_dims_arg(dims)),
                                          _abi.dptr(mcol), int(ortho), safemin, float(maxdist), float(atol), float(maxbasins),
                                          int(voxels_per_launch), vptr, cptr, o_dev, cap, C.byref(count), _stream(stream)))
    if out_ptrs is not None:
        return int(count.value)
    return [(float(val[q]), cen[q].copy()) for q in range(min(int(count.value), cap))]


class SitePartition(NamedTuple):
    """``sums[s]``, ``centres[s]`` (NaN for a site without a voxel), ``cap_bound``, ``count`` (the active voxels) of ``site_partition``;
    ``sums`` and ``centres`` are ``None`` where they went to device memory"""
    sums: np.ndarray
    centres: np.ndarray
    cap_bound: bool
    count: int


def site_partition(grid, sites, mat, *, counter=None, origin=0, device=0, stream=None, out_ptrs=None) -> SitePartition:
    """``ceg_grid_site_partition``: stages 2 and 3 of ``closest_to_sites`` in one device call, for any number of sites: every non-zero
    voxel of the map goes to its nearest site (``site_nearest`` with that ``origin``), and each site adds its voxels up in linear-index
    order under the cap (``_accumulate_closest``).  ``sites`` are taken as they are (``closest_to_sites`` snaps them first).  ``grid``: FP64
    or int64 bins with ``counter``, host array or ``(device_ptr, dims[, dtype])``.  ``out_ptrs = (sums_ptr, centres_ptr)``: device outputs."""
    lib = _abi.load_library()
    grid, bins, scale = _map_scale(grid, counter)
    gptr, g_dev, dims, dt, keep = _grid_arg(grid, (np.float64, np.int64))
    m, mcol = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    s = _sites_arg(sites)
    cap_bound, count = C.c_int32(0), C.c_int64(0)
    if out_ptrs is None:
        sums, cen = np.empty(len(s), dtype=np.float64), np.empty((len(s), 3), dtype=np.float64)
        sp, cp, o_dev = C.c_void_p(sums.ctypes.data), C.c_void_p(cen.ctypes.data), 0
    else:
        sums = cen = None
        sp, cp, o_dev = C.c_void_p(int(out_ptrs[0])), C.c_void_p(int(out_ptrs[1])), 1
    _abi.check(lib, lib.ceg_grid_site_partition(device, gptr, int(dt == np.int64), g_dev, scale, _abi.i32ptr(_dims_arg(dims)), _abi.dptr(mcol),
                                                int(ortho), safemin, _abi.dptr(s.ravel()), len(s), int(origin), sp, cp, o_dev,
                                                C.byref(cap_bound), C.byref(count), _stream(stream)))
    return SitePartition(sums, cen, bool(cap_bound.value), int(count.value))


def cluster_closer_than_host(ret, mat, maxdist):
    """``cluster_closer_than!`` (:613-642) on a list of ``(rho, pos)``: a later entry within ``maxdist`` of an earlier one is merged into
    it (value-weighted centre, the offset applied) unless the two together exceed 1.  -> the new list.  Plain Python floats."""
    m, _ = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    ml = m.tolist()
    ret = [(float(r), [float(x) for x in p]) for r, p in ret]
    n = len(ret)
    todelete = [False] * n
    for i1 in range(n):
        if todelete[i1]:
            continue
        rho1, pos1 = ret[i1]
        for i2 in range(i1 + 1, n):
            if todelete[i2]:
                continue
            rho2, pos2 = ret[i2]
            rho = rho1 + rho2
            if rho > 1:
                continue
            d, ofs = _pdwo_one(ml, ortho, safemin, [pos1[q] - pos2[q] for q in range(3)])
            if d >= maxdist:
                continue
            todelete[i2] = True
            pos1 = [(rho1 * pos1[q] + rho2 * (pos2[q] + ofs[q])) / rho for q in range(3)]
            rho1 = rho
            ret[i1] = (rho1, pos1)
    return [(r, np.asarray(p, dtype=np.float64)) for (r, p), dead in zip(ret, todelete) if not dead]


def cluster_closer_than(ret, mat, maxdist):
    """``ceg_cluster_closer_than``: the same loop in the library's host code (no device needed), the same bits."""
    lib = _abi.load_library()
    m, mcol = _mat_arg(mat)
    ortho, safemin = _periodic_setup(m)
    n = len(ret)
    rho = np.ascontiguousarray([r for r, _ in ret], dtype=np.float64).reshape(n)
    pos = np.ascontiguousarray([p for _, p in ret], dtype=np.float64).reshape(n, 3)
    count = C.c_int64(0)
    _abi.check(lib, lib.ceg_cluster_closer_than(_abi.dptr(rho), _abi.dptr(pos.reshape(-1)), n, _abi.dptr(mcol), int(ortho), safemin, float(maxdist),
                                                C.byref(count)))
    return [(float(rho[q]), pos[q].copy()) for q in range(int(count.value))]


def _accumulate_closest(values, dims, nsites, lin, site, off, deleted) -> ClosestSites:
    """stage 3 of ``closest_to_sites``: the voxels in linear-index order, each added to its nearest site unless that takes the site's
    sum above 1 (:425-434), and the centres of ``updated_sites_with_closest`` (:454): ``sum(((ijk + ofs.*dims) ./ dims) .* w) / s`` on
    0-based ``ijk``"""
    a, b, c = dims
    sums = [0.0] * nsites
    acc = [[0.0, 0.0, 0.0] for _ in range(nsites)]
    cap_bound = False
    vals = values[lin].tolist()
    for x, s, o, rho in zip(np.asarray(lin).tolist(), np.asarray(site).tolist(), np.asarray(off).tolist(), vals):
        if sums[s] + rho > 1:
            cap_bound = True
            continue
        sums[s] = sums[s] + rho
        w = (x % a, (x // a) % b, x // (a * b))
        for q in range(3):
            acc[s][q] += (w[q] + o[q] * dims[q]) / dims[q] * rho
    with np.errstate(invalid="ignore", divide="ignore"):
        centres = np.asarray(acc, dtype=np.float64).reshape(nsites, 3) / np.asarray(sums, dtype=np.float64)[:, None]
    return ClosestSites(np.asarray(sums, dtype=np.float64), centres, np.asarray(deleted, dtype=np.int64), cap_bound)


def _closest_to_sites(grid, sites, mat, counter, on_device, device=0, stream=None, prepared=None) -> ClosestSites:
    """``prepared``: what a caller that runs several rounds on one map has already -- ``(values, dims)`` for the host route, the map
    as ``site_partition`` takes it (device-resident) and ``dims`` for the device route"""
    if on_device:
        if prepared is None:
            grid = _as_density(grid)
            dims = tuple(int(d) for d in (grid[1] if isinstance(grid, tuple) else grid.shape))
        else:
            grid, dims = prepared
        kept, deleted = snap_sites(sites, dims)
        part = site_partition(grid, kept, mat, counter=counter, origin=0, device=device, stream=stream)
        return ClosestSites(part.sums, part.centres, np.asarray(deleted, dtype=np.int64), part.cap_bound)
    values, dims = _density_values(grid, counter, device, stream) if prepared is None else prepared
    kept, deleted = snap_sites(sites, dims)
    lin, site, off, _ = site_nearest_host(kept, dims, mat, bins=(values != 0).reshape(dims, order="F"), origin=0, want_dist=False)
    return _accumulate_closest(values, dims, len(kept), lin, site, off, deleted)


def closest_to_sites(grid, sites, mat, *, counter=None, device=0, stream=None) -> ClosestSites:
    """The partition of the non-zero voxels of a density map among ``sites`` (fractional, (n, 3)), device-backed: the sites are
    snapped and deduplicated (``snap_sites``), every non-zero voxel gets its nearest kept site with ``origin = 0``, and each site adds its
    voxels up in linear-index order under the reference's cap (a voxel that would take its site's sum above 1 is skipped, :430), all in
    one ``ceg_grid_site_partition`` call, for any number of sites.  ``grid``: an FP64 map, or int64 bins with ``counter``; host array or ``(device_ptr, dims[,
    dtype])``.

    Where this differs from ``closest_to_sites`` of the reference as written (:324-437): the reference first gives each site the
    voxels inside half its nearest-site distance, in breadth-first order, and breaks off when the running sum passes 1 (:347-382);
    and it measures the phase-2 distances one voxel off (``Tuple(tovisit) ./ dims`` on 1-based indices, ``origin = 1``).  The two
    agree whenever the cap does not bind, except at voxels whose two nearest sites differ in distance by at most
    ``2*|mat*(1 ./ dims)|``."""
    return _closest_to_sites(grid, sites, mat, counter, True, device, stream)


def closest_to_sites_host(grid, sites, mat, *, counter=None) -> ClosestSites:
    return _closest_to_sites(grid, sites, mat, counter, False)


def updated_sites_with_closest(closest: ClosestSites):
    """``updated_sites_with_closest`` (:447-456) -> list of ``(sum, centre)``; an empty site raises like the reference's ``error``"""
    if np.any(closest.sums == 0):
        raise ValueError("Encountered empty weight: please use a non-zero atol value.")
    return [(float(s), c.copy()) for s, c in zip(closest.sums, closest.centres)]


updated_sites_with_closest_host = updated_sites_with_closest


def _coalescing_basins(grid, maxdist, mat, counter, smooth, atol, crop, maxbasins, on_device, device=0, stream=None):
    """-> (the list of ``(value, centre)``, the sum of the map).  The map is read back once, for its sum and its maximum; on the device
    route the map, its smoothed form and the ranking stay in device memory from the smoothing to the last refinement round."""
    grid = _as_density(grid)
    values, dims = _density_values(grid, counter, device, stream)
    total = float(values.sum())
    n = values.size
    vgrid = values.reshape(dims, order="F")
    _crop = atol * float(values.max()) / 100 if crop is None else float(crop)                  # :676
    taps = None if smooth == 0 else [gaussian_taps(s) for s in smoothing_sigmas(dims, mat, smooth)]
    dmap = None
    if on_device:
        import torch
        lib = _abi.load_library()
        dev = torch.device("cuda", device)
        dmap, dvalues, keep = _device_map(grid, counter, values, dims, device)
        hold = [keep]
        if taps is None and dvalues is None:                                                   # bins, unsmoothed: their FP64 values
            hold.append(torch.from_numpy(values).to(dev))
            dvalues = (hold[-1].data_ptr(), dims, np.float64)
        if taps is not None:
            hold.append(torch.empty(n, dtype=torch.float64, device=dev))
            torch.cuda.synchronize(dev)
            smooth_grid(dmap, taps, scale=(1.0 / float(counter)) if dmap[2] == np.int64 else 1.0, device=device, stream=stream,
                        out_ptr=hold[-1].data_ptr())
            dvalues = (hold[-1].data_ptr(), dims, np.float64)
        t_lin = torch.empty(n, dtype=torch.int32, device=dev)
        t_sm = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        count = C.c_int64(0)
        _abi.check(lib, lib.ceg_grid_ranked(device, C.c_void_p(dvalues[0]), 1, _abi.i32ptr(_dims_arg(dims)), float(_crop), C.c_void_p(t_lin.data_ptr()),
                                            C.c_void_p(t_sm.data_ptr()), 1, n, C.byref(count), _stream(stream)))
        ret = grid_coalesce(t_lin.data_ptr(), t_sm.data_ptr(), dmap, mat, maxdist, atol, maxbasins, counter=counter, nranked=int(count.value),
                            device=device, stream=stream)
        del t_lin, t_sm
    else:
        smoothed = vgrid if taps is None else smooth_grid_host(vgrid, taps)
        lin, smval = ranked_above_host(smoothed, _crop)
        ret = coalesce_ranked_host(lin, smval, values[lin], dims, mat, maxdist, atol, maxbasins)
    cluster = cluster_closer_than if on_device else cluster_closer_than_host
    n1 = -1
    while len(ret) != n1:                                                                      # :720-729
        n1 = len(ret)
        if not ret:
            break
        pts = np.asarray([p for _, p in ret], dtype=np.float64).reshape(-1, 3)
        closest = _closest_to_sites(None, pts, mat, counter, on_device, device, stream, prepared=(dmap, dims) if on_device else (values, dims))
        ret = updated_sites_with_closest(closest)
        ret = cluster(ret, mat, maxdist)
        newret = [e for e in ret if e[0] >= atol]
        if not newret:
            break
        ret = newret
    return ret, total


def coalescing_basins(grid, maxdist, mat, *, counter=None, smooth=None, atol=0.1, crop=None, maxbasins=math.inf, device=0, stream=None):
    """``coalescing_basins(grid, maxdist, mat; smooth, atol, crop, maxbasins)`` (:661-731) -> list of ``(value, centre)``.  Smoothing
    (``smooth=None``: the voxel diagonal; 0: none), ranking and the nearest-site partition of every refinement round run on the
    device, and so do the greedy pass (``ceg_grid_coalesce``) and the sums and centres of a round (``ceg_grid_site_partition``);
    ``cluster_closer_than`` runs in the library on the host.  ``grid``: an
    FP64 map or int64 bins with ``counter``, host array or ``(device_ptr, dims[, dtype])``.  ``closest_to_sites`` is this package's
    (see its docstring for where it departs from the reference as written)."""
    return _coalescing_basins(grid, maxdist, mat, counter, smooth, atol, crop, maxbasins, True, device, stream)[0]


def coalescing_basins_host(grid, maxdist, mat, *, counter=None, smooth=None, atol=0.1, crop=None, maxbasins=math.inf):
    """The same composition from the ``*_host`` forms; never touches the library."""
    return _coalescing_basins(grid, maxdist, mat, counter, smooth, atol, crop, maxbasins, False)[0]


def _average_clusters(ret, total, rtol, ntol):
    ret = sorted(ret, key=lambda e: (e[0], *e[1]), reverse=True)                               # sort!(ret; rev=true), :282
    if rtol == 1:
        return ret
    max_total = rtol * total
    run = 0.0
    for i, (p, _) in enumerate(ret, start=1):                                                  # :286-292
        run += p
        if run >= max_total or i + 1 > ntol:
            return ret[:i]
    return ret


def average_clusters(grid, dist, mat, *, counter=None, smooth=None, crop=None, atol=0.0, rtol=1, ntol=math.inf, device=0, stream=None):
    """``average_clusters(bins, dist, mat; smooth, crop, atol, rtol, ntol)`` (averageclusters.jl:280-294): ``coalescing_basins`` with
    ``maxbasins = 2*ntol``, sorted by decreasing probability, cut by ``rtol`` and ``ntol``."""
    ret, total = _coalescing_basins(grid, dist, mat, counter, smooth, atol, crop, 2 * ntol, True, device, stream)
    return _average_clusters(ret, total, rtol, ntol)


def average_clusters_host(grid, dist, mat, *, counter=None, smooth=None, crop=None, atol=0.0, rtol=1, ntol=math.inf):
    ret, total = _coalescing_basins(grid, dist, mat, counter, smooth, atol, crop, 2 * ntol, False)
    return _average_clusters(ret, total, rtol, ntol)
