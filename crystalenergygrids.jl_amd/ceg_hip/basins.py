"""Grid analysis of the reference's ``src/basins.jl`` on the device: ``local_minima`` (:40-99), ``local_components`` (:279-313),
``compute_levels`` (:842-869), ``site_proximity_map!`` (:466-578), ``closest_from_proximity`` (:580-597), ``proximal_map`` (:607-610), ``local_basins`` (:195-264), ``decompose_basins`` (:765-797),
on top of ``ceg_grid_local_minima`` / ``ceg_grid_components`` / ``ceg_grid_site_proximity`` / ``ceg_grid_site_density`` /
``ceg_grid_basins``.

Everything is 0-based.  A grid argument is a NumPy array ``g[i, j, k]`` (any memory order; it is handed over in Julia's, first axis
fastest) or ``(device_ptr, (a, b, c))`` -- ``(device_ptr, (a, b, c), dtype)`` where both int64 and float64 are legal -- for an array that
is already in device memory in that order (a lattice of ``ceg_energy_grid_reduced``, the bins of the MC sampler).

The ``*_host`` functions are vectorised NumPy restatements of the same definitions, for where no device is wanted; they never touch
the library.  Not covered: ``coalescing_basins`` / ``average_clusters``, ``closest_to_sites``, ``energy_levels``,
the unwrapped coordinates of the reference's component lists and basin sets (a point is its wrapped index here).

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
           "circular_distance"]


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
