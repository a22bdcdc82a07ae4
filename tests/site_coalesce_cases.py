"""Cases of the device greedy pass (``ceg_grid_coalesce``), the site partition (``ceg_grid_site_partition``) and ``ceg_cluster_closer_than``,
shared by ``tests/test_site_coalesce_host.py`` and ``tests/test_gpu_site_coalesce.py``, and a restatement of the nearest-basin rule the
device pass follows, with the statistics the host file asserts on the inputs.  Nothing here touches a device.

A greedy case is ``(name, lin, smoothed, grid, counter, dims, mat, maxdist, atol, maxbasins)``: ``lin`` / ``smoothed`` the ranking, ``grid`` the
unsmoothed map (FP64, or int64 bins whose values are ``bins * (1/counter)``).  The expected basins of a small case come from the literal
loop of ``tests/site_extraction_cases.py``, those of a large one from the library's host pass, which the existing host tests tie to it.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import site_extraction_cases as SC

T = 64                 # voxels in flight that the cases are built around: one wave, and the batch of the batched form of the pass
THREADS = 1024         # GC_THREADS of csrc/ceg_grid_coalesce.hip: a thread takes the basins idx = t mod THREADS
CUTS = (0, 1, T + 1, 100)

DYADIC_DIMS = (16, 16, 16)
DYADIC_MAT = np.diag([16.0, 16.0, 16.0])              # 1 A voxels, every coordinate and every squared distance exact
SPARSE_DIMS = (32, 32, 32)
SPARSE_MAT = np.diag([32.0, 32.0, 32.0])


def _rng(*key):
    return np.random.default_rng([20250310, *key])


def lin_of(ijk, dims):
    return int(ijk[0] + dims[0] * (ijk[1] + dims[1] * ijk[2]))


def values_of(grid, counter):
    """the flat FP64 values of a map as every stage sees them"""
    flat = np.asarray(grid).ravel(order="F")
    if flat.dtype.kind in "iu":
        return flat.astype(np.float64) * (1.0 / float(counter))
    return flat.astype(np.float64)


def _case(name, voxels, dims, mat, maxdist, atol=0.1, maxbasins=math.inf, bins=False):
    """voxels: list of ((i, j, k), smoothed, value) in rank order, distinct voxels.  bins: values are counts over a counter of 3000"""
    grid = np.zeros(dims, dtype=np.int64 if bins else np.float64)
    lin, sm = [], []
    for ijk, s, v in voxels:
        assert grid[tuple(ijk)] == 0 or v == 0
        grid[tuple(ijk)] = v
        lin.append(lin_of(ijk, dims))
        sm.append(float(s))
    assert len(set(lin)) == len(lin)
    return (name, np.asarray(lin, dtype=np.int32), np.asarray(sm, dtype=np.float64), grid, 3000.0 if bins else None, dims, mat, maxdist, atol,
            maxbasins)


# ---------------------------------------------------------------------------------------------------------------- the rule
def nearest_rule(lin, smoothed, values, dims, mat, maxdist, atol, maxbasins=math.inf, batch=T):
    """The loop of :677-719 as the nearest-basin rule (see ``ceg_grid_coalesce`` in the header), in plain Python floats.
    -> (ret, stats): ``moved`` distance evaluations that took the search branch, ``ties`` voxels with two basins at the smallest distance,
    ``at_maxdist`` winners with ``d == maxdist``, and per ``batch`` consecutive voxels ``dirty`` voxels whose winner was changed or founded
    earlier in the batch, ``rescans`` voxels whose nearest and second-nearest basin as they stood at the start of the batch were both
    changed earlier in it."""
    a, b, c = dims
    m, ortho, safemin = SC.periodic_setup(mat)
    ret, snapshot, touched = [], [], set()
    st = dict(moved=0, ties=0, at_maxdist=0, dirty=0, rescans=0, founders=0, lone=0, absorbed=0, skipped=0)

    def isless(p, q):
        return p < q or (q != q and p == p)

    for r, (x, smval) in enumerate(zip(np.asarray(lin).tolist(), np.asarray(smoothed).tolist())):
        if r % batch == 0:
            snapshot, touched = list(ret), set()
        val = float(values[x])
        pos = [(x % a + 1) / a, ((x // a) % b + 1) / b, (x // (a * b) + 1) / c]
        best = None
        for idx, (_, cen) in enumerate(ret):
            d, ofs, moved = SC.periodic_distance_with_ofs(m, ortho, safemin, [pos[q] - cen[q] for q in range(3)])
            st["moved"] += moved
            if d > maxdist:
                continue
            if best is None or isless(d, best[0]):
                best = (d, idx, ofs, False)
            elif not isless(best[0], d):
                best = best[:3] + (True,)
        stale = []
        for idx, (_, cen) in enumerate(snapshot):
            d, _, _ = SC.periodic_distance_with_ofs(m, ortho, safemin, [pos[q] - cen[q] for q in range(3)])
            if not d > maxdist:
                stale.append((math.isnan(d), d, idx))
        stale.sort()
        if len(stale) >= 2 and stale[0][2] in touched and stale[1][2] in touched:
            st["rescans"] += 1
        if best is None:
            if smval >= atol:
                ret.append((val, pos))
                touched.add(len(ret) - 1)
                st["founders"] += 1
                if len(ret) >= maxbasins:
                    break
            elif val != 0:
                ret.append((val, [p * val / val for p in pos]))
                touched.add(len(ret) - 1)
                st["lone"] += 1
            else:
                st["skipped"] += 1
            continue
        d, idx, ofs, tie = best
        st["ties"] += tie
        st["at_maxdist"] += d == maxdist
        st["dirty"] += idx in touched
        v2, c2 = ret[idx]
        if val + v2 == 0:
            st["skipped"] += 1
            continue
        ret[idx] = (val + v2, [(pos[q] * val + (c2[q] + float(ofs[q])) * v2) / (val + v2) for q in range(3)])
        touched.add(idx)
        st["absorbed"] += 1
    return ret, st


# ---------------------------------------------------------------------------------------------------------------- small cases
def _cloud(centre, count, dims, key, reach=2):
    """`count` distinct voxels within `reach` of `centre` (wrapped), nearest first, the centre itself excluded"""
    offs = [(i, j, k) for i in range(-reach, reach + 1) for j in range(-reach, reach + 1) for k in range(-reach, reach + 1) if (i, j, k) != (0, 0, 0)]
    offs.sort(key=lambda o: (o[0] ** 2 + o[1] ** 2 + o[2] ** 2, o))
    return [tuple((centre[q] + o[q]) % dims[q] for q in range(3)) for o in offs[:count]]


@functools.lru_cache(maxsize=None)
def small_cases():
    """-> list of (case, expected statistics of ``nearest_rule`` that must hold (a dict of lower bounds or exact counts))"""
    d, m = DYADIC_DIMS, DYADIC_MAT
    out = []
    # every case of greedy_cases(): its values written into a map
    for name, lin, sm, val, dims, mat, maxdist, atol, maxbasins, _ in SC.greedy_cases():
        a, b, _c = dims
        vox = [((x % a, (x // a) % b, x // (a * b)), s, v) for x, s, v in zip(lin, sm, val)]
        out.append((_case("extraction-" + name, vox, dims, mat, maxdist, atol, maxbasins), {}))
    # one basin takes a whole batch and more: a founder and 70 voxels around it, all in range wherever the centre drifts to
    vox = [((8, 8, 8), 0.9, 0.5)] + [(p, 0.8 - 0.001 * q, 0.01 + 0.001 * q) for q, p in enumerate(_cloud((8, 8, 8), 70, d, 1))]
    out.append((_case("one-basin-takes-a-batch", vox, d, m, 6.0), dict(founders=1, absorbed=70, dirty=69)))
    # founded in the batch, the next voxel in range of it, twelve times over
    vox = []
    for q in range(12):
        p = (1 + 4 * (q % 4), 2 + 5 * (q // 4), 3)
        vox += [(p, 0.9 - 0.01 * q, 0.3), (((p[0] + 1) % 16, p[1], p[2]), 0.7 - 0.01 * q, 0.2)]
    out.append((_case("founded-then-hit", vox, d, m, 1.5), dict(founders=12, absorbed=12, dirty=12)))
    # three basins in a row founded in a first batch, which voxels of value 0 far from everything fill up (skipped); in the second batch
    # a voxel beside the first basin, one beside the second, then two between them: their two nearest basins are both dirty
    vox = [((2, 8, 8), 0.9, 0.4), ((6, 8, 8), 0.89, 0.4), ((12, 8, 8), 0.88, 0.4)]
    vox += [((q % 16, q // 16, 0), 0.05, 0.0) for q in range(T - 3)]
    vox += [((2, 9, 8), 0.8, 0.1), ((6, 9, 8), 0.79, 0.1), ((4, 8, 8), 0.78, 0.2), ((4, 9, 8), 0.77, 0.2)]
    out.append((_case("both-nearest-dirty", vox, d, m, 2.5), dict(founders=3, rescans=2, dirty=2, skipped=T - 3)))
    # a centre that drifts: the basin at x = 5 takes a heavy voxel at x = 7 and moves to 6.8; x = 8 is then in range of the current
    # centre only, x = 4 of the stale one only (it founds a basin)
    vox = [((5, 3, 3), 0.9, 0.1), ((7, 3, 3), 0.8, 0.9), ((8, 3, 3), 0.7, 0.2), ((4, 3, 3), 0.6, 0.2)]
    out.append((_case("drift", vox, d, m, 2.0), dict(founders=2, absorbed=2, dirty=2)))
    # exact ties: x = 6 is 2 from the basins at 4 and 8, d == maxdist; the lower index takes it.  Then the same with the second basin
    # changed first by a voxel of value 0 at its own distance (its centre stays, it is dirty), and a tie between the two again
    vox = [((4, 5, 5), 0.9, 0.25), ((8, 5, 5), 0.8, 0.25), ((6, 5, 5), 0.7, 0.125)]
    out.append((_case("tie-lower-index-at-maxdist", vox, d, m, 2.0), dict(founders=2, absorbed=1, ties=1, at_maxdist=1)))
    vox = [((4, 11, 5), 0.9, 0.25), ((8, 11, 5), 0.8, 0.25), ((9, 11, 5), 0.75, 0.0), ((6, 11, 5), 0.7, 0.125)]
    out.append((_case("tie-clean-against-dirty", vox, d, m, 2.0), dict(founders=2, absorbed=2, ties=1, dirty=1)))
    # value branches: zero with nothing in range (skipped) and with a basin in range (absorbed, the centre recomputed); a lone low
    # voxel (pos*val/val, 14 is no power of two away from 1); a negative value that cancels its basin; the lone push does not count
    # check maxbasins (three basins exist after it and the loop goes on); the third founder makes four and ends the loop, in mid-batch
    vox = [((1, 1, 1), 0.9, 0.5), ((9, 9, 9), 0.05, 0.0), ((2, 1, 1), 0.8, 0.0), ((6, 12, 2), 0.7, 0.3), ((7, 12, 2), 0.6, -0.3),
           ((13, 2, 6), 0.04, 0.07), ((9, 13, 2), 0.5, 0.2), ((12, 12, 12), 0.4, 0.1), ((3, 7, 12), 0.3, 0.1)]
    out.append((_case("value-branches", vox, d, m, 1.5, 0.1, 3.0), dict(founders=3, lone=1, skipped=2, absorbed=1)))
    out.append((_case("value-branches-skew", [(((p[0] * 3) % 12, (p[1] * 2) % 10, p[2]), s, v) for p, s, v in vox], SC.GREEDY_DIMS, SC.SKEW_MAT, 1.5,
                      0.1, 3.0), {}))
    # the lone push where pos*val/val is not pos: 9/12 and 4/10 times 0.09 do not divide back
    for cname, mat in (("ortho", SC.ORTHO_MAT), ("skew", SC.SKEW_MAT)):
        vox = [((1, 1, 1), 0.9, 0.5), ((8, 3, 7), 0.05, 0.09)]
        out.append((_case(f"lone-low-bits-{cname}", vox, SC.GREEDY_DIMS, mat, 1.5), dict(founders=1, lone=1)))
    # int64 bins: the same branches with counts over a counter
    vox = [((1, 1, 1), 0.9, 1500), ((2, 1, 1), 0.8, 700), ((9, 9, 9), 0.05, 211), ((6, 12, 2), 0.7, 913), ((7, 12, 2), 0.6, -913),
           ((7, 13, 2), 0.5, 47)]
    out.append((_case("bins", vox, d, m, 1.5, bins=True), dict(founders=2, lone=1, absorbed=2, skipped=1)))
    # the CIT-7 cell and the skew cell on random scattered voxels: the search branch of the distance is taken
    for cname, mat in (("cit7", SC.cit7_mat()), ("skew", SC.SKEW_MAT)):
        r = _rng(1)
        dims = SC.GREEDY_DIMS
        pick = r.choice(dims[0] * dims[1] * dims[2], size=2 * T + 1, replace=False)
        vox = [((int(x) % 12, (int(x) // 12) % 10, int(x) // 120), 0.9 - 0.003 * q, float(r.integers(1, 64)) / 256) for q, x in enumerate(pick)]
        out.append((_case(f"{cname}-scattered", vox, dims, mat, 2.5), dict(moved=1, dirty=1)))
    return out


def truncated(case, n):
    name, lin, sm, *rest = case
    return (f"{name}-first-{n}", lin[:n].copy(), sm[:n].copy(), *rest)


@functools.lru_cache(maxsize=None)
def length_cases():
    """the skew scattered ranking (2T + 1 voxels) cut at every length around the batch"""
    base = next(c for c, _ in small_cases() if c[0] == "skew-scattered")
    return [truncated(base, n) for n in (0, 1, T - 1, T, T + 1, 2 * T + 1)]


@functools.lru_cache(maxsize=None)
def expected_small(name):
    case = next(c for c in [c for c, _ in small_cases()] + length_cases() if c[0] == name)
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    flat = values_of(grid, counter)
    smoothed = np.zeros(flat.size)
    smoothed[lin] = sm
    ret, br = SC.greedy_literal(lin.tolist(), smoothed, flat, dims, mat, maxdist, atol, -math.inf, maxbasins)
    return ret, br


# ---------------------------------------------------------------------------------------------------------------- large cases
FOUNDER_COUNTS = (T - 1, T, T + 1, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)


@functools.lru_cache(maxsize=None)
def founder_case(nf):
    """`nf` founders on every second index of 32^3 in a 32 A cell, 2 A apart with maxdist 1.5, in a shuffled order, then one neighbour
    per founder at 1 A: in range of it, and at exactly the same distance of the next founder along the axis where that one exists (the
    lower index takes it)"""
    dims = SPARSE_DIMS
    r = _rng(2, nf)
    even = [(2 * i, 2 * j, 2 * k) for k in range(16) for j in range(16) for i in range(16)]
    order = r.permutation(nf)                                                     # a block of the lattice: most neighbours lie between two
    vox = [(even[q], 0.9 - 1e-5 * n, float(r.integers(1, 1024)) / 4096) for n, q in enumerate(order)]
    axes = r.integers(0, 3, size=nf)
    for n, q in enumerate(order):
        p = list(even[q])
        p[axes[n]] += 1
        vox.append((tuple(p), 0.5 - 1e-5 * n, float(r.integers(1, 1024)) / 4096))
    return _case(f"founders-{nf}", vox, dims, SPARSE_MAT, 1.5)


@functools.lru_cache(maxsize=None)
def random_map():
    """(40, 36, 44) skew map of scattered integer hits over a counter of 2^20 -> (bins, counter, dims, mat, maxdist)"""
    dims = (40, 36, 44)
    r = _rng(3)
    bins = np.zeros(dims, dtype=np.int64)
    for cen in r.random((30, 3)):
        for _ in range(60):
            p = np.floor(((cen + r.normal(scale=0.03, size=3)) % 1.0) * dims).astype(int)
            bins[tuple(p)] += int(r.integers(2**12, 2**16))
    return bins, float(2**20), dims, SC.SKEW_MAT, 1.2


# ---------------------------------------------------------------------------------------------------------------- partition
@functools.lru_cache(maxsize=None)
def partition_cases():
    """-> list of (name, grid, counter, dims, mat, sites)"""
    big = (70, 66, 65)
    cit7 = SC.cit7_mat()
    out = []
    r = _rng(4)
    very = _rng(6).random(big) < 0.0001                                            # about 30 voxels
    grid = np.where(very, r.uniform(0.001, 0.02, size=big), 0.0)
    for ns in (1, 2047, 2048, 2049, 4097):
        out.append((f"cit7-70x66x65-{ns}", grid, None, big, cit7, _rng(5, ns).random((ns, 3))))
    bins = np.where(very, r.integers(1, 2**20, size=big), 0).astype(np.int64)
    out.append(("cit7-70x66x65-bins-300", bins, float(2**26), big, cit7, _rng(5, 300).random((300, 3))))
    # generic FP64 values on a dense small map: three sites, one of them far from every voxel that is set (no voxel), one with one
    d = (12, 10, 14)
    g = np.zeros(d)
    g[2:6, 2:6, 2:6] = _rng(7).uniform(1e-3, 1e-2, size=(4, 4, 4))
    g[9, 8, 12] = 0.0123
    sites = np.array([[0.3, 0.35, 0.25], [0.8, 0.85, 0.9], [0.9, 0.2, 0.5]])
    out.append(("skew-generic-empty-and-single", g, None, d, SC.SKEW_MAT, sites))
    out.append(("skew-generic-one-site", g, None, d, SC.SKEW_MAT, sites[:1]))
    # the cap: along a row 0.6, 0.5 (skipped: 1.1 > 1), 0.3 (accepted: 0.9), 0.2 (skipped), 0.1 (accepted: 1.0, not above 1)
    g = np.zeros(d)
    for q, v in enumerate((0.6, 0.5, 0.3, 0.2, 0.1)):
        g[3 + q, 4, 5] = v
    g[10, 8, 12] = 0.25
    out.append(("ortho-cap", g, None, d, SC.ORTHO_MAT, np.array([[0.4, 0.45, 0.4], [0.85, 0.8, 0.85]])))
    return out


# ---------------------------------------------------------------------------------------------------------------- cluster
@functools.lru_cache(maxsize=None)
def cluster_cases():
    """-> list of (name, ret, mat, maxdist)"""
    out = []
    for cname, mat in (("ortho", SC.ORTHO_MAT), ("cit7", SC.cit7_mat())):
        r = _rng(8)
        for n in (0, 1, 2, 300):
            ret = [(float(r.uniform(0.01, 0.3)), r.uniform(-0.2, 1.2, size=3)) for _ in range(n)]
            if n == 2:
                ret[1] = (ret[1][0], ret[0][1] + 0.01)
            out.append((f"{cname}-{n}", ret, mat, 2.0))
        out.append((f"{cname}-cap", [(0.6, [0.5, 0.5, 0.5]), (0.5, [0.52, 0.5, 0.5]), (0.3, [0.5, 0.52, 0.5])], mat, 2.0))
        out.append((f"{cname}-chain", [(0.05, [0.1 + 0.02 * q, 0.3, 0.3]) for q in range(12)], mat, 8.0))
        out.append((f"{cname}-wrap", [(0.2, [0.99, 0.01, 0.5]), (0.3, [0.01, 0.98, 0.5]), (0.1, [1.02, -0.03, 0.52])], mat, 2.0))
    return out


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def many_basins_case():
    """a sparse map on which the greedy pass at ``atol = 0`` leaves more than 2048 basins: one count on every third index of 39^3 in a
    39 A cell (2197 voxels 3 A apart) and ``maxdist`` 1.2; unsmoothed, so no voxel in between is ranked.  A basin is founded one voxel
    diagonal from its voxel (``pos`` is 1-based), still nearer to it than to any other voxel, so no site stays empty.  Every value is a
    count over 2^22: sums of them are exact in any order."""
    dims = (39, 39, 39)
    r = _rng(9)
    bins = np.zeros(dims, dtype=np.int64)
    bins[::3, ::3, ::3] = r.integers(2**8, 2**12, size=(13, 13, 13))
    return bins, float(2**22), dims, np.diag([39.0, 39.0, 39.0]), 1.2, dict(atol=0.0, smooth=0)
