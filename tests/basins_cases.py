"""Literal, queue-based restatements of the reference's ``src/basins.jl`` in plain Python, and the cases the basins tests share.

The restatements follow the source line by line (cited as ``:N``), loops, queues and scan orders included; they are slow and meant
for small grids.  Grids are NumPy arrays ``g[i, j, k]``; inside the restatements indices are 1-based like the source, what they
return is 0-based.  Nothing here touches the library.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

from ceg_hip.hostmirror.utils import mat_from_parameters, prepare_periodic_distance_computations

SHAPES = [(1, 1, 1), (1, 5, 4), (2, 2, 2), (2, 7, 3), (3, 3, 3), (5, 7, 3), (17, 9, 33), (70, 66, 65)]
TOLERANCES = [-1.0, 0.0, 0.01, 1.0]


def mod1(x, n):
    return (x - 1) % n + 1


def grid_neighbors(I):
    """GridNeighbors (:4-23): +1 then -1 along each axis in turn"""
    for axis in range(3):
        for sign in (1, -1):
            yield tuple(I[q] + (sign if q == axis else 0) for q in range(3))


# ---------------------------------------------------------------------------------------------------------------- :40-99
def local_minima_literal(grid, tolerance=1e-2, maxima=False):
    """-> (list of 0-based (i, j, k) sorted as Julia sorts CartesianIndex, min_energy or None); raises AssertionError like :91"""
    a1, a2, a3 = grid.shape
    g = grid.tolist()
    lt = (lambda x, y: x > y) if maxima else (lambda x, y: x < y)
    localmins = []
    for i3 in range(1, a3 + 1):                                                   # :48-49
        for i2 in range(1, a2 + 1):
            for i1 in range(1, a1 + 1):
                val = g[i1 - 1][i2 - 1][i3 - 1]
                m1, p1 = mod1(i1 - 1, a1), mod1(i1 + 1, a1)                       # :51, :53
                m2, p2 = mod1(i2 - 1, a2), mod1(i2 + 1, a2)
                m3, p3 = mod1(i3 - 1, a3), mod1(i3 + 1, a3)
                ok = True
                for q3, n3 in enumerate((i3, m3, p3)):                            # :52-82, the same 26 comparisons (an axis of
                    for q2, n2 in enumerate((i2, m2, p2)):                        # length 1 compares the point with itself)
                        for q1, n1 in enumerate((i1, m1, p1)):
                            if q1 == q2 == q3 == 0:
                                continue
                            if not lt(val, g[n1 - 1][n2 - 1][n3 - 1]):
                                ok = False
                                break
                        if not ok:
                            break
                    if not ok:
                        break
                if ok:
                    localmins.append((i1, i2, i3))                                # :83
    if not localmins:
        return [], None                                                           # :89 throws on the empty minimum
    min_energy = min(g[i - 1][j - 1][k - 1] for i, j, k in localmins)             # :89
    if tolerance >= 0:
        assert min_energy < 0                                                     # :91
        max_threshold = min_energy + abs(min_energy * tolerance)                  # :92
        localmins = [p for p in localmins if not g[p[0] - 1][p[1] - 1][p[2] - 1] > max_threshold]      # :94-97
    localmins.sort(key=lambda p: (p[2], p[1], p[0]))                              # sort! of CartesianIndex
    return [(i - 1, j - 1, k - 1) for i, j, k in localmins], min_energy


# ---------------------------------------------------------------------------------------------------------------- :279-313, :842-869
def _components_literal(grid, seed_ok, neighbour_ok):
    a, b, c = dims = grid.shape
    g = grid.tolist()
    visited = np.zeros(dims, dtype=bool).tolist()
    labels = np.full(dims, -1, dtype=np.int32)
    seeds, sizes, sums = [], [], []
    for k in range(1, c + 1):                                                     # :283 / :848
        for j in range(1, b + 1):
            for i in range(1, a + 1):
                if visited[i - 1][j - 1][k - 1]:
                    continue
                tot = g[i - 1][j - 1][k - 1]
                if not seed_ok(tot):
                    continue
                visited[i - 1][j - 1][k - 1] = True
                Q = [(i, j, k)]
                for I in Q:                                                       # grows while it is iterated
                    for J in grid_neighbors(I):
                        iv, jv, kv = (mod1(x, n) for x, n in zip(J, dims))
                        if visited[iv - 1][jv - 1][kv - 1]:
                            continue
                        val = g[iv - 1][jv - 1][kv - 1]
                        if not neighbour_ok(val):
                            continue
                        tot += val
                        visited[iv - 1][jv - 1][kv - 1] = True
                        Q.append(J)
                rank = len(seeds)
                for J in Q:
                    labels[tuple(mod1(x, n) - 1 for x, n in zip(J, dims))] = rank
                seeds.append((i - 1) + a * ((j - 1) + b * (k - 1)))
                sizes.append(len(Q))
                sums.append(tot)
    return labels, seeds, sizes, sums


def local_components_literal(grid):
    """:279-301 before the atol / sort / rtol cut: (labels, seeds, sizes, sums) in the order of discovery"""
    nz = lambda v: not (v == 0)                                                   # iszero
    return _components_literal(grid, nz, nz)


def cut_components_literal(sums, total, atol=0.0, rtol=1.0, ntol=math.inf):
    """:300-311 -> the indices (into the order of discovery) that are kept, in the returned order"""
    ret = [(n, s) for n, s in enumerate(sums) if not s < atol]
    ret.sort(key=lambda t: -t[1])                                                 # stable, rev=true
    max_tot = total * rtol if rtol < 1 else math.inf
    tot = 0.0
    for pos, (_, s) in enumerate(ret, start=1):
        tot += s
        if pos > ntol or tot > max_tot:
            ret = ret[:pos - 1]
            break
    return [n for n, _ in ret]


def compute_levels_literal(grid, mine, maxe):
    """:842-869 on a mean lattice.  No case has a value equal to a bound, where seed (<=) and neighbour (<) differ."""
    return _components_literal(grid, lambda e: mine <= e <= maxe, lambda e: mine < e < maxe)[:3]


# ---------------------------------------------------------------------------------------------------------------- :466-578
def _matvec(m, v):
    return [m[r][0] * v[0] + m[r][1] * v[1] + m[r][2] * v[2] for r in range(3)]


def _norm2(v):
    return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]


def periodic_distance2(m, ortho, safemin2, v):
    """utils.jl:226-246 on a fractional difference"""
    v = [x + 0.5 - math.floor(x + 0.5) - 0.5 for x in v]
    ref2 = _norm2(_matvec(m, v))
    if ortho or ref2 <= safemin2:
        return ref2
    for i in range(3):
        v[i] += 1
        n2 = _norm2(_matvec(m, v))
        if n2 < ref2:
            return n2
        v[i] -= 2
        n2 = _norm2(_matvec(m, v))
        if n2 < ref2:
            return n2
        v[i] += 1
    return ref2


def julia_round(x):
    return int(np.rint(x))


def site_proximity_map_literal(sites, dims, mat, maxdist=2.0):
    """-> (site[a, b, c] int32 1-based / 0, offset[a, b, c, 3] int8, deleted 0-based indices)"""
    a, b, c = dims
    m = np.asarray(mat, dtype=np.float64).tolist()
    ortho, safemin = prepare_periodic_distance_computations(np.asarray(mat, dtype=np.float64))
    safemin2 = safemin ** 2
    protoskin = math.sqrt(_norm2(_matvec(m, [1 / a, 1 / b, 1 / c])))              # :470
    sites = [tuple(float(x) for x in s) for s in sites]
    Qs = [[(1 + julia_round(a * i), 1 + julia_round(b * j), 1 + julia_round(c * k))] for i, j, k in sites]      # :471
    deletesite, known = [], set()
    for idx, Q in enumerate(Qs):                                                  # :475-482
        if Q[0] in known:
            deletesite.append(idx)
        else:
            known.add(Q[0])
    Qs = [Q for idx, Q in enumerate(Qs) if idx not in deletesite]
    sites = [s for idx, s in enumerate(sites) if idx not in deletesite]
    n = len(sites)
    nextQs = [[] for _ in range(n)]
    for isite in range(n):                                                        # :487
        site, Q, nextQ = sites[isite], Qs[isite], nextQs[isite]
        todelete = []
        maxdist2 = absmaxdist2 = maxdist ** 2
        for i2 in range(n):                                                       # :495-500
            if i2 == isite:
                continue
            dsites2 = periodic_distance2(m, ortho, safemin2, [x - y for x, y in zip(site, sites[i2])])
            maxdist2 = min(maxdist2, dsites2)
        maxdist2 /= 4
        visited = np.zeros(dims, dtype=bool)
        visited[tuple(mod1(x, d) - 1 for x, d in zip(Q[0], dims))] = True
        for queue, nextqueue, tagged in ((Q, nextQ, False), (nextQ, None, True)):      # :518
            skin2 = (protoskin + math.sqrt(maxdist2)) ** 2
            for item in queue:
                I = item[0] if tagged else item
                for J in grid_neighbors(I):
                    j = tuple(mod1(x, d) - 1 for x, d in zip(J, dims))
                    if visited[j]:
                        continue
                    visited[j] = True
                    d2 = _norm2(_matvec(m, [s - (x - 1) / d for s, x, d in zip(site, J, dims)]))      # :526-528
                    if d2 >= maxdist2:
                        if nextqueue is not None and d2 < absmaxdist2:
                            nextqueue.append((J, d2))
                        if d2 >= skin2:
                            continue
                        todelete.append(len(queue))                               # 0-based position of the push below
                    queue.append((J, d2) if tagged else J)
            for pos in reversed(todelete):                                        # deleteat!
                del queue[pos]
            todelete.clear()
            maxdist2 = maxdist ** 2
    ret = np.zeros(dims, dtype=np.int32)
    ofs = np.zeros(tuple(dims) + (3,), dtype=np.int8)
    dist2s = np.full(dims, np.inf)
    for s, Q in enumerate(Qs, start=1):                                           # :554-563
        for pos in Q:
            o = tuple((x - 1) // d for x, d in zip(pos, dims))
            w = tuple(mod1(x, d) - 1 for x, d in zip(pos, dims))
            assert ret[w] == 0, f"point {w} seen in {ret[w]} and {s}"
            ret[w], ofs[w], dist2s[w] = s, o, 0.0
    for s, Q in enumerate(nextQs, start=1):                                       # :567-575
        for pos, d2 in Q:
            o = tuple((x - 1) // d for x, d in zip(pos, dims))
            w = tuple(mod1(x, d) - 1 for x, d in zip(pos, dims))
            if d2 < dist2s[w]:
                dist2s[w] = d2
                ret[w], ofs[w] = s, o
    return ret, ofs, deletesite


def closest_from_proximity_literal(grid, site, offset, numsites):
    """:580-597 -> list of (rho, [pos]) with FP64 accumulation as the reference's"""
    a, b, c = grid.shape
    ret = [None] * (numsites + 1)
    for isite in range(numsites + 1):
        rho, pos = 0.0, [0.0, 0.0, 0.0]
        for k in range(c):
            for j in range(b):
                for i in range(a):
                    if site[i, j, k] != isite:
                        continue
                    val = int(grid[i, j, k])
                    rho += val
                    o = offset[i, j, k]
                    for q, (w, d) in enumerate(((i, a), (j, b), (k, c))):
                        pos[q] += val * (int(o[q]) + w / d)
        with np.errstate(invalid="ignore", divide="ignore"):
            ret[numsites if isite == 0 else isite - 1] = (rho, [float(np.float64(p) / np.float64(rho)) for p in pos])
    return ret


# ---------------------------------------------------------------------------------------------------------------- minima cases
def _rng(*key):
    return np.random.default_rng([20240229, *key])


def _field(shape, seed):
    """random values in about [-3, 1]: some negative local minima at every shape that can have one"""
    return _rng(seed, *shape).uniform(-3.0, 1.0, size=shape)


def _planted(shape, points, base_seed=7):
    g = _rng(base_seed, *shape).uniform(1.0, 2.0, size=shape)
    for p, v in points:
        g[p] = v
    return g


@functools.lru_cache(maxsize=None)
def minima_cases():
    """-> list of (name, grid, tolerance, maxima).  Every case is legal (a negative extremum where tolerance >= 0) or has no
    extremum at all; the refusals are in minima_refusal_cases()."""
    cases = []
    for shape in SHAPES:
        g = _field(shape, 1)
        for tol in TOLERANCES:
            ref, ext = local_minima_literal(g, tol if (tol < 0) else -1.0)
            if tol >= 0 and ref and not ext < 0:
                continue
            cases.append((f"random-{'x'.join(map(str, shape))}-tol{tol}", g, tol, False))
        mx = -_field(shape, 2) - 4.0                                              # all negative: `minimum` over the maxima is < 0
        cases.append((f"maxima-{'x'.join(map(str, shape))}-all", mx, -1.0, True))
        cases.append((f"maxima-{'x'.join(map(str, shape))}-tol0.01", mx, 0.01, True))
    for shape in ((17, 9, 33), (70, 66, 65)):
        a, b, c = shape
        corner_edge_face = [((0, 0, 0), -10.0), ((a - 1, 4, 0), -9.95), ((5, 0, 10), -5.0), ((8, 4, c - 1), -1.0),
                            ((a - 1, b - 1, c // 2), -9.91), ((a // 2, b // 2, c // 2), -9.0)]
        g = _planted(shape, corner_edge_face)
        for tol in TOLERANCES:
            cases.append((f"wrap-{a}x{b}x{c}-tol{tol}", g, tol, False))
        plateau = _planted(shape, [((3, 3, 3), -20.0), ((4, 3, 3), -20.0), ((9, 5, 20), -2.0)])
        cases.append((f"plateau-{a}x{b}x{c}", plateau, -1.0, False))
        special = _planted(shape, [((3, 3, 3), -5.0), ((3, 4, 4), math.nan), ((10, 5, 20), -4.0), ((12, 2, 8), math.inf),
                                   ((a - 1, 0, c - 1), -3.0), ((6, 6, 6), math.nan)])
        special[13:16, 5:8, 24:28] = 1e100                                        # a blocked pocket: equal values, no extremum inside
        special[14, 6, 25] = -6.0                                                 # ... and a minimum walled in by it
        cases.append((f"special-{a}x{b}x{c}-all", special, -1.0, False))
        cases.append((f"special-{a}x{b}x{c}-tol1", special, 1.0, False))
        cases.append((f"special-{a}x{b}x{c}-maxima", np.where(np.isfinite(special), -special, special) - 3.0, -1.0, True))
    zeros = np.full((5, 7, 3), 1.0)
    zeros[2, 3, 1], zeros[3, 3, 1] = -0.0, 0.0                                    # -0.0 < 0.0 is false: neither is a minimum
    cases.append(("negative-zero", zeros, -1.0, False))
    cases.append(("constant-count0", np.full((5, 7, 3), -2.0), 0.01, False))
    return cases


def minima_refusal_cases():
    """extremum >= 0 with tolerance >= 0 (:91)"""
    pos = _planted((5, 7, 3), [((2, 3, 1), 0.5)])
    zero = _planted((17, 9, 33), [((2, 3, 1), 0.0)])
    return [("positive", pos, 0.0), ("positive-tol1", pos, 1.0), ("zero", zero, 0.01)]


def pinned_grid(shape, minima_1based, values, others=()):
    """a synthetic grid with the given minima planted (1-based positions, as runtests.jl writes them)"""
    pts = [(tuple(x - 1 for x in p), v) for p, v in zip(minima_1based, values)]
    pts += [(tuple(x - 1 for x in p), v) for p, v in others]
    return _planted(shape, pts, base_seed=11)


# ---------------------------------------------------------------------------------------------------------------- component cases
def _serpentine():
    g = np.zeros((32, 32, 4), dtype=np.int64)
    for j in range(0, 31, 2):
        g[0:31, j, 0] = 1 + j
    for n, j in enumerate(range(1, 30, 2)):
        g[30 if n % 2 == 0 else 0, j, 0] = 100 + j
    return g


@functools.lru_cache(maxsize=None)
def component_cases():
    """-> list of (name, grid) for CEG_COMPONENTS_NONZERO; int64 grids carry exact sums"""
    cases = []
    for shape in SHAPES:
        r = _rng(3, *shape)
        name = "x".join(map(str, shape))
        sparse = np.where(r.random(shape) < 0.35, r.integers(1, 2**40, size=shape), 0).astype(np.int64)
        cases.append((f"i64-sparse-{name}", sparse))
        dense = np.where(r.random(shape) < 0.7, r.integers(-5, 2**40, size=shape), 0).astype(np.int64)
        cases.append((f"i64-dense-{name}", dense))
        f = np.where(r.random(shape) < 0.3, r.normal(size=shape), 0.0)
        f.flat[r.integers(0, f.size)] = math.nan                                  # a NaN is active
        cases.append((f"f64-nan-{name}", f))
        cases.append((f"none-{name}", np.zeros(shape, dtype=np.int64)))
        cases.append((f"all-{name}", np.full(shape, 3, dtype=np.int64)))
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    cases.append(("checkerboard-8x8x8", (((i + j + k) % 2) * (1 + i + 8 * j)).astype(np.int64)))
    slabs = np.zeros((17, 9, 33), dtype=np.int64)
    slabs[0:2], slabs[15:17] = 5, 7
    cases.append(("slabs-through-the-face", slabs))
    cases.append(("serpentine-32x32x4", _serpentine()))
    return cases


@functools.lru_cache(maxsize=None)
def band_cases():
    """-> list of (name, grid, lo, hi): a smooth field, bounds no value equals"""
    cases = []
    for shape in ((5, 7, 3), (17, 9, 33), (70, 66, 65)):
        a, b, c = shape
        i, j, k = np.meshgrid(np.arange(a), np.arange(b), np.arange(c), indexing="ij")
        f = np.sin(2 * np.pi * i / a + 0.3) + np.cos(4 * np.pi * j / b) * np.sin(2 * np.pi * k / c + 1.1) + 0.01 * np.sqrt(2.0)
        for lo, hi in ((-0.3137, 0.4421), (0.9013, 5.0)):
            assert not np.any(f == lo) and not np.any(f == hi)
            cases.append((f"band-{a}x{b}x{c}-{lo}", f, lo, hi))
    return cases


@functools.lru_cache(maxsize=None)
def components_reference(name):
    for n, g in component_cases():
        if n == name:
            return local_components_literal(g)
    for n, g, lo, hi in band_cases():
        if n == name:
            return compute_levels_literal(g, lo, hi)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def minima_reference(name):
    for n, g, tol, mx in minima_cases():
        if n == name:
            return local_minima_literal(g, tol, mx)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- proximity cases
SKEW = dict(dims=(12, 10, 14), mat=mat_from_parameters((12.0, 11.0, 13.0), (80.0, 95.0, 105.0)))
ORTHO = dict(dims=(11, 10, 12), mat=np.diag([11.5, 11.0, 12.5]))
POW2 = dict(dims=(8, 8, 16), mat=np.diag([9.0, 9.5, 15.0]))


def proximity_distances(sites, dims, mat):
    """d2[s, i, j, k] by the definition, all 27 offsets, in exact-ish FP64 (for the margins only)"""
    a, b, c = dims
    w = np.stack(np.meshgrid(np.arange(a), np.arange(b), np.arange(c), indexing="ij"), axis=-1).astype(np.float64)
    out = np.full((len(sites),) + tuple(dims), np.inf)
    for s, x in enumerate(sites):
        for o in np.ndindex(3, 3, 3):
            v = np.asarray(x) - (w / np.asarray(dims, dtype=np.float64) + (np.asarray(o) - 1))
            d = v @ np.asarray(mat, dtype=np.float64).T
            out[s] = np.minimum(out[s], (d * d).sum(axis=-1))
    return out


def assert_margin(sites, dims, mat, maxdist):
    """a condition on the INPUT: no integer of the map can hinge on the order of the FP64 operations inside mat*x"""
    from ceg_hip.basins import snap_sites
    kept, _ = snap_sites(sites, dims)
    if not len(kept):
        return
    d2 = proximity_distances(kept, dims, mat)
    eps = 1e-9 * maxdist * maxdist
    assert np.all(np.abs(d2 - maxdist * maxdist) > eps), "a point sits on the maxdist sphere of a site"
    if len(kept) > 1:
        srt = np.sort(d2, axis=0)
        near = srt[0] < maxdist * maxdist + eps
        assert np.all((srt[1] - srt[0])[near] > eps), "a point is equidistant from two sites"


@functools.lru_cache(maxsize=None)
def proximity_cases():
    """-> list of (name, sites (n, 3), dims, mat, maxdist)"""
    cases = []
    for cname, cell in (("skew", SKEW), ("ortho", ORTHO)):
        for seed in (0, 1, 2):
            six = _rng(5, seed).random((6, 3))
            for maxdist in (1.2, 2.0, 3.0):
                cases.append((f"{cname}-six-{seed}-{maxdist}", six, cell["dims"], cell["mat"], maxdist))
        cases.append((f"{cname}-none", np.zeros((0, 3)), cell["dims"], cell["mat"], 2.0))
        cases.append((f"{cname}-one", np.array([[0.31, 0.62, 0.47]]), cell["dims"], cell["mat"], 2.0))
        faces = np.array([[0.985, 0.52, 0.03], [0.02, 0.97, 0.51], [0.5, 0.03, 0.975], [0.47, 0.45, 0.5]])
        cases.append((f"{cname}-faces", faces, cell["dims"], cell["mat"], 2.0))
        twins = np.array([[0.26, 0.31, 0.52], [0.27, 0.305, 0.515], [0.71, 0.66, 0.2], [0.262, 0.3, 0.52]])
        cases.append((f"{cname}-twins", twins, cell["dims"], cell["mat"], 2.0))
        close = np.array([[0.3, 0.3, 0.3], [0.42, 0.36, 0.33], [0.36, 0.45, 0.4], [0.3, 0.33, 0.52]])
        cases.append((f"{cname}-overlap", close, cell["dims"], cell["mat"], 3.0))
    for name, sites, dims, mat, maxdist in cases:
        assert_margin(sites, dims, mat, maxdist)
    return cases


@functools.lru_cache(maxsize=None)
def proximity_reference(name):
    for n, sites, dims, mat, maxdist in proximity_cases():
        if n == name:
            return site_proximity_map_literal(sites, dims, mat, maxdist)
    raise KeyError(name)


CENTRE_RTOL = 4 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def density_cases():
    """-> list of (name, bins int64, site, offset, nsites, check_centres).  On the power-of-two lattice every product and sum of the
    literal accumulation is exact, so its centres are one division from the exact ones: asserted here against exact rationals."""
    cases = []
    for cname, cell, centres in (("skew", SKEW, False), ("ortho", ORTHO, False), ("pow2", POW2, True)):
        sites = np.array([[0.985, 0.52, 0.03], [0.02, 0.97, 0.51], [0.5, 0.03, 0.975], [0.47, 0.45, 0.5], [0.2, 0.2, 0.8]])
        assert_margin(sites, cell["dims"], cell["mat"], 2.5)
        site, off, deleted = site_proximity_map_literal(sites, cell["dims"], cell["mat"], 2.5)
        assert not deleted
        r = _rng(9, *cell["dims"])
        bins = np.where(r.random(cell["dims"]) < 0.4, r.integers(1, 2**20 if centres else 2**40, size=cell["dims"]), 0).astype(np.int64)
        if centres:
            lit = closest_from_proximity_literal(bins, site, off, len(sites))
            for s in range(len(sites) + 1):
                sel = site == (0 if s == len(sites) else s + 1)
                rho = int(bins[sel].sum())
                assert rho > 0 and lit[s][0] == rho
                idx = np.argwhere(sel)
                for q in range(3):
                    exact = sum(Fraction(int(bins[tuple(p)])) * (int(off[tuple(p)][q]) + Fraction(int(p[q]), cell["dims"][q])) for p in idx) / rho
                    assert abs(Fraction(lit[s][1][q]) - exact) <= CENTRE_RTOL * abs(exact), (cname, s, q)
        cases.append((cname, bins, site, off, len(sites), centres))
    return cases
