"""Literal restatements of the part of the reference's ``src/basins.jl`` that turns a density map into sites, and the cases the
site-extraction tests share.

The restatements follow the source line by line (cited as ``:N`` for ``basins.jl``, ``utils.jl:N`` otherwise), loops, queues and
orders included, in plain Python floats: slow, for small grids.  Inside them indices are 1-based like the source.  Nothing here touches
the library.  Where the reference calls ``imfilter`` (:668) the restatement calls ``smooth_exact_fma``: the definition of
``ceg_grid_smooth`` evaluated with an exact fused multiply-add (rational arithmetic, one rounding per tap).
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction
from pathlib import Path

import numpy as np

import basins_cases as BC
from basins_cases import _matvec, _norm2, grid_neighbors, julia_round, mod1, periodic_distance2
from ceg_hip.hostmirror.utils import mat_from_parameters, prepare_periodic_distance_computations

U = 2.0 ** -53


def _rng(*key):
    return np.random.default_rng([20240817, *key])


def periodic_setup(mat):
    m = np.asarray(mat, dtype=np.float64)
    ortho, safemin = prepare_periodic_distance_computations(m)
    return m.tolist(), bool(ortho), float(safemin)


# ---------------------------------------------------------------------------------------------------------------- utils.jl:257-280
def _norm(m, v):
    return math.sqrt(_norm2(_matvec(m, v)))


def periodic_distance_with_ofs(m, ortho, safemin, buffer):
    """-> (d, ofs, moved): ``ofs`` a list of three ints, ``moved`` whether the search over +1 / -1 changed it"""
    buffer = list(buffer)
    ofs = [0, 0, 0]
    for i in range(3):                                                            # utils.jl:258-261
        diff = buffer[i] + 0.5
        ofs[i] = math.floor(diff)
        buffer[i] = diff - ofs[i] - 0.5
    ref = _norm(m, buffer)                                                        # utils.jl:262
    if ortho or ref <= safemin:                                                   # utils.jl:263
        return ref, ofs, False
    for i in range(3):                                                            # utils.jl:264-278
        buffer[i] += 1
        newnorm = _norm(m, buffer)
        if newnorm < ref:
            ofs[i] -= 1
            return newnorm, ofs, True
        buffer[i] -= 2
        newnorm = _norm(m, buffer)
        if newnorm < ref:
            ofs[i] += 1
            return newnorm, ofs, True
        buffer[i] += 1
    return ref, ofs, False


# ---------------------------------------------------------------------------------------------------------------- :400-422
def nearest_literal(sites, dims, mat, active=None, origin=1):
    """Phase 2 of ``closest_to_sites`` for every active voxel (``active[i, j, k]`` truthy; all of them without it), in the order of
    :402.  ``origin = 1`` is :415 as written.  -> (lin, site, ofs, dist, nmoved, ntied): 0-based linear indices and sites, cell
    offsets, distances, how many (voxel, site) pairs took the search branch, and how many voxels have two DISTINCT sites at the same
    smallest distance with different offsets -- there ``findmin`` (:422) compares the tuples ``(d, ofs)`` and need not return the
    lowest index; no case may have one."""
    a, b, c = dims
    m, ortho, safemin = periodic_setup(mat)
    sites = [tuple(float(x) for x in s) for s in np.asarray(sites, dtype=np.float64).reshape(-1, 3)]
    lin, site, ofs, dist = [], [], [], []
    nmoved = ntied = 0
    for k in range(1, c + 1):                                                     # :402
        for j in range(1, b + 1):
            for i in range(1, a + 1):
                if active is not None and not active[i - 1, j - 1, k - 1]:
                    continue
                w = (i - 1 + origin, j - 1 + origin, k - 1 + origin)
                ijk = (w[0] / a, w[1] / b, w[2] / c)                              # :415
                best = None
                for isite, s in enumerate(sites):
                    d, o, moved = periodic_distance_with_ofs(m, ortho, safemin, [s[q] - ijk[q] for q in range(3)])      # :416-417
                    nmoved += moved
                    if best is None or d < best[0]:
                        best = (d, o, isite)
                    elif d == best[0] and o != best[1] and s != sites[best[2]]:
                        ntied += 1
                lin.append((i - 1) + a * ((j - 1) + b * (k - 1)))
                site.append(best[2])
                ofs.append(best[1])
                dist.append(best[0])
    return (np.asarray(lin, dtype=np.int32), np.asarray(site, dtype=np.int32), np.asarray(ofs, dtype=np.int8).reshape(-1, 3),
            np.asarray(dist, dtype=np.float64), nmoved, ntied)


# ---------------------------------------------------------------------------------------------------------------- :324-437
def closest_to_sites_literal(grid, sites, mat):
    """``closest_to_sites`` as written -> (Qs, weights, deletesite, cap_bound): ``Qs[s]`` the unwrapped 1-based points of kept site ``s``,
    ``weights[s]`` their values, ``deletesite`` 0-based, ``cap_bound`` whether ``rho > 1`` (:377) or ``s + rho > 1`` (:430) fired."""
    a, b, c = dims = grid.shape
    g = grid.tolist()
    m, ortho, safemin = periodic_setup(mat)
    safemin2 = safemin ** 2
    protoskin = math.sqrt(_norm2(_matvec(m, [1 / a, 1 / b, 1 / c])))              # :328
    sites = [tuple(float(x) for x in s) for s in np.asarray(sites, dtype=np.float64).reshape(-1, 3)]
    Qs = [[(1 + julia_round(a * i), 1 + julia_round(b * j), 1 + julia_round(c * k))] for i, j, k in sites]      # :329
    deletesite, known = [], set()
    for idx, Q in enumerate(Qs):                                                  # :332-339
        if Q[0] in known:
            deletesite.append(idx)
        else:
            known.add(Q[0])
    Qs = [Q for idx, Q in enumerate(Qs) if idx not in deletesite]
    sites = [s for idx, s in enumerate(sites) if idx not in deletesite]
    n = len(sites)
    cap_bound = False

    def val(p):
        return g[mod1(p[0], a) - 1][mod1(p[1], b) - 1][mod1(p[2], c) - 1]

    for isite in range(n):                                                        # :347
        site, Q = sites[isite], Qs[isite]
        todelete = []
        maxdist2 = math.inf
        for i2 in range(n):                                                       # :354-359
            if i2 == isite:
                continue
            maxdist2 = min(maxdist2, periodic_distance2(m, ortho, safemin2, [x - y for x, y in zip(site, sites[i2])]))
        maxdist2 /= 4
        skin2 = (protoskin + math.sqrt(maxdist2)) ** 2
        visited = np.zeros(dims, dtype=bool)
        visited[tuple(mod1(x, d) - 1 for x, d in zip(Q[0], dims))] = True
        rho = val(Q[0])
        for I in Q:                                                               # :365, grows while it is iterated
            for J in grid_neighbors(I):
                j = tuple(mod1(x, d) - 1 for x, d in zip(J, dims))
                if visited[j]:
                    continue
                visited[j] = True
                d2 = _norm2(_matvec(m, [s - (x - 1) / d for s, x, d in zip(site, J, dims)]))      # :370-372
                if d2 >= skin2:
                    continue
                if d2 >= maxdist2:
                    todelete.append(len(Q))                                       # 0-based position of the push below
                Q.append(J)
                rho += val(J)
                if rho > 1:                                                       # :377
                    break
            if rho > 1:                                                           # :379
                cap_bound = True
                break
        for pos in reversed(todelete):                                            # :381
            del Q[pos]
    allvisited = np.zeros(dims, dtype=bool)
    for Q in Qs:                                                                  # :386-394
        for pos in Q:
            w = tuple(mod1(x, d) - 1 for x, d in zip(pos, dims))
            assert not allvisited[w]
            allvisited[w] = True
    tovisit = [(i, j, k) for k in range(1, c + 1) for j in range(1, b + 1) for i in range(1, a + 1)
               if not allvisited[i - 1, j - 1, k - 1] and g[i - 1][j - 1][k - 1] != 0]       # :402-406
    tosites = []
    for visit in tovisit:                                                         # :410-422, findmin over the tuples (d, ofs .* dims)
        ijk = tuple(x / d for x, d in zip(visit, dims))
        best = None
        for isite, site in enumerate(sites):
            d, ofs, _ = periodic_distance_with_ofs(m, ortho, safemin, [site[q] - ijk[q] for q in range(3)])
            key = (d, tuple(float(o * dd) for o, dd in zip(ofs, dims)))
            if best is None or key < best[0]:
                best = (key, isite)
        tosites.append(best)
    weights = [[val(p) for p in Q] for Q in Qs]                                   # :423
    sumweights = []                                                               # :424, left to right
    for ws in weights:
        tot = 0.0
        for w in ws:
            tot += w
        sumweights.append(tot)
    for visit, (key, jsite) in zip(tovisit, tosites):                             # :425-434
        s = sumweights[jsite]
        rho = g[visit[0] - 1][visit[1] - 1][visit[2] - 1]
        if s + rho > 1:
            cap_bound = True
            continue
        sumweights[jsite] = s + rho
        weights[jsite].append(rho)
        Qs[jsite].append(tuple(v + o for v, o in zip(visit, key[1])))
    return Qs, weights, deletesite, cap_bound


def updated_sites_with_closest_literal(Qs, weights, dims):
    """:447-456 -> list of (s, [centre]); the sums run left to right"""
    out = []
    for Q, ws in zip(Qs, weights):
        s = 0.0
        for w in ws:
            s += w
        if s == 0:
            raise ValueError("Encountered empty weight: please use a non-zero atol value.")
        acc = [0.0, 0.0, 0.0]
        for ijk, w in zip(Q, ws):
            for q in range(3):
                acc[q] += (ijk[q] - 1) / dims[q] * w
        out.append((s, [x / s for x in acc]))
    return out


def cluster_closer_than_literal(ret, mat, maxdist):
    """:613-642 -> the new list"""
    m, ortho, safemin = periodic_setup(mat)
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
            d, ofs, _ = periodic_distance_with_ofs(m, ortho, safemin, [x - y for x, y in zip(pos1, pos2)])
            if d >= maxdist:
                continue
            todelete[i2] = True
            pos1 = [(rho1 * p1 + rho2 * (p2 + float(o))) / rho for p1, p2, o in zip(pos1, pos2, ofs)]
            rho1 = rho
            ret[i1] = (rho1, pos1)
    return [e for e, dead in zip(ret, todelete) if not dead]


# ---------------------------------------------------------------------------------------------------------------- :677-719
def greedy_literal(sortedidx, smoothed, grid, dims, mat, maxdist, atol, crop, maxbasins=math.inf):
    """The loop of ``coalescing_basins`` over ``sortedidx`` (0-based linear indices by decreasing smoothed value); ``smoothed`` and ``grid``
    flat in Julia's order.  -> (ret, branches): ``branches`` counts the paths taken, ``maxsubmid`` the largest ``submid`` seen."""
    a, b, c = dims
    ab = a * b
    m, ortho, safemin = periodic_setup(mat)
    ret = []
    br = dict(new=0, absorb=0, merge=0, low_val_many=0, zero=0, maxbasins=0, lone_low=0, maxsubmid=0)
    for newidx0 in sortedidx:
        newidx = int(newidx0) + 1
        smval = float(smoothed[newidx - 1])
        if smval <= crop:                                                         # :679
            break
        val = float(grid[newidx - 1])
        k, retk = (newidx - 1) // ab + 1, (newidx - 1) % ab + 1                   # fldmod1, :681
        j, i = (retk - 1) // a + 1, (retk - 1) % a + 1                            # :682
        pos = [i / a, j / b, k / c]                                               # :683
        in_distance = []
        for idx, (_, center) in enumerate(ret):                                   # :685-690
            d, ofs, _ = periodic_distance_with_ofs(m, ortho, safemin, [p - q for p, q in zip(pos, center)])
            if d > maxdist:
                continue
            in_distance.append((idx, [float(o) for o in ofs], d))
        if not in_distance and smval >= atol:                                     # :691-693
            ret.append((val, pos))
            br["new"] += 1
            if len(ret) >= maxbasins:
                br["maxbasins"] += 1
                break
        else:
            if len(in_distance) > 1:                                              # :695-699
                in_distance.sort(key=lambda e: e[2])                              # stable
                if val < atol:
                    submid = 1
                    br["low_val_many"] += 1
                else:
                    submid = next((q + 1 for q, e in enumerate(in_distance) if e[2] < maxdist / 2), 1)
                br["maxsubmid"] = max(br["maxsubmid"], submid)
                del in_distance[submid:]
            newcenter = [p * val for p in pos]                                    # :700-706
            newval = val
            for j2, o2, _ in in_distance:
                val2, center2 = ret[j2]
                for q in range(3):
                    newcenter[q] += (center2[q] + o2[q]) * val2
                newval += val2
            if newval == 0:                                                       # :707
                br["zero"] += 1
                continue
            newcenter = [x / newval for x in newcenter]                           # :708
            if len(in_distance) == 1:                                             # :709-710
                ret[in_distance[0][0]] = (newval, newcenter)
                br["absorb"] += 1
            else:                                                                 # :712-716
                js = sorted(e[0] for e in in_distance)
                for j2 in reversed(js):
                    del ret[j2]
                ret.append((newval, newcenter))
                br["merge" if js else "lone_low"] += 1
    return ret, br


# ---------------------------------------------------------------------------------------------------------------- smoothing
def smooth_exact_fma(x, taps):
    """The definition of ``ceg_grid_smooth`` with an exact fma: ``acc = round(tap * x + acc)`` in rational arithmetic, ``t`` ascending, axis
    0, then 1, then 2.  For grids of a few thousand voxels."""
    x = np.asarray(x, dtype=np.float64)
    for axis, t in enumerate(taps):
        w = len(t) // 2
        n = x.shape[axis]
        src = np.moveaxis(x, axis, 0)
        out = np.empty_like(src)
        ft = [Fraction(float(v)) for v in t]
        for idx in np.ndindex(src.shape[1:]):
            col = [Fraction(float(v)) for v in src[(slice(None),) + idx]]
            for p in range(n):
                acc = 0.0
                for q in range(len(t)):
                    acc = float(ft[q] * col[(p + q - w) % n] + Fraction(acc))
                out[(p,) + idx] = acc
        x = np.moveaxis(out, 0, axis).copy()
    return x


def smooth_longdouble(x, taps):
    """The same three passes in ``np.longdouble`` with the FP64 taps: the reference of the derived bound"""
    x = np.asarray(x).astype(np.longdouble)
    for axis, t in enumerate(taps):
        w = len(t) // 2
        acc = np.zeros_like(x)
        for q in range(len(t)):
            acc = acc + np.longdouble(t[q]) * np.roll(x, -(q - w), axis=axis)
        x = acc
    return x


def smooth_bound(absref, taps):
    """``gamma_n * S(|x|)`` with ``n = L0 + L1 + L2 + 1``: one rounding per fma plus the scale, no slack"""
    n = sum(len(t) for t in taps) + 1
    gamma = np.longdouble(n) * np.longdouble(U) / (1 - np.longdouble(n) * np.longdouble(U))
    return gamma * absref


def coalescing_basins_literal(grid, maxdist, mat, smooth=None, atol=0.1, crop=None, maxbasins=math.inf):
    """``coalescing_basins`` (:661-731) as a whole, with ``closest_to_sites`` as written.  -> (ret, cap_bound)"""
    from ceg_hip.basins import gaussian_taps, smoothing_sigmas
    dims = grid.shape
    flat = grid.ravel(order="F")
    if smooth == 0:                                                               # :664-669
        smoothed = flat
    else:
        taps = [gaussian_taps(s) for s in smoothing_sigmas(dims, mat, smooth)]
        smoothed = smooth_exact_fma(grid, taps).ravel(order="F")
    order = sorted(range(flat.size), key=lambda x: -smoothed[x])                  # sortperm(...; rev=true): stable
    _crop = atol * float(flat.max()) / 100 if crop is None else crop              # :676
    ret, _ = greedy_literal(order, smoothed, flat, dims, mat, maxdist, atol, _crop, maxbasins)
    cap_bound = False
    n1 = -1
    while len(ret) != n1:                                                         # :720-729
        n1 = len(ret)
        Qs, weights, _, cb = closest_to_sites_literal(grid, [p for _, p in ret], mat)
        cap_bound |= cb
        ret = updated_sites_with_closest_literal(Qs, weights, dims)
        ret = cluster_closer_than_literal(ret, mat, maxdist)
        newret = [e for e in ret if e[0] >= atol]
        if not newret:
            return ret, cap_bound
        ret = newret
    return ret, cap_bound


# ---------------------------------------------------------------------------------------------------------------- cells
@functools.lru_cache(maxsize=None)
def cit7_mat():
    import ceg_hip
    ceg_hip.setdir_RASPA(Path(__file__).resolve().parent / "golden" / "raspa")
    return np.asarray(ceg_hip.load_framework_RASPA("CIT-7", "BoulfelfelSholl2021").mat, dtype=np.float64)


ORTHO_MAT = np.diag([11.5, 11.0, 12.5])
SKEW_MAT = mat_from_parameters((12.0, 11.0, 13.0), (80.0, 95.0, 105.0))


# ---------------------------------------------------------------------------------------------------------------- smoothing cases
def _taps(length, seed):
    """positive taps that sum to 1 up to rounding, no symmetry"""
    t = _rng(1, length, seed).uniform(0.5, 1.5, size=length)
    return t / t.sum()


@functools.lru_cache(maxsize=None)
def smooth_cases():
    """-> list of (name, shape, (taps0, taps1, taps2)).  The last two are not in the issue: one takes the 32-wide tile of the
    strided pass (99 and 129 taps, the first length past the switch and the longest) and a run that is no multiple of the tile, the
    other the 64-wide tile at its largest (97 taps on axes 1 and 2: 57 344 B of LDS)."""
    spec = [("1x1x1", (1, 1, 1), (1, 1, 1)), ("5x3x1-9", (5, 3, 1), (9, 9, 9)), ("7x130x4", (7, 130, 4), (129, 1, 3)),
            ("70x66x65-9", (70, 66, 65), (9, 9, 9)), ("70x66x65-17", (70, 66, 65), (1, 17, 1)), ("3x70x35-wide", (3, 70, 35), (3, 129, 99)),
            ("5x70x19-97", (5, 70, 19), (1, 97, 97))]
    return [(name, shape, tuple(_taps(L, q) if L > 1 else np.ones(1) for q, L in enumerate(lens))) for name, shape, lens in spec]


def smooth_input(shape, kind):
    """values in [0.5, 1.5) (FP64) or counts in [1, 2^40) (int64): far from the denormal range"""
    r = _rng(2, *shape)
    if kind == "f64":
        return r.uniform(0.5, 1.5, size=shape)
    return r.integers(1, 2**40, size=shape).astype(np.int64)


INT_SCALE = 1.0 / 3000.0


@functools.lru_cache(maxsize=None)
def smooth_reference(name, kind):
    """-> (x as the first rounding leaves it, longdouble reference, bound)"""
    _, shape, taps = next(c for c in smooth_cases() if c[0] == name)
    g = smooth_input(shape, kind)
    if kind == "f64":
        x = g
        ref = smooth_longdouble(x, taps)
    else:                                                # the bound counts the scale's rounding: the reference starts from the
        x = g.astype(np.float64) * INT_SCALE             # product in longdouble (40 + 53 bits into 64: one part in 2^64)
        ref = smooth_longdouble(g.astype(np.longdouble) * np.longdouble(INT_SCALE), taps)
    return x, ref, smooth_bound(np.abs(ref), taps)


# ---------------------------------------------------------------------------------------------------------------- ranking cases
@functools.lru_cache(maxsize=None)
def ranked_cases():
    """-> list of (name, grid FP64, crop, capacity or None)"""
    r = _rng(3)
    shape = (17, 9, 33)
    ties = r.integers(0, 6, size=shape).astype(np.float64)                        # 5049 voxels, six values: thousands of ties
    cases = [("ties", ties, 0.0, None), ("ties-crop2", ties, 2.0, None), ("none", ties, 5.0, None), ("all", ties + 1.0, 0.5, None)]
    for count in (2048, 2049):
        g = np.zeros(70 * 66 * 65)
        g[r.choice(g.size, size=count, replace=False)] = r.integers(1, 40, size=count).astype(np.float64) / 8
        cases.append((f"count-{count}", g.reshape((70, 66, 65), order="F"), 0.0, None))
    special = r.uniform(0.0, 1.0, size=(5, 7, 3))
    special[1, 2, 0] = special[4, 6, 2] = math.inf
    special[2, 2, 1] = math.nan
    special[0, 0, 0] = -0.0
    special[3, 1, 1] = -math.inf
    cases.append(("inf-nan", special, 0.0, None))
    cases.append(("short-capacity", ties, 0.0, 1000))
    cases.append(("1x1x1", np.full((1, 1, 1), 2.5), 0.0, None))
    return cases


def ranked_reference(g, crop):
    flat = g.ravel(order="F").tolist()
    sel = [x for x, v in enumerate(flat) if v > crop]
    order = sorted(sel, key=lambda x: (-flat[x], x))
    return order, [flat[x] for x in order]


# ---------------------------------------------------------------------------------------------------------------- nearest-site cases
def _half_cell_site(dims, origin):
    """a site exactly half a cell from the voxels j = 1 of a 3 x 2 x 5 grid along axis 1: (1 + origin)/2 and the sum are exact, so
    buffer + 0.5 is the integer 1.0 there, the edge of ``floor``"""
    assert dims[1] == 2
    return [0.4, (1 + origin) / 2 + 0.5, 0.6]


@functools.lru_cache(maxsize=None)
def nearest_cases():
    """-> list of (name, sites (n, 3), dims, mat, active bool[a, b, c] or None, capacity or None)"""
    r = _rng(4)
    cit7 = cit7_mat()
    cases = []
    small = (3, 2, 5)
    for cname, mat in (("cit7", cit7), ("ortho", ORTHO_MAT)):
        s3 = r.uniform(-0.2, 1.2, size=(3, 3))
        s3[2] = s3[0]                                                             # two identical sites: the lowest index wins
        cases.append((f"{cname}-1x1x1-one", r.random((1, 3)), (1, 1, 1), mat, None, None))
        cases.append((f"{cname}-3x2x5-one", r.random((1, 3)), small, mat, None, None))
        cases.append((f"{cname}-3x2x5-two", r.uniform(-3, 3, size=(2, 3)), small, mat, None, None))
        cases.append((f"{cname}-3x2x5-three-twins", s3, small, mat, None, None))
        half = np.asarray([_half_cell_site(small, 0), _half_cell_site(small, 1), [0.1, 0.7, 0.3]])
        cases.append((f"{cname}-3x2x5-half-cell", half, small, mat, None, None))
        sparse = r.random(small) < 0.3
        cases.append((f"{cname}-3x2x5-sparse", r.random((2, 3)), small, mat, sparse, None))
        cases.append((f"{cname}-3x2x5-empty", r.random((2, 3)), small, mat, np.zeros(small, dtype=bool), None))
        cases.append((f"{cname}-3x2x5-short", r.random((3, 3)), small, mat, None, 11))
    big = (70, 66, 65)
    sparse = _rng(5).random(big) < 0.004                                           # about 1200 voxels: the literal stays quick
    cases.append(("cit7-70x66x65-sparse", r.random((7, 3)), big, cit7, sparse, None))
    cases.append(("ortho-70x66x65-sparse-short", r.random((7, 3)), big, ORTHO_MAT, sparse, 500))
    very = _rng(6).random(big) < 0.0001                                            # about 30 voxels against 2048 sites
    cases.append(("cit7-70x66x65-2048", r.random((2048, 3)), big, cit7, very, None))
    # skewed enough for the search: 12 x 10 x 14 voxels all active
    cases.append(("cit7-12x10x14-all", r.uniform(-1, 2, size=(5, 3)), (12, 10, 14), cit7, None, None))
    return cases


@functools.lru_cache(maxsize=None)
def nearest_reference(name, origin):
    _, sites, dims, mat, active, _ = next(c for c in nearest_cases() if c[0] == name)
    return nearest_literal(sites, dims, mat, active, origin)


# ---------------------------------------------------------------------------------------------------------------- greedy cases
GREEDY_DIMS = (12, 10, 14)


def _lin(i, j, k, dims=GREEDY_DIMS):
    return i + dims[0] * (j + dims[1] * k)


@functools.lru_cache(maxsize=None)
def greedy_cases():
    """Hand-made rankings -> list of (name, lin, smoothed, values, dims, mat, maxdist, atol, maxbasins, expected branches)"""
    d = GREEDY_DIMS
    cases = []
    for cname, mat in (("ortho", ORTHO_MAT), ("skew", SKEW_MAT)):
        # three far-apart voxels: three new basins
        lin = [_lin(1, 1, 1), _lin(7, 5, 8), _lin(1, 6, 12)]
        cases.append((f"{cname}-new", lin, [0.9, 0.8, 0.7], [0.5, 0.25, 0.125], d, mat, 1.5, 0.1, math.inf, dict(new=3)))
        # neighbours of one voxel: absorbed one after the other
        lin = [_lin(5, 5, 5), _lin(6, 5, 5), _lin(5, 4, 5), _lin(4, 5, 6)]
        cases.append((f"{cname}-absorb", lin, [0.9, 0.8, 0.7, 0.6], [0.4, 0.3, 0.2, 0.1], d, mat, 2.5, 0.1, math.inf, dict(new=1, absorb=3)))
        # two basins 4 voxels apart, then the voxel between them with both in range: as :696-697 are written the list is sorted by
        # increasing distance, so findfirst is 1 whenever it finds anything and submid never exceeds 1: the voxel joins the nearer
        lin = [_lin(3, 5, 5), _lin(7, 5, 5), _lin(5, 5, 5), _lin(4, 5, 5)]
        cases.append((f"{cname}-several-in-range", lin, [0.9, 0.8, 0.7, 0.6], [0.4, 0.3, 0.2, 0.1], d, mat, 2.2, 0.1, math.inf,
                      dict(new=2, absorb=2, maxsubmid=1)))
        # the same with the middle voxel's value below atol
        cases.append((f"{cname}-low-val-several", lin, [0.9, 0.8, 0.7, 0.6], [0.4, 0.3, 0.05, 0.1], d, mat, 2.2, 0.1, math.inf,
                      dict(new=2, absorb=2, low_val_many=1)))
        # nothing in range and smval < atol: (val, pos*val/val) is appended; with val == 0 it is skipped
        lin = [_lin(1, 1, 1), _lin(7, 5, 8), _lin(1, 6, 12), _lin(8, 1, 3)]
        cases.append((f"{cname}-lone-low-and-zero", lin, [0.9, 0.05, 0.04, 0.03], [0.5, 0.3, 0.0, 0.07], d, mat, 1.5, 0.1, math.inf,
                      dict(new=1, lone_low=2, zero=1)))
        # the loop ends with the second basin
        cases.append((f"{cname}-maxbasins", [_lin(1, 1, 1), _lin(7, 5, 8), _lin(1, 6, 12)], [0.9, 0.8, 0.7], [0.5, 0.25, 0.125], d, mat, 1.5,
                      0.1, 2, dict(new=2, maxbasins=1)))
        # across the cell boundary: the offsets enter the centre
        lin = [_lin(0, 0, 0), _lin(11, 9, 13), _lin(11, 0, 0), _lin(0, 9, 0)]
        cases.append((f"{cname}-wrap", lin, [0.9, 0.8, 0.7, 0.6], [0.4, 0.3, 0.2, 0.1], d, mat, 2.5, 0.1, math.inf, dict(new=1, absorb=3)))
    return cases


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E = [("ortho", ORTHO_MAT, (24, 22, 26), ([0.02, 0.2, 0.2], [0.52, 0.7, 0.2], [0.52, 0.2, 0.7], [0.02, 0.7, 0.7])),
       ("cit7", None, (26, 22, 18), ([0.02, 0.2, 0.25], [0.52, 0.7, 0.25], [0.02, 0.7, 0.75]))]


@functools.lru_cache(maxsize=None)
def e2e_cases():
    """-> list of (name, grid FP64 or int64 bins, counter or None, mat, maxdist, kwargs, number of clouds).  Clouds of 48 hits within
    about 1.5 A of centres 7 A and more apart, on voxels of half an angstrom: the two nearest sites of a cloud's voxel then differ by
    far more than two voxel diagonals.  One centre sits at a cell face.  Every hit carries a random integer weight below 2^20 and the
    counter is 2^26: the values are generic (no two smoothed values tie unless one voxel alone feeds both) and yet every sum of them
    is exact in any order."""
    cases = []
    for cname, mat, dims, centres in E2E:
        mat = cit7_mat() if mat is None else mat
        r = _rng(7)
        bins = np.zeros(dims, dtype=np.int64)
        for cen in centres:
            for _ in range(48):
                p = np.floor(((np.asarray(cen) + r.normal(scale=0.035, size=3)) % 1.0) * dims).astype(int)
                bins[tuple(p)] += int(r.integers(2**19, 2**20))
        counter = 2**26                                                           # about 0.56 atoms per site and frame
        n = len(centres)
        cases.append((f"{cname}-bins", bins, counter, mat, 2.0, dict(atol=0.05), n))
        cases.append((f"{cname}-f64", bins.astype(np.float64) / counter, None, mat, 2.0, dict(atol=0.05), n))
        cases.append((f"{cname}-f64-nosmooth", bins.astype(np.float64) / counter, None, mat, 2.0, dict(atol=0.05, smooth=0), n))
    return cases
