"""Literal, queue-based restatements of ``local_basins`` / ``decompose_basins`` of the reference's ``src/basins.jl`` in plain Python, and
the cases the basin tests share.

The restatements follow the source line by line (cited as ``:N``): ``circular_distance`` :108-113, ``clean_cluster!`` :116-138,
``keep_shortest_distance!`` :140-172, ``local_basins`` :195-252, ``decompose_basins`` :765-792.  Inside them indices are 1-based and
unwrapped like the source; what they return is 0-based and wrapped.  They carry one switch, ``as_written``: ``True`` keeps the skip
of :153 (a basin whose last level holds exactly one point never processes that level) and also returns that point per basin;
``False`` processes that level like any other, which is the definition the device code follows.  Nothing here touches the library.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from basins_cases import SHAPES, _rng, grid_neighbors, local_minima_literal, minima_cases, mod1

MAX_OWNERS = 16


# ---------------------------------------------------------------------------------------------------------------- :108-138
def circular_distance_literal(a, mn):
    m, n = mn
    b = a // 2                                                                    # :109
    i, j = (m, n) if m <= n else (n, m)                                           # minmax
    if i < b < j:                                                                 # :111
        return min(j - i, i - j + a)
    return j - i


def clean_cluster_literal(basinsets, minima, cluster, dims):
    """:116-138 in place on ``basinsets``; ``minima`` 1-based.  -> the 0-based positions that were deleted"""
    if not cluster > 0:                                                           # :117
        return []
    a, b, c = dims
    nminima = len(minima)
    unions = list(range(nminima))
    for i1 in range(nminima):                                                     # :120
        a1, b1, c1 = minima[i1]
        for i2 in range(i1 + 1, nminima):
            a2, b2, c2 = minima[i2]
            if circular_distance_literal(a, (a1, a2)) + circular_distance_literal(b, (b1, b2)) + circular_distance_literal(c, (c1, c2)) <= cluster:
                unions[i2] = unions[i1]                                           # :125
    todelete = []
    for i in range(nminima):                                                      # :130
        j = unions[i]
        if i == j:
            continue
        basinsets[j] |= basinsets[i]
        todelete.append(i)
    for i in reversed(todelete):                                                  # deleteat!
        del basinsets[i]
    return todelete


# ---------------------------------------------------------------------------------------------------------------- :140-172
def keep_shortest_distance_literal(protobasinsets, dims, as_written):
    """-> (basinsets of unwrapped 1-based tuples, the wrapped 0-based sole last-level point of each basin or None)"""
    n = len(protobasinsets)
    basinsets = [set(Q) for Q, _ in protobasinsets]                               # :142
    dists_of = [list(d) for _, d in protobasinsets]
    sole = [None] * n
    old, new = set(), set()
    indices = [1] * n
    while True:
        noadvance = True
        for itask in range(n):
            basin = basinsets[itask]
            Q, dists = protobasinsets[itask][0], dists_of[itask]
            start = indices[itask]
            if not dists:                                                         # :152
                if start == len(Q):
                    sole[itask] = tuple(mod1(x, d) - 1 for x, d in zip(Q[-1], dims))
                    if as_written:
                        continue                                                  # :153
                stop = len(Q)
            else:
                noadvance = False
                stop = dists.pop(0) - 1                                           # :157
            indices[itask] = stop + 1
            for i in range(start, stop + 1):                                      # :160
                u = Q[i - 1]
                iu = tuple(mod1(x, d) for x, d in zip(u, dims))
                if iu in old:
                    basin.discard(u)
                new.add(iu)
        if noadvance:
            break
        old |= new
        new = set()
    return basinsets, sole


# ---------------------------------------------------------------------------------------------------------------- :195-252
def local_basins_literal(grid, minima0, *, maxima=False, cluster=0, skip_above=math.inf, maxdist=0, as_written=False):
    """``minima0``: 0-based starts.  -> dict(kept = the 0-based positions in ``minima0`` of the basins returned, in order; basins = their
    sets of wrapped 0-based points; levels = per basin {point: breadth-first level}; sole = per basin its sole last-level point or
    None (before ``cluster``)).  ``clean_cluster!`` gets the kept minima (the reference passes its in-place filtered list, :241-250)."""
    dims = grid.shape
    g = grid.tolist()
    lt = (lambda x, y: x > y) if maxima else (lambda x, y: x < y)
    skip = lambda v: v > skip_above
    minima = [tuple(int(x) + 1 for x in p) for p in minima0]
    protobasinsets, levels = [], []
    for start in minima:                                                          # :200
        visited = np.zeros(dims, dtype=bool).tolist()
        istart, jstart, kstart = start
        if skip(g[istart - 1][jstart - 1][kstart - 1]):                           # :204
            protobasinsets.append(([], []))
            levels.append({})
            continue
        visited[istart - 1][jstart - 1][kstart - 1] = True
        Q = [start]
        lev = {tuple(x - 1 for x in start): 0}
        current_dist, start_dist, dists, mark_dist = 0, 1, [1], False
        idx = 0
        while idx < len(Q):                                                       # :214, Q grows while it is iterated
            u = Q[idx]
            idx += 1
            if idx == start_dist:
                current_dist += 1
                mark_dist = True
            iu = tuple(mod1(x, d) for x, d in zip(u, dims))
            gu = g[iu[0] - 1][iu[1] - 1][iu[2] - 1]
            for v in grid_neighbors(u):
                iv = tuple(mod1(x, d) for x, d in zip(v, dims))
                if visited[iv[0] - 1][iv[1] - 1][iv[2] - 1]:
                    continue
                gv = g[iv[0] - 1][iv[1] - 1][iv[2] - 1]
                if skip(gv):
                    continue
                if (maxdist == 0 or current_dist < maxdist) and lt(gu, gv):      # :226
                    Q.append(v)
                    lev[tuple(x - 1 for x in iv)] = current_dist
                    if mark_dist:
                        start_dist = len(Q)
                        dists.append(start_dist)
                        mark_dist = False
                    visited[iv[0] - 1][iv[1] - 1][iv[2] - 1] = True
        protobasinsets.append((Q, dists))
        levels.append(lev)
    kept = [i for i, (Q, _) in enumerate(protobasinsets) if Q]                    # :239-241
    protobasinsets = [protobasinsets[i] for i in kept]
    levels = [levels[i] for i in kept]
    basinsets, sole = keep_shortest_distance_literal(protobasinsets, dims, as_written)      # :243
    empty2 = [t for t, s in enumerate(basinsets) if not s]                        # :244-246
    for t in reversed(empty2):
        del basinsets[t], kept[t], levels[t], sole[t]
    wrapped = [{tuple(mod1(x, d) - 1 for x, d in zip(u, dims)) for u in s} for s in basinsets]
    deleted = clean_cluster_literal(wrapped, [minima[i] for i in kept], cluster, dims)      # :250
    for t in reversed(deleted):
        del kept[t]
    return dict(kept=kept, basins=wrapped, levels=levels, sole=sole)


# ---------------------------------------------------------------------------------------------------------------- :765-792
def decompose_basins_literal(dims, basinsets):
    """``basinsets``: sets of 0-based wrapped points.  -> (points sorted as :790, {point: tuple of 0-based basin positions})"""
    a, b, c = dims
    n = len(basinsets)
    nodes = {}                                                                    # fill(Int[], size(grid)): absent = the empty vector
    refvectors = [(i,) for i in range(1, n + 1)]
    refidx = {(i,): i for i in range(1, n + 1)}
    pointsset = set()
    for iset, bset in enumerate(basinsets, start=1):                              # :772
        pointsset |= bset
        for i, j, k in bset:
            w = (mod1(i + 1, a), mod1(j + 1, b), mod1(k + 1, c))
            node = nodes.get(w, ()) + (iset,)                                     # push!
            ref = refidx.get(node)
            if ref is None:
                refvectors.append(node)
                refidx[node] = len(refvectors)
                ref = len(refvectors)
            nodes[w] = refvectors[ref - 1]                                        # :786 (after the pop!)
    points = sorted(pointsset, key=lambda p: (p[2], p[1], p[0]))                  # :790
    return points, {tuple(x - 1 for x in w): tuple(s - 1 for s in v) for w, v in nodes.items()}


# ---------------------------------------------------------------------------------------------------------------- expected arrays
def arrays_from_sets(dims, nstarts, kept, basins, levels):
    """what ``ceg_grid_basins`` returns, from the sets of a run without ``cluster``"""
    a, b, c = dims
    n = a * b * c
    level = np.full(n, -1, dtype=np.int32)
    owners = {}
    size = np.zeros(nstarts, dtype=np.int32)
    for idx, bset, lev in zip(kept, basins, levels):
        size[idx] = len(bset)
        for p in bset:
            lin = p[0] + a * (p[1] + b * p[2])
            owners.setdefault(lin, []).append(idx)
            assert level[lin] in (-1, lev[p]), "a point kept by two basins at different levels"
            level[lin] = lev[p]
    owner = np.full(n, -1, dtype=np.int32)
    nown = np.zeros(n, dtype=np.uint8)
    shared = []
    for lin in sorted(owners):
        o = sorted(owners[lin])
        owner[lin], nown[lin] = o[0], len(o)
        if len(o) > 1:
            shared += [(lin, x) for x in o]
    return dict(level=level.reshape(dims, order="F"), owner=owner.reshape(dims, order="F"), nowners=nown.reshape(dims, order="F"),
                shared=np.asarray(shared, dtype=np.int32).reshape(-1, 2), size=size)


# ---------------------------------------------------------------------------------------------------------------- cases
def _name(shape):
    return "x".join(map(str, shape))


def _smooth(shape, seed, noise=0.3):
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    a, b, c = shape
    return (np.sin(2 * np.pi * i / a + seed) + np.cos(2 * np.pi * j / b) * np.sin(4 * np.pi * k / c + 0.3)
            + noise * _rng(21, seed, *shape).normal(size=shape))


def _minima(g, maxima=False):
    return local_minima_literal(g, -1.0, maxima)[0]


def fan(radius):
    """(11, 11, 1): g = -(|i - 5| + |j - 5|), the starts = every point at that Manhattan radius from the centre, all of which own the
    centre: 4 * radius owners"""
    i, j, k = np.meshgrid(np.arange(11), np.arange(11), np.arange(1), indexing="ij")
    g = -(np.abs(i - 5) + np.abs(j - 5)).astype(np.float64)
    starts = [(int(p), int(q), 0) for q in range(11) for p in range(11) if abs(p - 5) + abs(q - 5) == radius]
    return g, starts


@functools.lru_cache(maxsize=None)
def basin_cases():
    """-> list of (name, grid, starts [0-based tuples], kwargs of local_basins (maxima / skip_above / maxdist), literal?).  ``literal``
    False: too large for one pure-Python search per start; its reference is the host NumPy form."""
    cases = []
    small = [s for s in SHAPES if s != (70, 66, 65)]
    for shape in small:
        g = _rng(31, *shape).uniform(-3.0, 1.0, size=shape)
        cases.append((f"random-{_name(shape)}", g, _minima(g), {}, True))
    big = (17, 9, 33)
    sm = _smooth(big, 1)
    cases.append((f"smooth-{_name(big)}", sm, _minima(sm), {}, True))
    rnd = _rng(31, *big).uniform(-3.0, 1.0, size=big)
    for md in (1, 2, 3, 7):
        cases.append((f"smooth-{_name(big)}-maxdist{md}", sm, _minima(sm), dict(maxdist=md), True))
        cases.append((f"random-{_name(big)}-maxdist{md}", rnd, _minima(rnd), dict(maxdist=md), True))
    mx = -_smooth(big, 2)
    cases.append((f"maxima-{_name(big)}", mx, _minima(mx, True), dict(maxima=True), True))
    mxr = -_rng(32, 5, 7, 3).uniform(-3.0, 1.0, size=(5, 7, 3))
    cases.append(("maxima-5x7x3", mxr, _minima(mxr, True), dict(maxima=True), True))
    # skip at a mid value: some starts are skipped, and the others' basins stop below it
    for nm, g in (("smooth", sm), ("random", rnd)):
        st = _minima(g)
        vals = sorted(g[p] for p in st)
        cut = 0.5 * (vals[len(vals) // 2 - 1] + vals[len(vals) // 2])
        assert any(g[p] > cut for p in st) and any(not g[p] > cut for p in st)
        cases.append((f"{nm}-{_name(big)}-skip", g, st, dict(skip_above=cut), True))
        cases.append((f"{nm}-{_name(big)}-skip-maxdist3", g, st, dict(skip_above=cut, maxdist=3), True))
    # a plateau: equal values give no edge
    pl = np.round(_smooth((9, 8, 10), 3, noise=0.0) * 2.0) / 2.0
    order = np.argsort(pl.ravel(order="F"), kind="stable")
    pst = [(int(x % 9), int((x // 9) % 8), int(x // 72)) for x in order[[0, 7, 40]]]
    cases.append(("plateau-9x8x10", pl, pst, {}, True))
    # NaN, +Inf, -Inf: as values on the way and as starts
    sp = rnd.copy()
    sp[3, 4, 5], sp[10, 2, 20], sp[7, 7, 7], sp[0, 0, 32] = math.nan, math.inf, -math.inf, math.nan
    spst = [p for p in _minima(sp) if p not in ((7, 7, 7),)] + [(3, 4, 5), (7, 7, 7), (10, 2, 20)]
    cases.append((f"special-{_name(big)}", sp, spst, {}, True))
    cases.append((f"special-{_name(big)}-skip", sp, spst, dict(skip_above=0.0), True))
    zeros = np.full((5, 7, 3), 1.0)
    zeros[2, 3, 1], zeros[3, 3, 1] = -0.0, 0.0                                    # -0.0 < 0.0 is false: no edge between the two starts
    cases.append(("negative-zero", zeros, [(2, 3, 1), (3, 3, 1)], {}, True))
    # starts that are no minima: one reachable from another (a minimum and the point uphill of it), and two adjacent ones
    m0 = _minima(sm)[0]
    up = max(((m0[0] + d) % 17 for d in (1, -1)), key=lambda i: sm[i, m0[1], m0[2]])
    user = [m0, (up, m0[1], m0[2]), (8, 4, 16), (9, 4, 16), (2, 2, 2)]
    assert len(set(user)) == len(user)
    cases.append((f"user-starts-{_name(big)}", sm, user, {}, True))
    cases.append((f"user-starts-{_name(big)}-maxdist3", sm, user, dict(maxdist=3), True))
    # the fan: 16 owners of one point, exactly the cap
    fg, fst = fan(4)
    cases.append(("fan-16", fg, fst, {}, True))
    # starts on every face, basins through every face
    faces = [(0, 4, 10), (16, 4, 20), (5, 0, 7), (5, 8, 9), (8, 4, 0), (8, 4, 32), (0, 0, 0), (16, 8, 32)]
    cases.append((f"faces-{_name(big)}", _smooth(big, 4, noise=0.05), faces, {}, True))
    wrap = next(g for n, g, tol, mxm in minima_cases() if n == "wrap-17x9x33-tol-1.0")
    cases.append(("wrap-17x9x33", wrap, _minima(wrap), {}, True))
    # 300 k points, at most 60 starts: the lowest minima of a smooth field with little noise
    large = (70, 66, 65)
    lg = _smooth(large, 5, noise=0.02)
    from ceg_hip.basins import local_minima_host
    lm = local_minima_host(lg, -1.0)
    lm = lm[np.argsort(lg[lm[:, 0], lm[:, 1], lm[:, 2]], kind="stable")[:60]]
    lst = sorted((tuple(int(x) for x in p) for p in lm), key=lambda p: (p[2], p[1], p[0]))
    assert 1 < len(lst) <= 60
    cases.append((f"smooth-{_name(large)}", lg, lst, {}, False))
    cases.append((f"smooth-{_name(large)}-maxdist7", lg, lst, dict(maxdist=7), False))
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def case(name):
    return next(c for c in basin_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def literal_reference(name, as_written=False, cluster=0):
    _, g, starts, kw, literal = case(name)
    assert literal
    return local_basins_literal(g, starts, as_written=as_written, cluster=cluster, **kw)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the arrays of ``ceg_grid_basins`` for a case: from the literal (as_written=False), or from the host NumPy form for the large ones"""
    _, g, starts, kw, literal = case(name)
    if literal:
        r = literal_reference(name)
        return arrays_from_sets(g.shape, len(starts), r["kept"], r["basins"], r["levels"])
    from ceg_hip.basins import local_basins_host
    b = local_basins_host(g, starts, **kw)
    return dict(level=b.level, owner=b.owner, nowners=b.nowners, shared=b.shared, size=b.size)
