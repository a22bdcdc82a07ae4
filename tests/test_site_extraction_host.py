"""Site extraction without a device: the host greedy pass of the library (``ceg_coalesce_ranked``) against the literal loop bit for bit,
the NumPy ``*_host`` forms of ``ceg_hip/basins.py`` against the literal restatements of ``tests/site_extraction_cases.py``, and the
conditions on the INPUTS that the GPU tests rely on (search branch taken, no ambiguous ties, separated smoothed values, a bounded share
of ambiguous voxels)."""
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import site_extraction_cases as SC
from ceg_hip import _abi, basins as B

ROOT = Path(__file__).resolve().parent.parent


def _ids(cases):
    return [c[0] for c in cases]


def _same(got, ref):
    """two lists of (value, centre): the same bits"""
    assert len(got) == len(ref)
    for (v, p), (rv, rp) in zip(got, ref):
        assert v == rv and list(map(float, p)) == list(map(float, rp))


# ---------------------------------------------------------------------------------------------------------------- taps, smoothing
def test_gaussian_taps():
    assert B.gaussian_taps(0.0).tolist() == [1.0]
    for sigma in (0.3, 1.0, 1.7, 2.0, 5.5):
        t = B.gaussian_taps(sigma)
        w = 2 * math.ceil(sigma)
        assert len(t) == 2 * w + 1 and np.array_equal(t, t[::-1]) and abs(t.sum() - 1.0) <= 4 * SC.U * len(t)
        assert t[w + 1] / t[w] == pytest.approx(math.exp(-1.0 / (2 * sigma * sigma)), rel=1e-14)
    with pytest.raises(ValueError):
        B.gaussian_taps(-1.0)
    sig = B.smoothing_sigmas((12, 10, 14), SC.ORTHO_MAT, 0.5)
    assert sig == pytest.approx((0.5 * 12 / 11.5, 0.5 * 10 / 11.0, 0.5 * 14 / 12.5), rel=1e-15)


@pytest.mark.parametrize("case", SC.smooth_cases()[:3], ids=_ids(SC.smooth_cases()[:3]))
def test_smooth_host_forms_agree(case):
    """the vectorised host form (a multiplication and an addition per tap) stays within twice the fma bound of the longdouble form, and
    the exact-fma restatement within the bound itself"""
    name, shape, taps = case
    x, ref, bound = SC.smooth_reference(name, "f64")
    got = B.smooth_grid_host(x, taps)
    assert np.all(np.abs(got.astype(np.longdouble) - ref) <= 2 * bound)
    if x.size <= 64:
        assert np.all(np.abs(SC.smooth_exact_fma(x, taps).astype(np.longdouble) - ref) <= bound)


def test_smooth_host_impulse_and_constant():
    taps = SC.smooth_cases()[1][2]                                                  # 9 taps per axis on 5 x 3 x 1: several wraps
    x = np.zeros((5, 3, 1))
    x[2, 1, 0] = 1.0
    want = np.zeros((5, 3, 1))
    for t0 in range(9):
        for t1 in range(9):
            for t2 in range(9):                                                     # y[p] takes taps[t + w] from x[p + t]: the impulse lands at p = 2 - t
                want[(2 - (t0 - 4)) % 5, (1 - (t1 - 4)) % 3, 0] += taps[0][t0] * taps[1][t1] * taps[2][t2]
    assert np.allclose(B.smooth_grid_host(x, taps), want, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------- ranking
@pytest.mark.parametrize("case", SC.ranked_cases(), ids=_ids(SC.ranked_cases()))
def test_ranked_host(case):
    name, g, crop, _ = case
    idx, val = SC.ranked_reference(g, crop)
    got_idx, got_val = B.ranked_above_host(g, crop)
    assert got_idx.tolist() == idx and got_val.tolist() == val
    with pytest.raises(ValueError):
        B.ranked_above_host(g, -1.0)


# ---------------------------------------------------------------------------------------------------------------- nearest site
@pytest.mark.parametrize("case", SC.nearest_cases(), ids=_ids(SC.nearest_cases()))
def test_nearest_host(case):
    name, sites, dims, mat, active, _ = case
    for origin in (0, 1):
        lin, site, ofs, dist, nmoved, ntied = SC.nearest_reference(name, origin)
        assert ntied == 0, "two distinct sites tie exactly with different offsets: findmin's answer is not the lowest index"
        got = B.site_nearest_host(sites, dims, mat, bins=None if active is None else active.astype(np.int64), origin=origin)
        assert np.array_equal(got[0], lin) and np.array_equal(got[1], site) and np.array_equal(got[2], ofs)
        assert np.array_equal(got[3], dist)                                        # to the bit
        if name.startswith("cit7") and "1x1x1" not in name and "empty" not in name:
            assert nmoved > 0, "the skewed cell must take the search branch"
        if name.startswith("ortho"):
            assert nmoved == 0


def test_nearest_half_cell_edge_is_exact():
    """the site of the half-cell case sits where ``buffer + 0.5`` is exactly 1.0 for the voxels j = 1"""
    for origin in (0, 1):
        y = SC._half_cell_site((3, 2, 5), origin)[1]
        assert (y - (1 + origin) / 2) + 0.5 == 1.0
    _, sites, dims, mat, _, _ = next(c for c in SC.nearest_cases() if c[0] == "ortho-3x2x5-half-cell")
    lin, site, ofs, dist, _, _ = SC.nearest_reference("ortho-3x2x5-half-cell", 0)
    assert any(s == 0 and o[1] == 1 for s, o in zip(site.tolist(), ofs.tolist()))


def test_cit7_is_not_ortho():
    _, ortho, safemin = SC.periodic_setup(SC.cit7_mat())
    assert not ortho and safemin > 0
    assert SC.periodic_setup(SC.ORTHO_MAT)[1]


# ---------------------------------------------------------------------------------------------------------------- greedy pass
@pytest.mark.parametrize("case", SC.greedy_cases(), ids=_ids(SC.greedy_cases()))
def test_greedy_pass_equals_the_literal_loop(case):
    name, lin, sm, val, dims, mat, maxdist, atol, maxbasins, expect = case
    n = dims[0] * dims[1] * dims[2]
    smoothed, grid = np.zeros(n), np.zeros(n)
    smoothed[lin], grid[lin] = sm, val
    ref, branches = SC.greedy_literal(lin, smoothed, grid, dims, mat, maxdist, atol, 0.0, maxbasins)
    for key, count in expect.items():
        assert branches[key] == count, (key, branches)
    _same(B.coalesce_ranked(lin, sm, val, dims, mat, maxdist, atol, maxbasins), ref)
    _same(B.coalesce_ranked_host(lin, sm, val, dims, mat, maxdist, atol, maxbasins), ref)


def test_greedy_pass_submid_never_exceeds_one():
    """:696-697 sort the in-distance list by INCREASING distance and then look for the first entry below ``maxdist/2``: if any entry
    is, the first is.  So ``submid`` is 1 on every input and the deletion of several merged basins (:712-716 with more than one
    index) cannot be reached as the reference is written; the library carries the general code all the same."""
    r = np.random.default_rng(99)
    dims, mat = SC.GREEDY_DIMS, SC.SKEW_MAT
    n = dims[0] * dims[1] * dims[2]
    grid = np.where(r.random(n) < 0.5, r.integers(0, 9, size=n) / 64.0, 0.0)
    smoothed = grid + r.integers(0, 3, size=n) / 128.0
    order, _ = SC.ranked_reference(smoothed.reshape(dims, order="F"), 0.0)
    ref, branches = SC.greedy_literal(order, smoothed, grid, dims, mat, 3.0, 0.05, 0.0)
    assert branches["maxsubmid"] == 1 and branches["merge"] == 0
    assert branches["absorb"] > 100 and branches["low_val_many"] > 10 and branches["new"] > 3
    _same(B.coalesce_ranked(order, smoothed[order], grid[order], dims, mat, 3.0, 0.05), ref)
    _same(B.coalesce_ranked_host(order, smoothed[order], grid[order], dims, mat, 3.0, 0.05), ref)


def test_greedy_pass_refusals_and_capacity():
    import ctypes as C
    lib = _abi.load_library()
    name, lin, sm, val, dims, mat, maxdist, atol, maxbasins, _ = SC.greedy_cases()[0]
    lin32, sm, val = np.asarray(lin, dtype=np.int32), np.asarray(sm), np.asarray(val)
    m = np.ascontiguousarray(np.asarray(mat).T).ravel()
    d32 = np.asarray(dims, dtype=np.int32)
    out_v, out_c, count = np.full(2, -7.0), np.full((2, 3), -7.0), C.c_int64(-1)

    def call(lin_arr, cap, md=maxdist):
        return lib.ceg_coalesce_ranked(_abi.i32ptr(lin_arr), _abi.dptr(sm), _abi.dptr(val), len(lin_arr), _abi.i32ptr(d32), _abi.dptr(m), 1, 1.0,
                                       md, atol, math.inf, _abi.dptr(out_v), _abi.dptr(out_c.ravel()), cap, C.byref(count))

    assert call(lin32, 1) == 0 and count.value == 3                               # the full count, one entry written
    assert out_v[0] == 0.5 and out_v[1] == -7.0 and np.all(out_c[1] == -7.0)
    bad = lin32.copy()
    bad[1] = dims[0] * dims[1] * dims[2]
    assert call(bad, 2) == -1 and b"outside the grid" in lib.ceg_last_error()
    assert call(lin32, 2, math.nan) == -1


def test_greedy_pass_under_the_sanitizers(tmp_path):
    """``csrc/ceg_coalesce.h`` with the stand-alone ``tests/native/coalesce_sanitize.cpp`` under -fsanitize=address,undefined"""
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "coalesce_sanitize"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-I", str(ROOT / "crystalenergygrids.jl_amd" / "csrc"), str(ROOT / "tests" / "native" / "coalesce_sanitize.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "coalesce ok" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- cluster_closer_than
def test_cluster_closer_than():
    for mat in (SC.ORTHO_MAT, SC.cit7_mat()):
        ret = [(0.3, [0.1, 0.1, 0.1]), (0.2, [0.98, 0.1, 0.12]), (0.6, [0.5, 0.5, 0.5]), (0.5, [0.52, 0.5, 0.5]), (0.1, [0.12, 0.08, 0.1]),
               (0.05, [0.5, 0.52, 0.48])]
        ref = SC.cluster_closer_than_literal(ret, mat, 2.0)
        assert len(ref) == 3                                                      # the pair that would exceed 1 is left apart
        _same(B.cluster_closer_than(ret, mat, 2.0), ref)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _ambiguous(values, dims, sites, mat):
    """the non-zero voxels whose two nearest sites differ in distance by at most 2*|mat*(1 ./ dims)|, at either origin"""
    diag = float(np.linalg.norm(np.asarray(mat) @ (1.0 / np.asarray(dims, dtype=np.float64))))
    nz = values.reshape(dims, order="F") != 0
    amb = None
    for origin in (0, 1):
        per_site = []
        for s in sites:
            _, _, _, d = B.site_nearest_host(np.asarray([s]), dims, mat, bins=nz.astype(np.int64), origin=origin)
            per_site.append(d)
        d = np.sort(np.asarray(per_site), axis=0)
        a = (d[1] - d[0] <= 2 * diag) if len(sites) > 1 else np.zeros(d.shape[1], dtype=bool)
        amb = a if amb is None else (amb | a)
    return np.flatnonzero(nz.ravel(order="F")), amb


@pytest.mark.parametrize("case", SC.e2e_cases(), ids=_ids(SC.e2e_cases()))
def test_closest_to_sites_host_against_the_reference_as_written(case):
    """per-site sums: ours equal the as-written ones once the voxels within the 2*diag ambiguity are set aside; the cap does not bind
    and the set-aside voxels are at most 5 % of the non-zero ones"""
    name, grid, counter, mat, maxdist, kw, nclouds = case
    values, dims = B._density_values(grid, counter)
    vgrid = values.reshape(dims, order="F")
    sites = np.asarray([p for _, p in B.coalescing_basins_host(grid, maxdist, mat, counter=counter, **kw)])
    assert len(sites) == nclouds
    Qs, weights, deleted, cap_bound = SC.closest_to_sites_literal(vgrid, sites, mat)
    assert not cap_bound and not deleted
    ours = B.closest_to_sites_host(grid, sites, mat, counter=counter)
    assert not ours.cap_bound and len(ours.deleted) == 0
    lin, amb = _ambiguous(values, dims, sites, mat)
    assert amb.sum() <= 0.05 * len(lin), f"{amb.sum()} of {len(lin)} voxels are ambiguous"
    clear = set(lin[~amb].tolist())
    a, b, c = dims
    ref_sums = []
    for Q, ws in zip(Qs, weights):                                                 # the reference's sums over the unambiguous voxels
        tot = 0.0
        for p, w in zip(Q, ws):
            x = (SC.mod1(int(p[0]), a) - 1) + a * ((SC.mod1(int(p[1]), b) - 1) + b * (SC.mod1(int(p[2]), c) - 1))
            if x in clear and w != 0:
                tot += w
        ref_sums.append(tot)
    _, site, _, _ = B.site_nearest_host(sites, dims, mat, bins=(vgrid != 0).astype(np.int64), origin=0)
    our_sums = np.zeros(len(sites))
    np.add.at(our_sums, site[~amb], values[lin[~amb]])                             # counts over a power of two: exact in any order
    assert our_sums.tolist() == ref_sums
    assert ours.sums.sum() == values.sum()                                        # every non-zero voxel went to a site


@pytest.mark.parametrize("case", SC.e2e_cases(), ids=_ids(SC.e2e_cases()))
def test_smoothed_values_are_separated(case):
    """what the GPU end-to-end test needs from its inputs: wherever two smoothed values above the crop differ, they differ by more than
    twice the smoothing bound, so round-off cannot reorder the ranking (below the crop the mirror images of a lone voxel do tie; they
    are not ranked); and no value is within the bound of atol or of the crop"""
    name, grid, counter, mat, maxdist, kw, nclouds = case
    if kw.get("smooth", None) == 0:
        return
    values, dims = B._density_values(grid, counter)
    taps = [B.gaussian_taps(s) for s in B.smoothing_sigmas(dims, mat)]
    ref = SC.smooth_longdouble(values.reshape(dims, order="F"), taps)
    bound = SC.smooth_bound(np.abs(ref), taps)
    crop = kw["atol"] * values.max() / 100
    flat, fb = ref.ravel(order="F"), bound.ravel(order="F")
    order = np.argsort(flat, kind="stable")
    gap = np.diff(flat[order])
    need = 2 * (fb[order][1:] + fb[order][:-1])
    ranked = flat[order][1:] > crop - 2 * fb[order][1:]                             # pairs whose upper value can be above the crop
    assert ranked.sum() > 1000 and np.all(gap[ranked] > need[ranked])
    for thr in (crop, kw["atol"]):
        assert np.all(np.abs(flat - thr) > 2 * fb)


@pytest.mark.parametrize("case", SC.e2e_cases(), ids=_ids(SC.e2e_cases()))
def test_coalescing_basins_host_pipeline(case):
    name, grid, counter, mat, maxdist, kw, nclouds = case
    ret = B.coalescing_basins_host(grid, maxdist, mat, counter=counter, **kw)
    values, dims = B._density_values(grid, counter)
    assert len(ret) == nclouds and sum(v for v, _ in ret) == values.sum()
    assert all(0.4 < v <= 1.0 for v, _ in ret)
    av = B.average_clusters_host(grid, maxdist, mat, counter=counter, **kw)
    assert [v for v, _ in av] == sorted((v for v, _ in ret), reverse=True)
    cut = B.average_clusters_host(grid, maxdist, mat, counter=counter, rtol=0.5, **kw)
    assert 1 <= len(cut) < len(av) and sum(v for v, _ in cut) >= 0.5 * values.sum() > sum(v for v, _ in cut[:-1])
    assert len(B.average_clusters_host(grid, maxdist, mat, counter=counter, rtol=0.999, ntol=2, **kw)) == 2      # :288: i + 1 > ntol


def test_coalescing_basins_literal_on_a_small_map():
    """the whole of ``coalescing_basins`` as written against the host composition on a map where the two must agree: sites far apart
    against the voxel size, so no voxel is ambiguous, and the cap never binds"""
    dims, mat = (16, 16, 16), np.diag([16.0, 16.0, 16.0])
    g = np.zeros(dims)
    for cen, vals in (((4, 4, 4), (24, 8, 8, 4)), ((12, 10, 4), (16, 8, 4, 4)), ((6, 12, 12), (20, 4, 4, 4))):
        g[cen] = vals[0]
        g[cen[0] + 1, cen[1], cen[2]] = vals[1]
        g[cen[0], cen[1] - 1, cen[2]] = vals[2]
        g[cen[0], cen[1], cen[2] + 1] = vals[3]
    g /= 64.0
    lit, cap_bound = SC.coalescing_basins_literal(g, 3.5, mat, atol=0.05)
    assert not cap_bound and len(lit) == 3
    got = B.coalescing_basins_host(g, 3.5, mat, atol=0.05)
    assert [v for v, _ in got] == [v for v, _ in lit]
    for (_, p), (_, q) in zip(got, lit):
        assert np.allclose(p, q, rtol=0, atol=4 * SC.U)


def test_integer_maps_of_any_width_are_bins():
    """a host array of int32 or uint16 counts is what the same counts are as int64; without a counter it is refused, not read as FP64"""
    name, bins, counter, mat, maxdist, kw, _ = SC.e2e_cases()[0]
    small = np.minimum(bins >> 8, 60000)                                           # fits uint16
    want = B.average_clusters_host(small, maxdist, mat, counter=counter >> 8, **kw)
    for dt in (np.int32, np.uint16):
        got = B.average_clusters_host(small.astype(dt), maxdist, mat, counter=counter >> 8, **kw)
        _same(got, want)
        assert np.array_equal(B.smooth_grid_host(small.astype(dt), [np.ones(1)] * 3, scale=0.5), small * 0.5)
        with pytest.raises(ValueError):
            B.closest_to_sites_host(small.astype(dt), np.array([[0.1, 0.2, 0.3]]), mat)
