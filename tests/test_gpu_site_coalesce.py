"""The sequential part of the site extraction on the device: ``ceg_grid_coalesce`` against the literal loop (small cases) and the library's
host pass (large ones), ``ceg_grid_site_partition`` against the NumPy ``site_nearest_host`` plus ``_accumulate_closest``, and the pipeline
through them against its ``*_host`` composition -- all with ``==`` on the bits.  Every greedy case runs from host arrays and from device
arrays with device outputs, at the default cut into launches and at 1, T + 1 and 100 voxels per launch, the large ones included.  The conditions on the inputs
these tests rely on are asserted in ``tests/test_site_coalesce_host.py``."""
import ctypes as C
import math

import numpy as np
import pytest

import site_coalesce_cases as CC
import site_extraction_cases as SC
from ceg_hip import _abi, basins as B

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
SMALL = [c for c, _ in CC.small_cases()]


def _ids(cases):
    return [c[0] for c in cases]


def _bits(ret):
    return [np.asarray([v, *p], dtype=np.float64).view(np.int64).tolist() for v, p in ret]


def _same(got, ref):
    assert len(got) == len(ref) and _bits(got) == _bits(ref)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(arr).ravel(order="F"))).cuda()


def _from_host(case, cut):
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    return B.grid_coalesce(lin, sm, grid, mat, maxdist, atol, maxbasins, counter=counter, voxels_per_launch=cut)


def _from_device(case, cut, capacity=None, nref=0):
    """device ranking, device map, device outputs with `capacity` entries (default: two more than needed) -> (count, basins read back);
    nothing is written past min(count, capacity)"""
    import torch
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    cap = nref + 2 if capacity is None else capacity
    dlin, dsm, dmap = _dev(lin), _dev(sm), _dev(grid)
    dval = torch.full((cap + 1,), -7.0, dtype=torch.float64, device="cuda")
    dcen = torch.full((cap + 1, 3), -7.0, dtype=torch.float64, device="cuda")
    count = B.grid_coalesce(dlin.data_ptr(), dsm.data_ptr(), (dmap.data_ptr(), dims, grid.dtype), mat, maxdist, atol, maxbasins, counter=counter,
                            nranked=len(lin), voxels_per_launch=cut, out_ptrs=(dval.data_ptr(), dcen.data_ptr()), capacity=cap)
    torch.cuda.synchronize()
    n = min(count, cap)
    assert (dval[n:] == -7.0).all() and (dcen[n:] == -7.0).all()
    val, cen = dval[:n].cpu().numpy(), dcen[:n].cpu().numpy()
    return count, [(float(val[q]), cen[q]) for q in range(n)]


def _check_all_routes(case, ref):
    for cut in CC.CUTS:
        _same(_from_host(case, cut), ref)
        count, got = _from_device(case, cut, nref=len(ref))
        assert count == len(ref)
        _same(got, ref)


# ---------------------------------------------------------------------------------------------------------------- greedy pass
@pytest.mark.parametrize("case", SMALL + CC.length_cases(), ids=_ids(SMALL + CC.length_cases()))
def test_greedy_small_cases_against_the_literal_loop(hip_lib, case):
    ref, _ = CC.expected_small(case[0])
    _check_all_routes(case, ref)


@pytest.mark.parametrize("nf", CC.FOUNDER_COUNTS)
def test_greedy_basin_counts_across_the_lane_and_workgroup_edges(hip_lib, nf):
    case = CC.founder_case(nf)
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    ref = B.coalesce_ranked(lin, sm, CC.values_of(grid, counter)[lin], dims, mat, maxdist, atol, maxbasins)
    assert len(ref) == nf
    _check_all_routes(case, ref)


def test_greedy_capacity_below_the_count(hip_lib):
    case = CC.founder_case(CC.T + 1)
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    ref = B.coalesce_ranked(lin, sm, CC.values_of(grid, counter)[lin], dims, mat, maxdist, atol, maxbasins)
    for cut in CC.CUTS:
        for cap in (0, 1, CC.T):
            count, got = _from_device(case, cut, capacity=cap)
            assert count == len(ref)
            _same(got, ref[:cap])
            _same(B.grid_coalesce(lin, sm, grid, mat, maxdist, atol, maxbasins, voxels_per_launch=cut, capacity=cap), ref[:cap])


@pytest.mark.parametrize("kind", ["bins", "f64"])
def test_greedy_random_map_ranked_on_the_device(hip_lib, kind):
    """(40, 36, 44) skew map, smoothed and ranked on the device with atol 0, the ranking left in device memory"""
    import torch
    bins, counter, dims, mat, maxdist = CC.random_map()
    grid, counter = (bins, counter) if kind == "bins" else (CC.values_of(bins, counter).reshape(dims, order="F"), None)
    values = CC.values_of(grid, counter)
    taps = [B.gaussian_taps(s) for s in B.smoothing_sigmas(dims, mat)]
    n = values.size
    dmap = _dev(grid)
    dsm = torch.empty(n, dtype=torch.float64, device="cuda")
    didx = torch.empty(n, dtype=torch.int32, device="cuda")
    dval = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dgrid = (dmap.data_ptr(), dims, grid.dtype)
    B.smooth_grid(dgrid, taps, scale=(1.0 / counter) if counter else 1.0, out_ptr=dsm.data_ptr())
    count = C.c_int64(0)
    _abi.check(hip_lib, hip_lib.ceg_grid_ranked(0, C.c_void_p(dsm.data_ptr()), 1, _abi.i32ptr(np.asarray(dims, dtype=np.int32)), 0.0,
                                                C.c_void_p(didx.data_ptr()), C.c_void_p(dval.data_ptr()), 1, n, C.byref(count), C.c_void_p(0)))
    nr = int(count.value)
    lin, smv = didx[:nr].cpu().numpy(), dval[:nr].cpu().numpy()
    ref = B.coalesce_ranked(lin, smv, values[lin], dims, mat, maxdist, 0.0)
    assert nr > 20 * CC.T and len(ref) >= 30
    for cut in CC.CUTS:                                                             # the ranking where ceg_grid_ranked left it
        _same(B.grid_coalesce(didx.data_ptr(), dval.data_ptr(), dgrid, mat, maxdist, 0.0, counter=counter, nranked=nr, voxels_per_launch=cut), ref)
    _check_all_routes((f"random-{kind}", lin, smv, grid, counter, dims, mat, maxdist, 0.0, math.inf), ref)


def test_greedy_refusals(hip_lib):
    case = next(c for c in SMALL if c[0] == "extraction-ortho-absorb")
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    n = grid.size
    for bad_index, at in ((n, 2), (-1, 0), (2**31 - 1, 3)):
        broken = lin.copy()
        broken[at] = bad_index
        for cut in (0, 1):
            with pytest.raises(_abi.CegError) as err:
                B.grid_coalesce(broken, sm, grid, mat, maxdist, atol, voxels_per_launch=cut)
            assert err.value.code == ERR_INVALID and "outside the grid" in str(err.value)
    for kw in (dict(maxdist=math.nan), dict(atol=math.nan), dict(maxbasins=math.nan)):
        args = dict(maxdist=maxdist, atol=atol, maxbasins=maxbasins)
        args.update(kw)
        with pytest.raises(_abi.CegError) as err:
            B.grid_coalesce(lin, sm, grid, mat, **args)
        assert err.value.code == ERR_INVALID
    m = np.ascontiguousarray(SC.ORTHO_MAT.T).ravel()
    m[4] = math.nan
    val, cen, count = np.zeros(8), np.zeros(24), C.c_int64(0)
    rc = hip_lib.ceg_grid_coalesce(0, C.c_void_p(lin.ctypes.data), C.c_void_p(sm.ctypes.data), 0, len(lin), C.c_void_p(grid.ctypes.data), 0, 0, 1.0,
                                   _abi.i32ptr(np.asarray(dims, dtype=np.int32)), _abi.dptr(m), 1, 5.0, maxdist, atol, math.inf, 0,
                                   C.c_void_p(val.ctypes.data), C.c_void_p(cen.ctypes.data), 0, 8, C.byref(count), C.c_void_p(0))
    assert rc == ERR_INVALID
    # a bin at 2^53 is refused at the voxel the loop reaches; one below it is taken
    bins = np.zeros(dims, dtype=np.int64)
    for x in lin.tolist():
        bins[x % dims[0], (x // dims[0]) % dims[1], x // (dims[0] * dims[1])] = 5
    x = int(lin[2])
    at = (x % dims[0], (x // dims[0]) % dims[1], x // (dims[0] * dims[1]))
    bins[at] = 2**53
    with pytest.raises(_abi.CegError) as err:
        B.grid_coalesce(lin, sm, bins, mat, maxdist, atol, counter=1.0)
    assert err.value.code == ERR_INVALID and "2^53" in str(err.value)
    bins[at] = 2**53 - 1
    got = B.grid_coalesce(lin, sm, bins, mat, maxdist, atol, counter=1.0)
    _same(got, B.coalesce_ranked(lin, sm, bins.ravel(order="F").astype(np.float64)[lin], dims, mat, maxdist, atol))


# ---------------------------------------------------------------------------------------------------------------- partition
_PART_REF = {}


def _partition_reference(name, origin):
    if (name, origin) not in _PART_REF:
        _, grid, counter, dims, mat, sites = next(c for c in CC.partition_cases() if c[0] == name)
        values = CC.values_of(grid, counter)
        lin, site, off, _ = B.site_nearest_host(sites, dims, mat, bins=(values != 0).reshape(dims, order="F"), origin=origin, want_dist=False)
        _PART_REF[(name, origin)] = (B._accumulate_closest(values, dims, len(sites), lin, site, off, []), len(lin))
    return _PART_REF[(name, origin)]


@pytest.mark.parametrize("origin", [0, 1])
@pytest.mark.parametrize("case", CC.partition_cases(), ids=_ids(CC.partition_cases()))
def test_site_partition(hip_lib, case, origin):
    import torch
    name, grid, counter, dims, mat, sites = case
    ref, nactive = _partition_reference(name, origin)
    got = B.site_partition(grid, sites, mat, counter=counter, origin=origin)
    ns = len(sites)
    dmap = _dev(grid)
    dsum = torch.full((ns + 1,), -7.0, dtype=torch.float64, device="cuda")
    dcen = torch.full((ns + 1, 3), -7.0, dtype=torch.float64, device="cuda")
    dgot = B.site_partition((dmap.data_ptr(), dims, grid.dtype), sites, mat, counter=counter, origin=origin,
                            out_ptrs=(dsum.data_ptr(), dcen.data_ptr()))
    torch.cuda.synchronize()
    assert dsum[ns] == -7.0 and (dcen[ns] == -7.0).all()
    for sums, cen, cap, count in (got, (dsum[:ns].cpu().numpy(), dcen[:ns].cpu().numpy(), dgot.cap_bound, dgot.count)):
        assert count == nactive and cap == ref.cap_bound
        assert np.array_equal(sums.view(np.int64), ref.sums.view(np.int64))
        real = ~np.isnan(ref.centres)                                               # an empty site is NaN on both sides, whatever its payload
        assert np.array_equal(np.isnan(cen), ~real) and np.array_equal(cen[real].view(np.int64), ref.centres[real].view(np.int64))


def test_site_partition_refusals_and_deleted_sites(hip_lib):
    name, grid, counter, dims, mat, sites = next(c for c in CC.partition_cases() if c[0] == "ortho-cap")
    with pytest.raises(_abi.CegError) as err:
        B.site_partition(grid, sites, mat, origin=2)
    assert err.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        B.site_partition(grid, np.zeros((0, 3)), mat)
    with pytest.raises(ValueError):
        B.site_partition(grid, np.array([[0.1, 64.5, 0.3]]), mat)
    big = np.zeros(dims, dtype=np.int64)
    big[1, 2, 3] = 2**53
    with pytest.raises(_abi.CegError) as err:
        B.site_partition(big, sites, mat, counter=2.0**60)
    assert err.value.code == ERR_INVALID and "2^53" in str(err.value)
    # site_nearest keeps its limit; closest_to_sites no longer has one, and deletes the sites that snap to an earlier one's voxel
    many = np.random.default_rng(0).random((_abi.SITE_PROXIMITY_MAX_SITES + 1, 3))
    with pytest.raises(_abi.CegError) as err:
        B.site_nearest(many, dims, mat)
    assert err.value.code == ERR_UNSUPPORTED
    twins = np.concatenate([sites, sites[:1] + np.array([1e-4, 0.0, 1e-4]), many])              # 4.8012 and 5.6014 round as 4.8 and 5.6
    hc, dc = B.closest_to_sites_host(grid, twins, mat), B.closest_to_sites(grid, twins, mat)
    assert 2 in dc.deleted.tolist() and np.array_equal(dc.deleted, hc.deleted) and dc.cap_bound == hc.cap_bound
    assert np.array_equal(dc.sums, hc.sums) and np.array_equal(dc.centres, hc.centres, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", SC.e2e_cases(), ids=_ids(SC.e2e_cases()))
def test_pipeline_through_the_device_stages(hip_lib, case):
    name, grid, counter, mat, maxdist, kw, nclouds = case
    want = B.coalescing_basins_host(grid, maxdist, mat, counter=counter, **kw)
    assert len(want) == nclouds
    _same(B.coalescing_basins(grid, maxdist, mat, counter=counter, **kw), want)
    dg = _dev(grid)
    _same(B.coalescing_basins((dg.data_ptr(), grid.shape, grid.dtype), maxdist, mat, counter=counter, **kw), want)
    _same(B.cluster_closer_than(want + want, mat, maxdist), B.cluster_closer_than_host(want + want, mat, maxdist))


def test_more_basins_than_the_site_limit_stage_by_stage(hip_lib):
    """atol = 0 leaves 2197 basins, more than ``site_nearest`` takes: the call used to end in CEG_ERR_UNSUPPORTED.  Each device stage
    against its library or host form on the same input, then the whole call against the composition of those forms."""
    bins, counter, dims, mat, maxdist, kw = CC.many_basins_case()
    values = CC.values_of(bins, counter)
    lin, smv = B.ranked_above_host(values.reshape(dims, order="F"), 0.0)
    dlin, dsm = B.ranked_above(values.reshape(dims, order="F"), 0.0)
    assert np.array_equal(dlin, lin) and np.array_equal(dsm, smv)
    ret = B.coalesce_ranked(lin, smv, values[lin], dims, mat, maxdist, kw["atol"])
    assert len(ret) > _abi.SITE_PROXIMITY_MAX_SITES
    _same(B.grid_coalesce(lin, smv, bins, mat, maxdist, kw["atol"], counter=counter), ret)
    rounds = 0
    n1 = -1
    while len(ret) != n1:
        n1 = len(ret)
        pts = np.asarray([p for _, p in ret])
        kept, deleted = B.snap_sites(pts, dims)
        l, s, o, _ = B.site_nearest_host(kept, dims, mat, bins=bins != 0, origin=0, want_dist=False)
        hc = B._accumulate_closest(values, dims, len(kept), l, s, o, deleted)
        dc = B.closest_to_sites(bins, pts, mat, counter=counter)
        assert np.array_equal(dc.sums, hc.sums) and np.array_equal(dc.centres, hc.centres) and dc.cap_bound == hc.cap_bound
        assert np.array_equal(dc.deleted, hc.deleted) and np.all(hc.sums > 0)
        ret = B.cluster_closer_than(B.updated_sites_with_closest(hc), mat, maxdist)
        ret = [e for e in ret if e[0] >= kw["atol"]]
        rounds += 1
    assert rounds >= 1 and len(ret) > _abi.SITE_PROXIMITY_MAX_SITES
    _same(B.coalescing_basins(bins, maxdist, mat, counter=counter, **kw), ret)
    got = B.average_clusters(bins, maxdist, mat, counter=counter, smooth=0)         # atol = 0 is the default
    _same(got, sorted(ret, key=lambda e: (e[0], *e[1]), reverse=True))
