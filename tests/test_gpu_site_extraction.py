"""From a density map to the sites on the device: ``ceg_grid_smooth`` against the longdouble form with the derived bound asserted per
element, ``ceg_grid_ranked`` and ``ceg_grid_site_nearest`` with ``==`` against the literal restatements of
``tests/site_extraction_cases.py``, and the device-backed ``coalescing_basins`` / ``average_clusters`` / ``closest_to_sites`` against
their ``*_host`` compositions, exactly.  Every case runs from host arrays through the bindings and from device arrays (torch tensors)
with device outputs through the C ABI.  The references are computed once per case (cached in the cases module); the conditions on the
inputs these tests rely on are asserted in ``tests/test_site_extraction_host.py``."""
import ctypes as C
import math

import numpy as np
import pytest

import site_extraction_cases as SC
from ceg_hip import _abi, basins as B

pytestmark = pytest.mark.gpu

NULL = C.c_void_p(0)
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def _ids(cases):
    return [c[0] for c in cases]


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(arr).ravel(order="F"))).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _dims(d):
    return _abi.i32ptr(np.asarray(d, dtype=np.int32))


def _same(got, ref):
    assert len(got) == len(ref)
    for (v, p), (rv, rp) in zip(got, ref):
        assert v == rv and np.array_equal(np.asarray(p), np.asarray(rp))


# ---------------------------------------------------------------------------------------------------------------- smoothing
def _smooth_device(hip_lib, g, scale, taps):
    """device input, device output, through the C ABI"""
    import torch
    dg = _dev(g)
    out = torch.full((g.size,), -7.0, dtype=torch.float64, device="cuda")
    t = [np.ascontiguousarray(x, dtype=np.float64) for x in taps]
    _abi.check(hip_lib, hip_lib.ceg_grid_smooth(0, _ptr(dg), int(g.dtype == np.int64), 1, scale, _dims(g.shape), _abi.dptr(t[0]), len(t[0]),
                                                _abi.dptr(t[1]), len(t[1]), _abi.dptr(t[2]), len(t[2]), _ptr(out), 1, NULL))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(g.shape, order="F")


@pytest.mark.parametrize("kind", ["f64", "i64"])
@pytest.mark.parametrize("case", SC.smooth_cases(), ids=_ids(SC.smooth_cases()))
def test_smooth_within_the_derived_bound(hip_lib, case, kind):
    name, shape, taps = case
    g = SC.smooth_input(shape, kind)
    scale = SC.INT_SCALE if kind == "i64" else 1.0
    x, ref, bound = SC.smooth_reference(name, kind)
    for got in (B.smooth_grid(g, taps, scale=scale), _smooth_device(hip_lib, g, scale, taps)):
        err = np.abs(got.astype(np.longdouble) - ref)
        print(f"{name}/{kind}: max err/bound {float((err / bound).max()):.3f}")
        assert got.shape == shape and np.all(err <= bound)
    if g.size <= 64:                                                               # the definition with an exact fma: the same bits
        assert np.array_equal(got, SC.smooth_exact_fma(x, taps))


def test_smooth_does_not_depend_on_the_tile(hip_lib):
    """a map shifted by whole voxels gives the shifted result, bit for bit: an element is one sequence of operations wherever it falls
    in a tile"""
    _, shape, taps = next(c for c in SC.smooth_cases() if c[0] == "70x66x65-9")
    g = SC.smooth_input(shape, "f64")
    base = B.smooth_grid(g, taps)
    shift = (37, 5, 11)
    assert np.array_equal(B.smooth_grid(np.roll(g, shift, axis=(0, 1, 2)), taps), np.roll(base, shift, axis=(0, 1, 2)))


@pytest.mark.parametrize("name", ["5x3x1-9", "70x66x65-9"])
def test_smooth_impulse_is_the_wrapped_outer_product(hip_lib, name):
    _, shape, taps = next(c for c in SC.smooth_cases() if c[0] == name)
    p0 = tuple(s // 2 for s in shape)
    g = np.zeros(shape)
    g[p0] = 1.0
    got = B.smooth_grid(g, taps)
    want = np.zeros(shape, dtype=np.longdouble)
    w = [len(t) // 2 for t in taps]
    prod = np.einsum("i,j,k->ijk", *[t.astype(np.longdouble) for t in taps])
    for t0 in range(len(taps[0])):
        for t1 in range(len(taps[1])):
            for t2 in range(len(taps[2])):                                          # y[p] takes taps[t + w] from x[p + t]: the impulse lands at p0 - t
                want[(p0[0] - t0 + w[0]) % shape[0], (p0[1] - t1 + w[1]) % shape[1], (p0[2] - t2 + w[2]) % shape[2]] += prod[t0, t1, t2]
    assert np.all(np.abs(got.astype(np.longdouble) - want) <= SC.smooth_bound(want, taps))
    if name == "70x66x65-9":                                                        # no wrap onto itself: three roundings, exactly
        far = np.roll(got, tuple(w[q] - p0[q] for q in range(3)), axis=(0, 1, 2))[:9, :9, :9]
        chain = (taps[0][::-1, None, None] * 1.0 * taps[1][None, ::-1, None]) * taps[2][None, None, ::-1]
        assert np.array_equal(far, chain) and np.count_nonzero(got) == 729


def test_smooth_constant(hip_lib):
    """a constant ``c`` under normalised taps comes back as ``c`` to within the bound ``gamma_n * S(|x|)`` with ``S(|x|) = c``"""
    _, shape, taps = next(c for c in SC.smooth_cases() if c[0] == "70x66x65-9")
    c = 0.7312
    got = B.smooth_grid(np.full(shape, c), taps)
    err = np.abs(got.astype(np.longdouble) - np.longdouble(c))
    bound = SC.smooth_bound(np.full(shape, c, dtype=np.longdouble), taps)
    print(f"constant: max |got - c| / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)


def test_smooth_refusals(hip_lib):
    g = np.ones((5, 3, 2))
    one, two, long_ = np.ones(1), np.ones(2) / 2, np.ones(131) / 131
    with pytest.raises(_abi.CegError) as err:
        B.smooth_grid(g, (one, two, one))
    assert err.value.code == ERR_INVALID
    with pytest.raises(_abi.CegError) as err:
        B.smooth_grid(g, (one, one, long_))
    assert err.value.code == ERR_UNSUPPORTED and "131" in str(err.value)
    big = np.ones((5, 3, 2), dtype=np.int64)
    big[4, 2, 1] = -2**53
    with pytest.raises(_abi.CegError) as err:
        B.smooth_grid(big, (one, one, one), scale=1.0)
    assert err.value.code == ERR_INVALID and "2^53" in str(err.value)
    big[4, 2, 1] = 2**53 - 1
    assert B.smooth_grid(big, (one, one, one), scale=1.0)[4, 2, 1] == float(2**53 - 1)
    dg = _dev(g)
    t = np.ones(1)
    assert hip_lib.ceg_grid_smooth(0, _ptr(dg), 0, 1, 1.0, _dims(g.shape), _abi.dptr(t), 1, _abi.dptr(t), 1, _abi.dptr(t), 1, _ptr(dg), 1,
                                   NULL) == ERR_INVALID                            # not in place


# ---------------------------------------------------------------------------------------------------------------- ranking
@pytest.mark.parametrize("case", SC.ranked_cases(), ids=_ids(SC.ranked_cases()))
def test_ranked(hip_lib, case):
    import torch
    name, g, crop, capacity = case
    idx, val = SC.ranked_reference(g, crop)
    got_idx, got_val = B.ranked_above(g, crop, capacity=7)                          # host arrays; the room grows on demand
    assert got_idx.tolist() == idx and got_val.tolist() == val
    cap = capacity if capacity is not None else len(idx) + 3
    dg = _dev(g)
    didx = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    dval = torch.full((cap + 1,), -7.0, dtype=torch.float64, device="cuda")
    count = C.c_int64(-1)
    _abi.check(hip_lib, hip_lib.ceg_grid_ranked(0, _ptr(dg), 1, _dims(g.shape), crop, _ptr(didx), _ptr(dval), 1, cap, C.byref(count), NULL))
    torch.cuda.synchronize()
    assert count.value == len(idx)
    n = min(cap, len(idx))
    assert didx[:n].cpu().tolist() == idx[:n] and dval[:n].cpu().tolist() == val[:n]
    assert (didx[n:] == -7).all() and (dval[n:] == -7.0).all()                      # nothing past min(count, capacity)
    # without the values
    _abi.check(hip_lib, hip_lib.ceg_grid_ranked(0, _ptr(dg), 1, _dims(g.shape), crop, _ptr(didx), NULL, 1, cap, C.byref(count), NULL))
    torch.cuda.synchronize()
    assert didx[:n].cpu().tolist() == idx[:n]


def test_ranked_refusals(hip_lib):
    g = np.ones((3, 2, 2))
    for crop in (-1.0, -0.0 - 1e-300, math.nan):
        with pytest.raises(_abi.CegError) as err:
            B.ranked_above(g, crop)
        assert err.value.code == ERR_INVALID
    assert len(B.ranked_above(g, -0.0)[0]) == 12                                   # -0.0 >= 0


# ---------------------------------------------------------------------------------------------------------------- nearest site
@pytest.mark.parametrize("origin", [1, 0])
@pytest.mark.parametrize("case", SC.nearest_cases(), ids=_ids(SC.nearest_cases()))
def test_site_nearest(hip_lib, case, origin):
    import torch
    name, sites, dims, mat, active, capacity = case
    lin, site, ofs, dist, _, _ = SC.nearest_reference(name, origin)
    bins = None if active is None else np.where(active, np.int64(-3), np.int64(0))
    got = B.site_nearest(sites, dims, mat, bins=bins, origin=origin, capacity=5)   # host arrays; the room grows on demand
    assert np.array_equal(got[0], lin) and np.array_equal(got[1], site) and np.array_equal(got[2], ofs)
    assert np.array_equal(got[3], dist)                                            # to the bit: contraction is off on both sides
    # device bins, device outputs, a capacity that may be short
    cap = capacity if capacity is not None else len(lin) + 2
    m, ortho, safemin = SC.periodic_setup(mat)
    mcol = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).T).ravel()
    s = np.ascontiguousarray(sites, dtype=np.float64)
    dbins = _dev(bins) if bins is not None else None
    dlin = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    dsite = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    dofs = torch.full((cap + 1, 3), -7, dtype=torch.int8, device="cuda")
    ddist = torch.full((cap + 1,), -7.0, dtype=torch.float64, device="cuda")
    count = C.c_int64(-1)
    _abi.check(hip_lib, hip_lib.ceg_grid_site_nearest(0, _dims(dims), _abi.dptr(mcol), int(ortho), safemin, _abi.dptr(s.ravel()), len(s), origin,
                                                      _ptr(dbins), 1, _ptr(dlin), _ptr(dsite), _ptr(dofs), _ptr(ddist), 1, cap, C.byref(count),
                                                      NULL))
    torch.cuda.synchronize()
    assert count.value == len(lin)
    n = min(cap, len(lin))
    assert np.array_equal(dlin[:n].cpu().numpy(), lin[:n]) and np.array_equal(dsite[:n].cpu().numpy(), site[:n])
    assert np.array_equal(dofs[:n].cpu().numpy(), ofs[:n]) and np.array_equal(ddist[:n].cpu().numpy(), dist[:n])
    assert (dlin[n:] == -7).all() and (dsite[n:] == -7).all() and (dofs[n:] == -7).all() and (ddist[n:] == -7.0).all()


def test_site_nearest_refusals(hip_lib):
    dims, mat = (3, 2, 5), SC.ORTHO_MAT
    ok = np.array([[0.1, 0.2, 0.3]])
    with pytest.raises(_abi.CegError) as err:
        B.site_nearest(ok, dims, mat, origin=2)
    assert err.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        B.site_nearest(np.array([[0.1, 64.5, 0.3]]), dims, mat)
    with pytest.raises(ValueError):
        B.site_nearest(np.zeros((0, 3)), dims, mat)
    with pytest.raises(_abi.CegError) as err:
        B.site_nearest(np.random.default_rng(0).random((_abi.SITE_PROXIMITY_MAX_SITES + 1, 3)), dims, mat)
    assert err.value.code == ERR_UNSUPPORTED
    # the library's own checks, past the bindings'
    m = np.ascontiguousarray(mat.T).ravel()
    out = np.zeros(64, dtype=np.int32)
    o8 = np.zeros((64, 3), dtype=np.int8)
    count = C.c_int64(0)
    for sites, ns in ((np.array([0.1, math.nan, 0.3]), 1), (np.array([0.1, -64.5, 0.3]), 1), (np.array([0.1, 0.2, 0.3]), 0)):
        rc = hip_lib.ceg_grid_site_nearest(0, _dims(dims), _abi.dptr(m), 1, 5.0, _abi.dptr(sites), ns, 0, NULL, 0, C.c_void_p(out.ctypes.data),
                                           C.c_void_p(out.ctypes.data), C.c_void_p(o8.ctypes.data), NULL, 0, 30, C.byref(count), NULL)
        assert rc == ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", SC.e2e_cases(), ids=_ids(SC.e2e_cases()))
def test_pipeline_equals_its_host_composition(hip_lib, case):
    name, grid, counter, mat, maxdist, kw, nclouds = case
    want = B.coalescing_basins_host(grid, maxdist, mat, counter=counter, **kw)
    assert len(want) == nclouds
    _same(B.coalescing_basins(grid, maxdist, mat, counter=counter, **kw), want)
    sites = np.asarray([p for _, p in want])
    hc, dc = B.closest_to_sites_host(grid, sites, mat, counter=counter), B.closest_to_sites(grid, sites, mat, counter=counter)
    assert np.array_equal(dc.sums, hc.sums) and np.array_equal(dc.centres, hc.centres) and dc.cap_bound == hc.cap_bound
    for extra in (dict(), dict(rtol=0.5), dict(rtol=0.999, ntol=2)):
        _same(B.average_clusters(grid, maxdist, mat, counter=counter, **kw, **extra),
              B.average_clusters_host(grid, maxdist, mat, counter=counter, **kw, **extra))
    # the map resident in device memory, as the MC sampler leaves it
    dg = _dev(grid)
    dev_grid = (dg.data_ptr(), grid.shape, grid.dtype)
    _same(B.average_clusters(dev_grid, maxdist, mat, counter=counter, **kw), B.average_clusters_host(grid, maxdist, mat, counter=counter, **kw))


def test_closest_to_sites_cap_and_deleted_sites(hip_lib):
    """two sites in one voxel (the second is deleted) and a cloud heavier than 1: the cap binds, on both routes alike"""
    name, grid, counter, mat, maxdist, kw, _ = SC.e2e_cases()[0]
    sites = np.array([[0.02, 0.2, 0.2], [0.0201, 0.2, 0.2], [0.52, 0.7, 0.2]])
    heavy = grid * 2
    hc, dc = B.closest_to_sites_host(heavy, sites, mat, counter=counter), B.closest_to_sites(heavy, sites, mat, counter=counter)
    assert hc.cap_bound and dc.cap_bound and hc.deleted.tolist() == [1] and dc.deleted.tolist() == [1]
    assert np.array_equal(dc.sums, hc.sums) and np.array_equal(dc.centres, hc.centres) and np.all(hc.sums <= 1)
