"""basins.jl on the device: ``ceg_grid_local_minima`` / ``ceg_grid_components`` / ``ceg_grid_site_proximity`` / ``ceg_grid_site_density``
against the literal, queue-based restatements of ``tests/basins_cases.py``.  Every integer is compared with ``==``; every case runs once
from host arrays through the bindings of ``ceg_hip/basins.py`` and once from device arrays (torch tensors) with device outputs through
the C ABI.  The references are computed once per case (cached in ``basins_cases``).

The last test is the reference's own end-to-end pin (``test/runtests.jl:35-36,48-49``): Ar and Na in CHA as in
``test_gpu_parity.py::test_reference_energy_grid_flow``, with the device ``local_minima`` on the energy grids."""
import ctypes as C
import math
import os
from pathlib import Path

import numpy as np
import pytest

import basins_cases as BC
from ceg_hip import _abi, basins as B

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c[0] for c in cases]


def _dev(arr):
    """a NumPy array -> a device tensor holding it flat in Julia's memory order"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(arr).ravel(order="F"))).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _dims(d):
    return _abi.i32ptr(np.asarray(d, dtype=np.int32))


NULL = C.c_void_p(0)


# ---------------------------------------------------------------------------------------------------------------- minima
@pytest.mark.parametrize("case", BC.minima_cases(), ids=_ids(BC.minima_cases()))
def test_local_minima(hip_lib, case):
    import torch
    name, g, tol, maxima = case
    ref, ext = BC.minima_reference(name)
    want_ext = math.inf if ext is None else ext
    got, gext = B.local_minima(g, tol, maxima=maxima, return_extremum=True, capacity=2)      # host array; the room grows on demand
    assert [tuple(r) for r in got.tolist()] == ref and gext == want_ext
    # device grid, device list, room for half of the minima: the full count and the head of the list
    cap = max(len(ref) // 2, 1)
    dg, dijk = _dev(g), torch.full((cap + 1, 3), -7, dtype=torch.int32, device="cuda")
    count, e = C.c_int64(-1), C.c_double(0.0)
    _abi.check(hip_lib, hip_lib.ceg_grid_local_minima(0, _ptr(dg), 1, _dims(g.shape), int(maxima), tol, _ptr(dijk), 1, cap, C.byref(count),
                                                      C.byref(e), NULL))
    torch.cuda.synchronize()
    assert count.value == len(ref) and e.value == want_ext
    n = min(cap, len(ref))
    assert [tuple(r) for r in dijk[:n].cpu().tolist()] == ref[:n]
    assert (dijk[n:] == -7).all()                                                  # nothing past min(count, capacity)


@pytest.mark.parametrize("case", BC.minima_refusal_cases(), ids=_ids(BC.minima_refusal_cases()))
def test_local_minima_refuses_a_non_negative_extremum(hip_lib, case):
    _, g, tol = case
    with pytest.raises(_abi.CegError) as err:
        B.local_minima(g, tol)
    assert err.value.code == -1 and "basins.jl:91" in str(err.value)
    assert len(B.local_minima(g, -1.0)) >= 1


def test_local_minima_on_a_stream_and_of_a_view(hip_lib):
    import torch
    name, g, tol, maxima = next(c for c in BC.minima_cases() if c[0] == "wrap-17x9x33-tol0.01")
    ref, _ = BC.minima_reference(name)
    st = torch.cuda.Stream()
    got = B.local_minima(np.ascontiguousarray(g), tol, stream=st.cuda_stream)      # C-ordered input: the binding reorders it
    assert [tuple(r) for r in got.tolist()] == ref
    dg = _dev(g)
    got = B.local_minima((dg.data_ptr(), g.shape), tol, stream=st.cuda_stream)
    assert [tuple(r) for r in got.tolist()] == ref


# ---------------------------------------------------------------------------------------------------------------- components
def _check_components_device(hip_lib, g, mode, lo, hi, ref):
    import torch
    labels, seeds, sizes = ref[0], ref[1], ref[2]
    sums = ref[3] if len(ref) > 3 and g.dtype == np.int64 else None
    n = g.size
    cap = max(len(seeds) // 2, 1)
    dg = _dev(g)
    dlab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dseed = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    dsize = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda")
    dsum = torch.full((cap + 1,), -7, dtype=torch.int64, device="cuda") if sums is not None else None
    count = C.c_int64(-1)
    _abi.check(hip_lib, hip_lib.ceg_grid_components(0, _ptr(dg), int(g.dtype == np.int64), 1, _dims(g.shape), mode, lo, hi, _ptr(dlab), 1,
                                                    _ptr(dseed), _ptr(dsize), _ptr(dsum), 1, cap, C.byref(count), NULL))
    torch.cuda.synchronize()
    assert count.value == len(seeds)
    assert np.array_equal(dlab.cpu().numpy().reshape(g.shape, order="F"), labels)
    k = min(cap, len(seeds))
    assert dseed[:k].cpu().tolist() == seeds[:k] and dsize[:k].cpu().tolist() == sizes[:k]
    assert (dseed[k:] == -7).all() and (dsize[k:] == -7).all()
    if sums is not None:
        assert dsum[:k].cpu().tolist() == sums[:k] and (dsum[k:] == -7).all()


@pytest.mark.parametrize("case", BC.component_cases(), ids=_ids(BC.component_cases()))
def test_components(hip_lib, case):
    name, g = case
    ref = BC.components_reference(name)
    comp = B.grid_components(g, capacity=3)
    assert np.array_equal(comp.labels, ref[0])
    assert comp.seed.tolist() == ref[1] and comp.size.tolist() == ref[2]
    if g.dtype == np.int64:
        assert comp.sum.tolist() == ref[3]
    else:
        assert comp.sum.size == 0
    _check_components_device(hip_lib, g, _abi.COMPONENTS_NONZERO, 0.0, 0.0, ref)


@pytest.mark.parametrize("case", BC.band_cases(), ids=_ids(BC.band_cases()))
def test_compute_levels(hip_lib, case):
    name, g, lo, hi = case
    ref = BC.components_reference(name)
    comp = B.compute_levels(g, lo, hi)
    assert np.array_equal(comp.labels, ref[0]) and comp.seed.tolist() == ref[1] and comp.size.tolist() == ref[2]
    _check_components_device(hip_lib, g, _abi.COMPONENTS_BAND, lo, hi, ref)


@pytest.mark.parametrize("kw", [dict(), dict(ntol=3), dict(atol=5.0, rtol=0.9, ntol=40)])
def test_local_components_cut_and_order(hip_lib, kw):
    for name in ("i64-sparse-17x9x33", "checkerboard-8x8x8"):
        g = dict(BC.component_cases())[name]
        _, seeds, sizes, sums = BC.components_reference(name)
        keep = BC.cut_components_literal(sums, int(g.sum()), **kw)
        dg = _dev(g)
        for arg in (g, (dg.data_ptr(), g.shape, np.int64)):
            comp = B.local_components(arg, **kw)
            assert comp.label.tolist() == keep and comp.sum.tolist() == [sums[n] for n in keep]
            assert comp.seed.tolist() == [seeds[n] for n in keep] and comp.size.tolist() == [sizes[n] for n in keep]
    f = dict(BC.component_cases())["f64-nan-5x7x3"]
    comp = B.local_components(np.nan_to_num(f, nan=0.25))
    host = B.local_components_host(np.nan_to_num(f, nan=0.25))
    assert comp.label.tolist() == host.label.tolist() and np.array_equal(comp.sum, host.sum)


def test_components_counts_only(hip_lib):
    g = dict(BC.component_cases())["checkerboard-8x8x8"]
    count = C.c_int64(-1)
    gf = np.asfortranarray(g)
    _abi.check(hip_lib, hip_lib.ceg_grid_components(0, C.c_void_p(gf.ctypes.data), 1, 0, _dims(g.shape), 0, 0.0, 0.0, NULL, 0, NULL, NULL, NULL,
                                                    0, 0, C.byref(count), NULL))
    assert count.value == 256


# ---------------------------------------------------------------------------------------------------------------- sites
@pytest.mark.parametrize("case", BC.proximity_cases(), ids=_ids(BC.proximity_cases()))
def test_site_proximity(hip_lib, case):
    import torch
    name, sites, dims, mat, maxdist = case
    site, off, deleted = BC.proximity_reference(name)
    gs, go, gd = B.site_proximity_map(sites, dims, mat, maxdist)
    assert gd.tolist() == deleted
    assert np.array_equal(gs, site) and np.array_equal(go, off)
    n = int(np.prod(dims))
    ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    do = torch.full((n, 3), -7, dtype=torch.int8, device="cuda")
    _, _, gd = B.site_proximity_map(sites, dims, mat, maxdist, out_ptrs=(ds.data_ptr(), do.data_ptr()))
    assert gd.tolist() == deleted
    assert np.array_equal(ds.cpu().numpy().reshape(dims, order="F"), site)
    assert np.array_equal(np.moveaxis(do.cpu().numpy().T.reshape((3,) + tuple(dims), order="F"), 0, -1), off)


def test_site_proximity_refuses_a_ball_that_meets_its_image(hip_lib):
    with pytest.raises(_abi.CegError) as err:
        B.site_proximity_map(np.array([[0.5, 0.5, 0.5]]), BC.SKEW["dims"], BC.SKEW["mat"], 4.5)
    assert err.value.code == -1 and "smallest width" in str(err.value)


@pytest.mark.parametrize("case", BC.density_cases(), ids=_ids(BC.density_cases()))
def test_site_density(hip_lib, case):
    import torch
    name, bins, site, off, ns, centres = case
    want_rho, want_mom = B.site_density_host(bins, site, off, ns)                  # equal to the literal sums: tests/test_basins_host.py
    rho, mom = B.site_density(bins, site, off, ns)
    assert np.array_equal(rho, want_rho) and np.array_equal(mom, want_mom)
    dbins, dsite = _dev(bins), _dev(site.astype(np.int32))
    doff = torch.from_numpy(np.ascontiguousarray(np.moveaxis(off, -1, 0).reshape(3, -1, order="F").T)).cuda()
    rho, mom = B.site_density((dbins.data_ptr(), bins.shape), dsite.data_ptr(), doff.data_ptr(), ns)
    assert np.array_equal(rho, want_rho) and np.array_equal(mom, want_mom)
    drho = torch.full((ns + 1,), -7, dtype=torch.int64, device="cuda")
    dmom = torch.full((ns + 1, 3), -7, dtype=torch.int64, device="cuda")
    _abi.check(hip_lib, hip_lib.ceg_grid_site_density(0, _ptr(dbins), 1, _ptr(dsite), _ptr(doff), 1, _dims(bins.shape), ns, _ptr(drho), _ptr(dmom),
                                                      1, NULL))
    torch.cuda.synchronize()
    assert np.array_equal(drho.cpu().numpy(), want_rho) and np.array_equal(dmom.cpu().numpy(), want_mom)
    if centres:
        lit = BC.closest_from_proximity_literal(bins, site, off, ns)
        got = B.closest_from_proximity(bins, site, off, ns)
        for s in range(ns + 1):
            assert got[s][0] == lit[s][0]
            assert np.all(np.abs(got[s][1] - np.asarray(lit[s][1])) <= BC.CENTRE_RTOL * np.abs(lit[s][1]))


def test_proximal_map(hip_lib):
    name, bins, site, off, ns, _ = BC.density_cases()[0]
    sites = np.array([[0.985, 0.52, 0.03], [0.02, 0.97, 0.51], [0.5, 0.03, 0.975], [0.47, 0.45, 0.5], [0.2, 0.2, 0.8]])
    rho, deleted = B.proximal_map(bins, sites, BC.SKEW["mat"], 2.5)
    want, _ = B.site_density_host(bins, site, off, ns)
    assert deleted.size == 0 and np.array_equal(rho, want.astype(np.float64))


def test_reference_minima_of_ar_and_na_in_cha(hip_lib, tmp_path):
    """runtests.jl:35-36 lists (56,88,49), (52,50,91), (51,51,91) for Ar at the default tolerance; the last two are diagonal
    neighbours, and the 26-neighbour rule of basins.jl:40-99 keeps the lower one (test_reference_energy_grid_flow pins the same
    two with NumPy).  runtests.jl:48-49: Na at tolerance 0.0, (29,60,60).  1-based here, as the reference writes them."""
    import ceg_hip as ceg
    from ceg_hip.energy import GpuEnergySetup
    golden = Path(__file__).parent / "golden"
    raspa = tmp_path / "raspa"
    raspa.mkdir()
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(golden / "raspa" / sub, raspa / sub)
    ceg.setdir_RASPA(raspa)
    try:
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96_Na_11812", "BoulfelfelSholl2021", "Ar", "TraPPE", blockfile=None)
        gs = GpuEnergySetup(setup)
        egrid = gs.energy_grid(0.3)
        gs.close()
        got, ext = B.local_minima(egrid, return_extremum=True)
        assert [tuple(r) for r in (got + 1).tolist()] == [(56, 88, 49), (52, 50, 91)]
        assert ext == egrid.min() == egrid[51, 49, 90]
        dg = _dev(egrid)
        got = B.local_minima((dg.data_ptr(), egrid.shape))
        assert [tuple(r) for r in (got + 1).tolist()] == [(56, 88, 49), (52, 50, 91)]
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021", "Na", "TraPPE")
        gs = GpuEnergySetup(setup)
        egrid = gs.energy_grid(0.3)
        gs.close()
        got = B.local_minima(egrid, 0.0)
        assert [tuple(r) for r in (got + 1).tolist()] == [(29, 60, 60)]
    finally:
        ceg.setdir_RASPA(golden / "raspa")
