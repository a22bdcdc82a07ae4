"""basins.jl without a device: the vectorised ``*_host`` forms of ``ceg_hip/basins.py`` against the literal, queue-based restatements
of ``tests/basins_cases.py`` on every case the GPU test uses; the two minima pins of the reference's ``runtests.jl:35-36,48-49`` on
synthetic grids with those minima planted; and the refusals of the four entry points that are decided before a device is looked for."""
import ctypes as C
import math

import numpy as np
import pytest

import basins_cases as BC
from ceg_hip import _abi, basins as B

INVALID = -1


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("case", BC.minima_cases(), ids=_ids(BC.minima_cases()))
def test_local_minima_host_equals_the_literal_loops(case):
    name, g, tol, maxima = case
    ref, ext = BC.minima_reference(name)
    got, gext = B.local_minima_host(g, tol, maxima=maxima, return_extremum=True)
    assert [tuple(r) for r in got.tolist()] == ref
    assert gext == (math.inf if ext is None else ext)
    if name.startswith(("wrap", "special")) and not maxima and tol < 0:
        assert len(ref) >= 4                       # the planted minima on the corner, edge and faces are found through the wrap


def test_the_cases_hold_what_they_are_named_for():
    grids = {n: g for n, g, *_ in BC.minima_cases()}
    refs = {n: BC.minima_reference(n)[0] for n in grids}
    neg = lambda n: [p for p in refs[n] if grids[n][p] < 0]                           # the noise around has minima of its own, all > 0
    assert neg("plateau-17x9x33") == [(9, 5, 20)] and refs["negative-zero"] == [] and refs["constant-count0"] == []
    sp = neg("special-17x9x33-all")
    assert (3, 3, 3) not in sp and (10, 5, 20) in sp and (14, 6, 25) in sp and (16, 0, 32) in sp      # NaN neighbour; walled in; corner
    assert refs["wrap-17x9x33-tol0.0"] == [(0, 0, 0)] and len(refs["wrap-17x9x33-tol0.01"]) == 3
    assert len(refs["wrap-17x9x33-tol1.0"]) == 6 and len(refs["wrap-17x9x33-tol-1.0"]) > 6
    assert any(len(refs[f"random-{s}-tol-1.0"]) == 0 for s in ("1x1x1", "2x2x2"))


@pytest.mark.parametrize("case", BC.minima_refusal_cases(), ids=_ids(BC.minima_refusal_cases()))
def test_local_minima_refuses_a_non_negative_extremum(case):
    _, g, tol = case
    with pytest.raises(AssertionError):
        BC.local_minima_literal(g, tol)
    with pytest.raises(ValueError, match="negative extremum"):
        B.local_minima_host(g, tol)
    assert len(B.local_minima_host(g, -1.0)) >= 1


def test_the_minima_pins_of_the_reference_suite():
    """runtests.jl:35-36 lists (56,88,49), (52,50,91), (51,51,91) for Ar in CHA at the default tolerance; the last two are diagonal
    neighbours, so the 26-neighbour rule of basins.jl:40-99 keeps the lower one only (tests/test_gpu_parity.py pins the same two on
    the real grid).  runtests.jl:48-49: Na in CHA, tolerance 0.0, the single minimum (29,60,60)."""
    shape = (100, 100, 100)
    ar = BC.pinned_grid(shape, [(56, 88, 49), (52, 50, 91)], [-1836.2, -1841.0165092850448],
                        others=[((51, 51, 91), -1832.66), ((20, 20, 20), -1700.0), ((80, 10, 5), -3.0)])
    got = B.local_minima_host(ar) + 1
    assert [tuple(r) for r in got.tolist()] == [(56, 88, 49), (52, 50, 91)]
    assert ar[50, 50, 90] < -1822.7 and ar[50, 50, 90] > ar[51, 49, 90]                  # within the tolerance, but next to a lower point
    na = BC.pinned_grid(shape, [(29, 60, 60)], [-1.9278944364761321e6], others=[((70, 70, 70), -1.9e6), ((1, 1, 1), -1.86e6)])
    got = B.local_minima_host(na, 0.0) + 1
    assert [tuple(r) for r in got.tolist()] == [(29, 60, 60)]
    assert len(B.local_minima_host(na, 0.1)) == 3


def _assert_components(comp, ref, sums=True):
    labels, seeds, sizes, ssum = ref[0], ref[1], ref[2], (ref[3] if len(ref) > 3 else None)
    assert np.array_equal(comp.labels, labels)
    assert comp.seed.tolist() == seeds and comp.size.tolist() == sizes
    if sums and ssum is not None:
        assert comp.sum.tolist() == ssum


@pytest.mark.parametrize("case", BC.component_cases(), ids=_ids(BC.component_cases()))
def test_components_host_equals_the_literal_queues(case):
    name, g = case
    ref = BC.components_reference(name)
    comp = B.grid_components_host(g)
    _assert_components(comp, ref, sums=g.dtype == np.int64)
    if name == "checkerboard-8x8x8":
        assert len(ref[1]) == 256 and set(ref[2]) == {1}
    if name in ("slabs-through-the-face", "serpentine-32x32x4") or name.startswith("all-"):
        assert len(ref[1]) == 1
    if name == "serpentine-32x32x4":
        assert ref[2] == [16 * 31 + 15]
    if name.startswith("none-"):
        assert ref[1] == [] and (comp.labels == -1).all()


@pytest.mark.parametrize("case", BC.band_cases(), ids=_ids(BC.band_cases()))
def test_compute_levels_host_equals_the_literal_queues(case):
    name, g, lo, hi = case
    _assert_components(B.compute_levels_host(g, lo, hi), BC.components_reference(name))


@pytest.mark.parametrize("kw", [dict(), dict(atol=2.0**41), dict(ntol=3), dict(rtol=0.5), dict(atol=5.0, rtol=0.9, ntol=40)])
def test_local_components_cut_and_order(kw):
    for name in ("i64-sparse-17x9x33", "i64-dense-5x7x3", "checkerboard-8x8x8"):
        g = dict(BC.component_cases())[name]
        _, seeds, sizes, sums = BC.components_reference(name)
        keep = BC.cut_components_literal(sums, int(g.sum()), **kw)
        comp = B.local_components_host(g, **kw)
        assert comp.label.tolist() == keep and comp.sum.tolist() == [sums[n] for n in keep]
        assert comp.seed.tolist() == [seeds[n] for n in keep] and comp.size.tolist() == [sizes[n] for n in keep]


@pytest.mark.parametrize("case", BC.proximity_cases(), ids=_ids(BC.proximity_cases()))
def test_proximity_host_equals_the_two_breadth_first_passes(case):
    name, sites, dims, mat, maxdist = case
    site, off, deleted = BC.proximity_reference(name)
    hs, ho, hd = B.site_proximity_map_host(sites, dims, mat, maxdist)
    assert hd.tolist() == deleted
    assert np.array_equal(hs, site) and np.array_equal(ho, off)
    if "faces" in name:
        assert {-1, 1} <= set(np.unique(off).tolist())
    if "twins" in name:
        assert deleted == ([1, 3] if name.startswith("ortho") else deleted) and len(deleted) >= 1
    if "none" in name:
        assert not site.any()


@pytest.mark.parametrize("case", BC.density_cases(), ids=_ids(BC.density_cases()))
def test_site_density_host_equals_the_literal_sums(case):
    name, bins, site, off, ns, centres = case
    lit = BC.closest_from_proximity_literal(bins, site, off, ns)
    rho, mom = B.site_density_host(bins, site, off, ns)
    for s in range(ns + 1):
        sel = site == (0 if s == ns else s + 1)
        assert rho[s] == int(bins[sel].sum())
        idx = np.argwhere(sel)
        for q in range(3):
            assert mom[s, q] == sum(int(bins[tuple(p)]) * (int(off[tuple(p)][q]) * bins.shape[q] + int(p[q])) for p in idx)
    assert rho.sum() == bins.sum()
    if centres:
        got = B.closest_from_proximity_host(bins, site, off, ns)
        for s in range(ns + 1):
            assert got[s][0] == lit[s][0]
            assert np.all(np.abs(got[s][1] - np.asarray(lit[s][1])) <= BC.CENTRE_RTOL * np.abs(lit[s][1]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _dims(*d):
    return _abi.i32ptr(np.asarray(d, dtype=np.int32))


def test_refusals_that_need_no_device():
    lib = _abi.load_library()
    g = np.zeros(8)
    gp = C.c_void_p(g.ctypes.data)
    count, ext = C.c_int64(-7), C.c_double(0.0)
    null = C.c_void_p(0)

    def minima(grid=gp, dims=(2, 2, 2), maxima=0, tol=-1.0, cap=0):
        return lib.ceg_grid_local_minima(0, grid, 0, _dims(*dims), maxima, tol, null, 0, cap, C.byref(count), C.byref(ext), null)
    assert minima(grid=null) == INVALID and minima(dims=(0, 2, 2)) == INVALID and minima(maxima=2) == INVALID
    assert minima(tol=math.nan) == INVALID and minima(cap=4) == INVALID            # room asked for, no array
    assert minima(dims=(2048, 1024, 1024)) == INVALID and b"int32" in lib.ceg_last_error()
    assert minima(dims=(65536, 65536, 1)) == INVALID

    def comps(grid=gp, i64=0, dims=(2, 2, 2), mode=0, lo=0.0, hi=1.0, ssum=null):
        return lib.ceg_grid_components(0, grid, i64, 0, _dims(*dims), mode, lo, hi, null, 0, null, null, ssum, 0, 0, C.byref(count), null)
    assert comps(grid=null) == INVALID and comps(mode=2) == INVALID and comps(dims=(2, -1, 2)) == INVALID
    assert comps(i64=1, mode=1) == INVALID and comps(mode=1, lo=math.nan) == INVALID
    assert comps(ssum=gp) == INVALID and b"int64 grid only" in lib.ceg_last_error()
    assert comps(dims=(2048, 1024, 1024)) == INVALID
    assert count.value == -7                                                       # nothing was written

    mat = np.ascontiguousarray(BC.SKEW["mat"].T).ravel()
    sites = np.array([0.5, 0.5, 0.5])
    out = np.zeros(12 * 10 * 14 * 4, dtype=np.int8)
    op = C.c_void_p(out.ctypes.data)

    def prox(maxdist=2.0, ns=1, m=mat, dims=BC.SKEW["dims"], s=sites):
        return lib.ceg_grid_site_proximity(0, _dims(*dims), _abi.dptr(m), _abi.dptr(s) if s is not None else None, ns, maxdist, op, op, 0, null)
    assert prox(maxdist=0.0) == INVALID and prox(maxdist=-1.0) == INVALID and prox(maxdist=math.inf) == INVALID
    assert prox(ns=-1) == INVALID and prox(s=None) == INVALID
    assert prox(ns=_abi.SITE_PROXIMITY_MAX_SITES + 1) == -5
    assert prox(maxdist=4.5) == INVALID and b"smallest width" in lib.ceg_last_error()       # the ball would meet its own image
    assert prox(m=np.zeros(9)) == INVALID
    assert not out.any()
    rc = prox(maxdist=3.0)
    assert rc in (0, -2)                                                           # legal: runs, or finds no device
    with pytest.raises(ValueError, match="smallest width"):
        B.site_proximity_map_host(sites.reshape(1, 3), BC.SKEW["dims"], BC.SKEW["mat"], 4.5)
    B.check_maxdist(BC.SKEW["dims"], BC.SKEW["mat"], 3.0)

    rho = np.zeros(16, dtype=np.int64)
    rp = C.c_void_p(rho.ctypes.data)
    assert lib.ceg_grid_site_density(0, null, 0, gp, gp, 0, _dims(2, 2, 2), 1, rp, rp, 0, null) == INVALID
    assert lib.ceg_grid_site_density(0, gp, 0, gp, gp, 0, _dims(2, 2, 2), -1, rp, rp, 0, null) == INVALID
    assert lib.ceg_grid_site_density(0, gp, 0, gp, gp, 0, _dims(2, 2, 2), 1, null, rp, 0, null) == INVALID


def test_binding_argument_checks():
    with pytest.raises(ValueError):
        B.local_minima(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="int32"):
        B.local_minima((1 << 20, (2048, 1024, 1024)))
    with pytest.raises(TypeError):
        B.grid_components(np.zeros((2, 2, 2), dtype=np.complex128))
    kept, deleted = B.snap_sites([[0.26, 0.31, 0.52], [0.27, 0.305, 0.515], [0.71, 0.66, 0.2]], (9, 8, 10))
    assert deleted.tolist() == [1] and len(kept) == 2
    assert B.snap_sites(np.zeros((0, 3)), (9, 8, 10))[0].shape == (0, 3)
