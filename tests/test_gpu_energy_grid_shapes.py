"""``ceg_energy_grid`` and ``ceg_energy_grid_reduced`` (csrc/ceg_egrid.hip) at the orientation counts their callers use -- 43 for a
linear symmetric guest, 70 for a non-linear one at num_rotate = 40 -- and around them, on rows of up to 145 points, with k-spaces of
0 to 316 vectors and molecules of 1 to 16 atoms: every compared element against the longdouble reference of
``tests/egrid_shape_cases.py`` within its derived bound; ``tests/test_egrid_shape_cases_host.py`` checks the cases, the reference
and the bound on the CPU.

What runs here (the launch lists are asserted on the CPU against the arithmetic of ``egrid_run``):
  * k_egrid_cross<1>, <2>, <3>, <4> as the only or last launch (nrot = 15, 16 | 17, 32 | 33, 43, 48 | 49, 64), <4> followed by <1>
    (65, 70) and <4>, <4>, <1> (129); the store guard r < nrot inside a tile and on a tile boundary;
  * rows of 1, 16, 17, 128, 129 and 145 points at nrot = 17 and 65: 1, 2 and 8 waves, blockIdx.y = 1 with one and two working
    waves beside idle ones;
  * nk = 0 (with a live Coulomb grid), 1, 15, 16, 17 and 316 at three rotation tiles; 1 and 16 atoms at nrot = 43;
  * two composite cases (nrot = 43, 70: two VdW grids on different cells, one atom without a grid, a random Coulomb grid, every term
    live) as host output, device output and host output in three slabs, bit-identical;
  * for every case with nrot >= 16 ``ceg_energy_grid_reduced``: min and argmin against the device's own elements bit for bit, the
    means at 77, 300 and 1000 K, unweighted and weighted, against the mirror of meanBoltzmann over those elements; device outputs
    for two cases; k_egrid_reduce<2>, <4> ... <8> against the single-temperature planes; the exact tie cases and the NaN case.

Measured on an MI355X, worst |got - reference| / bound per table (the float64 emulation on the CPU predicted 0.001 to 0.018):
  nrot = 15 .. 129 (17 x 3 x 2 points, 114 k-vectors)        0.0047   (nrot <= 43; 0.0033 at 48 .. 70, 0.0032 at 129, three launches)
  numA = 1 .. 145 at nrot = 17 and 65                         0.0049   (numA = 129, nrot = 65; blockIdx.y = 1: 0.0032 to 0.0049)
  nk = 0, 1, 15, 16, 17, 316                                  0.0195   (nk = 1; 0.0085, 0.0195, 0.0088, 0.0106, 0.0067, 0.0019)
  1 and 16 atoms at nrot = 43                                 0.0042   (0.0042, 0.0008)
  all terms at nrot = 43 and 70                               0.0026   (0.0026, 0.0013); the three routes bit-identical
  means of every case with nrot >= 16                         0.0018   of the bound 1e-12 sum(f|x|)/sum(f)
The cases with a handful of k-vectors sit higher because fewer terms average out under the same worst-case bound.  Nothing was
found wrong in csrc/ceg_egrid.hip: the production shapes are pinned, no fix was needed.
"""
import numpy as np
import pytest

import egrid_shape_cases as E
import interp_cases as IC

pytestmark = pytest.mark.gpu
LD = np.longdouble
TEMPS = (77.0, 300.0, 1000.0)
EIGHT_TEMPS = (50.0, 77.0, 150.0, 300.0, 500.0, 700.0, 1000.0, 2000.0)
DEVICE_OUTPUT_CASES = ("nrot129", "numA145-nrot65")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_elements(name, full):
    """every compared element inside its tolerance -> the worst ratio"""
    c = E.BY_NAME[name]
    e = E.expected(name)
    assert full.shape == (c.nrot,) + c.num and np.isfinite(full).all(), name
    got = full[e.idx]
    err = np.abs(got.astype(LD) - e.ref).astype(np.float64)
    ratio = err / e.tol
    worst = int(np.argmax(ratio))
    print(f"egrid-ratio {name}: launches {list(c.launches)}, {c.waves} waves x grid.y {c.grid_y}, nk = {E.inputs(name).k.nk}, {len(got)} of {full.size} "
          f"elements, worst |got - ref| / bound = {ratio[worst]:.4f} at (r, iA, iB, iC) = {tuple(int(i[worst]) for i in e.idx)}")
    assert np.all(err <= e.tol), (name, float(ratio[worst]), [tuple(int(i[q]) for i in e.idx) for q in np.nonzero(err > e.tol)[0][:8]])
    return float(ratio[worst])


def _assert_means(got, full, temps, w, what):
    worst = 0.0
    for t, T in enumerate(temps):
        ref, bound = E.mean_bound(full, T, w)
        assert not np.isnan(ref).any(), what
        inaccessible = ref >= 1e90
        assert np.all(got[t][inaccessible] >= 1e90), (what, T)
        ok = ~inaccessible
        err = np.abs(got[t] - ref)
        ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
        assert np.all(err[ok] <= bound[ok]), (what, T, ratio)
        worst = max(worst, ratio)
    return worst


def _device_reduction(dev, temps, w):
    """ceg_energy_grid_reduced into device memory on the current stream -> (mean, min, argmin) read back"""
    import torch
    nt, points = len(temps), dev.points
    d_mean = torch.full((nt * points,), float("nan"), dtype=torch.float64, device="cuda:0")
    d_min = torch.full((points,), float("nan"), dtype=torch.float64, device="cuda:0")
    d_amin = torch.full((points,), -1, dtype=torch.int32, device="cuda:0")
    dev.reduced(temps, w, out_ptrs=(d_mean.data_ptr(), d_min.data_ptr(), d_amin.data_ptr()), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dev.lattice(d_mean.cpu().numpy(), (nt,)), dev.lattice(d_min.cpu().numpy()), dev.lattice(d_amin.cpu().numpy())


def _device_elements(dev):
    import torch
    d_out = torch.full((dev.nrot * dev.points,), float("nan"), dtype=torch.float64, device="cuda:0")
    dev.elements(out_ptr=d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dev.elements_array(d_out.cpu().numpy())


def _check_reduction(dev, full, name, device_outputs):
    """min / argmin of the device's own elements bit for bit, the means against the mirror over those elements"""
    w = E.weights(dev.nrot)
    mean, mn, amin = dev.reduced(TEMPS)
    meanw, none_min, none_amin = dev.reduced(TEMPS, w, want_min=False, want_argmin=False)
    assert none_min is None and none_amin is None and amin.dtype == np.int32
    assert _same_bits(mn, full.min(axis=0)), name
    assert np.array_equal(amin, full.argmin(axis=0)), name
    worst = max(_assert_means(mean, full, TEMPS, None, name), _assert_means(meanw, full, TEMPS, w, name))
    print(f"egrid-reduce {name}: nrot = {dev.nrot}, {dev.points} points, argmin takes {len(np.unique(amin))} values (largest {amin.max()}), worst error of a "
          f"mean = {worst:.3g} of the bound 1e-12 sum(f|x|)/sum(f)")
    assert not _same_bits(mean, meanw)
    if device_outputs:
        d_mean, d_min, d_amin = _device_reduction(dev, TEMPS, w)
        assert _same_bits(d_mean, meanw) and _same_bits(d_min, mn) and _same_bits(d_amin, amin), name


def _run(lib, name):
    inp = E.inputs(name)
    dev = E.Device.of_case(lib, inp)
    try:
        full = dev.elements()
        _check_elements(name, full)
        if inp.case.nrot >= 16:
            _check_reduction(dev, full, name, name in DEVICE_OUTPUT_CASES)
        if name in DEVICE_OUTPUT_CASES:
            assert _same_bits(_device_elements(dev), full), name
    finally:
        dev.close()
    return full


@pytest.mark.parametrize("name", [c.name for c in E.NROT_CASES])
def test_orientation_counts(hip_lib, name):
    """k_egrid_cross<1 .. 4> alone, <4> + <1>, <4> + <4> + <1>; 17 x 3 x 2 points, 114 k-vectors, a Coulomb grid of zeros: the
    element is the reciprocal term alone"""
    _run(hip_lib, name)


@pytest.mark.parametrize("name", [c.name for c in E.NUMA_CASES])
def test_row_lengths(hip_lib, name):
    """1, 2 and 8 waves per workgroup, blockIdx.y = 1 with idle waves in the barriers of the k-chunk loop"""
    _run(hip_lib, name)


@pytest.mark.parametrize("name", [c.name for c in E.NK_CASES])
def test_kspace_sizes(hip_lib, name):
    """nk = 0 (has_recip_sum = 0 beside a live Coulomb grid), fewer than one chunk of 16, exactly one, and nk % 16 != 0, at three
    rotation tiles"""
    full = _run(hip_lib, name)
    if name == "nk0":
        assert len(np.unique(full)) > 100                                    # the direct term is live


@pytest.mark.parametrize("name", [c.name for c in E.NATOMS_CASES])
def test_molecule_sizes(hip_lib, name):
    _run(hip_lib, name)


@pytest.mark.parametrize("name", [c.name for c in E.COMPOSITE_CASES])
def test_all_terms_three_ways(hip_lib, monkeypatch, name):
    """VdW (two grids on different cells, one atom without a grid), direct and reciprocal terms at nrot = 43 and 70: host output,
    device output and host output with numC = 3 cut into three slabs are bit-identical, and so are the reductions"""
    inp = E.inputs(name)
    c = inp.case
    dev = E.Device.of_case(hip_lib, inp)
    try:
        full = dev.elements()
        _check_elements(name, full)
        _check_reduction(dev, full, name, True)
        assert _same_bits(_device_elements(dev), full)
        whole = dev.reduced(TEMPS, E.weights(c.nrot))
        plane = 8 * c.nrot * c.num[0] * c.num[1]
        monkeypatch.setenv("CEG_HIP_EGRID_SLAB_BYTES", str(plane + 100))     # one iC plane per slab: three slabs
        assert _same_bits(dev.elements(), full)
        slabbed = dev.reduced(TEMPS, E.weights(c.nrot))
        dev_slabbed = _device_reduction(dev, TEMPS, E.weights(c.nrot))
        for a, b, d in zip(whole, slabbed, dev_slabbed):
            assert _same_bits(a, b) and _same_bits(a, d)
    finally:
        dev.close()
    e = E.expected(name)
    assert (e.vdw != 0).all() and (e.direct != 0).all() and (e.recip != 0).all()


def test_every_number_of_temperatures(hip_lib):
    """k_egrid_reduce<2>, <4>, <5>, <6>, <7>, <8> at nrot = 43: the plane of a temperature is, bit for bit, the plane of that
    temperature asked for alone (k_egrid_reduce<1>), with weights"""
    name = "composite-nrot43"
    inp = E.inputs(name)
    w = E.weights(inp.case.nrot)
    dev = E.Device.of_case(hip_lib, inp)
    try:
        full = dev.elements()
        alone = [dev.reduced((T,), w, want_min=False, want_argmin=False)[0][0] for T in EIGHT_TEMPS]
        assert _assert_means(np.array(alone), full, EIGHT_TEMPS, w, name) <= 1.0
        for n in (2, 4, 5, 6, 7, 8):
            mean, mn, _amin = dev.reduced(EIGHT_TEMPS[:n], w, want_argmin=False)
            assert mean.shape == (n,) + inp.case.num and _same_bits(mn, full.min(axis=0))
            for t in range(n):
                assert _same_bits(mean[t], alone[t]), (n, t)
        assert all(not _same_bits(alone[0], a) for a in alone[1:])
    finally:
        dev.close()


@pytest.mark.parametrize("nrot", E.EXACT_NROT)
@pytest.mark.parametrize("variant", sorted(E.EXACT_VALUE))
def test_equal_elements_behind_a_block_mask(hip_lib, variant, nrot):
    """Every free element is the same number exactly (0.0, or 2 enc + static = 108.25), a mask of spheres blocks most orientations:
    min is that number and argmin the first free orientation -- found in every lane of the butterfly and in later rounds of a lane,
    ties between lanes decided by the index --, every mean is that number bit for bit, with and without weights; a point without
    a free orientation gives 1e100, 0 and means >= 1e90."""
    value = E.EXACT_VALUE[variant]
    num = E.EXACT_NUM[nrot]
    q, base = E.exact_molecule()
    blocked, _margin = E.exact_blocked(nrot)
    if variant == "zero":
        vdw = [IC.energy_grid(IC.cset(cell, dims), np.zeros((8,) + tuple(IC.cset(cell, dims).npoints), dtype=IC.F32), IC.VDW)
               for cell, dims in (("ortho", (7, 5, 3)), ("tric", (15, 13, 11)), ("tric", (3, 3, 3)))]
        dev = E.Device(hip_lib, vdw, None, None, q, base, E.rotations(nrot), num, block=E.block_mask())
    else:
        cs = IC.cset(*E.COULOMB_DIMS)
        coulomb = IC.energy_grid(cs, np.zeros((8,) + tuple(cs.npoints), dtype=IC.F32), IC.COULOMB)
        dev = E.Device(hip_lib, [None] * 3, coulomb, E.kset_of(("none",)), q, base, E.rotations(nrot), num, E.ENC, E.STATIC, block=E.block_mask())
    w = E.weights(nrot)
    try:
        full = dev.elements()
        mean, mn, amin = dev.reduced(TEMPS)
        meanw, mnw, aminw = dev.reduced(TEMPS, w)
    finally:
        dev.close()
    assert np.array_equal(full == 1e100, blocked), "the blocked elements are not those of the host"
    assert _same_bits(full[~blocked], np.full(int((~blocked).sum()), value))
    ff = E.first_free(blocked)
    some = ff < nrot
    assert _same_bits(mn, np.where(some, value, 1e100)) and _same_bits(mnw, mn)
    assert np.array_equal(amin, np.where(some, ff, 0)) and np.array_equal(aminw, amin)
    for m in (mean, meanw):
        for t in range(len(TEMPS)):
            assert _same_bits(m[t][some], np.full(int(some.sum()), value)), (variant, nrot, TEMPS[t])
            assert np.all(m[t][~some] >= 1e90)
    print(f"egrid-exact {variant} nrot = {nrot}: {some.sum()} points with a free orientation (first free up to {ff[some].max()}), {(~some).sum()} without")


def test_nan_elements(hip_lib):
    """One NaN datum in a VdW grid: wherever an element of a point is NaN, out_min is NaN and out_argmin the first NaN index
    (Julia's findmin, which np.argmin shares); elsewhere min and argmin of the elements as usual."""
    grids, q, base, rots, num = E.nan_case()
    dev = E.Device(hip_lib, grids, None, None, q, base, rots, num)
    try:
        full = dev.elements()
        _mean, mn, amin = dev.reduced()
    finally:
        dev.close()
    nan = np.isnan(full)
    has = nan.any(axis=0)
    assert has.any() and not has.all() and (nan.sum(axis=0) >= 2).any()
    assert np.all(np.isnan(mn[has])) and np.array_equal(amin[has], nan.argmax(axis=0)[has])
    assert (amin[has] > 0).any()
    assert np.array_equal(amin, np.argmin(full, axis=0))
    assert _same_bits(mn[~has], full.min(axis=0)[~has])
