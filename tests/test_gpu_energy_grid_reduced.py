"""``ceg_energy_grid_reduced`` on the GPU: the rotation axis of energy_grid collapsed per lattice point -- minimum, first
orientation that attains it, the reference's meanBoltzmann (src/utils.jl:415-443) at several temperatures -- without the elements
leaving the device.

min / argmin are compared bit for bit with ``ceg_energy_grid``'s own elements.  The means are compared with the host mirror of
meanBoltzmann over those elements, every point, with

    |got - ref| <= 1e-12 sum(f |x|) / sum(f),      f_k = w_k exp((m - x_k)/T),  m = min - 30 T      (f, x from the mirror)

Where the 1e-12 comes from: a term that is not flushed to zero has |(m - x)/T| <= 745, so the rounding of the argument moves f by
at most 745 * 2^-53 ~ 8e-14 relative; a device exp of a few ulp and the reordering of two sums of nrot <= 64 terms of
non-negative weight add less than 2e-14; 1e-12 is that bound with a factor of ten in hand.  Where the mirror gives >= 1e90
(every orientation inaccessible) the device must too."""
import ctypes as C
import math

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from ceg_hip.hostmirror.utils import mean_boltzmann
from test_gpu_energy_grid import (raspa_dir, setups, _lattice, _positions, _seven_rotations, _setup_terms)  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
TEMPS = (77.0, 300.0, 1000.0)
CASES = [("CHA_1.4_3b4eeb96_Na_11812", 1.5), ("CIT-7", 0.7)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _weights(nrot):
    """positive, non-uniform, spanning a factor of 40 (Lebedev weights of one order span less)"""
    return np.random.default_rng(590).uniform(0.05, 2.0, nrot)


def _mean_bound(full, T, w):
    """-> (mirror mean, 1e-12 sum(f |x|)/sum(f)), the factors formed like the mirror's"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        m = full.min(axis=0) - 30.0 * T
        f = np.exp((m[None] - full) / T)
        if w is not None:
            f = f * np.asarray(w)[:, None, None, None]
        return mean_boltzmann(full, T, w), 1e-12 * (f * np.abs(full)).sum(axis=0) / f.sum(axis=0)


def _assert_means(got, full, temps, w, what):
    """every point, none excluded -> worst error in units of the bound"""
    worst = 0.0
    for t, T in enumerate(temps):
        ref, bound = _mean_bound(full, T, w)
        assert not np.isnan(ref).any(), what
        inaccessible = ref >= 1e90
        assert np.all(got[t][inaccessible] >= 1e90), f"{what}, {T} K: an inaccessible point came out accessible"
        ok = ~inaccessible
        err = np.abs(got[t] - ref)
        ratio = (err[ok] / bound[ok]).max() if ok.any() else 0.0
        i = np.unravel_index(np.argmax(np.where(ok, err / bound, 0.0)), err.shape)
        print(f"  {what}, {T} K, {'weighted' if w is not None else 'unweighted'}: {ok.sum()} accessible + {inaccessible.sum()} inaccessible "
              f"points, worst |got - ref| / bound = {ratio:.3g} ({ratio * 1e-12:.3g} sum(f|x|)/sum(f)) at point {i}: got {got[t][i]!r}, "
              f"mirror {ref[i]!r}")
        assert np.all(err[ok] <= bound[ok]), f"{what}, {T} K: worst |got - ref| / bound = {ratio:.3g} at {i}"
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("framework,step", CASES)
def test_min_and_argmin_are_those_of_the_elements(hip_lib, setups, framework, step):
    """CO2, all terms, 7 rotations, lattice counts that are no multiples of 16: out_min / out_argmin against the host output of
    ceg_energy_grid for the same call, bit for bit, every point."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups(framework, "CO2")
    rots = _seven_rotations()
    gs = GpuEnergySetup(setup)
    try:
        full = gs.energy_grid_rotations(step, rots)
        red = gs.energy_grid_reduced(step, rots, want_min=True, want_argmin=True)
    finally:
        gs.close()
    assert all(n % 16 for n in full.shape[1:]) and full.shape[0] == 7
    assert not np.isnan(full).any()
    assert red.mean is None and red.min.shape == full.shape[1:] and red.argmin.dtype == np.int32
    assert _same_bits(red.min, full.min(axis=0))
    assert np.array_equal(red.argmin, full.argmin(axis=0))
    assert len(np.unique(red.argmin)) > 1


@pytest.mark.parametrize("framework,step", CASES)
def test_means_against_the_mirror_over_the_elements(hip_lib, setups, framework, step):
    """The same calls at 77, 300 and 1000 K, unweighted and with non-uniform positive weights."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups(framework, "CO2")
    rots = _seven_rotations()
    w = _weights(len(rots))
    gs = GpuEnergySetup(setup)
    try:
        full = gs.energy_grid_rotations(step, rots)
        plain = gs.energy_grid_reduced(step, rots, TEMPS)
        weighted = gs.energy_grid_reduced(step, rots, TEMPS, weights=w, want_min=False)
    finally:
        gs.close()
    assert plain.mean.shape == (3,) + full.shape[1:] and weighted.min is None and weighted.argmin is None
    assert _same_bits(plain.min, full.min(axis=0))
    worst = max(_assert_means(plain.mean, full, TEMPS, None, f"CO2 in {framework}"),
                _assert_means(weighted.mean, full, TEMPS, w, f"CO2 in {framework}"))
    print(f"  CO2 in {framework}: worst error of all means = {worst:.3g} of the bound")
    assert not _same_bits(plain.mean, weighted.mean)              # the weights are live
    assert (plain.mean[1] < 1e90).any() and (plain.mean[0] != plain.mean[2]).any()


def _test5_rotations():
    """Seven orientations without an antipodal pair.  CO2 is linear and symmetric: the last two of _seven_rotations (a rotation q
    and q diag(1, 1, -1)) turn the molecular axis to +-q[:, 2], the same placement with the oxygens exchanged, whose two
    energies differ by rounding only -- no reference could name the smaller.  The reflection is replaced by another rotation."""
    qm, _ = np.linalg.qr(np.random.default_rng(77).normal(size=(3, 3)))
    if np.linalg.det(qm) < 0:
        qm[:, 0] = -qm[:, 0]
    return np.concatenate([_seven_rotations()[:6], qm[None]])


def test_against_the_oracle_directly(hip_lib, oracle, setups):
    """CIT-7, 7 rotations, 300 K: the element array composed from the ORACLE's terms (not the device's), reduced by the mirror.
    Mean: the element tolerance of test_gpu_energy_grid._assert_matches, 1e-9 (|vdw| + |direct| + |recip|) + 1e-11 max|recip|,
    carried through the mean, sum(f tol)/sum(f).  argmin: equal wherever the oracle's two smallest elements are further apart
    than twice their tolerance, and also where they are the same multiple of the 1e100 of an inaccessible placement (an exact
    tie on both sides, first index); those two kinds of point must make up at least 99 % of the lattice.  min: the tolerance of
    the element it is."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT-7", "CO2")
    rots = _test5_rotations()
    T = 300.0
    num, (blocked, vdw, direct, recip) = _setup_terms(oracle, setup, rots, 0.7)
    elem = np.where(blocked, 1e100, vdw + (direct + recip))
    ok = ~blocked
    tol = np.where(blocked, 0.0, 1e-9 * (np.abs(vdw) + np.abs(direct) + np.abs(recip)) + 1e-11 * np.abs(recip[ok]).max())
    gs = GpuEnergySetup(setup)
    try:
        red = gs.energy_grid_reduced(0.7, rots, (T,), want_min=True, want_argmin=True)
    finally:
        gs.close()
    assert red.min.shape == num
    # argmin
    order = np.argsort(elem, axis=0, kind="stable")
    first, second = np.take_along_axis(elem, order[:1], 0)[0], np.take_along_axis(elem, order[1:2], 0)[0]
    tol12 = np.maximum(np.take_along_axis(tol, order[:1], 0)[0], np.take_along_axis(tol, order[1:2], 0)[0])
    separated = (second - first) > 2.0 * tol12
    sentinel = (first >= 1e100) & (second == first)
    decided = separated | sentinel
    print(f"  {separated.sum()} separated + {sentinel.sum()} tied inaccessible of {decided.size} points: {decided.mean():.4f} decided; "
          f"argmin differs at {(red.argmin != order[0]).sum()} points, {(red.argmin != order[0])[decided].sum()} of them decided")
    assert decided.mean() >= 0.99
    assert np.array_equal(red.argmin[decided], order[0][decided])
    # min
    assert np.all(red.min[first >= 1e100] == first[first >= 1e100])
    assert np.all(np.abs(red.min - first)[separated] <= np.take_along_axis(tol, order[:1], 0)[0][separated])
    # mean
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        f = np.exp(((first - 30.0 * T)[None] - elem) / T)
        tol_mean = (f * tol).sum(axis=0) / f.sum(axis=0)
    ref = mean_boltzmann(elem, T)
    inaccessible = ref >= 1e90
    assert np.all(red.mean[0][inaccessible] >= 1e90)
    acc = ~inaccessible
    err = np.abs(red.mean[0] - ref)
    print(f"  mean at {T} K: {acc.sum()} accessible points, worst |got - ref| / tolerance = {(err[acc] / tol_mean[acc]).max():.3g}")
    assert np.all(err[acc] <= tol_mean[acc])


def test_blocking_three_classes_of_point(hip_lib, setups):
    """CO2 in CIT7block, 7 rotations.  The carbon sits at the molecule's origin, so a lattice point on a blocked node blocks every
    orientation; next to a sphere some orientations reach into it; elsewhere none does.  All three classes occur."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT7block", "CO2")
    assert not setup.block.empty
    rots = _seven_rotations()
    step = 1.0
    num, steps = _lattice(setup.framework.mat, step)
    base = np.asarray(setup.molecule.position, dtype=np.float64).reshape(-1, 3)
    pos = _positions(base, rots, num, steps)
    blocked = np.array([any(setup.block[p] for p in mol) for mol in pos.reshape(-1, len(base), 3)]).reshape((len(rots),) + num)
    w = _weights(len(rots))
    gs = GpuEnergySetup(setup)
    try:
        full = gs.energy_grid_rotations(step, rots)
        red = gs.energy_grid_reduced(step, rots, TEMPS, want_min=True, want_argmin=True)
        redw = gs.energy_grid_reduced(step, rots, TEMPS, weights=w, want_min=False)
    finally:
        gs.close()
    assert np.all(full[blocked] == 1e100)
    nblocked = blocked.sum(axis=0)
    every, some, none = nblocked == len(rots), (nblocked > 0) & (nblocked < len(rots)), nblocked == 0
    print(f"  {every.sum()} points with every orientation blocked, {some.sum()} with some, {none.sum()} with none")
    assert every.sum() > 0 and some.sum() > 0 and none.sum() > 0
    # every orientation blocked
    assert np.all(red.min[every] == 1e100) and np.all(red.argmin[every] == 0)
    assert np.all(red.mean[:, every] >= 1e90) and np.all(redw.mean[:, every] >= 1e90)
    # all classes: the mirror over the full array
    assert _same_bits(red.min, full.min(axis=0)) and np.array_equal(red.argmin, full.argmin(axis=0))
    _assert_means(red.mean, full, TEMPS, None, "CO2 in CIT7block")
    _assert_means(redw.mean, full, TEMPS, w, "CO2 in CIT7block")
    # some blocked: the blocked orientations drop out -- the mirror over the free orientations alone
    checked = 0
    for i in zip(*np.nonzero(some)):
        free = ~blocked[(slice(None),) + i]
        col = full[(slice(None),) + i][free]
        if col.min() >= 1e90:
            continue                                              # the free orientations overlap the framework
        assert not blocked[red.argmin[i]][i]
        for t, T in enumerate(TEMPS):
            for got, wk in ((red.mean[t][i], None), (redw.mean[t][i], w[free])):
                ref = mean_boltzmann(col, T, wk)
                with np.errstate(over="ignore", under="ignore"):
                    f = np.exp((col.min() - 30.0 * T - col) / T) * (1.0 if wk is None else wk)
                assert abs(got - ref) <= 1e-12 * (f * np.abs(col)).sum() / f.sum(), (i, T, got, ref)
        checked += 1
    assert checked > 0


def test_invariance_slab_size_output_location_and_other_temperatures(hip_lib, setups, monkeypatch):
    """Three iC planes per slab (and one), device outputs (also slabbed), and 300 K asked for alone or between 77 and 1000 K:
    the same bits in every output."""
    import torch
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT-7", "CO2")
    rots = _seven_rotations()
    w = _weights(len(rots))
    gs = GpuEnergySetup(setup)
    try:
        whole = gs.energy_grid_reduced(0.7, rots, TEMPS, weights=w, want_min=True, want_argmin=True)
        alone = gs.energy_grid_reduced(0.7, rots, (300.0,), weights=w, want_min=False)
        numA, numB, numC = whole.min.shape
        assert numC == 14
        points = numA * numB * numC

        def on_device():
            d_mean = torch.full((3 * points,), float("nan"), dtype=torch.float64, device="cuda:0")
            d_min = torch.full((points,), float("nan"), dtype=torch.float64, device="cuda:0")
            d_amin = torch.full((points,), -1, dtype=torch.int32, device="cuda:0")
            shape = gs.energy_grid_reduced(0.7, rots, TEMPS, weights=w, out_device_ptrs=(d_mean.data_ptr(), d_min.data_ptr(), d_amin.data_ptr()),
                                           stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert shape == (numA, numB, numC)
            return (d_mean.cpu().numpy().reshape(3, numC, numB, numA).transpose(0, 3, 2, 1),
                    d_min.cpu().numpy().reshape(numC, numB, numA).transpose(2, 1, 0), d_amin.cpu().numpy().reshape(numC, numB, numA).transpose(2, 1, 0))
        dev = on_device()
        plane = 8 * len(rots) * numA * numB
        monkeypatch.setenv("CEG_HIP_EGRID_SLAB_BYTES", str(3 * plane + 100))
        slabs = gs.energy_grid_reduced(0.7, rots, TEMPS, weights=w, want_min=True, want_argmin=True)
        dev_slabs = on_device()
        monkeypatch.setenv("CEG_HIP_EGRID_SLAB_BYTES", "1")              # below one plane: one plane per slab
        planes = gs.energy_grid_reduced(0.7, rots, TEMPS, weights=w, want_min=True, want_argmin=True)
    finally:
        gs.close()
    assert np.isfinite(whole.mean).all()
    for other in (slabs, planes, dev, dev_slabs):
        for a, b in zip(whole, other):
            assert _same_bits(a, b)
    assert _same_bits(alone.mean[0], whole.mean[1])


def test_single_orientation_and_the_monoatomic_route(hip_lib, oracle, setups):
    """nrot = 1: mean == min == the element, bit for bit, argmin 0.  Na in CHA through this route: GpuEnergySetup.energy_grid(step)
    to the tolerance of test_single_orientation_agrees_with_the_monoatomic_route.  No temperature: min alone."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT-7", "CO2")
    rot = _seven_rotations()[5:6]
    gs = GpuEnergySetup(setup)
    try:
        full = gs.energy_grid_rotations(0.7, rot)
        red = gs.energy_grid_reduced(0.7, rot, TEMPS, want_min=True, want_argmin=True)
        only_min = gs.energy_grid_reduced(0.7, rot)
        only_argmin = gs.energy_grid_reduced(0.7, _seven_rotations(), want_min=False, want_argmin=True)
        seven = gs.energy_grid_rotations(0.7, _seven_rotations())
    finally:
        gs.close()
    assert _same_bits(red.min, full[0]) and not red.argmin.any()
    for t in range(3):
        assert _same_bits(red.mean[t], full[0])
    assert only_min.mean is None and only_min.argmin is None and _same_bits(only_min.min, full[0])
    assert only_argmin.min is None and np.array_equal(only_argmin.argmin, seven.argmin(axis=0))
    setup = setups("CHA_1.4_3b4eeb96", "Na")
    num, (blocked, vdw, direct, recip) = _setup_terms(oracle, setup, np.eye(3)[None], 1.5)
    gs = GpuEnergySetup(setup)
    try:
        na = gs.energy_grid_reduced(1.5, np.eye(3)[None], (300.0,))
        old = gs.energy_grid(1.5)
    finally:
        gs.close()
    tol = 1e-9 * (np.abs(vdw) + np.abs(direct) + np.abs(recip)) + 1e-11 * np.abs(recip).max()
    assert na.min.shape == num == old.shape
    assert np.all(np.abs(na.min - old) <= tol[0]) and np.all(np.abs(na.mean[0] - old) <= tol[0])


def test_refusals_launch_nothing(hip_lib, setups):
    """CEG_ERR_INVALID with a message for ntemps out of range, a temperature that is zero, negative, infinite or NaN, out_mean
    missing with ntemps > 0 (or given without), no output at all; the refusals of ceg_energy_grid unchanged.  The outputs keep
    what they held."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT-7", "CO2")
    gs = GpuEnergySetup(setup)
    try:
        args, keep, nrot, num = gs._egrid_arguments(2.5, _seven_rotations())
        points = int(np.prod(num))
        mean = np.full(9 * points, -7.0)
        mn = np.full(points, -7.0)
        amin = np.full(points, -7, dtype=np.int32)

        def call(temps, ntemps, p_mean, p_min, p_amin, args=args):
            t = np.ascontiguousarray(temps, dtype=np.float64)
            rc = hip_lib.ceg_energy_grid_reduced(*args, _abi.dptr(t) if len(t) else None, ntemps, None,
                                                 _abi.dptr(mean) if p_mean else None, mn.ctypes.data if p_min else None,
                                                 amin.ctypes.data if p_amin else None, 0, None)
            return rc, (hip_lib.ceg_last_error() or b"").decode()

        bad = [
            ("ntemps = -1", call([300.0], -1, True, True, True)),
            ("ntemps = 9", call([300.0] * 9, 9, True, True, True)),
            ("T = 0", call([300.0, 0.0], 2, True, True, True)),
            ("T < 0", call([-300.0], 1, True, True, True)),
            ("T = inf", call([math.inf], 1, True, True, True)),
            ("T = NaN", call([77.0, 300.0, math.nan], 3, True, True, True)),
            ("out_mean missing", call([300.0], 1, False, True, True)),
            ("out_mean without temperatures", call([], 0, True, True, True)),
            ("nothing requested", call([], 0, False, False, False)),
        ]
        for what, (rc, msg) in bad:
            assert rc == -1 and msg, (what, rc, msg)              # CEG_ERR_INVALID
        # the shared checks of ceg_energy_grid
        a = list(args)
        a[7] = 0                                                  # nrot
        rc, msg = call([300.0], 1, True, True, True, args=a)
        assert rc == -1 and "nrot" in msg
        a = list(args)
        a[2] = None                                               # recip without its coulomb grid's partner
        rc, msg = call([300.0], 1, True, True, True, args=a)
        assert rc == -1 and "recip" in msg
        assert np.all(mean == -7.0) and np.all(mn == -7.0) and np.all(amin == -7)
        # and the same buffers through a good call
        rc, msg = call([300.0], 1, True, True, True)
        assert rc == 0, msg
        assert np.all(mean[:points] != -7.0) and np.all(mean[points:] == -7.0) and np.all(mn != -7.0) and np.all(amin >= 0)
        del keep
        with pytest.raises(ValueError):
            gs.energy_grid_reduced(2.5, _seven_rotations(), (300.0,), weights=np.ones(3))       # 3 weights for 7 rotations
    finally:
        gs.close()
