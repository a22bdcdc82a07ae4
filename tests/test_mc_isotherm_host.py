"""The host arithmetic of an isotherm (ceg_hip.mcrng: isotherm_ncycles, accessible_volume, phiPV_div_k, MoveTable.for_gcmc) against
values worked out by hand, in integer or rational arithmetic where possible, and the argument checks of the chain plan's wrapper that
need no device."""
from fractions import Fraction

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from ceg_hip.energy import DeviceMonteCarloGroup


def test_isotherm_ncycles():
    """parameterinputs.jl:319, ceil(Int, ncycles * (1 + 1e3 / P)): 100 Pa runs eleven times the cycles, 1 MPa one in a thousand more"""
    assert mcrng.isotherm_ncycles(1000, 100.0) == 11000
    assert mcrng.isotherm_ncycles(3, 1e5) == 4                      # 3.03 -> 4
    assert [mcrng.isotherm_ncycles(3, p) for p in (500.0, 1000.0, 1e5)] == [9, 6, 4]
    assert mcrng.isotherm_ncycles(1000, 1e6) == 1001 and mcrng.isotherm_ncycles(0, 100.0) == 0
    assert isinstance(mcrng.isotherm_ncycles(5, 250), int) and mcrng.isotherm_ncycles(5, 250) == 25


def test_accessible_volume():
    """gcmc.jl:26-37 on cells whose determinant is an integer: det = 24 (upper triangular 2, 3, 4), 2 x 1 x 3 unit cells, a mask of 64
    points with 16 blocked -> 24 * 6 * 0.75 = 108, every factor exact in FP64"""
    cell = np.array([[2.0, 1.0, 0.5], [0.0, 3.0, 1.0], [0.0, 0.0, 4.0]])
    mask = np.zeros((4, 4, 4), dtype=np.uint8)
    mask[1, :, :] = 1
    assert int(mask.sum()) == 16
    assert mcrng.accessible_volume(mask, cell, (2, 1, 3)) == 108.0
    assert mcrng.accessible_volume(None, cell, (2, 1, 3)) == 144.0 == mcrng.accessible_volume(np.zeros((0,), dtype=np.uint8), cell, (2, 1, 3))
    assert mcrng.accessible_volume(mask.astype(bool), cell, 6) == 108.0
    assert mcrng.accessible_volume(np.ones((2, 2, 2)), cell, (1, 1, 1)) == 0.0
    # a left-handed cell keeps the sign of det, as the reference's det(unitcell) does
    assert mcrng.accessible_volume(None, cell[:, [1, 0, 2]], (1, 1, 1)) == -24.0


def test_phiPV_div_k():
    """simulation.jl:714-715: phi * (|P| V 1e-30 / 1.380649e-23) against the exact rational.  Four roundings and the two decimal
    constants, each within 2^-53 relative: the product within 6 * 2^-53, asserted at 8 * 2^-53."""
    for phi, P, V in ((0.98, 1e5, 2345.5), (1.0, 100.0, 1.0), (0.5, -2.5e6, 31000.0)):
        got = mcrng.phiPV_div_k(phi, P, V)
        exact = Fraction(phi) * abs(Fraction(P)) * Fraction(V) * Fraction(1, 10 ** 30) / Fraction(1380649, 10 ** 29)
        assert abs(Fraction(got) - exact) <= 8 * Fraction(1, 2 ** 53) * exact, (phi, P, V, got, float(exact))
    assert mcrng.phiPV_div_k(1.0, 1e5, 1000.0) == 1e5 * 1000.0 * 1e-30 / 1.380649e-23
    assert 7.2 < mcrng.phiPV_div_k(1.0, 1e5, 1000.0) < 7.3         # 1e-22 J / k = 7.243 K
    assert mcrng.phiPV_div_k(0.9, -1e5, 1000.0) == mcrng.phiPV_div_k(0.9, 1e5, 1000.0)


def test_for_gcmc():
    """parameterinputs.jl:274-279: a table without swap probability gets its cumulatives * 2 / 3 (swap 1/3), any other is kept"""
    mono = mcrng.MoveTable(True)
    assert mono.swap == 0.0
    got = mono.for_gcmc()
    assert got.cumulatives == tuple(c * 2 / 3 for c in (0.5, 0.5, 1.0, 1.0, 1.0)) and abs(got.swap - 1 / 3) < 1e-15
    assert got.cumulatives[2] == 2 / 3 and got.cumulatives[0] == 1 / 3
    poly = mcrng.MoveTable(False).for_gcmc()
    assert poly.cumulatives == (0.33 * 2 / 3, 0.66 * 2 / 3, 0.66 * 2 / 3, 0.66 * 2 / 3, 2 / 3)
    swapping = mcrng.MoveTable(translation=1, rotation=1, swap=2)
    assert swapping.for_gcmc() is swapping
    almost = mcrng.MoveTable(cumulatives=(0.25, 0.5, 0.75, 0.75, 1.0 - 1e-12))           # cumulatives[end] ≈ 1.0: isapprox, not ==
    assert almost.for_gcmc().cumulatives[0] == 0.25 * 2 / 3
    barely = mcrng.MoveTable(cumulatives=(0.25, 0.5, 0.75, 0.75, 1.0 - 1e-6))
    assert barely.for_gcmc() is barely
    assert got.for_gcmc() is got                                    # a second pass changes nothing


def test_chain_plan_arrays():
    """what DeviceMonteCarloGroup.set_chain_plan hands to the library, and what it refuses before any call"""
    arrays = DeviceMonteCarloGroup.chain_plan_arrays
    assert arrays(3) == (None, None)
    phi, stop = arrays(3, [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], [7, 0, 2 ** 62])
    assert phi.dtype == np.float64 and phi.shape == (3, 2) and phi.flags.c_contiguous and phi[2, 1] == 6.0
    assert stop.dtype == np.int64 and stop.tolist() == [7, 0, 2 ** 62]
    assert arrays(2, [1.0, 2.0])[0].shape == (2, 1)                 # one species: one value per chain
    assert arrays(2, np.asfortranarray(np.ones((2, 3))))[0].flags.c_contiguous
    assert arrays(2, None, np.array([1, 2], dtype=np.uint32))[1].dtype == np.int64
    assert arrays(2, None, [5, -1])[1].tolist() == [5, -1]          # (a negative stop is the library's refusal)
    for bad in (dict(phiPV_div_k=[[1.0, 2.0]]), dict(phiPV_div_k=np.ones((2, _abi.GCMC_MAX_SPECIES + 1))), dict(phiPV_div_k=np.ones((2, 0))),
                dict(phiPV_div_k=np.ones((2, 2, 2))), dict(phiPV_div_k=3.0), dict(stop_step=[1, 2, 3]), dict(stop_step=[1.0, 2.0]), dict(stop_step=5),
                dict(stop_step=np.array([1, 2 ** 63], dtype=np.uint64))):
        with pytest.raises(ValueError):
            arrays(2, **bad)
    assert _abi.McChainPlan(2, 0, None, None).nspecies == 2 and "ceg_mc_group_set_chain_plan" in _abi.PROTOTYPES
