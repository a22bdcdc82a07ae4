"""``ceg_energy_grid`` (energy_grid for polyatomic guests, all rotations in one device pass): what can be checked without a GPU --
the symbol at the three descriptions of the boundary, argument checking before any device call, the host mirror of the
reference's rotation matrices, and the factorisation of the reciprocal term that the kernel implements, restated in numpy."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from ceg_hip.hostmirror.ewald import ewald_context_constants

ROOT = Path(__file__).resolve().parent.parent


def test_entry_point_is_exported_declared_and_bound():
    header = (ROOT / "include" / "ceg_hip.h").read_text()
    assert re.search(r"CEG_API\s+int\s+ceg_energy_grid\s*\(", header)
    assert "ceg_energy_grid" in _abi.PROTOTYPES
    lib = _abi.load_library()
    assert hasattr(lib, "ceg_energy_grid")
    assert lib.ceg_abi_version() == 1                       # functions are only added
    julia = (ROOT / "crystalenergygrids.jl_amd" / "julia" / "CEGHip.jl").read_text()
    assert "(:ceg_energy_grid, LIB[])" in julia and "function energy_grid(setup::CEG.CrystalEnergySetup, step, num_rotate=40)" in julia


def _call(lib, *, natoms=3, nrot=2, out="buffer", coulomb=None, recip=None, num=(2, 3, 4)):
    n = max(natoms, 1)
    handles = (C.c_void_p * n)(*([None] * n))                # zero grids: valid, and all a GPU-less box can offer
    base = np.zeros(3 * n)
    q = np.zeros(n)
    rot = np.tile(np.eye(3).reshape(-1), max(nrot, 1))
    steps = np.ascontiguousarray(np.eye(3).reshape(-1) * 0.5)
    numv = np.array(num, dtype=np.int32)
    buf = np.empty(max(nrot, 1) * int(np.prod(num)))
    return lib.ceg_energy_grid(handles, coulomb, recip, _abi.dptr(base), _abi.dptr(q), natoms, _abi.dptr(rot), nrot, _abi.dptr(steps),
                               _abi.i32ptr(numv), None, None, None, None, None, None, 0.0, 0.0,
                               buf.ctypes.data if out == "buffer" else None, 0, None)


def test_arguments_are_checked_before_any_device_call():
    lib = _abi.load_library()
    assert _call(lib, out=None) == -1 and b"out" in lib.ceg_last_error()
    assert _call(lib, nrot=0) == -1 and b"nrot" in lib.ceg_last_error()
    assert _call(lib, natoms=17) == -5 and b"16" in lib.ceg_last_error()
    assert _call(lib, natoms=0) == -1
    assert _call(lib, num=(2, 0, 4)) == -1
    # recip without coulomb_grid: the handle is never dereferenced (any non-NULL address will do)
    dummy = np.zeros(64)
    assert _call(lib, recip=dummy.ctypes.data) == -1 and b"both" in lib.ceg_last_error()
    assert _call(lib, coulomb=dummy.ctypes.data) == -1
    if lib.ceg_device_count() > 0:
        return
    # well-formed arguments, no device: a loud failure, never a CPU result
    assert _call(lib) == -2 and b"no HIP device" in lib.ceg_last_error()


def test_rotation_matrices_restate_lebedev_jl():
    from ceg_hip.hostmirror.lebedev import rotation_matrices
    rotm = np.array([[-0.17963068200890037, -0.21953827352603253, -0.9589242746631385],
                     [-0.9599246581752935, 0.25228151379218244, 0.12206018362173197],
                     [0.21512198564550156, 0.9424208106021077, -0.2560577025515984]])          # lebedev.jl:4
    pts = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [1.0, 2.0, -2.0] / np.float64(3.0)])
    for islinear, nz in ((True, 1), (False, 5)):
        got = rotation_matrices(pts, islinear)
        assert got.shape == (nz * 3, 3, 3)
        for i in range(nz):
            th = 2.0 * np.pi * i / 5.0
            for j, p in enumerate(pts):
                v = rotm @ p                                                                   # :29
                # hcat(e1, e2, v) * zrot (:117-120), written out entry by entry
                want = np.array([[np.cos(th), -np.sin(th), v[0]],
                                 [np.sin(th), np.cos(th), v[1]],
                                 [0.0, 0.0, v[2]]])
                # the angle 2 pi i / 5 <= 5.03 written out here carries up to three roundings of 8.9e-16 (one ulp at 5) before
                # cos / sin see it; the mirror reduces the argument first, like Julia's cospi / sinpi
                assert np.allclose(got[i * 3 + j], want, rtol=0, atol=4e-15), (islinear, i, j)
    assert np.array_equal(rotation_matrices(pts, True), rotation_matrices(pts, False)[:3])        # i = 0: zrot = 1 exactly


def test_factorised_reciprocal_term_equals_the_per_placement_sum(oracle):
    """The kernel's formulation as a specification: S(k; o, R) = P_o(k) T_R(k) with P_o = PA[iA] PB[iB] PC[iC], hence
    E = 2 (sum_k Re(W_o T_R) + enc) + sum_k kf |T_R|^2 + static, W_o = kf conj(S_f) P_o -- against the oracle's compute_ewald on the
    explicit positions, to the tolerance of test_reciprocal_batch_vs_oracle."""
    from ceg_hip.hostmirror.lebedev import rotation_matrices
    fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021")
    ef = ceg.initialize_ewald(fw)
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", "BoulfelfelSholl2021")
    base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(co2.atomic_charge, dtype=np.float64)
    rng = np.random.default_rng(11)
    u = rng.normal(size=(4, 3))
    rots = np.concatenate([np.eye(3)[None], rotation_matrices(u / np.linalg.norm(u, axis=1)[:, None], True)])      # 5 rotations
    num = (4, 3, 5)
    steps = [fw.mat[:, a] / num[a] for a in range(3)]
    ijk = np.asarray(ef.kvec_ijk, dtype=np.float64)
    kf = np.asarray(ef.kfactors)
    sf = np.asarray(ef.StoreRigidChargeFramework)
    inv = np.asarray(ef.invmat)
    enc, static = ewald_context_constants(ef, ((co2,),))
    # the three phase tables and T_R
    tabs = [np.exp(2j * np.pi * np.arange(num[a])[:, None] * (ijk @ (inv @ steps[a]))[None, :]) for a in range(3)]
    rp = np.einsum("rij,aj->rai", rots, base)                                          # [rot, atom, 3]
    T = (q[None, :, None] * np.exp(2j * np.pi * np.einsum("rai,ki->rak", rp @ inv.T, ijk))).sum(axis=1)         # [rot, nk]
    selfterm = (kf[None] * np.abs(T) ** 2).sum(axis=1)
    got = np.empty((len(rots),) + num)
    pos = np.empty((len(rots),) + num + (len(base), 3))
    for iA in range(num[0]):
        for iB in range(num[1]):
            for iC in range(num[2]):
                W = kf * np.conj(sf) * tabs[0][iA] * tabs[1][iB] * tabs[2][iC]
                cross = (W[None] * T).real.sum(axis=1)
                got[:, iA, iB, iC] = 2.0 * (cross + enc) + selfterm + static
                pos[:, iA, iB, iC] = (iA * steps[0] + iB * steps[1] + iC * steps[2])[None, None] + rp
    ref = oracle.reciprocal_energies(ef, co2, pos.reshape(-1, len(base), 3)).reshape(got.shape)
    assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-11 * np.abs(ref).max()), np.abs(got - ref).max()
