"""``ceg_energy_grid`` on the GPU: energy_grid (src/grids.jl:346-424) of a polyatomic guest, every rotation and lattice point in one
device pass.  The expected value of EVERY element is composed from the oracle -- explicit positions generated here in numpy,
``oracle.interpolate_points`` per atom and grid, ``oracle.reciprocal_energies`` per placement, blocking by ``setup.block[...]`` --
and compared with

    |got - ref| <= 1e-9 (|vdw_ref| + |direct_ref| + |recip_ref|) + 1e-11 max|recip_ref|

(the tolerances of test_interpolation_batch_vs_oracle and test_reciprocal_batch_vs_oracle applied to the oracle's own term
magnitudes); elements the oracle gives as blocked must be 1e100 exactly."""
import ctypes as C
import dataclasses
import math
import os
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from ceg_hip.hostmirror.lebedev import rotation_matrices

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
FF = "BoulfelfelSholl2021"


@pytest.fixture(scope="module")
def raspa_dir(tmp_path_factory):
    """setup_RASPA writes its .grid files next to the structures: work on links in a scratch directory."""
    raspa = tmp_path_factory.mktemp("egrid") / "raspa"
    raspa.mkdir()
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(GOLDEN / "raspa" / sub, raspa / sub)
    ceg.setdir_RASPA(raspa)
    yield raspa
    ceg.setdir_RASPA(GOLDEN / "raspa")


@pytest.fixture(scope="module")
def setups(hip_lib, raspa_dir):
    cache = {}

    def get(framework, molecule):
        if (framework, molecule) not in cache:
            cache[framework, molecule] = ceg.setup_RASPA(framework, FF, molecule, "TraPPE")
        return cache[framework, molecule]
    return get


def _seven_rotations():
    """identity, four matrices of rotation_matrices (not orthogonal, as the reference's are not), a generic rotation, a reflection"""
    rng = np.random.default_rng(2024)
    u = rng.normal(size=(4, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(qm) < 0:
        qm[:, 0] = -qm[:, 0]
    refl = qm @ np.diag([1.0, 1.0, -1.0])
    return np.concatenate([np.eye(3)[None], rotation_matrices(u, True), qm[None], refl[None]])


def _lattice(mat, step):
    num = tuple(int(math.floor(np.linalg.norm(mat[:, a]) / step)) + 1 for a in range(3))
    return num, [mat[:, a] / num[a] for a in range(3)]


def _positions(base, rots, num, steps):
    """[nrot, numA, numB, numC, natoms, 3] in the operation order of grids.jl:389, :396, :409 (no fused multiply-adds)"""
    rots = np.asarray(rots, dtype=np.float64)
    rp = (rots[:, None, :, 0] * base[None, :, None, 0] + rots[:, None, :, 1] * base[None, :, None, 1]) + rots[:, None, :, 2] * base[None, :, None, 2]
    iA, iB, iC = np.meshgrid(np.arange(num[0]), np.arange(num[1]), np.arange(num[2]), indexing="ij")
    ofs = (iA[..., None] * steps[0] + iB[..., None] * steps[1]) + iC[..., None] * steps[2]
    return ofs[None, :, :, :, None, :] + rp[:, None, None, None, :, :]


def _oracle_terms(oracle, pos, vdw_grids, coulomb, charges, ef, molecule, block, enc_static=None):
    """-> (blocked, vdw, direct, recip), each [nrot, numA, numB, numC]"""
    shape, natoms = pos.shape[:4], pos.shape[4]
    flat = pos.reshape(-1, natoms, 3)
    vdw = np.zeros(len(flat))
    for a in range(natoms):
        if vdw_grids[a] is not None:
            v = oracle.interpolate_points(vdw_grids[a], flat[:, a])
            vdw = v if a == 0 else vdw + v
    direct = np.zeros(len(flat))
    recip = np.zeros(len(flat))
    if coulomb is not None:
        for a in range(natoms):
            d = charges[a] * oracle.interpolate_points(coulomb, flat[:, a])
            direct = d if a == 0 else direct + d
        recip = oracle.reciprocal_energies(ef, molecule, flat)
    blocked = np.zeros(len(flat), dtype=bool)
    if block is not None and not block.empty:
        blocked = np.array([any(block[p] for p in mol) for mol in flat])
    return blocked.reshape(shape), vdw.reshape(shape), direct.reshape(shape), recip.reshape(shape)


def _assert_matches(got, blocked, vdw, direct, recip, what):
    assert got.shape == blocked.shape, what
    assert np.all(got[blocked] == 1e100), f"{what}: blocked elements must be 1e100 exactly"
    ok = ~blocked
    ref = vdw + (direct + recip)
    tol = 1e-9 * (np.abs(vdw) + np.abs(direct) + np.abs(recip)) + 1e-11 * (np.abs(recip[ok]).max() if ok.any() else 0.0)
    err = np.abs(got - ref)
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.where(ok, err / tol, 0.0))
    print(f"  {what}: {ok.sum()} free + {blocked.sum()} blocked elements, worst |got - ref| / tolerance = {worst:.3g}")
    assert np.all(err[ok] <= tol[ok]), f"{what}: worst |got - ref| / tolerance = {worst:.3g}"


def _setup_terms(oracle, setup, rots, step):
    num, steps = _lattice(setup.framework.mat, step)
    base = np.asarray(setup.molecule.position, dtype=np.float64).reshape(-1, 3)
    pos = _positions(base, rots, num, steps)
    has_c = setup.coulomb.ewald_precision != -math.inf
    grids = [setup.grids[i] if setup.grids[i].ewald_precision == math.inf else None for i in setup.atomsidx]
    return num, _oracle_terms(oracle, pos, grids, setup.coulomb if has_c else None, setup.charges, setup.ewald, setup.molecule, setup.block)


@pytest.mark.parametrize("framework,step,expect_num", [("CIT-7", 0.7, (19, 17, 14)), ("CHA_1.4_3b4eeb96", 1.5, None)])
def test_co2_all_terms_host_and_device_output(hip_lib, oracle, setups, framework, step, expect_num):
    """CO2 in a charged framework: VdW, direct and reciprocal terms, 7 rotations, lattice counts that are no multiples of 16;
    host output and device output (read back through torch) are bit-identical."""
    import torch
    from ceg_hip.energy import GpuEnergySetup
    setup = setups(framework, "CO2")
    rots = _seven_rotations()
    num, terms = _setup_terms(oracle, setup, rots, step)
    if expect_num is not None:
        assert num == expect_num
    assert all(n % 16 for n in num)
    gs = GpuEnergySetup(setup)
    try:
        got = gs.energy_grid_rotations(step, rots)
        assert got.shape == (7,) + num
        d_out = torch.full((num[2], num[1], num[0], 7), float("nan"), dtype=torch.float64, device="cuda:0")
        shape = gs.energy_grid_rotations(step, rots, out_device_ptr=d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert shape == (7,) + num
        dev = d_out.cpu().numpy().transpose(3, 2, 1, 0)
    finally:
        gs.close()
    _assert_matches(got, *terms, f"CO2 in {framework}")
    assert np.array_equal(got, dev, equal_nan=True), "host and device output differ"
    assert (terms[3] != 0.0).all() and (terms[2] != 0.0).any()          # the Coulomb terms are live


def test_single_orientation_agrees_with_the_monoatomic_route(hip_lib, oracle, setups):
    """nrot = 1, identity, Na in CHA: the same numbers as GpuEnergySetup.energy_grid(step) (whose reciprocal term comes from
    ceg_recip_energy: other arithmetic, so the tolerance and not bit identity) and as the host energy_point at the origin."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CHA_1.4_3b4eeb96", "Na")
    num, (blocked, vdw, direct, recip) = _setup_terms(oracle, setup, np.eye(3)[None], 1.5)
    gs = GpuEnergySetup(setup)
    try:
        got = gs.energy_grid_rotations(1.5, np.eye(3)[None])
        old = gs.energy_grid(1.5)
    finally:
        gs.close()
    assert got.shape == (1,) + num and old.shape == num
    _assert_matches(got, blocked, vdw, direct, recip, "Na in CHA vs the oracle")
    tol = 1e-9 * (np.abs(vdw) + np.abs(direct) + np.abs(recip)) + 1e-11 * np.abs(recip).max()
    assert np.all(np.abs(got[0] - old) <= tol[0])
    hv, hc = ceg.energy_point(setup, [[0.0, 0.0, 0.0]])
    assert abs(got[0, 0, 0, 0] - (hv + hc)) <= tol[0, 0, 0, 0]


def test_blocking_spheres_across_a_periodic_boundary(hip_lib, oracle, setups):
    """CO2 in CIT7block: the blocked mask is the host energy_point's on every element, blocked and free elements both occur
    (69 of the 504 identity placements are blocked at this step by the host mirror), free elements carry the oracle's value.

    Lattice points of this test lie ON the cell face a = 0 (the C atom of three orientations at (-2.152, 3.607, 3.808) A among
    them), where the side a point is wrapped to follows from the last bit of invmat * p: the device and the host mirror both sum
    that product like the reference's SMatrix product, left to right without fused multiply-adds."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT7block", "CO2")
    assert not setup.block.empty
    rots = _seven_rotations()[[0, 2, 5]]
    step = 1.5
    num, terms = _setup_terms(oracle, setup, rots, step)
    gs = GpuEnergySetup(setup)
    try:
        got = gs.energy_grid_rotations(step, rots)
    finally:
        gs.close()
    base = np.asarray(setup.molecule.position, dtype=np.float64).reshape(-1, 3)
    pos = _positions(base, rots, num, _lattice(setup.framework.mat, step)[1])
    host = np.array([ceg.energy_point(setup, list(mol)) for mol in pos.reshape(-1, len(base), 3)]).reshape(got.shape + (2,))
    # a blocked placement is (1e100, 0) on the host (grids.jl:313); a free one whose VdW interpolation meets the 5e6 rule is
    # (1e100, coulomb), which sums to 1e100 as well: both are "inaccessible" elements of the reference's grid
    host_blocked = (host[..., 0] == 1e100) & (host[..., 1] == 0.0)
    assert np.array_equal(host_blocked, terms[0])
    print(f"  {host_blocked.sum()} blocked, {((host.sum(axis=-1) == 1e100) & ~host_blocked).sum()} behind the 5e6 rule, "
          f"{(host.sum(axis=-1) != 1e100).sum()} accessible elements")
    assert np.all(got[host_blocked] == 1e100)
    # the elements that carry 1e100 (blocked, or one atom behind the 5e6 rule) are the host's, and so are the inaccessible ones
    assert np.array_equal(got == 1e100, host.sum(axis=-1) == 1e100)
    assert np.array_equal(got >= 1e100, host_blocked | (terms[1] >= 1e100))
    assert host_blocked.any() and (got != 1e100).any()
    _assert_matches(got, *terms, "CO2 in CIT7block")


def _call_abi(lib, handles, coulomb, recip, base, charges, rots, steps, num, enc=0.0, static=0.0):
    natoms, nrot = len(base), len(rots)
    hs = (C.c_void_p * natoms)(*handles)
    rot_cm = np.ascontiguousarray(np.asarray(rots, dtype=np.float64).transpose(0, 2, 1).reshape(-1))
    st = np.ascontiguousarray(np.stack(steps).reshape(-1))
    numv = np.array(num, dtype=np.int32)
    out = np.full(nrot * int(np.prod(num)), np.nan)
    _abi.check(lib, lib.ceg_energy_grid(hs, coulomb, recip, _abi.dptr(np.ascontiguousarray(base).reshape(-1)),
                                        _abi.dptr(np.ascontiguousarray(charges, dtype=np.float64)), natoms, _abi.dptr(rot_cm), nrot,
                                        _abi.dptr(st), _abi.i32ptr(numv), None, None, None, None, None, None, enc, static,
                                        out.ctypes.data, 0, None))
    return out.reshape(num[2], num[1], num[0], nrot).transpose(3, 2, 1, 0)


def test_vdw_only_through_the_c_abi(hip_lib, oracle, setups):
    """coulomb_grid = recip = NULL: the Ar VdW grid of CHA + Na for each of three atoms at CO2's geometry, 5 rotations: the sum of the
    three oracle interpolations; the charges passed along change nothing (Coulomb terms exactly 0)."""
    from ceg_hip.interp import GridInterpolator
    setup = setups("CHA_1.4_3b4eeb96_Na_11812", "Ar")
    g = setup.grids[setup.atomsidx[0]]
    assert g.ewald_precision == math.inf
    base = np.array([[0.0, 0.0, 1.149], [0.0, 0.0, 0.0], [0.0, 0.0, -1.149]])
    rots = _seven_rotations()[:5]
    num, steps = _lattice(setup.framework.mat, 1.5)
    pos = _positions(base, rots, num, steps)
    blocked, vdw, direct, recip = _oracle_terms(oracle, pos, [g, g, g], None, None, None, None, None)
    it = GridInterpolator(g)
    try:
        got = _call_abi(hip_lib, [it._h] * 3, None, None, base, [-0.3256, 0.6512, -0.3256], rots, steps, num)
        again = _call_abi(hip_lib, [it._h] * 3, None, None, base, [0.0, 0.0, 0.0], rots, steps, num)
    finally:
        it.close()
    assert not direct.any() and not recip.any()
    _assert_matches(got, blocked, vdw, direct, recip, "three Ar grids at CO2's geometry")
    assert np.array_equal(got, again)
    assert (vdw >= 1e100).any() and (vdw < 0).any()


def test_slabbed_host_output_is_bit_identical(hip_lib, setups, monkeypatch):
    """CEG_HIP_EGRID_SLAB_BYTES forced down to three iC planes: five slabs for the 14 planes of CIT-7 at 0.7 A, the same bits."""
    from ceg_hip.energy import GpuEnergySetup
    setup = setups("CIT-7", "CO2")
    rots = _seven_rotations()
    gs = GpuEnergySetup(setup)
    try:
        whole = gs.energy_grid_rotations(0.7, rots)
        plane = 8 * 7 * whole.shape[1] * whole.shape[2]
        assert whole.shape[3] == 14
        monkeypatch.setenv("CEG_HIP_EGRID_SLAB_BYTES", str(3 * plane + 100))
        slabs = gs.energy_grid_rotations(0.7, rots)
        monkeypatch.setenv("CEG_HIP_EGRID_SLAB_BYTES", "1")              # below one plane: one plane per slab
        planes = gs.energy_grid_rotations(0.7, rots)
    finally:
        gs.close()
    assert np.array_equal(whole, slabs) and np.array_equal(whole, planes)
    assert np.isfinite(whole).all()


def test_sixteen_atoms_and_the_trilinear_branch(hip_lib, oracle, setups):
    """The atom limit: a 16-atom rigid molecule with random charges on a 5 x 6 x 7 lattice, 3 rotations, its reciprocal term against
    the numpy formula of test_reciprocal_rows_layout_edge_cases (direct term from the oracle, no VdW grids).  Then
    EnergyGrid.higherorder == false on every grid of a small case: the trilinear branch of the interpolant passes through."""
    from ceg_hip.energy import GpuEnergySetup, ReciprocalEwald
    from ceg_hip.interp import GridInterpolator
    setup = setups("CIT-7", "CO2")
    rng = np.random.default_rng(16)
    base = rng.uniform(-3.0, 3.0, (16, 3))
    q = rng.uniform(-1.0, 1.0, 16)
    rots = _seven_rotations()[[0, 3, 6]]
    num = (5, 6, 7)
    steps = [setup.framework.mat[:, a] / num[a] for a in range(3)]
    pos = _positions(base, rots, num, steps)
    ef = setup.ewald
    it, rec = GridInterpolator(setup.coulomb), ReciprocalEwald(ef)
    try:
        got = _call_abi(hip_lib, [None] * 16, it._h, rec._h, base, q, rots, steps, num)
    finally:
        it.close(); rec.close()
    flat = pos.reshape(-1, 16, 3)
    direct = sum(q[a] * oracle.interpolate_points(setup.coulomb, flat[:, a]) for a in range(16)).reshape(got.shape)
    ijk = np.asarray(ef.kvec_ijk, dtype=np.float64)
    kf, sf = np.asarray(ef.kfactors), np.asarray(ef.StoreRigidChargeFramework)
    frac = np.einsum("ij,naj->nai", np.asarray(ef.invmat), flat)
    S = (q[None, :, None] * np.exp(2j * np.pi * np.einsum("nai,ki->nak", frac, ijk))).sum(axis=1)
    want = (2.0 * (kf * (np.conj(sf)[None] * S).real).sum(axis=1) + (kf * np.abs(S) ** 2).sum(axis=1)).reshape(got.shape)
    assert np.all(np.abs((got - direct) - want) <= 1e-9 * np.abs(want).max() + 1e-9 * np.abs(direct))
    # trilinear grids
    flatgrids = [dataclasses.replace(g, higherorder=False) if g.csetup is not None else g for g in setup.grids]
    tri = dataclasses.replace(setup, grids=flatgrids, coulomb=dataclasses.replace(setup.coulomb, higherorder=False))
    rots2 = _seven_rotations()[[0, 5]]
    num2, (blocked, vdw, direct2, recip) = _setup_terms(oracle, tri, rots2, 2.5)
    gs = GpuEnergySetup(tri)
    try:
        got2 = gs.energy_grid_rotations(2.5, rots2)
    finally:
        gs.close()
    nan = np.isnan(vdw) | np.isnan(direct2)                      # an index beyond its axis: BoundsError in Julia, NaN in both here
    assert np.array_equal(np.isnan(got2), nan) and not nan.all()
    keep = ~nan
    _assert_matches(np.where(keep, got2, 0.0), blocked, np.where(keep, vdw, 0.0), np.where(keep, direct2, 0.0), np.where(keep, recip, 0.0),
                    "trilinear grids")
    whole = GpuEnergySetup(setup)
    try:
        assert not np.array_equal(whole.energy_grid_rotations(2.5, rots2), got2, equal_nan=True)      # the branch was taken
    finally:
        whole.close()
