"""The reciprocal Ewald kernel k_recip<C_IN_LDS, WAVES> (csrc/ceg_recip.hip) over every launch shape and k-space edge, against the
longdouble reference of ``tests/recip_cases.py`` within its derived bound; ``tests/test_recip_cases_host.py`` checks the cases, the
reference and the bound on the CPU.

What runs here (asserted through ``ceg_recip_launch_shape``):
  * all eight instantiations -- <true, 8 / 4 / 2 / 1> and <false, 8 / 4 / 2 / 1> -- at n = 517 (per_wave = 1, ragged last workgroup);
  * <true, W> with per_wave = 2, 4 and 8 for every W, at n = 2048 per_wave W + r with a partial and (W > 1) an empty wave in the last
    workgroup: bit for bit the per_wave = 1 result of the same positions in chunks, which is compared with the reference;
  * k-space edges (no k-vector, one, an axis with ks = 0, one long row, exactly 64 / 65 / 128 / 129 segments, holes + duplicates +
    shuffled order, the 400-entry box, tables of exactly 64 KiB, dynamic LDS within 3200 bytes of 64 KiB), geometry edges (rint
    ties, +-1e4 A, coincident atoms, zero and net charges) and the routes (reused I/O buffers, a non-default stream, a replaced
    structure factor, the ReciprocalEwald wrapper on the CHA fixture).

Measured on an MI355X, worst |got - reference| / bound per group (the float64 emulation on the CPU predicted about 0.003):
  variant matrix at per_wave = 1 (eight instantiations)      0.0041   (<true, 8>; <false, *> 0.0004 to 0.0012)
  per_wave = 2, 4, 8 on <true, 8 / 4 / 2 / 1>                0.0051   (<true, 8>, per_wave = 4; every batch bit-identical to per_wave = 1)
  k-space edges                                              0.058    (one row of 21 consecutive i, 2 atoms; an axis with ks = 0: 0.013 to
                                                                       0.031; 64 / 65 / 128 / 129 segments 0.004 to 0.009; 400-entry box 0.016)
  LDS edges (tables of 64 KiB, dynamic LDS 63872 / 65024 B)  0.0089   (launched and correct: no refusal above 64 KiB in all)
  geometry and charges                                       0.0048   (+-1e4 A; rint ties 0.0003)
  routes                                                     0.0041
The edges with a handful of k-vectors sit higher than the many-vector cases because fewer terms average out under the same
worst-case bound; nothing came near 1.  Nothing was found wrong in the kernel: no fix was needed.
"""
import ctypes as C

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi

import recip_cases as RC

pytestmark = pytest.mark.gpu

CELL = RC.general_cell()
ENC, STATIC = -7.5, 123.25
LDS_VARIANTS = [v for v in sorted(RC.VARIANTS) if RC.VARIANTS[v][3][0]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check(h, q, pos, got, idx, what, enc=ENC, static=STATIC, sf=None):
    """|got - reference| <= bound at the placements ``idx``; prints the worst ratio."""
    pos = np.asarray(pos).reshape(-1, len(q), 3)
    ref = h.reference(q, pos[idx], enc, static, sf=sf)
    tol = h.bound(q, pos[idx], enc, static, sf=sf)
    err = np.abs(got[idx].astype(RC.LD) - ref).astype(np.float64)
    assert np.all(np.isfinite(got[idx]))
    worst = float((err / tol).max()) if np.all(tol > 0) else (0.0 if np.all(err == 0) else np.inf)
    print(f"recip-ratio {what}: worst |got - ref| / bound = {worst:.5f} over {len(idx)} placements")
    assert np.all(err <= tol), (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------ a. the variant matrix
@pytest.mark.parametrize("name", sorted(RC.VARIANTS))
def test_every_instantiation_one_placement_per_wave(hip_lib, name):
    _ks, _rho, natoms, (c_in_lds, waves) = RC.VARIANTS[name]
    k = RC.variant_kset(name)
    n = RC.N_RAGGED
    assert RC.launch_shape(k, natoms, n)[:3] == (waves, c_in_lds, 1)
    q, model = RC.molecule(natoms, natoms)
    pos = RC.placements(model, n, natoms)
    h = RC.Handle(k, CELL)
    try:
        got = h.energies(q, pos, ENC, STATIC)
        # which wave and workgroup evaluates a placement does not enter its arithmetic
        assert np.array_equal(bits(got), bits(h.energies_chunked(q, pos, 259, ENC, STATIC)))
        check(h, q, pos, got, RC.check_subset(n, 1, waves), f"variants {name} n={n}")
    finally:
        h.close()


@pytest.mark.parametrize("per_wave", [2, 4, 8])
@pytest.mark.parametrize("name", LDS_VARIANTS)
def test_several_placements_per_wave(hip_lib, name, per_wave):
    """The loop over the placements of a wave: the `next` prefetch, the p1 clamp, a partial and an empty range in the last
    workgroup.  The arithmetic of a placement does not depend on per_wave or on the wave that runs it, so the big batch must equal
    the same positions evaluated in chunks small enough for per_wave = 1, bit for bit: a difference is state carried between
    placements."""
    _ks, _rho, natoms, (c_in_lds, waves) = RC.VARIANTS[name]
    k = RC.variant_kset(name)
    n = RC.big_n(per_wave, waves)
    chunk = RC.per_wave_one_chunk(waves)
    assert RC.launch_shape(k, natoms, n)[:3] == (waves, True, per_wave) and RC.launch_shape(k, natoms, chunk)[:3] == (waves, True, 1)
    q, model = RC.molecule(natoms, natoms)
    pos = RC.placements(model, n, 10 * natoms + per_wave)
    h = RC.Handle(k, CELL)
    try:
        big = h.energies(q, pos, ENC, STATIC)
        small = h.energies_chunked(q, pos, chunk, ENC, STATIC)
        differ = np.nonzero(bits(big) != bits(small))[0]
        assert len(differ) == 0, (name, per_wave, len(differ), differ[:8], differ[-8:])
        check(h, q, pos, small, RC.check_subset(n, per_wave, waves), f"per_wave {name} per_wave={per_wave} n={n}")
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ b. k-space edges
EDGES = RC.edge_ksets()
N_EDGE = 130


@pytest.mark.parametrize("natoms", [2, 5])
@pytest.mark.parametrize("name", sorted(n for n in EDGES if n != "tab-64k"))
def test_kspace_edges(hip_lib, name, natoms):
    k = EDGES[name]
    if name.startswith("seg"):
        nseg = int(name[3:])
        nr, _ns, got_seg = RC.layout(k)
        assert got_seg == nseg and nr == (nseg + 63) // 64          # 65 and 129: an odd / even last round with one segment in it
    q, model = RC.molecule(natoms, 3)
    pos = RC.placements(model, N_EDGE, natoms)
    h = RC.Handle(k, CELL)
    try:
        got = h.energies(q, pos, ENC, STATIC)
        if k.nk == 0:
            assert np.array_equal(bits(got), bits(np.full(N_EDGE, 2.0 * ENC + STATIC)))
        check(h, q, pos, got, np.arange(N_EDGE), f"edges {name} natoms={natoms}")
    finally:
        h.close()


@pytest.mark.parametrize("natoms", [1, 4])
def test_largest_kspace_box(hip_lib, natoms):
    """ks = (133, 66, 66): stride 400, i0 up to 133 and j + ky, k + kz up to 132 in the nine-bit fields of the descriptors."""
    k = RC.box400()
    assert k.stride == 400 and RC.launch_shape(k, natoms, N_EDGE)[0] == (4 if natoms == 1 else 1)
    q, model = RC.molecule(natoms, 4)
    pos = RC.placements(model, N_EDGE, natoms)
    h = RC.Handle(k, CELL)
    try:
        check(h, q, pos, h.energies(q, pos, ENC, STATIC), np.arange(N_EDGE), f"edges box400 natoms={natoms}")
        # natoms x stride > 4096: one wave's tables pass 64 KiB -- refused, nothing written
        q11 = np.ones(11)
        out = np.full(3, np.nan)
        rc = hip_lib.ceg_recip_energy(h.h, _abi.dptr(np.zeros(3 * 11 * 3)), _abi.dptr(q11), 11, 3, 0.0, 0.0, _abi.dptr(out))
        assert rc == -5 and b"LDS" in hip_lib.ceg_last_error() and np.all(np.isnan(out))
    finally:
        h.close()


def test_tables_of_exactly_64_kib(hip_lib):
    """16 atoms x stride 256: the tables of the single wave fill 64 KiB of dynamic LDS exactly (the constants stay in global
    memory), beside the kernel's 3200 bytes of static LDS."""
    k = EDGES["tab-64k"]
    assert RC.launch_shape(k, 16, N_EDGE) == (1, False, 1, 65536)
    q, model = RC.molecule(16, 5)
    pos = RC.placements(model, N_EDGE, 16)
    h = RC.Handle(k, CELL)
    try:
        check(h, q, pos, h.energies(q, pos, ENC, STATIC), np.arange(N_EDGE), "lds tab-64k natoms=16")
    finally:
        h.close()


@pytest.mark.parametrize("natoms", [2, 5])
def test_dynamic_lds_within_the_static_arrays_of_64_kib(hip_lib, natoms):
    """tab_bytes + c_bytes in (64 KiB - 3200, 64 KiB]: the budget of the launch leaves the kernel's static LDS (s_pos, s_q) out, so
    the workgroup asks for more than 64 KiB in all.  gfx950 has 160 KiB per CU: the launch succeeds and the energies are right."""
    k = RC.window_kset(natoms)
    waves, c_in_lds, _pw, lds = RC.launch_shape(k, natoms, N_EDGE)
    assert c_in_lds and 65536 - RC.LDS_STATIC < lds <= 65536 < lds + RC.LDS_STATIC
    q, model = RC.molecule(natoms, 6)
    pos = RC.placements(model, N_EDGE, natoms)
    h = RC.Handle(k, CELL)
    try:
        check(h, q, pos, h.energies(q, pos, ENC, STATIC), np.arange(N_EDGE), f"lds window natoms={natoms} lds={lds}")
    finally:
        h.close()


def test_refusals(hip_lib):
    k = EDGES["nk1"]
    h = RC.Handle(k, CELL)
    try:
        out = np.full(2, np.nan)
        p = np.zeros(2 * 17 * 3)
        assert hip_lib.ceg_recip_energy(h.h, _abi.dptr(p), _abi.dptr(np.ones(17)), 0, 2, 0.0, 0.0, _abi.dptr(out)) == -1
        assert hip_lib.ceg_recip_energy(h.h, _abi.dptr(p), _abi.dptr(np.ones(17)), 17, 2, 0.0, 0.0, _abi.dptr(out)) == -5
        assert hip_lib.ceg_recip_energy_device(h.h, None, _abi.dptr(np.ones(17)), 17, 0, 0.0, 0.0, None, None) == -5
        assert hip_lib.ceg_recip_energy_device(h.h, None, _abi.dptr(np.ones(17)), 0, 0, 0.0, 0.0, None, None) == -1
        assert np.all(np.isnan(out))
    finally:
        h.close()
    # stride 401
    big = RC.with_constants((134, 66, 66), [[1, 0, 0]], 1)
    hh = C.c_void_p()
    z = np.zeros(1)
    rc = hip_lib.ceg_recip_create(C.byref(hh), 0, _abi.i32ptr(np.ascontiguousarray(big.ijk.reshape(-1))), _abi.dptr(big.kf), _abi.dptr(z), _abi.dptr(z), 1,
                                  _abi.i32ptr(big.ks), _abi.dptr(RC.colmajor(CELL)))
    assert rc == -5 and not hh.value


# ------------------------------------------------------------------------------------------------ c. geometry and charges
def test_geometry_and_charges(hip_lib):
    k = RC.variant_kset("lds-8")
    assert np.all(CELL != 0.0)                                       # a rotated general cell: nine non-zero entries
    h = RC.Handle(k, CELL)
    try:
        q, model = RC.molecule(3, 7)
        # far placements: the bound scales with them
        far = RC.placements(model, 96, 1, spread=1e4)
        tol_near, tol_far = h.bound(q, RC.placements(model, 96, 1), ENC, STATIC), h.bound(q, far, ENC, STATIC)
        assert np.median(tol_far) > 50 * np.median(tol_near)
        check(h, q, far, h.energies(q, far, ENC, STATIC), np.arange(96), "geometry far +-1e4")
        # coincident atoms
        co = RC.placements(np.array([model[0], model[0], model[2]]), 64, 2)
        check(h, q, co, h.energies(q, co, ENC, STATIC), np.arange(64), "geometry coincident atoms")
        # one zero charge, a net charge
        qn = np.array([0.0, 0.8, 0.5])
        pos = RC.placements(model, 64, 3)
        got = h.energies(qn, pos, ENC, STATIC)
        check(h, qn, pos, got, np.arange(64), "geometry zero + net charge")
        # all charges zero: every term is an exact zero
        got = h.energies(np.zeros(3), pos, ENC, STATIC)
        assert np.array_equal(bits(got), bits(np.full(64, 2.0 * ENC + STATIC)))
        # one placement
        one = h.energies(q, pos[:1], ENC, STATIC)
        assert one.shape == (1,) and bits(one)[0] == bits(h.energies(q, pos, ENC, STATIC))[0]
        check(h, q, pos[:1], one, np.arange(1), "geometry n=1")
    finally:
        h.close()


def test_atoms_on_lattice_and_half_lattice_points(hip_lib):
    """A cell with power-of-two edges (32, 16, 64 A): atoms at multiples of half an edge have fractional coordinates that are
    half-integers exactly, so rint sees ties in f and again in m f."""
    inv = np.diag([1.0 / 32.0, 1.0 / 16.0, 1.0 / 64.0])
    k = RC.variant_kset("lds-8")
    h = RC.Handle(k, inv)
    try:
        rng = np.random.default_rng(12)
        half = rng.integers(-9, 10, (96, 3, 3)).astype(np.float64)              # in units of half an edge
        half[0] = 0.0                                                            # all three atoms on the origin
        half[1] = [[1, 1, 1], [-1, -1, -1], [3, -5, 7]]
        pos = half * np.array([16.0, 8.0, 32.0])
        f = pos @ inv.T
        assert np.all(f * 2 == np.rint(f * 2)) and np.any(f != np.rint(f))
        q, _model = RC.molecule(3, 8)
        check(h, q, pos, h.energies(q, pos, ENC, STATIC), np.arange(96), "geometry lattice and half-lattice points")
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ d. routes
def test_host_route_reuses_its_buffers(hip_lib):
    """ceg_recip_energy keeps its device buffers between calls and only grows them: n = 5, 40000, 3 on ONE handle, each equal to
    what a fresh handle returns."""
    k = RC.variant_kset("lds-8")
    q, model = RC.molecule(3, 9)
    h = RC.Handle(k, CELL)
    try:
        for n in (5, 40000, 3):
            pos = RC.placements(model, n, n)
            got = h.energies(q, pos, ENC, STATIC)
            fresh = RC.Handle(k, CELL)
            try:
                assert np.array_equal(bits(got), bits(fresh.energies(q, pos, ENC, STATIC))), n
            finally:
                fresh.close()
            idx = RC.check_subset(n, 1, 8)
            check(h, q, pos, got, idx, f"routes host buffers n={n}")
    finally:
        h.close()


@pytest.mark.parametrize("n", [RC.N_RAGGED, RC.big_n(2, 8)])
def test_device_route_on_a_non_default_stream(hip_lib, n):
    import torch
    k = RC.variant_kset("lds-8")
    q, model = RC.molecule(3, 10)
    pos = RC.placements(model, n, 77)
    h = RC.Handle(k, CELL)
    try:
        host = h.energies(q, pos, ENC, STATIC)
        d_pos = torch.from_numpy(np.ascontiguousarray(pos.reshape(-1))).to("cuda:0")
        d_out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0")
        assert s.cuda_stream != 0
        h.energies_device(q, d_pos.data_ptr(), n, d_out.data_ptr(), ENC, STATIC, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(host))
    finally:
        h.close()


def test_replaced_structure_factor_then_eight_placements_per_wave(hip_lib):
    k = RC.variant_kset("lds-8")
    n = RC.big_n(8, 8)
    q, model = RC.molecule(3, 11)
    pos = RC.placements(model, n, 78)
    _kf, sf2 = RC.constants(k.nk, np.random.default_rng(99))
    h = RC.Handle(k, CELL)
    try:
        before = h.energies(q, pos[:64], 0.0, 0.0)
        h.set_structure_factor(sf2)
        got = h.energies(q, pos, 0.0, 0.0)
        assert not np.array_equal(bits(got[:64]), bits(before))
        check(h, q, pos, got, RC.check_subset(n, 8, 8), "routes replaced structure factor per_wave=8", 0.0, 0.0, sf=sf2)
        fresh = RC.Handle(RC.KSet(k.ks, k.ijk, k.kf, sf2), CELL)
        try:
            assert np.array_equal(bits(got), bits(fresh.energies(q, pos, 0.0, 0.0)))
        finally:
            fresh.close()
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ e. the wrapper on a fixture
@pytest.mark.parametrize("molname", ["Na", "CO2"])
def test_wrapper_on_the_cha_fixture_at_eight_placements_per_wave(hip_lib, oracle, molname):
    from ceg_hip.energy import ReciprocalEwald
    fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021")
    ef = ceg.initialize_ewald(fw, (1, 1, 1))
    mol = ceg.load_molecule_RASPA(molname, "TraPPE", "BoulfelfelSholl2021")
    base = np.asarray(mol.position, dtype=np.float64).reshape(-1, 3)
    n = RC.big_n(8, 8)
    chunk = RC.per_wave_one_chunk(8)
    pos = np.random.default_rng(31).uniform(-40, 60, (n, 1, 3)) + base[None]
    rec = ReciprocalEwald(ef)
    try:
        assert rec.launch_shape(len(base), n)[:3] == (8, True, 8) and rec.launch_shape(len(base), chunk)[:3] == (8, True, 1)
        got = rec.energies(mol, pos)
        small = np.concatenate([rec.energies(mol, pos[b:b + chunk]) for b in range(0, n, chunk)])
        assert np.array_equal(bits(got), bits(small))
        for part in (slice(0, 4096), slice(n - 4096, n)):
            ref = oracle.reciprocal_energies(ef, mol, pos[part])
            assert np.all(np.abs(got[part] - ref) <= 1e-10 * np.abs(ref) + 1e-11 * np.abs(ref).max()), (molname, part)
    finally:
        rec.close()
