"""The device-resident MC state (ceg_mc_*, ceg_mc_group_*, ceg_mc_group_sweep) with rigid molecules of 2 to 16 atoms on every
route: the framework term, the reciprocal term, the structure-factor updates, the bookkeeping of the atom slots, groups and sweeps
-- all of which every other module runs with Na (1 atom) and CO2 (3 atoms) only.  The reference is the ORACLE's state
(oracle/montecarlo.OracleMonteCarlo, generic in the atom count) on the same derived setup.  Run with `pytest -m gpu` on an MI355X.

Species.  The Na + 4 CO2 CIT-7 setup of test_gpu_consumers is built once; setups are derived from it by replacing ffidx, positions
and models.  A synthetic species of m atoms is a compact rigid cluster: atom a has the kind KIND_CYCLE[a % 7] of (O_co2, Na, C_co2)
-- the three kinds with a VdW grid in that setup, so grid pointer and charge vary along the atoms -- at an offset drawn uniformly
in a ball of RADIUS around the site (fixed seed per species).  Sites are the carbon of the fixture's first CO2 and its copies
translated by vectors of the unit cell (the MC cell is its 2x3x3 supercell), which are as open as the original; every molecule is
the cluster turned by a rotation of its own.

LDS of k_mcw_ewald on this fixture (computed by _lds_table from ks, the k-vectors and ceg_recip_layout; asserted in
test_lds_table_of_the_fixture): ks = (7, 9, 8), 1793 k-vectors, stride = 8 + 19 + 17 = 44, nrounds = 5, nslots = 32,
c_bytes = 24*64*32 + 4*320 = 50 432; tables 16 m stride = 704 m bytes per wave; WAVES = the largest of 8/4/2/1 with
c_bytes + WAVES * tables <= 72 KiB:

     m  WAVES  dynamic LDS      m  WAVES  dynamic LDS      m  WAVES  dynamic LDS      m  WAVES  dynamic LDS
     1    8    56 064 B         5    4    64 512 B         9    2    63 104 B        13    2    68 736 B (>64K)
     2    8    61 696 B         6    4    67 328 B (>64K) 10    2    64 512 B        14    2    70 144 B (>64K)
     3    8    67 328 B (>64K)  7    4    70 144 B (>64K) 11    2    65 920 B (>64K) 15    2    71 552 B (>64K)
     4    8    72 960 B (>64K)  8    4    72 960 B (>64K) 12    2    67 328 B (>64K) 16    2    72 960 B (>64K)

No m <= 16 reaches WAVES = 1 on this fixture (it would take tables of more than 11 648 B per wave, m >= 17).  SIZES = (2, 4, 5, 8,
16) reach k_mcw_ewald<., 8> (m = 2, 4), <., 4> (m = 5, 8) and <., 2> (m = 16), i.e. every instantiation some m <= 16 reaches, and
m = 4, 8, 16 launch with 72 960 B of dynamic LDS (+ 3 200 / 1 664 / 896 B static), the largest size the selection can give and above
64 KiB.  (CO2 itself already asks for 67 328 B on this fixture, so test_mc_large_batches_take_the_wave_kernels has been launching
above 64 KiB all along.)

Observed on an MI355X (gfx950):
  * every launch above 64 KiB of dynamic LDS -- 72 960 B with WAVES = 8 (m = 4), 4 (m = 8) and 2 (m = 16) -- was accepted without
    hipFuncSetAttribute and gave rows within 1e-10 of the one-workgroup kernel and within 1e-9 of the oracle; nothing had to be
    changed in the library, and no defect was found at any size on any route.
  * RADIUS = 0.8 A.  The oracle alone was asked first: clusters of 0.25 ... 0.9 A at the sites, turned at random, are open in
    60 of 60 placements for every size, and in 58 to 60 of 60 after a displacement of +-0.35 A, so the radius did not have to
    shrink below a molecule's own size; blocked rows come from the jumps and from one placement per batch put where the framework
    blocks the fixture's third CO2.
  * share of the compared rows that the oracle finds open in all four columns: replay 113, 114, 114, 113, 106 of 120 (m = 2, 4,
    5, 8, 16); routes 9 of 11 displacement rows at every size and 10, 9, 10, 8, 8 of 11 insertion rows; large batch 14 of 15;
    mixed sizes 186 of 204 (both pair loops); group 16 of 18; sweep 308 of 320.  Every case has at least one blocked row.
  * the whole module takes about 2 s, no test more than 0.2 s (the fixture 0.5 s).
"""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi, mcrng
from test_gpu_consumers import _mc_setup, _rotation
from test_gpu_mc_chains import _check, _displace
from test_gpu_mc_sweep import SEED, _device_order, _rule, _same_state, _step_sizes

pytestmark = pytest.mark.gpu

SIZES = (2, 4, 5, 8, 16)
RADIUS = 0.8                     # A: the radius of the ball the atoms of a cluster are drawn in
SUPERCELL = (2, 3, 3)            # the MC cell of _mc_setup in unit cells of CIT-7
KIND_CYCLE = (0, 1, 2, 0, 2, 1, 0)          # index into (O_co2, Na, C_co2); its period 7 divides no size used here
# unit-cell translations of the site: the first two hold CO2, the others the clusters
CO2_CELLS = ((0, 0, 0), (1, 1, 1))
CELLS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 2, 0), (0, 0, 2), (1, 2, 0), (1, 0, 2), (0, 2, 1),
         (0, 1, 2), (1, 2, 1), (1, 1, 2), (0, 2, 2), (1, 2, 2))
MCW_FRAME_ROWS, MCW_WAVES = 4, 4            # csrc/ceg_mc.hip
UNSUPPORTED = -5                            # CEG_ERR_UNSUPPORTED


# ------------------------------------------------------------------ the LDS table of the fixture
def _lds_table(lib, ef):
    """m -> (WAVES, dynamic LDS bytes) of k_mcw_ewald as launch_wave_kernels picks them, and (stride, nrounds, nslots, c_bytes)"""
    ks = np.asarray(ef.kspace.ks, dtype=np.int32)
    ijk = np.ascontiguousarray(ef.kvec_ijk, dtype=np.int32)
    nr, ns = C.c_int32(), C.c_int32()
    assert lib.ceg_recip_layout(_abi.i32ptr(ijk.reshape(-1)), len(ijk), _abi.i32ptr(ks), C.byref(nr), C.byref(ns), None, None) == 0
    stride = int(ks[0] + 1 + 2 * ks[1] + 1 + 2 * ks[2] + 1)
    c_bytes = 24 * 64 * ns.value + 4 * ((64 * nr.value + 3) & ~3)
    table = {}
    for m in range(1, 17):
        waves = 8
        while waves > 1 and c_bytes + waves * 16 * m * stride > 72 * 1024:
            waves >>= 1
        table[m] = (waves, c_bytes + waves * 16 * m * stride)
    return table, (stride, nr.value, ns.value, c_bytes)


LDS_TABLE = {1: (8, 56064), 2: (8, 61696), 3: (8, 67328), 4: (8, 72960), 5: (4, 64512), 6: (4, 67328), 7: (4, 70144), 8: (4, 72960),
             9: (2, 63104), 10: (2, 64512), 11: (2, 65920), 12: (2, 67328), 13: (2, 68736), 14: (2, 70144), 15: (2, 71552), 16: (2, 72960)}


# ------------------------------------------------------------------ species, derived setups, chains
def _kinds3(mc):
    """1-based force-field indices of (O_co2, Na, C_co2) in the fixture"""
    return (mc.ffidx[1][0], mc.ffidx[0][0], mc.ffidx[1][1])


def _species(mc, m, variant=0, radius=None):
    """(ffidx, offsets[m, 3]) of the synthetic m-atom species; `variant` gives another geometry with the same kinds"""
    k3 = _kinds3(mc)
    ids = [k3[KIND_CYCLE[a % 7]] for a in range(m)]
    rng = np.random.default_rng(9000 + 100 * variant + m)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return ids, d * ((RADIUS if radius is None else radius) * rng.uniform(0.0, 1.0, (m, 1)) ** (1.0 / 3.0))


def _site(mc, cell):
    """the carbon of the fixture's first CO2 translated by `cell` unit cells"""
    unit = np.asarray(mc.mat, dtype=np.float64) / np.asarray(SUPERCELL, dtype=np.float64)[None, :]
    return mc.positions[1][0][1] + unit @ np.asarray(cell, dtype=np.float64)


def _place(mc, offsets, cell, rng, shift=0.0):
    """the cluster at the site of `cell`, turned by a rotation of its own (and shifted by up to `shift` A per axis)"""
    return _site(mc, cell) + offsets @ _rotation(rng).T + (rng.uniform(-shift, shift, 3) if shift else 0.0)


def _derive(mc, species, counts, seed, na=1, nco2=2):
    """a setup with the kinds [Na, CO2, species ...]: `na` Na where the fixture has it, `nco2` CO2 at CO2_CELLS, counts[s] molecules of
    species[s] at CELLS in turn"""
    rng = np.random.default_rng(seed)
    out = copy.copy(mc)
    out.ffidx = [list(mc.ffidx[0]), list(mc.ffidx[1])] + [list(ids) for ids, _d in species]
    co2 = mc.positions[1][0]
    positions = [[mc.positions[0][0].copy() for _ in range(na)], [co2 + (_site(mc, c) - co2[1]) for c in CO2_CELLS[:nco2]]]
    cells = iter(CELLS)
    for (ids, d), n in zip(species, counts):
        positions.append([_place(mc, d, next(cells), rng) for _ in range(n)])
    out.positions = positions
    out.models = [np.array(x, dtype=np.float64) for x in mc.models[:2]] + [d.copy() for _ids, d in species]
    out.sums = None
    return out


def _chain(setup, mcd, oracle=True):
    """a DeviceMonteCarlo of the derived setup on the owner's grids, and its oracle"""
    from ceg_hip.energy import DeviceMonteCarlo
    from oracle.montecarlo import OracleMonteCarlo
    _mc, owner = setup
    dev = DeviceMonteCarlo(mcd, grids_from=owner)
    omc = None
    if oracle:
        omc = OracleMonteCarlo.from_setup(mcd)
        omc.compute_ewald()
    return dev, omc


def _is_open(r):
    return bool((np.abs(r) < 1e90).all())


class _Share:
    """rows compared with the oracle: how many, how many open in all four columns (on the ORACLE's values)"""

    def __init__(self):
        self.rows = self.open = 0

    def check(self, row, r, what):
        _check(row, r, what)
        self.rows += 1
        self.open += _is_open(r)

    def finish(self, what):
        print(f"{what}: {self.open} of {self.rows} compared rows open ({self.open / self.rows:.2f})")
        assert 2 * self.open >= self.rows, (what, self.open, self.rows)          # at least half open in all four columns
        assert self.open < self.rows, (what, "no blocked row")                   # at least one blocked


def _sync_host(dev, omc):
    """DeviceMonteCarlo.state counts the atoms in dev.mc.positions: give it the oracle's"""
    dev.mc.positions = [[p.copy() for p in kind] for kind in omc.positions]


def _check_state(dev, omc, what):
    _sync_host(dev, omc)
    pos, sf = dev.state()
    assert np.array_equal(pos, omc.flat_positions()), what
    osf = omc.total_structure_factor()
    assert np.abs(sf - osf).max() <= 1e-9 * np.abs(osf).max(), what


@pytest.fixture(scope="module")
def setup(hip_lib, tmp_path_factory):
    """the Na + 4 CO2 CIT-7 setup, built once for the module; `owner` owns the grid interpolators"""
    from ceg_hip.energy import DeviceMonteCarlo
    try:
        _M, mc = _mc_setup(tmp_path_factory.mktemp("mc_sizes"))
        own = copy.copy(mc)
        own.positions = [[p.copy() for p in kind] for kind in mc.positions]
        owner = DeviceMonteCarlo(own)
        yield mc, owner
        owner.close()
    finally:
        ceg.setdir_RASPA(Path(__file__).parent / "golden" / "raspa")


# ------------------------------------------------------------------ the table
def test_lds_table_of_the_fixture(setup):
    """The table of the module docstring is what the fixture gives, and SIZES reach every k_mcw_ewald instantiation that some
    m <= 16 reaches, the sizes above 64 KiB among them."""
    mc, owner = setup
    table, (stride, nrounds, nslots, c_bytes) = _lds_table(owner._lib, mc.ewald)
    assert (stride, nrounds, nslots, c_bytes) == (44, 5, 32, 50432)
    assert table == LDS_TABLE
    assert {table[m][0] for m in SIZES} == {w for w, _b in table.values()}
    above = [m for m in table if 64 * 1024 < table[m][1] <= 72 * 1024]
    assert above and set(above) & set(SIZES)
    assert max(b for _w, b in table.values()) == max(table[m][1] for m in SIZES)      # the largest launch is among them


# ------------------------------------------------------------------ 1. replay per size
@pytest.mark.parametrize("m", SIZES)
def test_replay_per_size(setup, m):
    """Na + 2 CO2 + 4 molecules of the m-atom species: 60 steps of translation / rotation (about atom m // 2) / jump on one random
    molecule each, ceg_mc_trial with one placement (the three-workgroup split), both rows against the oracle at 1e-9 |ref| + 1e-7 per
    open column and blocked where the oracle is blocked.  Acceptance is energy-independent as in test_mc_replay_1000_moves
    (step % 3 != 0); the jumps sit at steps 3, 9, 15 ... and so are never accepted, except the one of step 51, which is -- with all
    of them accepted two steps in three most molecules would end blocked, and the condition on open rows could not hold.  At the
    end: positions bit-equal, total structure factor to 1e-9, and the same after one ceg_mc_set_guests of the final state."""
    mc, _owner = setup
    mcd = _derive(mc, [_species(mc, m)], [4], seed=10 + m)
    dev, omc = _chain(setup, mcd)
    mols = [(i, j) for i, kind in enumerate(mcd.positions) for j in range(len(kind))]
    rng = np.random.default_rng(2024 + m)
    share = _Share()
    naccept = big = 0
    for step in range(60):
        idx = mols[int(rng.integers(len(mols)))] if step % 2 else (2, int(rng.integers(4)))       # every other step one of the m-atom molecules
        cur = omc.positions[idx[0]][idx[1]]
        jump = step % 6 == 3
        new = cur + (mc.mat @ rng.uniform(-1.5, 1.5, 3) if jump else rng.uniform(-0.35, 0.35, 3))
        if len(cur) > 1 and step % 2 == 0:
            c = new[len(cur) // 2]
            new = c + (new - c) @ _rotation(rng).T
        got = dev.trial(idx, new[None])
        share.check(got[0], omc.movement_energy(idx), (m, step, idx, "before"))
        share.check(got[1], omc.movement_energy(idx, new), (m, step, idx, "after"))
        big += idx[0] == 2
        if step % 3 != 0 or step == 51:
            dev.accept(idx, new)
            omc.update(idx, new)
            naccept += 1
    assert naccept == 41 and big >= 30
    share.finish(f"replay m = {m}")
    _check_state(dev, omc, m)
    dev.refresh()                                                # ceg_mc_set_guests of the final state: k_mc_sf_molecules at size m
    _check_state(dev, omc, (m, "after set_guests"))
    for idx in ((2, 0), (2, 3), (1, 0)):
        _check(dev.trial(idx, np.empty((0, len(mcd.ffidx[idx[0]]), 3)))[0], omc.movement_energy(idx), (m, idx, "after set_guests"))
    dev.close()


# ------------------------------------------------------------------ 2. every trial route
def _routes(monkeypatch, call, split=True):
    """`call` through the wave kernels, one workgroup per row and (split) the three-workgroup split -> the wave rows.  The relations
    are those of test_mc_large_batches_take_the_wave_kernels."""
    monkeypatch.setenv("CEG_HIP_MC_WAVE_MIN", "0")
    wave = call()
    monkeypatch.setenv("CEG_HIP_MC_WAVE_MIN", "1000000000")
    monkeypatch.setenv("CEG_HIP_MC_SPLIT_MAX", "0")
    group = call()                                               # one workgroup per row
    if split:
        monkeypatch.setenv("CEG_HIP_MC_SPLIT_MAX", "1000000000")
        three = call()                                           # the three terms of a row on three workgroups
        assert np.array_equal(three, group, equal_nan=True)      # the same arithmetic in the same order
    monkeypatch.delenv("CEG_HIP_MC_SPLIT_MAX")
    monkeypatch.delenv("CEG_HIP_MC_WAVE_MIN")
    assert np.array_equal(np.abs(wave) >= 1e90, np.abs(group) >= 1e90)
    for c in range(4):
        ok = (np.abs(group[:, c]) < 1e90) & np.isfinite(group[:, c])
        scale = float(np.percentile(np.abs(group[ok, c]), 75)) if ok.any() else 0.0
        err = np.abs(wave[ok, c] - group[ok, c])
        bad = err > 1e-10 * np.abs(group[ok, c]) + 1e-11 * scale + 1e-300
        assert not bad.any(), (c, float(err.max()), scale, wave[ok, c][bad][:4], group[ok, c][bad][:4])
    return wave


def _batches(mc, mcd, omc, rng, n):
    """n displacements of the second m-atom molecule (every fifth a jump anywhere in and beyond the cell, every third turned) and n
    insertion placements of the species (at the sites, turned and shifted; every fifth anywhere); placement 6 of both sits where
    the fixture's third CO2 is blocked"""
    idx = (2, 1)
    cur = omc.positions[2][1]
    m = len(cur)
    disp = _displace(rng, cur, n)
    far = np.arange(n) % 5 == 1
    disp[far] = cur[None] + (rng.uniform(-1.5, 1.5, (int(far.sum()), 3)) @ mc.mat.T)[:, None, :]
    d = mcd.models[2]
    ins = np.array([_place(mc, d, CELLS[4 + int(rng.integers(len(CELLS) - 4))], rng, shift=0.35) for _ in range(n)])     # sites nobody sits at
    ins[far] = (rng.uniform(0.0, 1.0, (int(far.sum()), 3)) @ mc.mat.T)[:, None, :] + d[None]
    wall = mc.positions[1][2][1]                                 # the carbon of the fixture's third CO2, which the framework blocks
    disp[6] = wall + (cur - cur.mean(axis=0))
    ins[6] = wall + d
    return idx, disp.reshape(n, m, 3), ins.reshape(n, m, 3)


@pytest.mark.parametrize("m", SIZES)
def test_trial_routes_per_size(setup, monkeypatch, m):
    """One displacement batch (302 rows) and one insertion batch (301 rows) of the m-atom species through the wave kernels
    (k_mcw_frame, k_mcw_ewald<., WAVES of the table>, k_mcw_pairs*), one workgroup per row and the three-workgroup split: split ==
    one workgroup bit for bit, wave against one workgroup at 1e-10 |value| + 1e-11 of the column's upper quartile; rows 0 ... 7 (the
    stored structure factor; one row per wave of the first workgroup of every wave kernel, which takes one placement per wave at this
    batch size), two in the middle and the last against the oracle.  Neither batch is a multiple of 4 MCW_FRAME_ROWS or of 8 WAVES: the
    last workgroup of each wave kernel is partly filled.  m = 16 also through the device-pointer entry points."""
    mc, owner = setup
    mcd = _derive(mc, [_species(mc, m)], [4], seed=20 + m)
    dev, omc = _chain(setup, mcd)
    rng = np.random.default_rng(404 + m)
    for j in (0, 1, 2):                                           # accepted moves first: sf_tot and sf_mol are device-updated values
        new = _displace(rng, omc.positions[2][j], 1)[0]
        dev.accept((2, j), new); omc.update((2, j), new)
    n = 301
    waves = LDS_TABLE[m][0]
    for rows in (n, n + 1):
        assert rows % (4 * MCW_FRAME_ROWS) and rows % (MCW_WAVES * 8) and rows % (8 * waves)
    idx, disp, ins = _batches(mc, mcd, omc, rng, n)
    sample = [0, 1, 2, 3, 4, 5, 6, 7, 100, 211]
    share = _Share()
    rows = _routes(monkeypatch, lambda: dev.trial(idx, disp))
    assert rows.shape == (n + 1, 4)
    for r in sample + [n]:
        share.check(rows[r], omc.movement_energy(idx) if r == 0 else omc.movement_energy(idx, disp[r - 1]), (m, "displacement", r))
    share.finish(f"routes m = {m}, displacements")
    share = _Share()
    rows_i = _routes(monkeypatch, lambda: dev.trial_insert(2, ins))
    assert rows_i.shape == (n, 4)
    for r in sample + [n - 1]:
        share.check(rows_i[r], omc.insertion_energy(2, ins[r]), (m, "insertion", r))
    share.finish(f"routes m = {m}, insertions")
    if m == 16:
        import torch
        d_trial = torch.tensor(disp, dtype=torch.float64, device="cuda")
        d_rows = torch.full((n + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
        dev.trial_device(idx, d_trial.data_ptr(), n, d_rows.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_allclose(d_rows.cpu().numpy(), rows, rtol=1e-10, atol=1e-7)      # (the device route always takes the wave kernels)
        d_ins = torch.tensor(ins, dtype=torch.float64, device="cuda")
        d_rows_i = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
        dev.trial_insert_device(2, d_ins.data_ptr(), n, d_rows_i.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_allclose(d_rows_i.cpu().numpy(), rows_i, rtol=1e-10, atol=1e-7)
    dev.close()


def test_wave_kernels_with_several_placements_per_wave(setup, monkeypatch):
    """A wave of the wave kernels takes more than one placement only when the batch fills the device (rows / (waves x placements)
    >= 2048): no other test is that large, so the numbering of the corner evaluations THROUGH the placements of a wave in
    k_mcw_frame has only ever seen one placement.  65 613 rows of the 5-atom species: four placements of 80 evaluations per wave of
    k_mcw_frame (five passes of 64, every placement straddling two), eight per wave of k_mcw_ewald<., 4> and of the pair kernel;
    against one workgroup per row on all rows, and against the oracle on a sample."""
    mc, _owner = setup
    m = 5
    mcd = _derive(mc, [_species(mc, m)], [4], seed=25)
    dev, omc = _chain(setup, mcd)
    rng = np.random.default_rng(505)
    n = 65612
    assert (n + 1) // (MCW_WAVES * MCW_FRAME_ROWS) >= 2048 and (n + 1) // (LDS_TABLE[m][0] * 8) >= 2048 and (n + 1) % 32
    idx, disp, _ins = _batches(mc, mcd, omc, rng, 400)
    trial = disp[rng.integers(400, size=n)] + rng.uniform(-0.05, 0.05, (n, 1, 3))
    rows = _routes(monkeypatch, lambda: dev.trial(idx, trial), split=False)
    share = _Share()
    for r in (0, 1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 40000, n - 2, n - 1, n):
        share.check(rows[r], omc.movement_energy(idx) if r == 0 else omc.movement_energy(idx, trial[r - 1]), ("large batch", r))
    share.finish("large batch m = 5")
    dev.close()


# ------------------------------------------------------------------ 3. mixed sizes share the atom slots
@pytest.mark.parametrize("cells", [False, True])
def test_mixed_sizes_share_the_atom_slots(setup, monkeypatch, cells):
    """One chain with species of 1, 2, 3, 5 and 16 atoms (Na, S2, CO2, S5, S16): 120 steps of displacement, displacement,
    removal, insertion in turn.  The atom slots of a removed molecule are kept per size and reused by the next insertion of that size; any
    other insertion appends.  The script starts with: remove a 16-atom molecule, insert a 5- and a 2-atom one (they append behind
    the hole), insert a 16-atom one (it takes the hole), insert another (it appends: the arrays grow); sizes and molecules are
    random after that.  Every index returned by insert / remove equals the oracle's, every trial row (insertion, deletion, before,
    after) agrees with the oracle; at the end positions bit-equal in molecule order and the structure factor to 1e-9.  Once with the
    exhaustive pair loop, once with neighbour cells of 1 A (CEG_HIP_MC_CELLS=1, CEG_HIP_MC_BIN=1): the atoms of a cluster spread over
    several cells, an accepted jump moves all 16 atoms to other cells (32 cell operations, the limit MC_MAX_CELL_OPS)."""
    mc, _owner = setup
    sizes = (2, 5, 16)
    species = [_species(mc, s) for s in sizes]
    mcd = _derive(mc, species, [1, 1, 2], seed=33)
    if cells:
        monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
        monkeypatch.setenv("CEG_HIP_MC_BIN", "1.0")
    dev, omc = _chain(setup, mcd)
    if cells:
        monkeypatch.delenv("CEG_HIP_MC_CELLS")
        monkeypatch.delenv("CEG_HIP_MC_BIN")
    assert (dev.neighbour_cells() is not None) == cells
    rng = np.random.default_rng(77)
    sites = CO2_CELLS + CELLS                                     # insertions may share a site with a molecule: large, finite energies
    share = _Share()
    script = [("remove", 4), ("insert", 3), ("insert", 2), ("insert", 4), ("insert", 4)]
    nins = nrem = naccept = njump = 0
    inserted = {k: 0 for k in range(5)}

    def nmol(kind):
        return len(omc.positions[kind])

    for step in range(120):
        what, kind = script.pop(0) if script else (("insert", "remove", "move", "move")[(step + 1) % 4], int(rng.integers(5)))
        jump = what == "move" and step % 16 == 5                 # steps 5, 21, 37 ...: a 16-atom molecule anywhere in and beyond the cell
        if jump and nmol(4):
            kind = 4
        m = len(mcd.ffidx[kind])
        if what == "insert":
            shape = mcd.models[kind] - mcd.models[kind].mean(axis=0)
            if rng.random() < 0.85:
                at = _site(mc, sites[int(rng.integers(len(sites)))]) + rng.uniform(-0.3, 0.3, 3)
            else:
                at = mc.mat @ rng.uniform(0, 1, 3)
            trials = np.array([at + shape @ _rotation(rng).T for _ in range(3)])
            rows = dev.trial_insert(kind, trials)
            for t in (0, 2):
                share.check(rows[t], omc.insertion_energy(kind, trials[t]), (step, "insert", kind, t))
            assert dev.insert(kind, trials[1]) == omc.add(kind, trials[1]), (step, kind)
            nins += 1
            inserted[kind] += 1
        elif what == "remove":
            if nmol(kind) < 2:
                continue
            j = int(rng.integers(nmol(kind)))
            row = dev.trial((kind, j), np.empty((0, m, 3)))[0]
            share.check(row, omc.movement_energy((kind, j)), (step, "delete", kind, j))
            assert dev.remove((kind, j)) == omc.remove((kind, j)), (step, kind, j)
            nrem += 1
        else:
            if not nmol(kind):
                continue
            j = int(rng.integers(nmol(kind)))
            cur = omc.positions[kind][j]
            new = cur + mc.mat @ rng.uniform(-1.5, 1.5, 3) if jump else _displace(rng, cur, 1)[0]
            got = dev.trial((kind, j), new[None])
            share.check(got[0], omc.movement_energy((kind, j)), (step, "before", kind, j))
            share.check(got[1], omc.movement_energy((kind, j), new), (step, "after", kind, j))
            if step % 3:                                         # energy-independent acceptance pattern
                dev.accept((kind, j), new)
                omc.update((kind, j), new)
                naccept += 1
                njump += jump and m == 16
    assert nins >= 30 and nrem >= 15 and naccept >= 30 and njump >= 3 and all(v > 0 for v in inserted.values()), (nins, nrem, naccept, njump, inserted)
    share.finish(f"mixed sizes, cells {cells}")
    _check_state(dev, omc, cells)
    for kind in range(5):                                        # and every kind still answers from the renumbered slots
        if nmol(kind):
            _check(dev.trial((kind, nmol(kind) - 1), np.empty((0, len(mcd.ffidx[kind]), 3)))[0], omc.movement_energy((kind, nmol(kind) - 1)), kind)
    dev.close()


# ------------------------------------------------------------------ 4. groups and sweeps
def _group_chains(setup, seed):
    """four chains: Na + 2 CO2 + 2 molecules of a large species each -- 5, 8, 16 atoms and 16 atoms of the same kinds in another geometry"""
    mc, _owner = setup
    out = []
    for c, (m, variant) in enumerate(((5, 0), (8, 0), (16, 0), (16, 1))):
        mcd = _derive(mc, [_species(mc, m, variant)], [2], seed=seed + c)
        out.append(_chain(setup, mcd) + (mcd,))
    return [x[0] for x in out], [x[1] for x in out], [x[2] for x in out]


def test_group_trial_and_accept_with_large_molecules(setup):
    """K = 4 chains holding species of 5, 8, 16 and 16 atoms: one ceg_mc_group_trial with a move of the large molecule in every chain
    and one call with 16-atom insertions in two chains, a move and an idle chain, against the single-handle rows (columns 0, 2, 3
    bit-identical, column 1 to 1e-12 relative) and the oracle; one ceg_mc_group_accept, then every chain's state against the oracle."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    devs, omcs, mcds = _group_chains(setup, 40)
    rng = np.random.default_rng(41)
    share = _Share()

    def same(r, single, what):
        assert r.shape == single.shape, what
        for col in (0, 2, 3):
            assert np.array_equal(r[:, col], single[:, col]), (what, col, r, single)
        np.testing.assert_allclose(r[:, 1], single[:, 1], rtol=1e-12, atol=0.0)

    with DeviceMonteCarloGroup(devs) as group:
        trials = [_displace(rng, omcs[c].positions[2][c % 2], 2) for c in range(4)]
        trials[1][1] = omcs[1].positions[2][1] + mc.mat @ rng.uniform(-1.5, 1.5, 3)          # a jump: blocked almost surely
        moves = [("move", (2, c % 2), trials[c]) for c in range(4)]
        rows = group.trial(moves)
        for c in range(4):
            same(rows[c], devs[c].trial((2, c % 2), trials[c]), ("move", c))
            share.check(rows[c][0], omcs[c].movement_energy((2, c % 2)), (c, "before"))
            for t in range(2):
                share.check(rows[c][1 + t], omcs[c].movement_energy((2, c % 2), trials[c][t]), (c, "after", t))
        ins = [np.array([_place(mc, mcds[c].models[2], CELLS[5 + t], rng, shift=0.3) for t in range(3)]) for c in (2, 3)]
        ins[0][2] = mcds[2].models[2] + mc.mat @ rng.uniform(0, 1, 3)
        moves = [None, ("move", (2, 0), trials[1][:1]), ("insert", 2, ins[0]), ("insert", 2, ins[1])]
        rows = group.trial(moves)
        assert rows[0] is None
        same(rows[1], devs[1].trial((2, 0), trials[1][:1]), "move beside insertions")
        for k, c in enumerate((2, 3)):
            same(rows[c], devs[c].trial_insert(2, ins[k]), ("insert", c))
            for t in range(3):
                share.check(rows[c][t], omcs[c].insertion_energy(2, ins[k][t]), (c, "insert", t))
        group.accept([((2, c % 2), trials[c][0]) for c in range(4)])
        for c in range(4):
            omcs[c].update((2, c % 2), trials[c][0])
        for c in range(4):
            _check_state(devs[c], omcs[c], c)
            _check(devs[c].trial((2, c % 2), np.empty((0, len(mcds[c].ffidx[2]), 3)))[0], omcs[c].movement_energy((2, c % 2)), (c, "after accept"))
    share.finish("group")
    for d in devs[::-1]:
        d.close()


def test_sweep_with_large_molecules(setup):
    """The same four chains through ceg_mc_group_sweep: 40 logged steps, p_rotation = 0.5, the large species rotating about atom
    m - 1 (chains 0, 2) or m // 2 (chains 1, 3), step sizes chosen by _step_sizes on chain 0 (chain 3: dmax = 6 A, so that trials are blocked).  Every record against mcrng.propose
    (molecule, kind, u exactly; positions to 1e-12 A; the unused rows of `positions` zero), both rows against the chain's oracle at
    the logged placement, the accepted flag against the rule on the logged rows, the final state against the oracle's replay; both
    move kinds are accepted and rejected.  The same sweep without a log leaves the identical state, bit for bit."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S, T = 4, 40, 400.0
    devs, omcs, mcds = _group_chains(setup, 50)
    twins, _o, _m = _group_chains(setup, 50)
    sizes = (5, 8, 16, 16)
    bead = [[0, 1, (sizes[c] - 1) if c % 2 == 0 else sizes[c] // 2] for c in range(K)]
    orders = [_device_order(d) for d in devs]
    beads = [[bead[c][i] for i, _j in orders[c]] for c in range(K)]
    dmax, thetamax = _step_sizes(omcs[0], beads[0], T)
    dmaxs = [dmax, dmax, dmax, 6.0]                              # chain 3 is thrown about the cell: blocked trials
    kw = dict(temperature=T, dmax=dmaxs, thetamax=thetamax, p_rotation=0.5, bead=bead)
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(twins) as quiet:
        stats, log = group.sweep(S, SEED, 0, log=True, **kw)
        qstats = quiet.sweep(S, SEED, 0, **kw)
        assert qstats.tobytes() == stats.tobytes()
        for x, y in zip(devs, twins):
            assert _same_state(x, y)
    share = _Share()
    exempt, seen, large = 0, set(), 0
    for s in range(S):
        for c in range(K):
            rec, omc, order = log[s, c], omcs[c], orders[c]
            pr = mcrng.propose(SEED, s, c, [omc.positions[i][j] for i, j in order], dmaxs[c], thetamax, 0.5, beads[c])
            assert (rec["molecule"], rec["kind"]) == (pr.molecule, pr.kind), (s, c)
            assert rec["u"] == pr.u, (s, c)
            idx = order[pr.molecule]
            m = len(omc.ffidx[idx[0]])
            placed = rec["positions"][:m].copy()
            assert np.abs(placed - pr.positions).max() <= 1e-12, (s, c, placed, pr.positions)
            assert not rec["positions"][m:].any()
            share.check(rec["rows"][0], omc.movement_energy(idx), (s, c, "before"))
            share.check(rec["rows"][1], omc.movement_energy(idx, placed), (s, c, "after"))
            ok, e = _rule(rec["rows"], rec["u"], T)
            if e is not None and abs(rec["u"] - e) < 1e-12:
                exempt += 1
            else:
                assert bool(rec["accepted"]) == ok, (s, c, rec)
            large += m > 3
            if m > 3:
                seen.add((int(pr.kind), bool(rec["accepted"])))
            if rec["accepted"]:
                omc.update(idx, placed)
    assert exempt <= 1, exempt
    assert len(seen) == 4, seen                                  # both move kinds of the LARGE molecules accepted and rejected
    assert large >= S * K // 4, large
    share.finish("sweep")
    for c in range(K):
        _check_state(devs[c], omcs[c], c)
    for d in twins[::-1] + devs[::-1]:
        d.close()


# ------------------------------------------------------------------ 5. the limit
def test_seventeen_atoms_are_refused_cleanly(setup):
    """ceg_mc_trial_insert, ceg_mc_insert and ceg_mc_set_guests with a 17-atom molecule return CEG_ERR_UNSUPPORTED; after each
    refusal the handle answers a trial with the same row as before, and its state is the one it had."""
    mc, _owner = setup
    mcd = _derive(mc, [_species(mc, 16)], [2], seed=60)
    dev, _omc = _chain(setup, mcd, oracle=False)
    lib, h = dev._lib, dev._h
    trial = _displace(np.random.default_rng(61), mcd.positions[2][0], 2)
    before = dev.trial((2, 0), trial)
    pos0, sf0 = dev.state()
    ids, d = _species(mc, 16)
    kinds = np.ascontiguousarray([ix - 1 for ix in ids] + [ids[0] - 1], dtype=np.int32)
    p17 = np.ascontiguousarray(np.concatenate([_site(mc, CELLS[9]) + d, _site(mc, CELLS[9])[None] + 0.3]).reshape(-1))
    out = np.full((1, 4), np.nan)

    def unchanged(what):
        assert np.array_equal(dev.trial((2, 0), trial), before), what
        pos, sf = dev.state()
        assert np.array_equal(pos, pos0) and np.array_equal(sf, sf0), what

    assert lib.ceg_mc_trial_insert(h, _abi.i32ptr(kinds), 17, _abi.dptr(p17), 1, _abi.dptr(out.reshape(-1))) == UNSUPPORTED
    assert np.isnan(out).all()
    unchanged("trial_insert")
    mol = C.c_int32(-7)
    assert lib.ceg_mc_insert(h, _abi.i32ptr(kinds), 17, _abi.dptr(p17), C.byref(mol)) == UNSUPPORTED
    assert mol.value == -7
    unchanged("insert")
    first = np.array([0, 1, 18], dtype=np.int32)                 # a Na, then a 17-atom molecule
    k18 = np.ascontiguousarray(np.concatenate([[mcd.ffidx[0][0] - 1], kinds]), dtype=np.int32)
    p18 = np.ascontiguousarray(np.concatenate([mcd.positions[0][0].reshape(-1), p17]))
    assert lib.ceg_mc_set_guests(h, _abi.dptr(p18), _abi.i32ptr(k18), _abi.i32ptr(first), 2) == UNSUPPORTED
    unchanged("set_guests")
    # 16 atoms are taken by all three
    assert lib.ceg_mc_trial_insert(h, _abi.i32ptr(kinds), 16, _abi.dptr(p17), 1, _abi.dptr(out.reshape(-1))) == 0
    assert np.isfinite(out).all()
    dev.close()
