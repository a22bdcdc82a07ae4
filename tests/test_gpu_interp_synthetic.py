"""Both device implementations of ``interpolate_grid`` (csrc/ceg_consumers.h) and the block-mask kernels (csrc/ceg_block.hip) on the
synthetic cases of ``tests/interp_cases.py``; ``tests/test_interp_cases_host.py`` checks the cases, the reference and the bound
on the CPU.  Run with `pytest -m gpu` on an MI355X.

Every interpolation check has one form (``IC.check_values`` / ``IC.check_rows``): 1e100 where the longdouble reference is blocked
(>= 1e90 in a Monte-Carlo column), NaN where it is NaN, |got - reference| <= K 2^-53 T elsewhere, K = 128 derived in interp_cases.

Routes:
  interp_point   ceg_interp_points through GridInterpolator on every grid and point of the catalogue; one handle over batches of 1,
                 255, 256, 257, 1000, 3 and 0 points; ceg_interp_points_device on a non-default stream from a device-resident grid
                 (k_to_node_major from device memory), bit-identical to the host entry point; ceg_interp_set_higherorder(0).
  interp_corner  empty-box Monte-Carlo handles on synthetic setups (IC.mc_setup: kinds whose VdW grids differ in dims, a kind
                 without a grid, a Coulomb grid of other dims again, no Coulomb grid, a blocking grid, a VdW-declared blocking
                 grid in the Coulomb slot, whose 1e100 goes into column 1 without the charge): ceg_mc_trial_insert (the
                 one-workgroup kernel, mc_trial_row), ceg_mc_trial_insert_device (k_mcw_frame) at every fill of a workgroup and,
                 with 32 771 rows, at four placements per wave; displacements with row 0 read from the atom records; a chain group;
                 ceg_mc_baseline and ceg_mc_group_baseline (the baseline kernel) with a free slot among the molecules.
  block masks    ceg_block_from_grid on single-entry and random value arrays, ceg_block_spheres with 0, 1, 257 and 2048 spheres, the
                 refusal of 2049 and the strict comparison on a sphere surface, bit for bit against IC / the oracle.

Observed on an MI355X, worst |got - reference| / (2^-53 T) per route, to be held against the derived K = 128 (test_zz_report prints
them; the float64 oracle on the CPU reaches 6.2):
  ceg_interp_points            random 5.3, poly 4.4, poly-vdw 5.8, one-hot 1.4, blocking 3.0, huge 0.75
  ceg_interp_points_device     4.0 (bit-identical to the host entry point)          no-derivatives branch   3.4
  mc_trial_row, insertions     column 0 0.43, column 1 0.86                         displacements           0.04, 0.15 (split: the same)
  k_mcw_frame, insertions      column 0 1.7,  column 1 1.7                          displacements           0.06, 0.15
  k_mcw_frame, 4 per wave      0.41, 0.46 (bit-identical to one placement per wave)
  group trial                  0.05, 0.10                                           baseline kernel         vdw 0.001, direct 0.005
The Monte-Carlo figures are small because T is summed over the atoms of a molecule (of a chain, for the baseline) while the
errors of the atoms do not line up.  The launch of k_block_spheres with 2048 spheres (exactly 64 KiB of dynamic LDS) is accepted.
The whole module takes about 4 s, the catalogue of ceg_interp_points 0.7 s, no other test more than 0.2 s."""
import math

import numpy as np
import pytest

from ceg_hip import _abi

import interp_cases as IC

pytestmark = pytest.mark.gpu

OBSERVED = {}          # route -> worst ratio seen in this run (printed by test_zz_report)
UNSUPPORTED = -5       # CEG_ERR_UNSUPPORTED
MCW_FRAME_ROWS, MCW_WAVES = 4, 4            # csrc/ceg_mc.hip


def _note(route, worst):
    OBSERVED[route] = max(OBSERVED.get(route, 0.0), float(worst))


def _interpolator(eg, **kw):
    from ceg_hip.interp import GridInterpolator
    return GridInterpolator(eg, **kw)


def _case(name):
    return next(c for c in IC.catalogue() if c.name == name)


# ------------------------------------------------------------------------------------------------ interp_point
def test_interp_points_on_every_grid_and_point(hip_lib):
    worst = {}
    for case in IC.catalogue():
        it = _interpolator(case.eg)
        try:
            got = it(case.pts)
        finally:
            it.close()
        w = IC.check_values(got, case.eg, case.pts, case.name, ref=case.ref)
        worst[case.family] = max(worst.get(case.family, 0.0), w)
    for family, w in worst.items():
        _note(f"ceg_interp_points/{family}", w)
    assert set(worst) == {"random", "poly", "poly-vdw", "one-hot", "blocking", "huge"}


def test_one_handle_over_growing_and_shrinking_batches(hip_lib):
    """the handle keeps its device buffers between calls and only grows them; n = 0 returns at once"""
    case = _case("random-vdw/tric/15x13x11")
    value, T, cell, blocked, skip = case.ref
    it = _interpolator(case.eg)
    try:
        start = 0
        for n in (1, 255, 256, 257, 1000, 3):
            sel = slice(start, start + n)
            got = it(case.pts[sel])
            IC.check_values(got, case.eg, case.pts[sel], n, ref=(value[sel], T[sel], cell[sel], blocked[sel], skip[sel]))
            start += n
        assert start <= len(case.pts)
        out = np.full(2, -7.0)
        assert hip_lib.ceg_interp_points(it._h, _abi.dptr(np.zeros(3)), 0, _abi.dptr(out)) == 0
        assert (out == -7.0).all()
        assert len(it(np.empty((0, 3)))) == 0
    finally:
        it.close()


@pytest.mark.parametrize("name", ["random-vdw/ortho/7x5x3", "poly-vdw/tric/15x13x11", "random-coulomb/tric/1x3x5"])
def test_device_entry_point_on_a_stream(hip_lib, name):
    """a handle created on a device-resident grid (k_to_node_major reads device memory), ceg_interp_points_device on a non-default
    stream: bit-identical to the host entry point of a handle that uploaded the same grid"""
    import torch
    case = _case(name)
    dev = torch.device("cuda", 0)
    d_grid = torch.from_numpy(np.ascontiguousarray(case.eg.grid)).to(dev)
    d_pts = torch.from_numpy(case.pts).to(dev)
    d_out = torch.full((len(case.pts),), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    it = _interpolator(case.eg, device_ptr=d_grid.data_ptr())
    host = _interpolator(case.eg)
    try:
        it.on_device(d_pts.data_ptr(), len(case.pts), d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        got = d_out.cpu().numpy()
        want = host(case.pts)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
        _note("ceg_interp_points_device", IC.check_values(got, case.eg, case.pts, name, ref=case.ref))
    finally:
        host.close()
        it.close()


@pytest.mark.parametrize("cell", list(IC.CELLS))
def test_no_derivatives_branch(hip_lib, cell):
    """ceg_interp_set_higherorder(0): channel 1 with trilinear weights in the reference's index order; NaN beyond an axis, which the
    cubic (3,3,3) grid never shows and the (7,5,3) grid does"""
    for dims in ((3, 3, 3), (7, 5, 3)):
        cs = IC.cset(cell, dims)
        eg = IC.energy_grid(cs, IC.random_data(cs, 77), IC.VDW, higherorder=False)
        pts = IC.all_points(cs, seed=4)
        value, T = IC.reference_noderiv(eg, pts)
        it = _interpolator(eg)
        try:
            got = it(pts)
        finally:
            it.close()
        assert np.array_equal(np.isnan(got), np.isnan(value)), (cell, dims)
        assert np.isnan(got).any() == (dims == (7, 5, 3))
        m = ~np.isnan(value)
        assert (np.abs(got[m].astype(IC.LD) - value[m]) <= IC.bound(T[m])).all(), (cell, dims)
        _note("no-derivatives", IC.ratio(got[m], value[m], T[m]))


# ------------------------------------------------------------------------------------------------ interp_corner: Monte-Carlo handles
SETUPS = {"full": (True, False, False), "no-coulomb": (False, False, False), "blocking": (True, True, False), "coulomb-vdw": (True, False, True)}


@pytest.fixture(scope="module")
def chains(hip_lib):
    """(cell, setup name) -> (MonteCarloSetup, DeviceMonteCarlo on an empty box)"""
    from ceg_hip.energy import DeviceMonteCarlo
    out = {}
    for cell in IC.CELLS:
        for name, flags in SETUPS.items():
            mc = IC.mc_setup(cell, *flags)
            out[cell, name] = (mc, DeviceMonteCarlo(mc))
    yield out
    for _mc, dev in out.values():
        dev.close()


ALL_CHAINS = [(cell, name) for cell in IC.CELLS for name in SETUPS]


def _check_insert_rows(rows, mc, species, pos, what, route):
    w0, w1, nblocked, ncoulomb = IC.check_rows(rows, mc, mc.ffidx[species], pos, what)
    assert rows.shape == (len(pos), 4)
    assert (rows[:, 2] == 0.0).all() and (rows[:, 3] == 0.0).all(), what          # an empty box, no Ewald sums
    if mc.coulomb.ewald_precision == -math.inf:
        assert (rows[:, 1] == 0.0).all(), what
    _note(f"{route}/column 0", w0)
    _note(f"{route}/column 1", w1)
    return np.array([nblocked, ncoulomb])


def _seen(counts, name):
    """rows blocked in column 0 come from the blocking setup only, rows with 1e100 in column 1 from the coulomb-vdw setup only"""
    return (counts[0] > 0) == (name == "blocking") and (counts[1] > 0) == (name == "coulomb-vdw")


def _device_insert(dev, species, pos):
    import torch
    d_trial = torch.tensor(pos, dtype=torch.float64, device="cuda")
    d_rows = torch.full((len(pos), 4), float("nan"), dtype=torch.float64, device="cuda")
    dev.trial_insert_device(species, d_trial.data_ptr(), len(pos), d_rows.data_ptr())
    torch.cuda.synchronize()
    return d_rows.cpu().numpy()


@pytest.mark.parametrize("cell,name", ALL_CHAINS)
def test_insertion_rows_one_workgroup_kernel(chains, monkeypatch, cell, name):
    """ceg_mc_trial_insert with 1, 2 and 7 rows of every species: one workgroup per row (mc_trial_row)"""
    mc, dev = chains[cell, name]
    monkeypatch.setenv("CEG_HIP_MC_WAVE_MIN", "1000000000")
    rng = np.random.default_rng(21)
    seen = np.zeros(2, dtype=np.int64)
    for species in range(len(mc.ffidx)):
        for n in (1, 2, 7):
            pos = IC.mc_placements(mc, species, n, rng)
            rows = dev.trial_insert(species, pos)
            seen += _check_insert_rows(rows, mc, species, pos, (cell, name, species, n), "mc_trial_row")
    assert _seen(seen, name), seen


@pytest.mark.parametrize("cell,name", ALL_CHAINS)
def test_insertion_rows_wave_kernels(chains, monkeypatch, cell, name):
    """ceg_mc_trial_insert_device (always k_mcw_frame) with 1, 3, 4, 5, 16, 17 and 65 rows: a single wave, a partly and a wholly
    filled workgroup, one row more, several workgroups; 16 m evaluations per row that are no multiple of 64 for m = 1, 3, 5.  The host
    entry point with CEG_HIP_MC_WAVE_MIN=0 returns the same bytes."""
    mc, dev = chains[cell, name]
    rng = np.random.default_rng(22)
    seen = np.zeros(2, dtype=np.int64)
    for species in range(len(mc.ffidx)):
        for n in (1, 3, 4, 5, 16, 17, 65):
            pos = IC.mc_placements(mc, species, n, rng)
            rows = _device_insert(dev, species, pos)
            seen += _check_insert_rows(rows, mc, species, pos, (cell, name, species, n), "k_mcw_frame")
            monkeypatch.setenv("CEG_HIP_MC_WAVE_MIN", "0")
            host = dev.trial_insert(species, pos)
            monkeypatch.delenv("CEG_HIP_MC_WAVE_MIN")
            assert host.tobytes() == rows.tobytes(), (cell, name, species, n)
    assert _seen(seen, name), seen


@pytest.mark.parametrize("name", ["blocking", "coulomb-vdw"])
@pytest.mark.parametrize("species", [1, 3])
def test_four_placements_per_wave(chains, species, name):
    """A wave of k_mcw_frame takes more than one placement only when the batch fills the device: 32 771 rows give four per wave (their
    16 m = 48 or 80 evaluations numbered through and taken 64 at a time) and a ragged last wave.  The arithmetic of a row does not
    depend on the wave that runs it: bit for bit the rows of the same placements in batches of 4096 (one placement per wave), which
    are compared with the reference on a sample."""
    mc, dev = chains["tric", name]
    m = len(mc.ffidx[species])
    assert 16 * m % 64
    n = 32771
    assert n // (MCW_WAVES * MCW_FRAME_ROWS) >= 2048 and 4096 // (MCW_WAVES * 2) < 2048 and n % (MCW_WAVES * MCW_FRAME_ROWS)
    rng = np.random.default_rng(23)
    base = IC.mc_placements(mc, species, 512, rng)
    pos = base[rng.integers(512, size=n)] + rng.uniform(-0.5, 0.5, (n, 1, 3))
    pos[:512] = base                                             # the tiny-negative, node and blocked atoms as they are
    big = _device_insert(dev, species, pos)
    small = np.concatenate([_device_insert(dev, species, pos[b:b + 4096]) for b in range(0, n, 4096)])
    differ = np.nonzero((big.view(np.int64) != small.view(np.int64)).any(axis=1))[0]
    assert len(differ) == 0, (len(differ), differ[:8], differ[-8:])
    pick = np.unique(np.concatenate([np.arange(0, 40), rng.integers(n, size=200), np.arange(n - 20, n)]))
    assert _seen(_check_insert_rows(big[pick], mc, species, pos[pick], ("four per wave", species), "k_mcw_frame, 4 per wave"), name)


@pytest.mark.parametrize("cell,name", ALL_CHAINS)
def test_displacement_rows_and_row_zero(monkeypatch, cell, name):
    """ceg_mc_set_guests with molecules of 3, 5 and 16 atoms; ceg_mc_trial of each through the one-workgroup kernel, its
    three-workgroup split and the wave kernels: row 0, read from the atom records, equals the reference at the stored positions and,
    bit for bit, row 1 of the same call when the first trial placement is the stored one"""
    from ceg_hip.energy import DeviceMonteCarlo
    mc = IC.mc_setup(cell, *SETUPS[name])
    rng = np.random.default_rng(24)
    seen = np.zeros(2, dtype=np.int64)
    held = {1: 0, 3: 0, 5: 0}                                    # species index -> molecule index
    for s in held:
        mc.positions[s] = [IC.mc_placements(mc, s, 3, rng)[s % 3]]          # rows 0, 1, 2 of IC.mc_placements in turn
    dev = DeviceMonteCarlo(mc)
    try:
        for s in held:
            ids = mc.ffidx[s]
            stored = mc.positions[s][0]
            trial = np.concatenate([stored[None], IC.mc_placements(mc, s, 6, rng)])
            ref_pos = np.concatenate([stored[None], trial])
            for route, env in (("mc_trial_row", {"CEG_HIP_MC_WAVE_MIN": "1000000000", "CEG_HIP_MC_SPLIT_MAX": "0"}),
                               ("mc_trial_row, split", {"CEG_HIP_MC_WAVE_MIN": "1000000000", "CEG_HIP_MC_SPLIT_MAX": "1000000000"}),
                               ("k_mcw_frame", {"CEG_HIP_MC_WAVE_MIN": "0"})):
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                rows = dev.trial((s, 0), trial)
                for k in env:
                    monkeypatch.delenv(k)
                assert rows.shape == (8, 4)
                w0, w1, nb, nc = IC.check_rows(rows, mc, ids, ref_pos, (cell, name, s, route))
                seen += (nb, nc)
                if name == "coulomb-vdw" and s in (1, 3):        # the stored molecule holds an atom in the blocked cell of the Coulomb slot
                    assert rows[0, 1] >= 1e90
                _note(f"{route}, displacement/column 0", w0)
                _note(f"{route}, displacement/column 1", w1)
                assert rows[0, :2].tobytes() == rows[1, :2].tobytes(), (cell, name, s, route, rows[:2])
                assert (rows[:, 3] == 0.0).all()
        assert _seen(seen, name), seen
    finally:
        dev.close()


def _filled_chain(mc_of, rng, species_list, grids_from=None):
    """a DeviceMonteCarlo holding one molecule of every species in `species_list`"""
    from ceg_hip.energy import DeviceMonteCarlo
    mc = mc_of()
    for s in species_list:
        mc.positions[s] = mc.positions[s] + [IC.mc_placements(mc, s, 3, rng)[s % 3]]          # rows 0, 1, 2 of IC.mc_placements in turn
    return mc, DeviceMonteCarlo(mc, grids_from=grids_from)


@pytest.mark.parametrize("name", ["blocking", "coulomb-vdw"])
@pytest.mark.parametrize("cell", list(IC.CELLS))
def test_group_trial_with_a_move_an_insertion_and_an_idle_chain(hip_lib, cell, name):
    """K = 3 chains of different contents on one set of grids; one ceg_mc_group_trial with a move, an insertion and an idle chain"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    rng = np.random.default_rng(25)
    made = []
    try:
        for species_list in ((1, 3), (0, 5, 5), (6, 2, 4)):
            made.append(_filled_chain(lambda: IC.mc_setup(cell, *SETUPS[name]), rng, species_list, grids_from=made[0][1] if made else None))
        (mc0, dev0), (mc1, dev1), (_mc2, dev2) = made
        with DeviceMonteCarloGroup([dev0, dev1, dev2]) as group:
            moved = np.concatenate([mc0.positions[3][0][None], IC.mc_placements(mc0, 3, 4, rng)])
            ins = IC.mc_placements(mc1, 4, 5, rng)
            rows = group.trial([("move", (3, 0), moved), ("insert", 4, ins), None])
            assert rows[2] is None and rows[0].shape == (6, 4) and rows[1].shape == (5, 4)
            w0, w1, nb, nc = IC.check_rows(rows[0], mc0, mc0.ffidx[3], np.concatenate([mc0.positions[3][0][None], moved]), (cell, "group move"))
            assert rows[0][0, :2].tobytes() == rows[0][1, :2].tobytes()
            v0, v1, nb1, nc1 = IC.check_rows(rows[1], mc1, mc1.ffidx[4], ins, (cell, "group insert"))
            assert _seen((nb, nc), name) and _seen((nb1, nc1), name), (nb, nc, nb1, nc1)
            _note("group trial/column 0", max(w0, v0))
            _note("group trial/column 1", max(w1, v1))
    finally:
        for _mc, dev in made[::-1]:
            dev.close()


@pytest.mark.parametrize("cell,name", [(cell, name) for cell in IC.CELLS for name in ("full", "blocking", "coulomb-vdw")])
def test_baseline_kernel_with_a_free_slot(hip_lib, cell, name):
    """ceg_mc_baseline and ceg_mc_group_baseline on a chain of six molecules (1, 3, 4, 5, 8 and 16 atoms) after one ceg_mc_remove, so
    that a slot is free among the five left: framework_vdw and framework_direct against the sums over all atoms, the bound summed over
    the atoms (the sum over molecules adds one rounding per molecule to the 98 of the derivation: 103 < K); with a blocking grid in
    the Coulomb slot framework_direct is 1e100 per atom in a blocked cell (four placed there, others by chance), whatever their charges; a member of a group
    returns the bytes the handle returns alone"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    rng = np.random.default_rng(26)
    blocking = name == "blocking"
    mc, dev = _filled_chain(lambda: IC.mc_setup(cell, *SETUPS[name]), rng, (0, 1, 2, 3, 4, 5))
    other = None
    try:
        dev.remove((2, 0))
        mc.positions[2] = []
        rec = dev.baseline_record()
        assert (int(rec["nmol"]), int(rec["natoms"])) == (5, 1 + 3 + 5 + 8 + 16)
        v0, t0, v1, t1 = (IC.LD(0) for _ in range(4))
        blocked, nb1 = False, 0
        for _i, _j, ids, p in mc.molecules():
            a0, b0, blk, a1, b1, n1 = IC.column_reference(mc, ids, p[None])
            v0, t0, v1, t1, blocked, nb1 = v0 + a0[0], t0 + b0[0], v1 + a1[0], t1 + b1[0], blocked or bool(blk[0]), nb1 + int(n1[0])
        assert blocked == blocking and (nb1 >= 4 if name == "coulomb-vdw" else nb1 == 0)          # four placed there; the hot node blocks 4 of the 15 cells
        if blocked:
            assert rec["framework_vdw"] >= 1e90
        else:
            assert abs(IC.LD(float(rec["framework_vdw"])) - v0) <= IC.bound(t0), (float(rec["framework_vdw"]), float(v0))
            _note("baseline/framework_vdw", IC.ratio(np.array([rec["framework_vdw"]]), np.array([v0]), np.array([t0])))
        if nb1:
            assert abs(float(rec["framework_direct"]) - nb1 * 1e100) <= 2.0 ** -50 * nb1 * 1e100, (float(rec["framework_direct"]), nb1)
        else:
            assert abs(IC.LD(float(rec["framework_direct"])) - v1) <= IC.bound(t1), (float(rec["framework_direct"]), float(v1))
            _note("baseline/framework_direct", IC.ratio(np.array([rec["framework_direct"]]), np.array([v1]), np.array([t1])))
        assert rec["inter"] == 0.0 and rec["recip_framework"] == 0.0 and rec["recip_guests"] == 0.0
        _mc2, other = _filled_chain(lambda: IC.mc_setup(cell, *SETUPS[name]), rng, (5, 1), grids_from=dev)
        alone = [dev.baseline_record().tobytes(), other.baseline_record().tobytes()]
        with DeviceMonteCarloGroup([dev, other]) as group:
            recs = group.baseline_records()
            assert [recs[0].tobytes(), recs[1].tobytes()] == alone
    finally:
        if other is not None:
            other.close()
        dev.close()


# ------------------------------------------------------------------------------------------------ block masks
def _block_from_grid(lib, value, on_device):
    import torch
    dims = np.ascontiguousarray([n - 1 for n in value.shape], dtype=np.int32)
    out = np.full(value.shape, 0xAB, dtype=np.uint8)
    value = np.ascontiguousarray(value, dtype=np.float32)
    if on_device:
        d_value = torch.from_numpy(value).to("cuda")
        torch.cuda.synchronize()
        ptr = d_value.data_ptr()
    else:
        ptr = value.ctypes.data
    _abi.check(lib, lib.ceg_block_from_grid(0, ptr, int(on_device), _abi.i32ptr(dims), 5e6, out.ctypes.data))
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("dims", IC.DIMS)
def test_block_from_grid(hip_lib, dims, on_device):
    """one entry at the first cell, an interior cell, the last cell origin and the last node of each axis -- 5e6f, the float above,
    +inf, NaN, -inf -- and a random array with a tenth of the entries hot: the mask bit-equal to the scatter of grids.jl:190-201"""
    for name, value, count in IC.block_single_entry_cases(dims) + [("random", IC.block_random_case(dims), None)]:
        got = _block_from_grid(hip_lib, value, on_device)
        assert np.array_equal(got, IC.block_from_grid_reference(value)), (dims, name, on_device)
        if count is not None:
            assert int(got.sum()) == count, (dims, name)


def _block_spheres(lib, cs, centers, radius2, fill=0xAB, expect=0):
    dims, delta, shift, mat, inv, ortho, safemin2 = IC.sphere_abi_args(cs)
    n = len(radius2)
    c = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1)
    r2 = np.ascontiguousarray(radius2, dtype=np.float64)
    out = np.full(tuple(cs.npoints), fill, dtype=np.uint8)
    rc = lib.ceg_block_spheres(0, _abi.i32ptr(dims), _abi.dptr(delta), _abi.dptr(shift), _abi.dptr(mat), _abi.dptr(inv), ortho, safemin2,
                               _abi.dptr(c) if n else None, _abi.dptr(r2) if n else None, n, out.ctypes.data)
    assert rc == expect, (rc, lib.ceg_last_error())
    return out


SPHERE_GRIDS = [(cell, dims) for cell in IC.CELLS for dims in ((7, 5, 3), (15, 13, 11))]


@pytest.mark.parametrize("cell,dims", SPHERE_GRIDS)
def test_block_spheres(hip_lib, oracle, cell, dims):
    """0 spheres (all zeros), 1, 257 (two passes of the staging loop) and 2048 (exactly 64 KiB of dynamic LDS) against the oracle, bit
    for bit; 2049 refused with the output untouched"""
    cs = IC.cset(cell, dims)
    assert not _block_spheres(hip_lib, cs, np.empty((0, 3)), np.empty(0)).any()
    for n in (1, 257, 2048):
        centers, r2 = IC.sphere_case(cs, n, seed=n)
        got = _block_spheres(hip_lib, cs, centers, r2)
        assert set(np.unique(got)) <= {0, 1}
        ref = oracle.block_spheres(cs, centers, r2)
        assert 0.2 <= ref.mean() <= 0.8
        assert np.array_equal(got.astype(bool), ref), (cell, dims, n, int((got.astype(bool) != ref).sum()))
    centers, r2 = IC.sphere_case(cs, 2049, seed=5)
    out = _block_spheres(hip_lib, cs, centers, r2, fill=0x5C, expect=UNSUPPORTED)
    assert (out == 0x5C).all()
    assert b"2048" in hip_lib.ceg_last_error()


@pytest.mark.parametrize("cell,dims", SPHERE_GRIDS)
def test_block_sphere_surface_is_open(hip_lib, oracle, cell, dims):
    """a sphere centred on a lattice point whose radius2 is exactly the squared distance to the x-neighbour leaves the neighbour
    open (strict <); the next double closes it"""
    cs = IC.cset(cell, dims)
    centre, neighbour, r2 = IC.sphere_boundary_case(oracle, cs)
    c = IC.lattice_point(cs, centre)[None]
    open_ = _block_spheres(hip_lib, cs, c, np.array([r2])).astype(bool)
    closed = _block_spheres(hip_lib, cs, c, np.array([np.nextafter(r2, np.inf)])).astype(bool)
    assert open_[centre] and not open_[neighbour] and closed[centre] and closed[neighbour]
    assert np.array_equal(open_, oracle.block_spheres(cs, c, np.array([r2])))
    assert np.array_equal(closed, oracle.block_spheres(cs, c, np.array([np.nextafter(r2, np.inf)])))


def test_zz_report():
    """A printing aid, no check of its own: the worst ratio per route of the tests that ran before it in this process (every ratio is
    asserted where it is measured, in IC.check_values / IC.check_rows); partial under -k or with the tests spread over processes."""
    for route in sorted(OBSERVED):
        print(f"interp-observed {route}: {OBSERVED[route]:.3f}")
