"""The sampler of a chain group (ceg_mc_group_set_sampler / _sample / _sampler_read / _sampler_reset, kernel k_mcg_sample): density
maps and the per-cycle series taken on the device while a sweep runs.  The reference is the host restatement in ceg_hip.mcrng
(bin_index / bin_positions, held to hand-computed cases by tests/test_mc_sampler_host.py) applied to the positions that
mcrng.replay_positions recovers from the sweep's log: the bins must be EQUAL, integer for integer.  Run with `pytest -m gpu` on an MI355X."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi, mcrng
from test_gpu_mc_sweep import SEED, _close, _copy, _device_order, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES

pytestmark = pytest.mark.gpu

FF = "BoulfelfelSholl2021"
CHA = "CHA_1.4_3b4eeb96_Na_11812"
SWAP_HEAVY = mcrng.MoveTable(translation=1, rotation=1, random_reinsertion=1, swap=5)
GCMC_CASE = (3.0e4, SEED + 902)         # (phiPV_div_k, seed) of the GCMC test: the run holds accepted insertions and an accepted deletion
# (R, t) on the fractional coordinates of the unit cell: inversion, a cyclic permutation with a translation of 1/3, a mirror with a glide
SYMMETRIES = [(-np.eye(3), np.zeros(3)),
              (np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), np.full(3, 1.0 / 3.0)),
              (np.diag([1.0, -1.0, 1.0]), np.array([0.5, 0.0, 0.25]))]


@pytest.fixture(scope="module")
def cha(hip_lib, tmp_path_factory):
    """CHA + Na (the cations belong to the framework) with 6 CO2 at random places of the MC cell: the setup and the chain that owns
    the grids, built once for the module"""
    from pathlib import Path
    from ceg_hip.energy import DeviceMonteCarlo
    from ceg_hip.hostmirror import montecarlo as M
    golden = Path(__file__).parent / "golden" / "raspa"
    raspa = tmp_path_factory.mktemp("mc_sampler") / "raspa"
    raspa.mkdir()
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(golden / sub, raspa / sub)
    try:
        ceg.setdir_RASPA(raspa)
        co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", FF)
        base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
        fw = ceg.load_framework_RASPA(CHA, FF)
        rng = np.random.default_rng(5)
        centres = rng.uniform(0.0, 1.0, (6, 3)) @ np.asarray(fw.mat, dtype=np.float64).T
        mc = M.setup_montecarlo(CHA, FF, [co2.with_positions(c + base) for c in centres], gridstep=0.3)
        owner = DeviceMonteCarlo(_copy(mc))
        # the start state instead of the random places: two molecules at open sites (framework VdW energy, column 0 of the insertion
        # row, below 0) and four pressed against the framework (500 to 5000 K: not blocked, so the energy sums of a sweep stay finite,
        # but ready to be deleted), all 5 A apart
        cand = rng.uniform(0.0, 1.0, (2000, 3)) @ np.asarray(mc.mat, dtype=np.float64).T
        rows = np.concatenate([owner.trial_insert(0, cand[q:q + 200, None, :] + base[None, :, :]) for q in range(0, len(cand), 200)])
        inv = np.asarray(mc.invmat, dtype=np.float64)
        sites, want = [], [2, 4]
        for c, row in zip(cand, rows):
            which = 0 if row[0] < 0.0 else (1 if 500.0 < row[0] < 5000.0 else None)
            if which is None or want[which] == 0:
                continue
            if all(np.linalg.norm((((c - q) @ inv.T) - np.round((c - q) @ inv.T)) @ np.asarray(mc.mat).T) > 5.0 for q in sites):
                sites.append(c)
                want[which] -= 1
        assert want == [0, 0], want
        mc = _copy(mc, [[c + base for c in sites[:6]]])
        owner.mc.positions = [[p.copy() for p in mc.positions[0]]]
        owner.refresh()
        yield mc, owner
        owner.close()
    finally:
        ceg.setdir_RASPA(golden)


def _new_chains(fixture, k, positions=None):
    from ceg_hip.energy import DeviceMonteCarlo
    mc, owner = fixture
    return [DeviceMonteCarlo(_copy(mc, positions), grids_from=owner) for _ in range(k)]


def _kinds(mc):
    """0-based force-field kind of every atom of every species"""
    return [[ix - 1 for ix in ids] for ids in mc.ffidx]


def _start(dev):
    """(species, positions) of the chain's molecules in device molecule order"""
    order = _device_order(dev)
    return [i for i, _j in order], [np.array(dev.mc.positions[i][j], dtype=np.float64) for i, j in order]


def _host_bins(samp, frames_of_chain, kinds):
    """bins [nmaps, nchannels, nc, nb, na] of frames_of_chain[c] = [(species, positions) per frame] through mcrng.bin_positions"""
    na, nb, nc = samp["dims"]
    bins = np.zeros((samp["nmaps"], samp["nchannels"], nc, nb, na), dtype=np.int64)
    for c, frames in enumerate(frames_of_chain):
        m = int(samp["chain_map"][c])
        if m < 0:
            continue
        for spec, mols in frames:
            per_channel = {}
            for s, p in zip(spec, mols):
                for a, kind in enumerate(kinds[s]):
                    ch = int(samp["channels"][kind])
                    if ch >= 0:
                        per_channel.setdefault(ch, []).append(p[a])
            for ch, pts in per_channel.items():
                mcrng.bin_positions(bins[m, ch], samp["unit_invmat"], np.array(pts), samp["symmetries"])
    return bins


def _replayed_frames(starts, log, first, frames, atoms_per_species):
    """per chain, (species, positions) after each of the absolute steps `frames`, from the chain's column of the log"""
    out = []
    for c, (spec, pos) in enumerate(starts):
        states = list(mcrng.replay_positions(pos, log[:, c], atoms_per_species, start_species=spec))
        out.append([states[s - first] for s in frames])
    return out


def _check_counts(series, frames_of_chain, frames, nspecies, what):
    for c, states in enumerate(frames_of_chain):
        for f, (spec, mols) in enumerate(states):
            rec = series[f, c]
            assert rec["step"] == frames[f], (what, c, f, rec)
            assert rec["nmol"] == len(mols) and rec["natoms"] == sum(len(p) for p in mols), (what, c, f, rec, len(mols))
            if nspecies:
                assert list(rec["count"]) == [spec.count(i) for i in range(nspecies)] + [0] * (_abi.GCMC_MAX_SPECIES - nspecies), (what, c, f, rec)
            else:
                assert not rec["count"].any(), (what, c, f, rec)


def test_gcmc_sweep_bins_and_series_against_the_log_replay(cha):
    """CHA + Na with CO2, K = 4, chain_map = [0, 0, 1, -1], channels C -> 0, O -> 1 (Na, a framework kind here, -> -1), a swap-heavy
    move table, first_step = 5, every = 8, from_step = 16, a 1 A map on the MC cell (dims 28).  The issue's 96 steps end on step
    100, which is no frame: 99 steps end on step 103, the eleventh frame.  Bins equal to bin_positions over replay_positions at the
    frame steps; step, nmol, natoms, count of every record equal to the replay's; the deltas of the last frame equal to the returned
    statistics bit for bit, those of earlier frames equal to the running sums of the log's rows to 1e-12 * largest |row entry| *
    accepted moves.  The run must hold an accepted insertion and an accepted deletion in a binned chain (a freed and a refilled slot
    pass through the frames): GCMC_CASE does (14 insertions, 1 deletion); it was found on the device among (3e4, 3e3, 3e5) x four seeds."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = cha
    K, S, first, every, start = 4, 99, 5, 8, 16
    frames = mcrng.sampler_frames(first, S, every, start)
    assert frames[-1] == first + S - 1 and len(frames) == 11
    devs = _new_chains(cha, K)
    T = np.array([300.0, 800.0, 1200.0, 1000.0])
    sid = np.arange(K, dtype=np.uint32) * 7 + 3
    sym = mc.ff.symbols
    channels = {"C_co2": 0, "O_co2": 1, "Na": -1} if {"C_co2", "O_co2", "Na"} <= set(sym) else None
    assert channels is not None, sym
    kinds = _kinds(mc)
    phi, seed = GCMC_CASE
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species([SWAP_HEAVY], [phi])
        group.set_sampler(every, from_step=start, step=1.0, channels=channels, chain_map=[0, 0, 1, -1], series_capacity=len(frames))
        samp = group.sampler
        assert all(24 <= d <= 32 for d in samp["dims"]), samp["dims"]
        starts = [_start(d) for d in devs]
        stats, log = group.sweep_gcmc(S, seed, first, temperature=T, dmax=0.5, thetamax=1.0, species=table, max_molecules=16, stream_id=sid, log=True)
        bins, series, total = group.sampler_read()
    binned = log[:, :3]
    ins = int(((binned["kind"] == 5) & (binned["accepted"] != 0)).sum())
    dele = int(((binned["kind"] == 6) & (binned["accepted"] != 0)).sum())
    print(f"phiPV_div_k {phi:g}, seed {seed:#x}: accepted insertions {ins}, deletions {dele} in the binned chains")
    assert ins > 0 and dele > 0, (ins, dele)
    assert series.shape == (len(frames), K)
    states = _replayed_frames(starts, log, first, frames, [len(k) for k in kinds])
    _check_counts(series, states, frames, 1, "gcmc")
    want = _host_bins(samp, states, kinds)
    print(f"bins: {int(bins.sum())} counts on a map of {samp['dims']}, {int((bins != want).sum())} bins differ")
    assert np.array_equal(bins, want)
    assert bins[0].sum() > 0 and bins[1].sum() > 0 and bins[:, 1].sum() == 2 * bins[:, 0].sum()           # two O per C
    assert list(total) == [len(frames) * 2, len(frames) * 1]
    # the running sums: recomputed left to right from the log's rows
    t = table[0]
    assert np.abs(stats["delta_moves"]).max() < 1e90 and np.abs(stats["delta_swaps"]).max() < 1e90      # no blocked molecule left its place
    for c in range(K):
        moves = swaps = 0.0
        scale, accepted, f = 0.0, 0, 0
        for s in range(S):
            rec = log[s, c]
            if rec["accepted"]:
                accepted += 1
                scale = max(scale, float(np.abs(rec["rows"]).max()))          # (accepted records only: tighter than every row seen)
                rows = rec["rows"]
                if rec["kind"] <= 4:
                    b = ((rows[0][0] + rows[0][1]) + rows[0][2]) + rows[0][3]
                    a = ((rows[1][0] + rows[1][1]) + rows[1][2]) + rows[1][3]
                    moves += a - b
                else:
                    ins = rec["kind"] == 5
                    diff, _thr = mcrng.swap_threshold(rows[1] if ins else rows[0], float(T[c]), int(rec["n_species"]), float(t["phiPV_div_k"]),
                                                      float(t["self_reciprocal"]), float(rec["tc"]), bool(ins))
                    swaps += diff
            if first + s in frames:
                rec_f = series[f, c]
                tol = 1e-12 * scale * max(accepted, 1)
                print(f"chain {c} frame {f}: delta_moves {rec_f['delta_moves']:.6e} (log {moves:.6e}), delta_swaps {rec_f['delta_swaps']:.6e} (log {swaps:.6e}), tol {tol:.1e}")
                assert abs(rec_f["delta_moves"] - moves) <= tol and abs(rec_f["delta_swaps"] - swaps) <= tol, (c, f)
                f += 1
        assert series[-1, c]["delta_moves"].tobytes() == stats[c]["delta_moves"].tobytes(), c
        assert series[-1, c]["delta_swaps"].tobytes() == stats[c]["delta_swaps"].tobytes(), c
        assert series[-1, c]["nmol"] == stats[c]["nmol"] and list(series[-1, c]["count"]) == list(stats[c]["count"]), c
    _close(devs)


def test_plain_sweep_bins_and_series_against_the_log_replay(setup):
    """The same through ceg_mc_group_sweep on the Na + 4 CO2 CIT-7 chains, the map on the UNIT cell (supercell 2x3x3) with the three
    symmetry operations: count all zero, delta_swaps == 0, delta_moves of the last frame == stats.delta bit for bit."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    K, S, first, every, start = 3, 43, 5, 8, 16
    frames = mcrng.sampler_frames(first, S, every, start)
    assert frames == [23, 31, 39, 47]
    devs = _new_chains(setup, K)
    kinds = _kinds(mc)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(every, from_step=start, step=1.0, supercell=(2, 3, 3), channels={kinds[0][0]: 0, kinds[1][0]: 1, kinds[1][1]: 2},
                          chain_map=[1, -1, 0], symmetries=SYMMETRIES, series_capacity=8)
        samp = group.sampler
        starts = [_start(d) for d in devs]
        stats, log = group.sweep(S, SEED + 910, first, temperature=[300.0, 500.0, 900.0], dmax=0.5, thetamax=1.0, p_rotation=0.5,
                                 stream_id=[4, 9, 2], log=True)
        bins, series, total = group.sampler_read()
    assert (log["accepted"] != 0).sum() > 0
    states = _replayed_frames(starts, log, first, frames, None)
    _check_counts(series, states, frames, 0, "plain")
    want = _host_bins(samp, states, kinds)
    assert np.array_equal(bins, want)
    assert bins.sum() == 2 * len(frames) * (1 + 3) * 13 and list(total) == [len(frames) * 4 * 18] * 2
    for c in range(K):
        assert not series[:, c]["delta_swaps"].any()
        assert series[-1, c]["delta_moves"].tobytes() == stats[c]["delta"].tobytes(), c
        running, f = 0.0, 0
        for s in range(S):
            rec = log[s, c]
            if rec["accepted"]:
                rows = rec["rows"]
                running += (((rows[1][0] + rows[1][1]) + rows[1][2]) + rows[1][3]) - (((rows[0][0] + rows[0][1]) + rows[0][2]) + rows[0][3])
            if first + s in frames:
                done = log["accepted"][:s + 1, c] != 0
                tol = 1e-12 * float(np.abs(log["rows"][:s + 1, c][done]).max(initial=0.0)) * max(int(done.sum()), 1)
                assert abs(series[f, c]["delta_moves"] - running) <= tol, (c, f)
                f += 1
    _close(devs)


def _edge_points(unit, supercell, dims, rng):
    """the edge cases of tests/test_mc_sampler_host.py carried to a cell, plus 500 random points"""
    n = np.asarray(dims, dtype=np.float64)
    frac = [np.zeros(3), np.array([3.0, -2.0, 7.0]), np.array([1.0, 1.0, 1.0]) / n, np.array([2.0, 1.0, 3.0]) / n, (n - 1.0) / n,
            np.array([0.25, 0.5, 0.75]), np.array([5.3125, -2.65625, 0.875]), np.array([0.5, 0.1, 0.9]) + np.array([1.0, 2.0, 1.0])]
    pts = [unit @ f for f in frac] + [np.full(3, -1e-20), np.zeros(3), unit @ np.array([1.0, 0.0, 0.0]), -(unit @ np.array([0.0, 1.0, 0.0]))]
    mc_cell = unit * np.asarray(supercell, dtype=np.float64)[None, :]
    return np.concatenate([np.array(pts), rng.uniform(-2.0, 3.0, (500, 3)) @ mc_cell.T])


def _set_atoms(dev, points, kinds):
    """`points` as one-atom molecules of the given kinds, straight through ceg_mc_set_guests"""
    pos = np.ascontiguousarray(points, dtype=np.float64)
    k = np.ascontiguousarray(kinds, dtype=np.int32)
    first = np.arange(len(pos) + 1, dtype=np.int32)
    _abi.check(dev._lib, dev._lib.ceg_mc_set_guests(dev._h, _abi.dptr(pos.reshape(-1)), _abi.i32ptr(k), _abi.i32ptr(first), len(pos)))


@pytest.mark.parametrize("case", ["cha", "cit7", "cit7-symmetries"])
def test_edge_placements_through_sample(cha, setup, case):
    """One-atom molecules put at the CPU test's edge positions (bin edges, lattice points, y = -1e-20, images several cells away) and at
    500 random places, across K = 2 chains, on the triclinic CHA cell and on the CIT-7 2x3x3 MC cell folded onto its unit cell, once
    with three symmetry operations: one frame through ceg_mc_group_sample, bins exactly those of bin_positions, step == -1."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    fixture, supercell = (cha, (1, 1, 1)) if case == "cha" else (setup, (2, 3, 3))
    mc = fixture[0]
    unit = np.asarray(mc.mat, dtype=np.float64) / np.asarray(supercell, dtype=np.float64)[None, :]
    dims = tuple(int(x) for x in np.floor(np.linalg.norm(unit, axis=0) / 0.7))
    pts = _edge_points(unit, supercell, dims, np.random.default_rng(21))
    ka, kb = sorted({k for ids in _kinds(mc) for k in ids})[:2]
    kinds = np.where(np.arange(len(pts)) % 3 == 0, ka, kb)
    cut = 270                                                   # chain 0: two tiles, chain 1: one
    devs = _new_chains(fixture, 2, [[] for _ in mc.positions])
    _set_atoms(devs[0], pts[:cut], kinds[:cut])
    _set_atoms(devs[1], pts[cut:], kinds[cut:])
    syms = SYMMETRIES if case.endswith("symmetries") else ()
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(1, dims=dims, supercell=supercell, channels={ka: 1, kb: 0}, chain_map=[0, 0], symmetries=syms, series_capacity=1)
        samp = group.sampler
        group.sample()
        bins, series, total = group.sampler_read()
        with pytest.raises(_abi.CegError) as full:               # the series is full
            group.sample()
        assert full.value.code == -1
    want = np.zeros_like(bins)
    for ch, k in ((1, ka), (0, kb)):
        mcrng.bin_positions(want[0, ch], samp["unit_invmat"], pts[kinds == k], samp["symmetries"])
    assert np.array_equal(bins, want)
    assert bins.sum() == len(pts) * (1 + len(syms)) and list(total) == [(1 + len(syms)) * int(np.prod(supercell)) * 2]
    # the edge points themselves, one by one
    edge = mcrng.bin_index(samp["unit_invmat"], dims, pts[:12])
    assert all(bins[0, 1 if kinds[q] == ka else 0, edge[q, 2], edge[q, 1], edge[q, 0]] >= 1 for q in range(12))
    assert series.shape == (1, 2)
    for c, n in enumerate((cut, len(pts) - cut)):
        rec = series[0, c]
        assert (rec["step"], rec["nmol"], rec["natoms"]) == (-1, n, n) and not rec["count"].any() and rec["delta_moves"] == 0.0 == rec["delta_swaps"]
    _close(devs)


def test_a_chain_of_more_than_one_tile_beside_an_empty_chain(setup):
    """4 Na + 104 CO2 + 156 X of the many-molecules fixture (472 atom slots: two tiles of k_mcg_sample), four molecules removed so that
    free slots lie in both tiles, beside an EMPTY chain: two frames through sample(), two through a plain sweep.  Every bin sum equals
    atoms of the channel x frames, the bins are exact against the host, the empty chain's records are zero."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_many_molecules import ROUTES, _device_chain, _populate, _three_kinds
    mc, _owner = setup
    mcd = _three_kinds(mc)
    positions = _populate(mcd, list(ROUTES["counts"]), 7300)
    big = _device_chain(setup, mcd, positions)
    for i, j in ROUTES["holes"]:                                 # the last molecule of the kind takes index j (montecarlo.jl:798-808)
        big.remove((i, j))
        big.mc.positions[i][j] = big.mc.positions[i][-1]
        big.mc.positions[i].pop()
    empty = _device_chain(setup, mcd, [[], [], []])
    kinds = _kinds(mcd)
    natoms = sum(len(p) for kind in big.mc.positions for p in kind)
    assert natoms > 256 and sum(len(k) for k in big.mc.positions[1]) >= 100
    channel_of = {kinds[0][0]: 0, kinds[1][0]: 1, kinds[1][1]: 2}
    S, every = 16, 8
    with DeviceMonteCarloGroup([big, empty]) as group:
        group.set_sampler(every, step=1.0, supercell=(2, 3, 3), channels=channel_of, chain_map=[0, 0], series_capacity=4)
        samp = group.sampler
        start = _start(big)
        group.sample()
        group.sample()
        stats, log = group.sweep(S, SEED + 920, 0, temperature=500.0, dmax=0.4, thetamax=0.8, p_rotation=0.5, stream_id=[6, 7], log=True)
        bins, series, total = group.sampler_read()
    assert series.shape == (4, 2) and list(series[:, 0]["step"]) == [-1, -1, 7, 15]
    assert (log["accepted"][:, 0] != 0).sum() > 0
    swept = _replayed_frames([start], log, 0, [7, 15], None)[0]
    states = [[start, start] + swept, [([], [])] * 4]
    want = _host_bins(samp, states, kinds)
    assert np.array_equal(bins, want)
    spec0 = start[0]
    per_channel = [0, 0, 0]
    for s in spec0:
        for kind in kinds[s]:
            per_channel[channel_of[kind]] += 1
    assert [int(bins[0, ch].sum()) for ch in range(3)] == [4 * n for n in per_channel] and sum(per_channel) == natoms
    for f in range(4):
        assert (series[f, 0]["nmol"], series[f, 0]["natoms"]) == (len(spec0), natoms)
        assert (series[f, 1]["nmol"], series[f, 1]["natoms"]) == (0, 0) and series[f, 1]["delta_moves"] == 0.0
    _close([big, empty])


def _gcmc_args(group, K):
    table = group.gcmc_species([NA_MOVES, CO2_MOVES], [3000.0, 3000.0])
    return dict(temperature=np.linspace(300.0, 900.0, K), dmax=0.5, thetamax=1.0, species=table, max_molecules=12,
                stream_id=np.arange(K, dtype=np.uint32) * 5 + 2)


def _state_bytes(dev):
    n = sum(len(dev.mc.ffidx[i]) * len(kind) for i, kind in enumerate(dev._slot))
    nk = len(dev.mc.ewald.kfactors) if dev.mc.ewald.alpha != 0.0 else 0
    pos, re, im = np.zeros((n, 3)), np.zeros(max(nk, 1)), np.zeros(max(nk, 1))
    _abi.check(dev._lib, dev._lib.ceg_mc_get_state(dev._h, _abi.dptr(pos.reshape(-1)) if n else None, _abi.dptr(re), _abi.dptr(im)))
    return pos.tobytes() + re.tobytes() + im.tobytes()


def test_the_sweep_is_untouched_by_the_sampler(setup):
    """The same GCMC sweep on two identical groups, one with a sampler (map, symmetries, a frame every third step): statistics, log
    and ceg_mc_get_state of every chain identical byte for byte."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 3, 60
    results = []
    for sampled in (False, True):
        devs = _new_chains(setup, K)
        with DeviceMonteCarloGroup(devs) as group:
            if sampled:
                group.set_sampler(3, step=0.8, supercell=(2, 3, 3), symmetries=SYMMETRIES, series_capacity=S)
            stats, log = group.sweep_gcmc(S, SEED + 930, 11, log=True, **_gcmc_args(group, K))
            if sampled:
                bins, series, _total = group.sampler_read()
                assert len(series) == 20 and bins.sum() > 0
        results.append((stats.tobytes(), log.tobytes(), [_state_bytes(d) for d in devs], int(stats["accepted"].sum())))
        _close(devs)
    assert results[0][:3] == results[1][:3]
    assert results[0][3] > 0


def test_accumulation_reset_capacity_and_series_only(setup):
    """Two sweeps append to bins and series; reset zeroes both; a sweep whose frames exceed what is left of series_capacity returns
    CEG_ERR_INVALID with chain states, bins and frames unchanged; a sampler without a map keeps the series alone."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 2
    devs = _new_chains(setup, K)
    with DeviceMonteCarloGroup(devs) as group:
        args = _gcmc_args(group, K)
        group.set_sampler(4, step=1.0, supercell=(2, 3, 3), series_capacity=5)
        group.sweep_gcmc(8, SEED + 940, 0, **args)                          # frames after steps 3, 7
        b1, s1, t1 = group.sampler_read()
        assert list(s1[:, 0]["step"]) == [3, 7] and list(t1) == [2 * 18 * 2]
        group.sweep(12, SEED + 941, 8, temperature=400.0, dmax=0.5, thetamax=1.0)      # 11, 15, 19 through the plain sweep
        b2, s2, t2 = group.sampler_read()
        assert list(s2[:, 1]["step"]) == [3, 7, 11, 15, 19] and s2[:2].tobytes() == s1.tobytes()
        assert b2.sum() == b1.sum() + int(s2[2:]["natoms"].sum()) and (b2 >= b1).all() and list(t2) == [5 * 18 * 2]
        # the series is full: one more frame does not fit; nothing moves
        before = [_state_bytes(d) for d in devs]
        with pytest.raises(_abi.CegError) as e:
            group.sweep_gcmc(4, SEED + 942, 20, **args)
        assert e.value.code == -1 and "frames" in str(e.value)
        with pytest.raises(_abi.CegError) as e:
            group.sweep(4, SEED + 942, 20, temperature=400.0, dmax=0.5, thetamax=1.0)
        assert e.value.code == -1
        b3, s3, _t = group.sampler_read()
        assert [_state_bytes(d) for d in devs] == before and np.array_equal(b3, b2) and s3.tobytes() == s2.tobytes()
        group.sweep_gcmc(3, SEED + 942, 20, **args)                         # steps 20 .. 22: no frame, allowed
        assert len(group.sampler_read()[1]) == 5
        group.sampler_reset()
        b4, s4, t4 = group.sampler_read()
        assert not b4.any() and s4.shape == (0, K) and list(t4) == [0]
        group.sweep_gcmc(4, SEED + 943, 24, **args)                         # room again; the records start at the front
        b5, s5, _t = group.sampler_read()
        assert list(s5[:, 0]["step"]) == [27] and b5.sum() == int(s5["natoms"].sum())
        # series only
        group.set_sampler(2, from_step=30, series_capacity=3)
        group.sweep_gcmc(6, SEED + 944, 28, **args)                         # 28 .. 33: frames after 31, 33
        b6, s6, t6 = group.sampler_read()
        assert b6 is None and len(t6) == 0 and list(s6[:, 0]["step"]) == [31, 33]
        assert all(s6[f, c]["nmol"] == s6[f, c]["count"].sum() and s6[f, c]["natoms"] >= s6[f, c]["nmol"] for f in range(2) for c in range(K))
        # removed: sweeps run as before, reading is refused
        group.set_sampler(None)
        group.sweep_gcmc(4, SEED + 945, 34, **args)
        with pytest.raises(RuntimeError):
            group.sampler_read()
        assert devs[0]._lib.ceg_mc_group_sampler_read(group._h, None, None, None) == -1
    _close(devs)


def test_bad_specs_are_refused_and_the_earlier_sampler_stays(setup):
    """Every bad spec of the header gives CEG_ERR_INVALID; afterwards the sampler installed before is still in force (a frame through
    sample() lands in its map)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 2
    devs = _new_chains(setup, K)
    nkinds = devs[0].mc.ff.nkinds
    lib = devs[0]._lib
    inv = np.linalg.inv(np.asarray(devs[0].mc.mat, dtype=np.float64))
    cmap, kch = np.zeros(K, dtype=np.int32), np.zeros(nkinds, dtype=np.int32)
    sym = np.zeros((2, 3, 4))
    sym[:, :, :3] = np.eye(3)

    def spec(**over):
        f = dict(every=4, from_step=0, series_capacity=4, dims=(5, 6, 7), nmaps=1, nchannels=1, nkinds=nkinds, nsym=2, unit_invmat=inv.T.reshape(-1),
                 chain_map=cmap, kind_channel=kch, sym=sym)
        f.update(over)
        ptr = lambda a: None if a is None else a.ctypes.data
        keep.append(f)
        return _abi.MC_SAMPLER(f["every"], f["from_step"], f["series_capacity"], (C.c_int32 * 3)(*f["dims"]), f["nmaps"], f["nchannels"], f["nkinds"],
                               f["nsym"], 0, (C.c_double * 9)(*f["unit_invmat"]), ptr(f["chain_map"]), ptr(f["kind_channel"]), ptr(f["sym"]))

    keep = []
    bad_inv, bad_sym = inv.T.reshape(-1).copy(), sym.copy()
    bad_inv[4] = np.inf
    bad_sym[1, 2, 3] = np.nan
    bad = dict(every_zero=dict(every=0), every_negative=dict(every=-3), from_step=dict(from_step=-1), capacity=dict(series_capacity=-1),
               mixed_dims=dict(dims=(5, 0, 7)), negative_dim=dict(dims=(5, -1, 7)), nmaps=dict(nmaps=0), nchannels=dict(nchannels=0),
               chain_map_high=dict(chain_map=np.array([0, 1], dtype=np.int32)), chain_map_low=dict(chain_map=np.array([-2, 0], dtype=np.int32)),
               kind_channel_high=dict(kind_channel=np.full(nkinds, 1, dtype=np.int32)),
               kind_channel_low=dict(kind_channel=np.full(nkinds, -2, dtype=np.int32)), invmat=dict(unit_invmat=bad_inv), sym=dict(sym=bad_sym),
               nsym_high=dict(nsym=192, sym=np.zeros((192, 3, 4))), nsym_negative=dict(nsym=-1), no_chain_map=dict(chain_map=None),
               no_kind_channel=dict(kind_channel=None), no_sym=dict(sym=None), too_many_bins=dict(dims=(2048, 1024, 1024)),
               nsym_high_without_a_map=dict(dims=(0, 0, 0), nsym=192))
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(1, dims=(3, 4, 5), series_capacity=len(bad) + 1)
        for f, (name, over) in enumerate(bad.items()):
            s = spec(**over)
            assert lib.ceg_mc_group_set_sampler(group._h, C.addressof(s)) == -1, name
            assert b"sampler" in lib.ceg_last_error(), name
            group.sample()
            bins, series, _total = group.sampler_read()
            assert bins.shape == (1, 1, 5, 4, 3) and len(series) == f + 1 and bins.sum() == 26 * (f + 1), name
        for kw in (dict(chain_map=[-1, -1]), dict(channels=[-1] * nkinds)):             # the wrapper names these before the library is asked
            with pytest.raises(ValueError):
                group.set_sampler(1, dims=(3, 4, 5), series_capacity=2, **kw)
        assert group.sampler["dims"] == (3, 4, 5) and len(group.sampler_read()[1]) == len(bad)
        good = spec()
        assert lib.ceg_mc_group_set_sampler(group._h, C.addressof(good)) == 0                 # the base of the bad ones is a valid spec
        frames = C.c_int64(-1)
        assert lib.ceg_mc_group_sampler_read(group._h, None, None, C.byref(frames)) == 0 and frames.value == 0
        assert lib.ceg_mc_group_set_sampler(None, C.addressof(good)) == -1
        assert lib.ceg_mc_group_sample(None) == -1 and lib.ceg_mc_group_sampler_reset(None) == -1
    _close(devs)


def test_empty_chains_still_give_their_records(setup):
    """A plain sweep of two empty chains with no log launches nothing per step; with a sampler the frames are still taken: one record per
    chain and frame with zero molecules and atoms, nothing binned."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    devs = _new_chains(setup, 2, [[] for _ in mc.positions])
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(2, dims=(3, 4, 5), series_capacity=3)
        stats = group.sweep(5, SEED + 950, 0, temperature=300.0, dmax=0.5, thetamax=1.0)
        bins, series, total = group.sampler_read()
    assert not stats["translation_trials"].any() and not bins.any() and list(total) == [2 * 2]
    assert series.shape == (2, 2) and list(series[:, 1]["step"]) == [1, 3] and not series["nmol"].any() and not series["natoms"].any()
    _close(devs)
