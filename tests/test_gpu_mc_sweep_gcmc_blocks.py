"""Block pockets in the GCMC sweeps of a chain group (ceg_mc_group_set_blocks): the inblockpocket test and the 1000-attempt retry loop
of choose_step! (src/simulation.jl:271-326) resolved on the device.  Every record of a sweep -- attempt index and pocket flag
included -- is checked against ceg_hip.mcrng.propose_gcmc(..., blocks=...) and the ORACLE's state, as test_gpu_mc_sweep_gcmc does
without masks.  The masks: a synthetic species mask of 40 spheres of 2.1 A at random fractional centres on the framework's 0.15 A
lattice (0.69 of the CIT-7 unit cell), and the real atom masks, BlockFile(grid) of the fixture's VdW grids.
Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from ceg_hip.hostmirror.coordinates import offsetpoint
from test_gpu_mc_sweep import SEED, _chains, _close, _device_order, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES, Replay, _clone, _distinct_states, _follow, _mcrng_species, _tail

pytestmark = pytest.mark.gpu

RETRIED = (2, 4, 5)


@pytest.fixture(scope="module")
def masks(setup, tmp_path_factory):
    """(species blocks [Na: none, CO2: the spheres], atom blocks per force-field index) of the fixture"""
    from ceg_hip.grids import blockfile_from_grid_gpu, parse_blockfile_gpu
    mc, _owner = setup
    cset = next(g.csetup for g in mc.grids if g is not None)
    centers = np.random.default_rng(2024).random((40, 3))
    file = tmp_path_factory.mktemp("blocks") / "spheres.block"
    file.write_text("40\n" + "".join(f"{x:.6f} {y:.6f} {z:.6f} 2.1\n" for x, y, z in centers))
    spheres = parse_blockfile_gpu(file, cset)
    assert 0.6 < spheres.block.mean() < 0.8, spheres.block.mean()
    atoms = [None if g is None else blockfile_from_grid_gpu(g) for g in mc.grids]
    for ids in mc.ffidx:
        assert all(atoms[ix - 1] is not None and 0.05 < atoms[ix - 1].block.mean() < 0.999 for ix in ids)
    return [None, spheres], atoms


class TrackedBlocks(mcrng.Blocks):
    """mcrng.Blocks that remembers how close a tested coordinate came to a half-integer of the lattice, where the verdict would hang
    on the last bit of the arithmetic"""

    def __init__(self, species, atoms=()):
        super().__init__(species, atoms)
        self.margin = 0.5

    def _track(self, b, point, half):
        if b is not None and not b.empty:
            off = (b.csetup.size / b.csetup.dims) / 2.0 if half else 0.0
            x = offsetpoint(np.asarray(point, dtype=np.float64) + off, b.csetup)
            self.margin = min(self.margin, float(np.abs(x - np.floor(x) - 0.5).min()))

    def species_blocked(self, i, point):
        self._track(self.species[i], point, False)
        return super().species_blocked(i, point)

    def atom_blocked(self, kind, point):
        if self.atoms:
            self._track(self.atoms[kind], point, True)
        return super().atom_blocked(kind, point)


class BlockReplay(Replay):
    """Replay with the masks: the proposal comes from propose_gcmc(..., blocks=...), a pocket-blocked step is followed here (no row, no
    decision), every other step by Replay.step on that proposal; the attempt index and the pocket flag of every record are checked."""

    def __init__(self, *args, blocks):
        super().__init__(*args)
        self.blocks = blocks
        self.species = [s._replace(kinds=tuple(int(x) for x in t["kinds"][:t["m"]])) for s, t in zip(self.species, self.table)]
        self.pocket = self.attempts = 0
        self.cover = set()
        self.attempt_log = []

    def step(self, seed, step, sid, rec=None, what=None):
        omc, tab = self.omc, self.tab
        pr = mcrng.propose_gcmc(seed, step, sid, [i for i, _j in tab], [omc.positions[i][j] for i, j in tab], self.species, self.mc.mat,
                                self.dmax, self.thetamax, self.cap, self.blocks)
        kind = pr.kind
        if rec is not None:                      # no record is exempt
            assert rec["flags"] >> 16 == pr.attempt and bool(rec["flags"] & 8) == pr.pocket, (what, rec, pr)
        if pr.spent or pr.capacity:
            assert (pr.attempt, pr.pocket) == (0, False)
        else:
            self.attempts += pr.attempt
            if kind != 6:
                self.attempt_log.append(pr.attempt)
            if pr.attempt >= 16:
                self.cover.add("second pass")
            if kind in RETRIED and pr.attempt > 0 and not pr.pocket:
                self.cover.add(("retried", kind))
            if kind == 5 and pr.pocket and pr.attempt < 999:
                self.cover.add("insertion: bead free, pocket-blocked")
            if kind not in RETRIED and pr.pocket:
                self.cover.add(("pocket", kind))
        if not pr.pocket:
            before = self.accepted[5]
            with mock.patch.object(mcrng, "propose_gcmc", lambda *a, **k: pr):
                super().step(seed, step, sid, rec, what)
            if kind == 5 and pr.attempt > 0 and self.accepted[5] > before:
                self.cover.add("insertion: retried and accepted")
            return
        exhausted = len(pr.positions) == 0
        assert (kind in RETRIED and pr.attempt == 999) if exhausted else True, pr
        self.records += 1
        if rec is not None:
            m = int(self.table[pr.species]["m"])
            assert (rec["species"], rec["kind"], rec["n_species"], rec["molecule"]) == (pr.species, kind, pr.n_species, pr.molecule), (what, rec, pr)
            assert rec["u"] == pr.u and rec["flags"] == (8 | pr.attempt << 16) and not rec["accepted"], (what, rec)
            assert not rec["rows"].any() and rec["tc"] == 0.0, (what, rec)
            if exhausted:
                assert not rec["positions"].any(), (what, rec)
            else:
                assert np.abs(rec["positions"][:m] - pr.positions).max() <= 1e-12 and not rec["positions"][m:].any(), (what, rec, pr)
        self.trials[kind] += 1
        self.blocked += 1
        self.pocket += 1

    def check_counts(self, group_counts, c):
        pocket, attempts = group_counts
        assert (int(pocket[c]), int(attempts[c])) == (self.pocket, self.attempts), (c, pocket, attempts, self.pocket, self.attempts)


WANTED = {("retried", 2), ("retried", 4), "insertion: retried and accepted", "insertion: bead free, pocket-blocked", ("pocket", 0), ("pocket", 3),
          "second pass"}


def _block_replays(devs, omcs, table, T, dmax, thetamax, caps, blocks):
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (len(devs),))
    reps = [BlockReplay(d.mc, o, _device_order(d), table, T[c], dmax, thetamax, caps[c], blocks=blocks) for c, (d, o) in enumerate(zip(devs, omcs))]
    for rep in reps:
        rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
    return reps


def test_gcmc_blocks_replay_against_the_oracle(setup, masks):
    """4 chains x 150 steps with the species mask and the atom masks; CO2 with all six move kinds.  The candidate (phiPV_div_k, step
    sizes, seed) is picked on the CPU: the first whose PREDICTED run holds every case of WANTED and the outcomes the test without masks
    asks for, and in which no tested coordinate comes within 1e-9 lattice units of a half-integer."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 4, 150
    species_blocks, atom_blocks = masks
    devs, omcs = _chains(setup, K, oracle=True)
    _distinct_states(devs, omcs)
    T = np.linspace(100.0, 1000.0, K)
    sid = np.arange(K, dtype=np.uint32) * 5 + 2
    first = 2 ** 32 - 70
    caps = [12] * K
    with DeviceMonteCarloGroup(devs) as group:
        chosen = None
        for phi, dmax, thetamax, seed in ((3e5, 0.5, 1.0, SEED), (3e6, 1.0, 2.0, SEED + 1), (3e4, 0.25, 0.5, SEED + 2), (3e5, 0.5, 1.0, SEED + 3),
                                          (3e7, 0.5, 1.0, SEED + 4), (3e5, 1.0, 1.0, SEED + 5), (3e6, 0.5, 1.0, SEED + 6), (3e5, 0.5, 2.0, SEED + 7)):
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [phi, phi]))
            tracked = TrackedBlocks(species_blocks, atom_blocks)
            pred = _block_replays(devs, [_clone(o) for o in omcs], table, T, dmax, thetamax, caps, tracked)
            for s in range(S):
                for c, rep in enumerate(pred):
                    rep.step(seed, first + s, int(sid[c]))
            cover = set().union(*[rep.cover for rep in pred])
            seen = set().union(*[rep.seen for rep in pred])
            print(f"candidate phiPV_div_k {phi}, dmax {dmax}, thetamax {thetamax}: missing {WANTED - cover}, outcomes {sorted(seen)}, "
                  f"margin {tracked.margin:.3e}")
            if WANTED <= cover and tracked.margin > 1e-9 and {(5, True), (5, False), (6, True)} <= seen:
                chosen = (phi, dmax, thetamax, seed, table)
                break
        assert chosen is not None, "no candidate exercises every branch on the oracle"
        phi, dmax, thetamax, seed, table = chosen
        group.set_blocks(species_blocks, atom_blocks)
        stats, log = group.sweep_gcmc(S, seed, first, temperature=T, dmax=dmax, thetamax=thetamax, species=table, max_molecules=caps,
                                      stream_id=sid, log=True)
        counts = group.block_counts()
    assert log.shape == (S, K)
    reps = _block_replays(devs, omcs, table, T, dmax, thetamax, caps, mcrng.Blocks(species_blocks, atom_blocks))
    _follow(reps, log, seed, first, sid)
    exempt = sum(rep.exempt for rep in reps)                 # (decisions within 1e-12 of their threshold, as in the test without masks)
    assert exempt <= 0.01 * S * K, exempt
    cover = set().union(*[rep.cover for rep in reps])
    assert WANTED <= cover, WANTED - cover
    for c, rep in enumerate(reps):
        rep.check_stats(stats[c], c)
        rep.check_counts(counts, c)
        rep.check_state(devs[c], c)
        assert ((log["flags"][:, c] & 8) != 0).sum() == rep.pocket
    attempts = np.concatenate([rep.attempt_log for rep in reps])
    print(f"gcmc blocks replay: {K} chains x {S} steps, pocket-blocked {[r.pocket for r in reps]}, attempt index mean {attempts.mean():.2f} "
          f"max {attempts.max()}, {int((attempts >= 16).sum())} of 16 and above, trials {sum(r.trials for r in reps)}, "
          f"accepted {sum(r.accepted for r in reps)}")
    _close(devs)


def test_gcmc_blocks_exhaustion(setup, masks):
    """One chain, CO2 with an all-ones species mask (Na with none), 12 steps: every random_translation, random_reinsertion and insertion
    of CO2 runs out of attempts (index 999, pocket flag, no positions), its translations and rotations are pocket-blocked at attempt 0,
    and no CO2 moves."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from ceg_hip.grids import BlockFile
    S = 12
    cset = masks[0][1].csetup
    full = BlockFile(cset, np.ones(tuple(int(d) + 1 for d in cset.dims), dtype=bool))
    co2 = mcrng.MoveTable(translation=1, rotation=1, random_translation=2, random_rotation=1, random_reinsertion=2, swap=2)
    devs, omcs = _chains(setup, 1, oracle=True)
    before = [p.copy() for p in omcs[0].positions[1]]
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species([NA_MOVES, co2], [1e9, 1e9]))
        group.set_blocks([None, full])
        # (the species and the kind of a step follow from the seed alone: the first seed with every retried kind and a single-proposal
        #  kind of CO2 among the 12 steps)
        for seed in range(SEED + 100, SEED + 200):
            picks = [mcrng.propose_gcmc(seed, s, 0, [0, 1], [omcs[0].positions[0][0], before[0]], _mcrng_species(table), devs[0].mc.mat, 0.5, 1.0, 12)
                     for s in range(S)]
            kinds = {p.kind for p in picks if p.species == 1}
            if {2, 4, 5} <= kinds and kinds & {0, 1, 3} and 6 not in kinds:
                break
        else:
            raise AssertionError("no seed with the wanted kinds")
        stats, log = group.sweep_gcmc(S, seed, 0, temperature=300.0, dmax=0.5, thetamax=1.0, species=table, max_molecules=12, log=True)
        counts = group.block_counts()
    reps = _block_replays(devs, omcs, table, 300.0, 0.5, 1.0, [12], mcrng.Blocks([None, full]))
    _follow(reps, log, seed, 0, [0])
    seen = set()
    for rec in log[:, 0]:
        if rec["species"] != 1:
            assert not rec["flags"] & 8 and rec["flags"] >> 16 == 0, rec
            continue
        seen.add(int(rec["kind"]))
        want = 8 | 999 << 16 if rec["kind"] in RETRIED else 8
        assert rec["flags"] == want and not rec["accepted"] and not rec["rows"].any(), rec
        assert rec["positions"].any() == (rec["kind"] not in RETRIED), rec
    assert {2, 4, 5} <= seen and seen & {0, 1, 3}, seen
    reps[0].check_stats(stats[0], 0)
    reps[0].check_counts(counts, 0)
    reps[0].check_state(devs[0], 0)
    assert len(devs[0].mc.positions[1]) == len(before) and all(np.array_equal(a, b) for a, b in zip(devs[0].mc.positions[1], before))
    assert counts[0][0] == reps[0].pocket == (log["species"][:, 0] == 1).sum()
    _close(devs)


def test_gcmc_without_masks_is_the_sweep_it_was(setup, masks):
    """Three groups from one state, 100 steps: one never given masks, one given all-NULL masks (the resolve stage runs and finds every
    first attempt free), one given the real masks and then cleared.  Logs, statistics and states are the same bytes."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 2, 100
    species_blocks, atom_blocks = masks
    kw = dict(temperature=[300.0, 700.0], dmax=0.4, thetamax=0.8, max_molecules=[10, 10], stream_id=[4, 9], log=True)
    runs = []
    for variant in ("never", "null", "cleared"):
        devs, _ = _chains(setup, K)
        with DeviceMonteCarloGroup(devs) as group:
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [5000.0, 5000.0]))
            if variant == "null":
                group.set_blocks([None, None], [None] * len(atom_blocks))
            elif variant == "cleared":
                group.set_blocks(species_blocks, atom_blocks)
                group.set_blocks(None)
            stats, log = group.sweep_gcmc(S, SEED + 60, 7, species=table, **kw)
            assert not group.block_counts()[0].any() and not group.block_counts()[1].any()
            runs.append((stats.tobytes(), log.tobytes(), [tuple(x.tobytes() for x in d.state()) for d in devs]))
        _close(devs)
    assert runs[0] == runs[1], "all-NULL masks changed the sweep"
    assert runs[0] == runs[2], "cleared masks changed the sweep"
    log = np.frombuffer(runs[0][1], dtype=_abi.GCMC_RECORD_DTYPE)
    assert (log["accepted"] != 0).any() and not (log["flags"] >> 3).any()


def test_gcmc_blocks_refusals_leave_the_state_alone(setup, masks):
    """Masks for another number of species, a species' atom kind without an atom block, the plain sweep with masks installed: each is
    refused before anything is launched."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    species_blocks, atom_blocks = masks
    devs, _ = _chains(setup, 2)
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0)
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [1000.0, 1000.0]))
        before = [d.state() for d in devs]

        def unchanged():
            for d, (p, sf) in zip(devs, before):
                p2, sf2 = d.state()
                assert np.array_equal(p, p2) and np.array_equal(sf, sf2)

        group.set_blocks(species_blocks[1:], atom_blocks)                      # one species block for a table of two
        with pytest.raises(_abi.CegError) as ei:
            group.sweep_gcmc(5, SEED, 0, species=table, max_molecules=8, **good)
        assert ei.value.code == -1 and "nspecies" in str(ei.value)
        unchanged()
        top = int(max(t["kinds"][:t["m"]].max() for t in table))
        group.set_blocks(species_blocks, atom_blocks[:top])                    # the highest kind of the table has no atom block
        with pytest.raises(_abi.CegError) as ei:
            group.sweep_gcmc(5, SEED, 0, species=table, max_molecules=8, **good)
        assert ei.value.code == -1 and "atom block" in str(ei.value)
        unchanged()
        group.set_blocks(species_blocks, atom_blocks)
        params = dict(p_rotation=0.5, **good)
        stats = np.zeros(2, dtype=_abi.SWEEP_STATS_DTYPE)
        sid, T, z, pr = np.arange(2, dtype=np.uint32), np.full(2, 300.0), np.full(2, 0.5), np.full(2, 0.5)
        beads = np.zeros(16, dtype=np.int32)
        sp = _abi.SweepParams(1, 0, sid.ctypes.data, T.ctypes.data, z.ctypes.data, z.ctypes.data, pr.ctypes.data, beads.ctypes.data)
        assert group._lib.ceg_mc_group_sweep(group._h, C.addressof(sp), 5, stats.ctypes.data, None) == -5          # CEG_ERR_UNSUPPORTED
        with pytest.raises(_abi.CegError) as ei:
            group.sweep(5, SEED, 0, **params)
        assert ei.value.code == -5 and "block" in str(ei.value)
        unchanged()
        # bad masks are refused too, and leave the installed ones in place
        table_b = np.zeros(1, dtype=_abi.MC_BLOCK_DTYPE)
        assert group._lib.ceg_mc_group_set_blocks(group._h, table_b.ctypes.data, 1, None, 0) == -1                  # dims 0
        assert group._lib.ceg_mc_group_set_blocks(group._h, None, 9, None, 0) == -1
        with pytest.raises(_abi.CegError):
            group.sweep(5, SEED, 0, **params)
        group.set_blocks(None)
        out = group.sweep(5, SEED, 0, **params)                                # cleared: a valid call follows
        assert (out["translation_trials"] + out["rotation_trials"] == 5).all()
    _close(devs)
