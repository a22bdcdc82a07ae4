"""GCMC sweeps of a chain group (ceg_mc_group_sweep_gcmc): species, move kind (all six of mcmoves.jl:1-8), molecule, proposal,
decision and update -- insertions and deletions included -- of S steps of K chains on the device, the molecule table owned by the
device.  The log is checked record by record against ceg_hip.mcrng.propose_gcmc, against the ORACLE's state of every chain
(oracle/montecarlo.OracleMonteCarlo: movement_energy / insertion_energy, update / add / remove), against
hostmirror.modify_species_dryrun and against the swap rule in NumPy.  Run with `pytest -m gpu` on an MI355X."""
import copy
import ctypes as C

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from ceg_hip.hostmirror import montecarlo as M
from test_gpu_mc_chains import _check
from test_gpu_mc_sweep import SEED, _chains, _close, _copy, _device_order, _rule, setup  # noqa: F401  (setup: the module's fixture)

pytestmark = pytest.mark.gpu

DISPLACEMENTS = (0, 1, 2, 3, 4)
NA_MOVES = mcrng.MoveTable(translation=1, random_translation=1)
CO2_MOVES = mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1, random_reinsertion=2, swap=4)
SWAP_ONLY = mcrng.MoveTable(swap=1)


def _clone(omc):
    o = copy.copy(omc)
    o.positions = [[p.copy() for p in kind] for kind in omc.positions]
    if omc.sums_re is not None:
        o.sums_re, o.sums_im = omc.sums_re.copy(), omc.sums_im.copy()
    return o


def _mcrng_species(table):
    return [mcrng.GcmcSpecies(t["model"][:t["m"]].copy(), int(t["bead"]), mcrng.MoveTable(cumulatives=t["cumulative"])) for t in table]


def _tail(table):
    """The species table with a tail correction: the fixture's setup carries none (tail_cross is None), and the table is an input of
    the call -- framework rows of -40 ... K and a symmetric cross matrix of a few to -150 K, so that the change of a swap is of the
    order of the insertion energies of CO2 (1e3 K) and enters the decisions."""
    ns = len(table)
    t = table.copy()
    fw = [-40.0, -120.0, -15.0, -300.0]
    cross = np.array([[-3.0, -8.0, -1.5, -20.0], [-8.0, -150.0, -4.0, -60.0], [-1.5, -4.0, -0.75, -9.0], [-20.0, -60.0, -9.0, -200.0]])
    for i in range(ns):
        t["tail_framework"][i] = fw[i]
        t["tail_cross"][i][:ns] = cross[i, :ns]
    return t


def _tc(table, omc, i, num):
    """hostmirror.modify_species_dryrun on the rows of the species table and the oracle's counts"""
    ns = len(table)
    return M.modify_species_dryrun([float(x) for x in table["tail_framework"]], np.array(table["tail_cross"][:, :ns]),
                                   [len(k) for k in omc.positions], i, num)


class Replay:
    """One chain followed on the oracle: `tab[d]` = [species, index in the oracle's kind] of device molecule d.  step(..., rec=None)
    decides with the rule on the oracle's rows (the prediction); with a record it checks the record and follows its decision."""

    def __init__(self, mc, omc, order, table, T, dmax, thetamax, cap):
        self.mc, self.omc, self.tab = mc, omc, [list(x) for x in order]
        self.table, self.species = table, _mcrng_species(table)
        self.T, self.dmax, self.thetamax, self.cap = float(T), dmax, thetamax, cap
        self.seen, self.exempt, self.records = set(), 0, 0
        self.trials, self.accepted = np.zeros(7, dtype=np.int64), np.zeros(7, dtype=np.int64)
        self.blocked = self.capacity = self.spent = 0
        self.delta = [0.0, 0.0]
        self.scale = 1.0
        self.peak = len(self.tab)
        self.tc_nonzero = self.flips = 0
        self.seen_species = set()
        self.events = []          # every decided step: (kind, device molecule index, nmol before the step, accepted, species)

    def step(self, seed, step, sid, rec=None, what=None):
        omc, tab = self.omc, self.tab
        pr = mcrng.propose_gcmc(seed, step, sid, [i for i, _j in tab], [omc.positions[i][j] for i, j in tab], self.species,
                                self.mc.mat, self.dmax, self.thetamax, self.cap)
        i, kind = pr.species, pr.kind
        t = self.table[i]
        m = int(t["m"])
        self.records += 1
        if rec is not None:
            assert (rec["species"], rec["kind"], rec["n_species"]) == (i, kind, pr.n_species), (what, rec, pr)
            assert rec["u"] == pr.u, what
            assert bool(rec["flags"] & 1) == pr.spent and bool(rec["flags"] & 4) == pr.capacity, (what, rec)
        if pr.spent or pr.capacity:
            if rec is not None:
                assert rec["molecule"] == pr.molecule and not rec["accepted"] and not rec["rows"].any() and not rec["positions"].any(), (what, rec)
            if pr.spent:
                self.spent += 1
            else:
                self.capacity += 1
                self.trials[5] += 1
            return
        if rec is not None:
            assert rec["molecule"] == pr.molecule, (what, rec, pr)
        placed = pr.positions
        if rec is not None:
            placed = rec["positions"][:len(pr.positions)].copy()
            if kind != 6:
                assert np.abs(placed - pr.positions).max() <= 1e-12, (what, placed, pr.positions)
            assert not rec["positions"][len(pr.positions):].any(), what
        idx = None if kind == 5 else tuple(tab[pr.molecule])
        zero = np.zeros(4)
        before = zero if kind == 5 else omc.movement_energy(idx)
        after = zero if kind == 6 else (omc.insertion_energy(i, placed) if kind == 5 else omc.movement_energy(idx, placed))
        rows = np.array([before, after])
        if rec is not None:
            for r in (0, 1):
                if (kind, r) in ((5, 0), (6, 1)):
                    assert not rec["rows"][r].any(), (what, rec)
                else:
                    _check(rec["rows"][r], rows[r], (what, "row", r))
            rows = rec["rows"]
        self.scale = max(self.scale, float(np.abs(rows).clip(max=1e90).max()))
        tc = 0.0
        if kind <= 4:
            ok, e = _rule(rows, pr.u, self.T)
            near = e is not None and abs(pr.u - e) <= 1e-12 * e
            diff = float(rows[1].sum() - rows[0].sum())
            blocked = rows[1][0] >= 1e90
        else:
            tc = _tc(self.table, omc, i, 1 if kind == 5 else -1)
            self.tc_nonzero += tc != 0.0
            if rec is not None:
                assert abs(rec["tc"] - tc) <= 1e-12 * max(1.0, abs(tc)), (what, rec["tc"], tc)
                tc = float(rec["tc"])
            row = rows[1] if kind == 5 else rows[0]
            # a swap whose decision the tail-correction change turns round
            self.flips += mcrng.swap_rule(row, pr.u, self.T, pr.n_species, float(t["phiPV_div_k"]), float(t["self_reciprocal"]), 0.0, kind == 5) != \
                mcrng.swap_rule(row, pr.u, self.T, pr.n_species, float(t["phiPV_div_k"]), float(t["self_reciprocal"]), tc, kind == 5)
            diff, thr = mcrng.swap_threshold(row, self.T, pr.n_species, float(t["phiPV_div_k"]), float(t["self_reciprocal"]), tc, kind == 5)
            ok = mcrng.swap_rule(row, pr.u, self.T, pr.n_species, float(t["phiPV_div_k"]), float(t["self_reciprocal"]), tc, kind == 5)
            blocked = kind == 5 and row[0] >= 1e90
            near = not blocked and np.isfinite(thr) and abs(pr.u - thr) <= 1e-12 * thr
        if rec is not None:
            assert bool(rec["flags"] & 2) == bool(blocked), (what, rec)
            if near:
                self.exempt += 1
            else:
                assert bool(rec["accepted"]) == ok, (what, rec, ok)
            ok = bool(rec["accepted"])
        self.trials[kind] += 1
        self.accepted[kind] += ok
        self.blocked += bool(blocked)
        self.seen.add((kind, bool(ok)))
        self.seen_species.add((i, kind, bool(ok)))
        self.events.append((kind, pr.molecule, len(tab), bool(ok), i))
        if not ok:
            return
        self.delta[0 if kind <= 4 else 1] += diff
        if kind <= 4:
            omc.update(idx, placed)
        elif kind == 5:
            tab.append([i, omc.add(i, placed)])
            self.peak = max(self.peak, len(tab))
        else:
            j = idx[1]
            last = omc.remove(idx)                          # the oracle's molecule (i, last) is now (i, j)
            for e in tab:
                if e[0] == i and e[1] == last:
                    e[1] = j
            tab[pr.molecule] = tab[-1]                      # the device's last molecule takes the index of the deleted one
            tab.pop()

    def covered(self):
        want = {(5, True), (5, False), (6, True), (6, False)} | {(k, True) for k in DISPLACEMENTS}
        return want <= self.seen

    def check_stats(self, st, what):
        assert list(st["trials"]) == list(self.trials) and list(st["accepted"]) == list(self.accepted), (what, st, self.trials, self.accepted)
        assert (st["blocked"], st["capacity"], st["spent"]) == (self.blocked, self.capacity, self.spent), (what, st)
        assert st["nmol"] == len(self.tab) and list(st["count"][:len(self.omc.positions)]) == [len(k) for k in self.omc.positions], (what, st)
        if abs(self.delta[0]) < 1e90:                     # (a blocked molecule that left its place: -1e100, nothing to compare)
            assert abs(st["delta_moves"] - self.delta[0]) <= 1e-9 * self.scale * max(1, self.accepted[:5].sum()), (what, st, self.delta)
        if abs(self.delta[1]) < 1e90:
            assert abs(st["delta_swaps"] - self.delta[1]) <= 1e-9 * self.scale * max(1, self.accepted[5:].sum()), (what, st, self.delta)

    def check_state(self, dev, what):
        """positions and molecule order exactly (device order), the species table the wrapper rebuilt, the structure factor to 1e-9"""
        omc = self.omc
        assert [[len(k) for k in dev._slot]] == [[len(k) for k in omc.positions]], what
        assert [i for i, _j in self.tab] == [i for i, _j in _device_order(dev)], what
        n = sum(len(omc.positions[i][j]) for i, j in self.tab)
        pos, re, im = np.empty((n, 3)), np.empty(max(len(omc.ef.kfactors), 1)), np.empty(max(len(omc.ef.kfactors), 1))
        _abi.check(dev._lib, dev._lib.ceg_mc_get_state(dev._h, _abi.dptr(pos.reshape(-1)) if n else None, _abi.dptr(re), _abi.dptr(im)))
        want = np.concatenate([omc.positions[i][j] for i, j in self.tab]) if self.tab else np.empty((0, 3))
        assert np.array_equal(pos, want), what
        # the wrapper's host side: species by species in device order
        for i, kind in enumerate(dev._slot):
            members = [e for e in self.tab if e[0] == i]
            assert len(dev.mc.positions[i]) == len(members), what
            for p, (_i, j) in zip(dev.mc.positions[i], members):
                assert np.array_equal(p, omc.positions[i][j]), what
        if omc.has_ewald:
            osf = omc.total_structure_factor()
            sf = re[:len(osf)] + 1j * im[:len(osf)]
            assert np.abs(sf - osf).max() <= 1e-9 * max(np.abs(osf).max(), self.sf_scale if hasattr(self, "sf_scale") else 0.0, 1e-300), what


def _replays(devs, omcs, table, T, dmax, thetamax, caps):
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (len(devs),))
    return [Replay(d.mc, o, _device_order(d), table, T[c], dmax, thetamax, caps[c]) for c, (d, o) in enumerate(zip(devs, omcs))]


def _follow(reps, log, seed, first, sid):
    for s in range(log.shape[0]):
        for c, rep in enumerate(reps):
            rep.step(seed, first + s, int(sid[c]), log[s, c], (s, c))


def _distinct_states(devs, omcs):
    from test_gpu_mc_chains import _displace
    for c, (d, o) in enumerate(zip(devs, omcs)):
        rng = np.random.default_rng(700 + c)
        for s in range(2 + c):
            kind = s % 2
            j = int(rng.integers(len(o.positions[kind])))
            new = _displace(rng, o.positions[kind][j], 1)[0]
            d.accept((kind, j), new)
            o.update((kind, j), new)


def test_gcmc_replay_against_the_oracle(setup):
    """4 chains in states of their own, 150 steps, 100 ... 1000 K; Na: translation + random_translation, CO2: all six kinds with a
    swap share of 0.4.  phiPV_div_k and the step sizes are picked on the CPU (mcrng + the oracle): the first candidate whose
    PREDICTED run holds accepted and rejected insertions and deletions and an accepted move of every displacement kind."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 4, 150
    devs, omcs = _chains(setup, K, oracle=True)
    _distinct_states(devs, omcs)
    T = np.linspace(100.0, 1000.0, K)
    sid = np.arange(K, dtype=np.uint32) * 5 + 2
    first = 2 ** 32 - 70
    caps = [12] * K
    with DeviceMonteCarloGroup(devs) as group:
        chosen = None
        for phi, dmax, thetamax, seed in ((3000.0, 0.5, 1.0, SEED), (30000.0, 1.0, 2.0, SEED + 1), (300.0, 0.25, 0.5, SEED + 2), (3e5, 0.5, 1.0, SEED + 3),
                                          (1000.0, 0.5, 1.0, SEED + 4), (10000.0, 0.5, 1.0, SEED + 5)):
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [phi, phi]))
            pred = _replays(devs, [_clone(o) for o in omcs], table, T, dmax, thetamax, caps)
            for s in range(S):
                for c, rep in enumerate(pred):
                    rep.step(seed, first + s, int(sid[c]))
            seen = set().union(*[rep.seen for rep in pred])
            print(f"candidate phiPV_div_k {phi}, dmax {dmax}, thetamax {thetamax}: predicted outcomes {sorted(seen)}")
            pred[0].seen = seen
            flips = sum(rep.flips for rep in pred)
            print(f"  swaps whose decision the tail-correction change turns round: {flips}")
            if pred[0].covered() and flips > 0:
                chosen = (phi, dmax, thetamax, seed, table)
                break
        assert chosen is not None, "no candidate exercises every branch on the oracle"
        phi, dmax, thetamax, seed, table = chosen
        assert CO2_MOVES.swap >= 0.3 and table["self_reciprocal"][1] > 0.0
        stats, log = group.sweep_gcmc(S, seed, first, temperature=T, dmax=dmax, thetamax=thetamax, species=table, max_molecules=caps,
                                      stream_id=sid, log=True)
    assert log.shape == (S, K)
    reps = _replays(devs, omcs, table, T, dmax, thetamax, caps)
    for rep, d in zip(reps, devs):                       # (the wrapper has already moved d._slot / d.mc.positions to the final state)
        rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
    _follow(reps, log, seed, first, sid)
    exempt = sum(rep.exempt for rep in reps)
    assert exempt <= 0.01 * S * K, exempt
    seen = set().union(*[rep.seen for rep in reps])
    reps[0].seen = seen
    assert reps[0].covered(), seen
    nswaps = sum(int(rep.trials[5:].sum()) - rep.capacity for rep in reps)
    assert sum(rep.tc_nonzero for rep in reps) == nswaps > 0 and sum(rep.flips for rep in reps) > 0
    for c, rep in enumerate(reps):
        rep.check_stats(stats[c], c)
        rep.check_state(devs[c], c)
    print(f"gcmc replay: {K} chains x {S} steps, exempt {exempt}, trials {sum(r.trials for r in reps)}, accepted {sum(r.accepted for r in reps)}, "
          f"final counts {[list(s['count'][:2]) for s in stats]}")
    _close(devs)


def _empty_chains(setup, k):
    from ceg_hip.energy import DeviceMonteCarlo
    from oracle.montecarlo import OracleMonteCarlo
    mc, owner = setup
    devs, omcs = [], []
    for _ in range(k):
        d = DeviceMonteCarlo(_copy(mc, [[], []]), grids_from=owner)
        o = OracleMonteCarlo.from_setup(d.mc)
        o.compute_ewald()
        devs.append(d)
        omcs.append(o)
    return devs, omcs


def test_gcmc_from_and_to_an_empty_box(setup):
    """Swap-only species, chains created empty: a large phiPV_div_k fills the box (deletions at N = 0 are spent steps), a second sweep
    with a tiny one empties it again; state and statistics against the oracle replay after each."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 2, 60
    devs, omcs = _empty_chains(setup, K)
    caps = [16, 16]
    sid = np.array([3, 8], dtype=np.uint32)
    with DeviceMonteCarloGroup(devs) as group:
        for phase, phi in enumerate((1e12, 1e-100)):          # (Na sits at -2e4 ... -4e4 K: exp(E / T) is 1e-30 ... 1e-60 at 300 K)
            table = _tail(group.gcmc_species([SWAP_ONLY, SWAP_ONLY], [phi, phi]))
            stats, log = group.sweep_gcmc(S, SEED + 10, phase * S, temperature=[300.0, 600.0], dmax=0.5, thetamax=1.0, species=table,
                                          max_molecules=caps, stream_id=sid, log=True)
            reps = _replays(devs, omcs, table, [300.0, 600.0], 0.5, 1.0, caps)
            for rep in reps:
                rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))] if phase == 0 else rep_tabs.pop(0)
            _follow(reps, log, SEED + 10, phase * S, sid)
            rep_tabs = [rep.tab for rep in reps]
            for c, rep in enumerate(reps):
                rep.sf_scale = 1.0
                rep.check_stats(stats[c], (phase, c))
                rep.check_state(devs[c], (phase, c))
                if phase == 0:
                    assert rep.spent > 0 and rep.accepted[5] > 0 and stats[c]["nmol"] > 0, (c, stats[c])
                else:
                    assert rep.accepted[6] > 0 and stats[c]["nmol"] < before[c], (c, stats[c], before)
            before = [int(s["nmol"]) for s in stats]
            print(f"phase {phase}: nmol {before}, spent {[r.spent for r in reps]}, accepted ins/del {[list(r.accepted[5:]) for r in reps]}")
        # down to the empty box: as many more steps as it takes deletions (every deletion is accepted at this phiPV_div_k)
        stats = group.sweep_gcmc(400, SEED + 10, 2 * S, temperature=[300.0, 600.0], dmax=0.5, thetamax=1.0, species=table, max_molecules=caps,
                                 stream_id=sid)
        assert [int(s["nmol"]) for s in stats] == [0, 0] and all(s["spent"] > 0 for s in stats), stats
        for d in devs:
            pos, sf = d.state()
            assert pos.shape == (0, 3) and d._slot == [[], []]
    _close(devs)


def test_gcmc_capacity(setup):
    """max_molecules = current + 1 with a large phiPV_div_k: the capacity counter is > 0, the count never exceeds the cap, and the
    state equals the oracle replay with those steps rejected."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 2, 150
    devs, omcs = _chains(setup, K, oracle=True)
    caps = [6, 6]                                        # Na + 4 CO2 + 1
    with DeviceMonteCarloGroup(devs) as group:
        # (Na is bound by 2e4 K and more: at this phiPV_div_k its insertion is accepted wherever it is not blocked and it is never
        #  deleted, so the chains reach the cap and stay there once the fixture's blocked CO2 have been deleted)
        table = _tail(group.gcmc_species([mcrng.MoveTable(translation=1, swap=1), mcrng.MoveTable(translation=1, swap=3)], [1e9, 1e9]))
        stats, log = group.sweep_gcmc(S, SEED + 20, 0, temperature=[200.0, 800.0], dmax=0.3, thetamax=0.5, species=table, max_molecules=caps, log=True)
    reps = _replays(devs, omcs, table, [200.0, 800.0], 0.3, 0.5, caps)
    for rep in reps:
        rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
    _follow(reps, log, SEED + 20, 0, np.arange(K))
    for c, rep in enumerate(reps):
        rep.check_stats(stats[c], c)
        rep.check_state(devs[c], c)
        assert stats[c]["capacity"] > 0 and rep.peak <= caps[c] and stats[c]["nmol"] <= caps[c], (c, stats[c], rep.peak)
        assert ((log["flags"][:, c] & 4) != 0).sum() == stats[c]["capacity"]
    _close(devs)


def test_gcmc_state_afterwards_is_an_ordinary_state(setup):
    """After a sweep with swaps: ceg_mc_trial on every molecule gives the oracle's row; ceg_mc_insert / ceg_mc_remove from the host and
    another sweep work; one sweep of S steps = two of S / 2 with first_step continued, bit for bit (positions, structure factor,
    table, statistics, log)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 2, 60
    kw = dict(temperature=[300.0, 700.0], dmax=0.4, thetamax=0.8, max_molecules=[10, 10], stream_id=[4, 9], log=True)
    a, omcs = _chains(setup, K, oracle=True)
    b, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(a) as ga, DeviceMonteCarloGroup(b) as gb:
        table = _tail(ga.gcmc_species([NA_MOVES, CO2_MOVES], [5000.0, 5000.0]))
        sa, la = ga.sweep_gcmc(S, SEED + 30, 100, species=table, **kw)
        s1, l1 = gb.sweep_gcmc(S // 2, SEED + 30, 100, species=table, **kw)
        s2, l2 = gb.sweep_gcmc(S // 2, SEED + 30, 100 + S // 2, species=table, **kw)
        assert la.tobytes() == np.concatenate([l1, l2]).tobytes()
        for name in ("trials", "accepted", "blocked", "capacity", "spent"):
            assert np.array_equal(sa[name], s1[name] + s2[name]), name
        assert np.array_equal(sa["count"], s2["count"]) and np.array_equal(sa["nmol"], s2["nmol"])
        assert (sa["accepted"][:, 5:].sum(axis=0) > 0).all(), sa["accepted"]            # insertions and deletions happened
        reps = _replays(a, omcs, table, kw["temperature"], 0.4, 0.8, [10, 10])
        for rep in reps:
            rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
        _follow(reps, la, SEED + 30, 100, kw["stream_id"])
        for x, y, rep in zip(a, b, reps):
            assert x._slot == y._slot
            px, sx = x.state()
            py, sy = y.state()
            assert np.array_equal(px, py) and np.array_equal(sx, sy)
            rep.check_state(x, "after the sweep")
            # an ordinary state: the row of every molecule through the per-handle entry point
            for d, (i, j) in enumerate(rep.tab):
                jj = x._slot[i].index(d)
                _check(x.trial((i, jj), np.empty((0, len(rep.omc.positions[i][j]), 3)))[0], rep.omc.movement_energy((i, j)), ("trial", d))
        # insert / remove from the host (a freed run is reused, the last molecule renumbered), then another sweep
        for x, rep in zip(a, reps):
            new = rep.omc.positions[1][0] + np.array([0.3, -0.2, 0.1])
            x.insert(1, new)
            rep.tab.append([1, rep.omc.add(1, new)])
            d = x._slot[1][0]
            i, j = rep.tab[d]
            x.remove((1, 0))
            last = rep.omc.remove((i, j))
            for e in rep.tab:
                if e[0] == i and e[1] == last:
                    e[1] = j
            rep.tab[d] = rep.tab[-1]
            rep.tab.pop()
            x.mc.positions[1] = [rep.omc.positions[1][jj] for ii, jj in (rep.tab[dd] for dd in x._slot[1])]
        s3, l3 = ga.sweep_gcmc(30, SEED + 30, 500, species=table, **kw)
        tabs = [rep.tab for rep in reps]
        reps = _replays(a, omcs, table, kw["temperature"], 0.4, 0.8, [10, 10])
        for rep, tab in zip(reps, tabs):
            rep.tab = tab
        _follow(reps, l3, SEED + 30, 500, kw["stream_id"])
        for c, rep in enumerate(reps):
            rep.check_stats(s3[c], ("second", c))
            rep.check_state(a[c], ("second", c))
    _close(b)
    _close(a)


class _ExactFF:
    """The force field of the fixture with one more rule on the pair (0, 0): an exponential of amplitude 0 and decay 100 / A, i.e. 0 K
    at every distance.  Its decay times the cutoff is above 700, which is what makes ceg_mc_create take the exact pair functions
    (libm exp / erfc) instead of the fast ones for the whole handle; the oracle reads the same table."""

    def __init__(self, ff):
        self._ff = ff

    def __getattr__(self, name):
        return getattr(self._ff, name)

    def pair_table(self):
        rules, offsets = self._ff.pair_table()
        at = int(offsets[1])
        out = np.zeros(len(rules) + 1, dtype=rules.dtype)
        out[:at], out[at + 1:] = rules[:at], rules[at:]
        out[at]["kind"], out[at]["p"] = 6, (0.0, 100.0, 0.0)            # CEG_EXPONENTIAL
        offsets = offsets.copy()
        offsets[1:] += 1
        return out, offsets


def test_gcmc_shapes_one_and_sixteen_atoms_fast_and_exact_chains(setup):
    """Kinds [Na, CO2, a 1-atom species, a 16-atom rigid cluster] (built as in test_gpu_mc_molecule_sizes), the last two as swap
    species; chain 0 with the fast pair functions, chain 1 with the exact ones, in one group: one trial launch per class in every
    step.  A sweep with a huge phiPV_div_k (insertions wherever the framework does not block), one with a tiny one (deletions); every
    record, the statistics and the final state against the oracle replay.  Both new species are inserted and deleted."""
    from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup
    from oracle.montecarlo import OracleMonteCarlo
    from test_gpu_mc_molecule_sizes import _derive, _species
    mc, owner = setup
    species = [_species(mc, 1), _species(mc, 16)]
    devs, omcs = [], []
    for c in range(2):
        mcd = _derive(mc, species, (1, 1), 4100 + c)
        mcd.tail_framework, mcd.tail_cross = [], None        # (the fixture's rows cover its two kinds; _tail gives the table four)
        if c == 1:
            mcd.ff = _ExactFF(mc.ff)
        devs.append(DeviceMonteCarlo(mcd, grids_from=owner))
        omcs.append(OracleMonteCarlo.from_setup(mcd))
        omcs[-1].compute_ewald()
    moves = [NA_MOVES, mcrng.MoveTable(translation=1, rotation=1, random_reinsertion=1), mcrng.MoveTable(random_translation=5, swap=1),
             mcrng.MoveTable(rotation=1, random_rotation=1, random_reinsertion=1, swap=5)]
    # (a 16-atom cluster put down at random is blocked by the framework nearly everywhere: 600 steps, about 45 insertion trials per
    #  chain, a phiPV_div_k that accepts whatever is not blocked, and a cap the 1-atom species does not fill in the meantime)
    caps, sid, T = [40, 40], np.array([2, 7], dtype=np.uint32), [300.0, 500.0]
    tabs = [[[i, j] for i, kind in enumerate(o.positions) for j in range(len(kind))] for o in omcs]
    seen = set()
    with DeviceMonteCarloGroup(devs) as group:
        first = 0
        for phase, (phi, S) in enumerate(((1e200, 600), (1e-100, 100))):
            table = _tail(group.gcmc_species(moves, [1.0, 1.0, phi, phi]))
            assert list(table["m"]) == [1, 3, 1, 16]
            stats, log = group.sweep_gcmc(S, SEED + 40, first, temperature=T, dmax=0.4, thetamax=0.8, species=table, max_molecules=caps,
                                          stream_id=sid, log=True)
            reps = _replays(devs, omcs, table, T, 0.4, 0.8, caps)
            for rep, tab in zip(reps, tabs):
                rep.tab = tab
            _follow(reps, log, SEED + 40, first, sid)
            first += S
            tabs = [rep.tab for rep in reps]
            for c, rep in enumerate(reps):
                rep.check_stats(stats[c], (phase, c))
                rep.check_state(devs[c], (phase, c))
                seen |= {(c,) + x for x in rep.seen_species}
            print(f"phase {phase}: counts {[list(s['count'][:4]) for s in stats]}, exempt {[r.exempt for r in reps]}")
    for i in (2, 3):                                     # the 1-atom and the 16-atom species: inserted and deleted, rejected insertions too
        got = {(kind, ok) for _c, sp, kind, ok in seen if sp == i}
        assert {(5, True), (5, False), (6, True)} <= got, (i, sorted(seen))
    assert {c for c, sp, kind, ok in seen if sp == 3 and kind >= 5 and ok} == {0, 1}, sorted(seen)      # 16 atoms swapped on both classes
    _close(devs)


def test_plain_sweep_after_a_gcmc_sweep_on_the_same_group(setup):
    """The group keeps one device block for both kinds of sweep, and it only grows.  On one group of 2 chains (Na + 3 CO2 each), 8 steps
    each with logs: a plain sweep, a GCMC sweep that needs a larger block (species table, the chains' tables, the species of the
    molecules, the stacks of freed slots for max_molecules = 10), the plain sweep again.  The third call's log and statistics are those
    of the same plain sweep run alone on a fresh group over chains in the same state, byte for byte: nothing stale is read after the
    block grew."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    K, S = 2, 8
    start = [mc.positions[0], mc.positions[1][:3]]
    common = dict(temperature=[300.0, 700.0], dmax=0.4, thetamax=0.8, stream_id=[4, 9], log=True)
    a, _ = _chains(setup, K, positions=start)
    b, _ = _chains(setup, K, positions=start)
    with DeviceMonteCarloGroup(a) as ga:
        table = _tail(ga.gcmc_species([NA_MOVES, CO2_MOVES], [5000.0, 5000.0]))
        _sa1, la1 = ga.sweep(S, SEED + 70, 0, p_rotation=0.5, **common)
        _sa2, la2 = ga.sweep_gcmc(S, SEED + 70, S, species=table, max_molecules=[10, 10], **common)
        sa3, la3 = ga.sweep(S, SEED + 70, 2 * S, p_rotation=0.5, **common)
    with DeviceMonteCarloGroup(b) as gb:                             # the same two sweeps bring the twins into the same state
        _sb1, lb1 = gb.sweep(S, SEED + 70, 0, p_rotation=0.5, **common)
        _sb2, lb2 = gb.sweep_gcmc(S, SEED + 70, S, species=table, max_molecules=[10, 10], **common)
    assert la1.tobytes() == lb1.tobytes() and la2.tobytes() == lb2.tobytes()
    with DeviceMonteCarloGroup(b) as fresh:                          # a new group: its block is allocated for this sweep alone
        sb3, lb3 = fresh.sweep(S, SEED + 70, 2 * S, p_rotation=0.5, **common)
    assert la3.tobytes() == lb3.tobytes()
    assert sa3.tobytes() == sb3.tobytes()
    assert (la3["molecule"] >= 0).all() and (sa3["translation_trials"] + sa3["rotation_trials"] == S).all()
    for x, y in zip(a, b):
        px, sx = x.state()
        py, sy = y.state()
        assert np.array_equal(px, py) and np.array_equal(sx, sy)
    _close(b)
    _close(a)


def test_gcmc_chain_without_capacity_in_front(setup):
    """max_molecules = 0 for an empty first chain: its insertions are counted in `capacity`, and the table of the chain behind it is
    reported at the documented offset (the sum of max_molecules in front of it)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S = 40
    d0, o0 = _empty_chains(setup, 1)
    d1, o1 = _chains(setup, 1, oracle=True)
    devs, omcs, caps = d0 + d1, o0 + o1, [0, 8]
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species([mcrng.MoveTable(translation=1, swap=1), CO2_MOVES], [5000.0, 5000.0]))
        stats, log = group.sweep_gcmc(S, SEED + 50, 0, temperature=[300.0, 900.0], dmax=0.4, thetamax=0.8, species=table, max_molecules=caps, log=True)
    reps = _replays(devs, omcs, table, [300.0, 900.0], 0.4, 0.8, caps)
    for rep in reps:
        rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
    _follow(reps, log, SEED + 50, 0, np.arange(2))
    for c, rep in enumerate(reps):
        rep.sf_scale = 1.0
        rep.check_stats(stats[c], c)
        rep.check_state(devs[c], c)
    assert stats[0]["capacity"] > 0 and stats[0]["nmol"] == 0 and stats[0]["spent"] + stats[0]["capacity"] == S
    assert stats[1]["nmol"] == len(reps[1].tab) >= 1
    _close(devs[::-1])


def test_gcmc_refusals_leave_the_state_alone(setup, monkeypatch):
    """One case per refusal of the header; ceg_mc_get_state returns after each exactly what it returned before."""
    from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup
    mc, owner = setup
    K = 2
    devs, _ = _chains(setup, K)
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0, max_molecules=8)
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [1000.0, 1000.0]))
        before = [d.state() for d in devs]
        slots = [copy.deepcopy(d._slot) for d in devs]

        def unchanged():
            for d, (p, sf), sl in zip(devs, before, slots):
                p2, sf2 = d.state()
                assert np.array_equal(p, p2) and np.array_equal(sf, sf2) and d._slot == sl

        def edited(i, field, value, index=None):
            t = table.copy()
            if index is None:
                t[field][i] = value
            else:
                t[field][i][index] = value
            return t

        bad_tables = [edited(1, "m", 0), edited(1, "m", 17), edited(1, "m", 2), edited(1, "bead", 3), edited(0, "kinds", 99, 0),
                      edited(1, "kinds", int(table["kinds"][0][0]), 0), edited(1, "cumulative", 0.05, 1), edited(1, "cumulative", 1.5, 4),
                      edited(1, "cumulative", float("nan"), 0), edited(1, "phiPV_div_k", 0.0), edited(1, "phiPV_div_k", float("inf")),
                      edited(1, "self_reciprocal", float("nan")), edited(0, "tail_cross", float("inf"), 1), edited(1, "model", float("nan"), (0, 0)),
                      np.concatenate([table] * 5)]
        for t in bad_tables:
            with pytest.raises(_abi.CegError) as ei:
                group.sweep_gcmc(5, SEED, 0, species=t, **good)
            assert ei.value.code == -1, t
            unchanged()
        for change in (dict(max_molecules=4), dict(max_molecules=[8, -1]), dict(temperature=[300.0, 0.0]), dict(dmax=float("nan")),
                       dict(thetamax=-1.0), dict(stream_id=[6, 6])):
            with pytest.raises(_abi.CegError) as ei:
                group.sweep_gcmc(5, SEED, 0, species=table, **{**good, **change})
            assert ei.value.code == -1, change
            unchanged()
        with pytest.raises(_abi.CegError) as ei:
            group.sweep_gcmc(-1, SEED, 0, species=table, **good)
        assert ei.value.code == -1
        # species that do not match the handles' molecules: the wrapper's own table, handed over in the wrong order
        stats = np.zeros(K, dtype=_abi.GCMC_STATS_DTYPE)
        sid, T, z = np.arange(K, dtype=np.uint32), np.full(K, 300.0), np.full(K, 0.5)
        cap = np.full(K, 8, dtype=np.int32)
        wrong = np.ascontiguousarray([1, 0, 1, 1, 1] * K, dtype=np.int32)
        params = _abi.GcmcParams(1, 0, sid.ctypes.data, T.ctypes.data, z.ctypes.data, z.ctypes.data, 2, 0, table.ctypes.data, wrong.ctypes.data,
                                 cap.ctypes.data, None)
        assert owner._lib.ceg_mc_group_sweep_gcmc(group._h, C.addressof(params), 5, stats.ctypes.data, None) == -1
        assert owner._lib.ceg_mc_group_sweep_gcmc(group._h, None, 5, stats.ctypes.data, None) == -1
        unchanged()
        # a member marked inconsistent
        monkeypatch.setenv("CEG_HIP_MC_INJECT_FAILURE", "accept")
        with pytest.raises(_abi.CegError):
            devs[1].accept((0, 0), mc.positions[0][0] + 0.1)
        monkeypatch.delenv("CEG_HIP_MC_INJECT_FAILURE")
        with pytest.raises(_abi.CegError) as ei:
            group.sweep_gcmc(5, SEED, 0, species=table, **good)
        assert ei.value.code == -3 and "chain 1" in str(ei.value)
        devs[1].refresh()
        unchanged()
        stats = group.sweep_gcmc(5, SEED, 0, species=table, **good)                     # a valid call follows
        assert all(s["trials"].sum() + s["spent"] == 5 for s in stats)
    _close(devs)
    monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
    cells = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    monkeypatch.delenv("CEG_HIP_MC_CELLS")
    plain = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    with DeviceMonteCarloGroup([plain, cells]) as group:
        before = [d.state() for d in (plain, cells)]
        with pytest.raises(_abi.CegError) as ei:
            group.sweep_gcmc(5, SEED, 0, species=table, **good)
        assert ei.value.code == -5 and "chain 1" in str(ei.value)
        for d, (p, sf) in zip((plain, cells), before):
            p2, sf2 = d.state()
            assert np.array_equal(p, p2) and np.array_equal(sf, sf2)
    cells.close()
    plain.close()


def test_of_two_faults_the_first_is_reported(setup):
    """The order of the refusals: the species table before the cycles, the cycles before the chains, then chain by chain, and within
    a chain temperature / dmax / thetamax, stream id, kinds, max_molecules.  Each call carries two faults; the one that the order
    puts first is the one reported, and nothing is launched or changed."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 2
    devs, _ = _chains(setup, K)
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0, max_molecules=8)
    nan = float("nan")
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [1000.0, 1000.0]))
        bead = table.copy()
        bead["bead"][1] = 3                                          # (CO2 has three atoms)
        before = [d.state() for d in devs]
        slots = [copy.deepcopy(d._slot) for d in devs]

        def refused(call, what):
            with pytest.raises(_abi.CegError) as ei:
                call()
            assert ei.value.code == -1 and what in str(ei.value), (what, str(ei.value))
            for d, (p, sf), sl in zip(devs, before, slots):
                p2, sf2 = d.state()
                assert np.array_equal(p, p2) and np.array_equal(sf, sf2) and d._slot == sl

        refused(lambda: group.sweep_gcmc(5, SEED, 0, species=bead, **{**good, "dmax": [nan, 0.5]}), "species 1: the bead lies outside")
        # the same species together with a cycle description that cycles_check refuses (cycle0 < 1)
        refused(lambda: group.sweep_gcmc_cycles(2, 3, SEED, 0, cycle0=0, species=bead, **good), "species 1: the bead lies outside")
        # every chain of the fixture holds five molecules
        refused(lambda: group.sweep_gcmc(5, SEED, 0, species=table, **{**good, "dmax": [nan, 0.5], "max_molecules": [4, 8]}), "chain 0: dmax")
        refused(lambda: group.sweep_gcmc(5, SEED, 0, species=table, **{**good, "max_molecules": [4, 8], "temperature": [300.0, nan]}),
                "chain 0: max_molecules")
    _close(devs)
