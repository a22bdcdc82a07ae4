"""Device MC sweeps and GCMC on chains of hundreds of molecules: the sizes at which the group kernels take the branches that the
Na + 4 CO2 fixture never reaches -- the scan across waves of gcmc_select (a molecule found by a thread of waves 1 to 3, the prefix
of the waves in front added), its chunk of two molecules per thread once nmol passes 256, the second pass of the exhaustive pair
loop of mc_trial_row (atom slots beyond 256, with holes left by deletions), and the per-molecule state, the renumbering of the last
molecule and the wrapper's rebuilt tables at those sizes.  The reference is oracle/montecarlo.OracleMonteCarlo + ceg_hip.mcrng, record
by record, through the Replay of test_gpu_mc_sweep_gcmc with its tolerances.  Run with `pytest -m gpu` on an MI355X.

Populations.  The CIT-7 2x3x3 MC cell and its grids are those of the Na + 4 CO2 setup; only the guests change.  Molecules are put
down one after the other at uniformly drawn places, each turned by a rotation of its own, and kept where no atom comes closer than
MIN_SEP to an atom already placed and the framework's VdW energy of the molecule (the ORACLE's interpolation) is below OPEN: open
sites, so that the rows are finite and moves are accepted.  The one-atom species X is the m = 1 species of
test_gpu_mc_molecule_sizes (an O_co2 atom, charge -0.35: the box is not neutral, and the oracle forms the same sums).

Coverage.  Every test chooses its parameters from a short list on the CPU, with the run PREDICTED on the oracle, takes the first
candidate whose predicted run reaches every branch named in its docstring, fails if there is none, and asserts the same on the
device's log.  The atom slots (first slot of every molecule, the stacks of freed runs, the high-water mark) are followed by _Slots,
a host model of the documented policy (an insertion takes the run freed last by its species, else fresh slots at the high-water
mark; the last molecule takes the index of a deleted one and keeps its slots): it serves the coverage assertions only.

Verified here: chains of about 136 and of 250 to 270 molecules (up to about 500 atom slots).  NOT verified: thousands of molecules (chunks
of more than two molecules per thread, more than two passes of the pair loop)."""
import copy

import numpy as np
import pytest

from ceg_hip import mcrng
from test_gpu_consumers import _rotation
from test_gpu_mc_chains import _check
from test_gpu_mc_molecule_sizes import _species
from test_gpu_mc_sweep import SEED, _close, _copy, _device_order, _rule, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc import NA_MOVES, Replay, _clone, _ExactFF, _tail

pytestmark = pytest.mark.gpu

MIN_SEP = 2.4          # A, between atoms of different molecules at placement
OPEN = 5000.0          # K: a placement is kept where the framework's VdW energy of the molecule is below this
X_MOVES = mcrng.MoveTable(translation=1, random_translation=1, swap=8)
NA_SWAPS = mcrng.MoveTable(translation=2, random_translation=1, swap=3)
CO2_SWAPS = mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1, random_reinsertion=1, swap=10)


# ------------------------------------------------------------------ populations
def _three_kinds(mc):
    """the setup with the kinds [Na, CO2, X] and no molecules"""
    ids, d = _species(mc, 1)
    out = copy.copy(mc)
    out.ffidx = [list(mc.ffidx[0]), list(mc.ffidx[1]), list(ids)]
    out.models = [np.array(x, dtype=np.float64) for x in mc.models[:2]] + [d.copy()]
    out.positions = [[], [], []]
    out.tail_framework, out.tail_cross = [], None
    out.sums = None
    return out


def _two_kinds(mc):
    out = _copy(mc, [[], []])
    out.tail_framework, out.tail_cross = [], None
    out.sums = None
    return out


def _populate(mcd, counts, seed):
    """counts[i] molecules of kind i of `mcd` at open sites, MIN_SEP apart; the larger molecules first.  The places are drawn 20 000 at
    a time and those where the framework blocks the molecule's centre atom are dropped in one call of the oracle's interpolation."""
    from oracle import oracle as O
    from oracle.montecarlo import OracleMonteCarlo
    probe = OracleMonteCarlo.from_setup(mcd)
    rng = np.random.default_rng(seed)
    mat, inv = np.asarray(mcd.mat, dtype=np.float64), np.asarray(mcd.invmat, dtype=np.float64)
    beads = mcrng.default_beads(mcd)
    atoms = np.empty((0, 3))
    out = [[] for _ in counts]
    for i in sorted(range(len(counts)), key=lambda i: -len(mcd.ffidx[i])):
        model = np.asarray(mcd.models[i], dtype=np.float64).reshape(-1, 3)
        shape = model - model[beads[i]]
        for _batch in range(20):
            if len(out[i]) == counts[i]:
                break
            centres = rng.uniform(0.0, 1.0, (20000, 3)) @ mat.T
            centres = centres[O.interpolate_points(probe.grids[mcd.ffidx[i][beads[i]] - 1], centres, nthreads=1) < OPEN]
            for centre in centres:
                pos = centre + shape @ _rotation(rng).T
                if len(atoms):
                    f = (pos[:, None, :] - atoms[None, :, :]) @ inv.T
                    d = (f - np.round(f)) @ mat.T
                    if ((d * d).sum(axis=2) < MIN_SEP * MIN_SEP).any():
                        continue
                if len(pos) > 1 and not probe.framework_interactions(i, pos)[0] < OPEN:
                    continue
                out[i].append(pos)
                atoms = np.concatenate([atoms, pos])
                if len(out[i]) == counts[i]:
                    break
        assert len(out[i]) == counts[i], ("the MC cell does not hold this population", i, len(out[i]))
    return out


def _oracle(mcd, positions, late=()):
    from oracle.montecarlo import OracleMonteCarlo
    omc = OracleMonteCarlo.from_setup(_copy(mcd, positions))
    omc.compute_ewald()
    for i, p in late:
        omc.add(i, p)
    return omc


def _initial_order(counts, late=()):
    """device molecule index -> [kind, index in kind] after ceg_mc_set_guests of `counts` (kind by kind) and the insertions `late`"""
    order = [[i, j] for i, n in enumerate(counts) for j in range(n)]
    n = list(counts)
    for i, _p in late:
        order.append([i, n[i]])
        n[i] += 1
    return order


def _remove_from_order(order, idx):
    """`order` after ceg_mc_remove of molecule idx = (kind, index in kind): the last molecule of the kind takes the index in the
    kind, the last molecule of the device the device index"""
    i, j = idx
    d = order.index([i, j])
    last = max(e[1] for e in order if e[0] == i)
    for e in order:
        if e == [i, last]:
            e[1] = j
    order[d] = order[-1]
    order.pop()
    return d


def _device_chain(setup, mcd, positions, late=(), exact=False):
    """a DeviceMonteCarlo of `positions` on the owner's grids; `late`: (kind, positions) inserted afterwards by ceg_mc_insert, so that
    these molecules sit at the last device indices"""
    from ceg_hip.energy import DeviceMonteCarlo
    _mc, owner = setup
    m = _copy(mcd, positions)
    if exact:
        m.ff = _ExactFF(mcd.ff)
    dev = DeviceMonteCarlo(m, grids_from=owner)
    for i, p in late:
        dev.insert(i, p)
        m.positions[i].append(np.array(p, dtype=np.float64))
    return dev


def _species_table(mcd, moves, phi):
    """DeviceMonteCarloGroup.gcmc_species needs the first chain's setup only: callable without a device for the prediction"""
    from types import SimpleNamespace
    from ceg_hip.energy import DeviceMonteCarloGroup
    return _tail(DeviceMonteCarloGroup.gcmc_species(SimpleNamespace(chains=[SimpleNamespace(mc=mcd)]), moves, phi))


# ------------------------------------------------------------------ the oracle side of a sweep, and what it reached
def _on_oracle(mcd, omcs, tabs, table, T, dmax, thetamax, caps, seed, first, sid, nsteps, log=None):
    """`nsteps` steps of every chain on the oracle: predicted (log None), or checked against and following the device's log"""
    reps = [Replay(mcd, o, tab, table, T[c], dmax, thetamax, caps[c]) for c, (o, tab) in enumerate(zip(omcs, tabs))]
    for s in range(nsteps):
        for c, rep in enumerate(reps):
            rep.step(seed, first + s, int(sid[c]), None if log is None else log[s, c], (s, c))
    return reps


class _Slots:
    """The atom slots of one chain, followed on the host (see the module docstring)."""

    def __init__(self, sizes, order):
        self.sizes = list(sizes)
        self.first, self.hw = [], 0
        for i, _j in order:
            self.first.append(self.hw)
            self.hw += self.sizes[i]
        self.free = [[] for _ in sizes]

    def remove(self, d, i):
        self.free[i].append(self.first[d])
        self.first[d] = self.first[-1]
        self.first.pop()

    def begin_sweep(self):
        """between sweeps the freed runs pass through the handle's lists by atom count: those of m atoms go to the first species of m atoms"""
        for i, m in enumerate(self.sizes):
            head = self.sizes.index(m)
            if head != i:
                self.free[head] += self.free[i]
                self.free[i] = []

    def follow(self, events):
        """-> per event None, ("reused", first slot) or ("fresh", high-water mark before) for an accepted insertion"""
        out = []
        for kind, mol, _nmol, ok, i in events:
            info = None
            if ok and kind == 5:
                if self.free[i]:
                    info = ("reused", self.free[i].pop())
                else:
                    info = ("fresh", self.hw)
                    self.hw += self.sizes[i]
                self.first.append(info[1])
            elif ok and kind == 6:
                self.remove(mol, i)
            out.append(info)
        return out


def _summary(what, reps):
    ev = [e for r in reps for e in r.events]
    nmol = [e[2] for e in ev]
    print(f"{what}: {sum(r.records for r in reps)} records, {sum(r.exempt for r in reps)} exempt, nmol {min(nmol)} ... {max(nmol)}, "
          f"largest selected molecule index {max(e[1] for e in ev)}, trials per kind {list(sum(r.trials for r in reps))}, "
          f"accepted per kind {list(sum(r.accepted for r in reps))}, spent {sum(r.spent for r in reps)}, capacity {sum(r.capacity for r in reps)}")


def _finish(reps, devs, stats, what):
    exempt, records = sum(r.exempt for r in reps), sum(r.records for r in reps)
    assert exempt <= 0.01 * records, (what, exempt, records)
    for c, rep in enumerate(reps):
        rep.check_stats(stats[c], (what, c))
        rep.check_state(devs[c], (what, c))


# ------------------------------------------------------------------ shape 1: the second and third wave
SECOND_WAVE = dict(counts=(2, 0, 120), late=(2, 12), cap=150, nsteps=150, T=(400.0, 900.0), sid=(3, 11), first=2 ** 32 - 40,
                   # (phiPV_div_k of [Na, CO2, X], dmax, thetamax, seed)
                   candidates=(((1.0, 30.0, 1000.0), 0.5, 1.0, SEED + 101), ((1.0, 3.0, 3000.0), 0.5, 1.0, SEED + 100),
                               ((1.0, 0.3, 10000.0), 0.25, 0.5, SEED + 102), ((1.0, 3.0, 300.0), 1.0, 2.0, SEED + 103),
                               ((1.0, 300.0, 3000.0), 0.5, 1.0, SEED + 104)))
CO2_ALL = mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1, random_reinsertion=3, swap=4)
X_ALL = mcrng.MoveTable(translation=1, random_translation=1, swap=2)
SECOND_WAVE_MOVES = [NA_MOVES, CO2_ALL, X_ALL]


def _missing_second_wave(reps):
    """what the run of `reps` did NOT reach of: every kind 0 ... 6 on a molecule of device index >= 64, some index >= 128, an accepted
    deletion at an index below 64 while the last molecule (which takes that index) sits at 64 or beyond, accepted and rejected
    insertions and deletions, an accepted move of every displacement kind"""
    ev = [e for r in reps for e in r.events]
    missing = [f"kind {k} at an index >= 64" for k in range(7) if not any(e[0] == k and e[1] >= 64 for e in ev)]
    if not any(e[1] >= 128 and e[0] != 5 for e in ev):
        missing.append("a molecule of index >= 128")
    if not any(k == 6 and ok and mol < 64 <= nmol - 1 for k, mol, nmol, ok, _i in ev):
        missing.append("a deletion that moves the last molecule across index 64")
    seen = set().union(*[r.seen for r in reps])
    missing += [f"outcome {x}" for x in sorted({(5, True), (5, False), (6, True), (6, False)} | {(k, True) for k in range(5)}) if x not in seen]
    return missing


def _second_wave_population(mc):
    """[Na, CO2, X]: 2 Na + 120 X uploaded, then 2 Na and 12 CO2 inserted by ceg_mc_insert, so that Na sits at the device indices 0, 1,
    122, 123 and CO2 -- the species with every move kind -- at 124 ... 135"""
    P = SECOND_WAVE
    mcd = _three_kinds(mc)
    pos = _populate(mcd, [P["counts"][0] + P["late"][0], P["late"][1], P["counts"][2]], 7100)
    positions = [pos[0][:P["counts"][0]], [], pos[2]]
    late = [(0, p) for p in pos[0][P["counts"][0]:]] + [(1, p) for p in pos[1]]
    return mcd, positions, late


def _choose_second_wave(mcd, positions, late):
    P = SECOND_WAVE
    K = len(P["T"])
    order = _initial_order(P["counts"], late)
    base = _oracle(mcd, positions, late)
    for phi, dmax, thetamax, seed in P["candidates"]:
        table = _species_table(mcd, SECOND_WAVE_MOVES, list(phi))
        pred = _on_oracle(mcd, [_clone(base) for _ in range(K)], [order] * K, table, P["T"], dmax, thetamax, [P["cap"]] * K, seed, P["first"],
                          P["sid"], P["nsteps"])
        missing = _missing_second_wave(pred)
        _summary(f"predicted, phiPV_div_k {phi}, dmax {dmax}, thetamax {thetamax}", pred)
        print(f"  not reached: {missing}")
        if not missing:
            return phi, dmax, thetamax, seed, table
    raise AssertionError("no candidate reaches every branch on the oracle")


def test_gcmc_replay_molecules_in_the_second_and_third_wave(setup):
    """2 chains of 4 Na + 12 CO2 + 120 X (136 molecules, 160 atom slots; Na at the device indices 0, 1, 122, 123, CO2 at 124 ... 135),
    max_molecules 150, 150 steps at 400 K and 900 K; Na: translation + random_translation, CO2: all six kinds, X: translation,
    random_translation and swaps; the species table with the tail correction (whose rows grow with the counts: 12 CO2 keep the change
    of a CO2 swap at a few 1e3 K, where both decisions occur).  The molecule of a step lies in waves 0 to 2 of gcmc_select's scan, so
    the counts of the waves in front enter its index.  Reached, on
    the prediction and on the device's log: every kind on a molecule of index >= 64, an index >= 128, a deletion that moves the last
    molecule from beyond index 64 to below it."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    P = SECOND_WAVE
    K, S, T, caps = len(P["T"]), P["nsteps"], P["T"], [P["cap"]] * len(P["T"])
    mcd, positions, late = _second_wave_population(mc)
    phi, dmax, thetamax, seed, table = _choose_second_wave(mcd, positions, late)
    devs = [_device_chain(setup, mcd, positions, late) for _ in range(K)]
    omcs = [_oracle(mcd, positions, late) for _ in range(K)]
    tabs = [[list(x) for x in _device_order(d)] for d in devs]
    assert tabs[0] == _initial_order(P["counts"], late)
    with DeviceMonteCarloGroup(devs) as group:
        stats, log = group.sweep_gcmc(S, seed, P["first"], temperature=T, dmax=dmax, thetamax=thetamax, species=table, max_molecules=caps,
                                      stream_id=P["sid"], log=True)
    assert log.shape == (S, K)
    reps = _on_oracle(mcd, omcs, tabs, table, T, dmax, thetamax, caps, seed, P["first"], P["sid"], S, log)
    _summary("second wave, device log", reps)
    _finish(reps, devs, stats, "second wave")
    assert not _missing_second_wave(reps), _missing_second_wave(reps)
    _close(devs)


# ------------------------------------------------------------------ shape 2: across 256 molecules, atom slots beyond 256
ACROSS = dict(counts=(0, 101, 155), late=2, holes=((2, 154), (2, 153), (1, 100), (1, 99)), cap=270, nsteps=150, T=(300.0, 700.0), sid=(5, 2),
              first=1000,
              # (phiPV_div_k of [Na, CO2, X] in the filling sweep and in the emptying one, dmax, thetamax, seed)
              candidates=(((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.4, 0.8, SEED + 200), ((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.4, 0.8, SEED + 201),
                          ((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.25, 0.5, SEED + 202), ((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.5, 1.0, SEED + 203),
                          ((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.4, 0.8, SEED + 204), ((1e200, 1e200, 1e200), (1e-100, 1e-100, 1e-100), 0.4, 0.8, SEED + 205)))
ACROSS_MOVES = [NA_SWAPS, CO2_SWAPS, X_MOVES]


def _missing_across(phases, slots):
    """`phases`: the Replays of the filling and of the emptying sweep; `slots`: what _Slots.follow gave for their events, chain by
    chain.  -> what the two sweeps did NOT reach of the list in the docstring of the test"""
    missing = []
    for c in range(len(phases[0])):
        fill, empty = phases[0][c].events, phases[1][c].events
        low = [s for s, e in enumerate(fill) if e[2] <= 256]
        if not (low and any(e[2] >= 258 for e in fill[low[0]:])):
            missing.append(f"chain {c}: nmol <= 256, later >= 258")
        if not any(e[2] < 256 for e in empty):
            missing.append(f"chain {c}: nmol < 256 again")
    ev = [e for ph in phases for r in ph for e in r.events]
    info = [x for ph in slots for chain in ph for x in chain]
    if not any(k <= 4 and mol >= 256 and nmol > 256 for k, mol, nmol, _ok, _i in ev):
        missing.append("a displacement of a molecule of index >= 256")
    if not any(k == 6 and ok and mol >= 256 and nmol > 256 for k, mol, nmol, ok, _i in ev):
        missing.append("an accepted deletion of a molecule of index >= 256")
    if not any(x is not None and x[0] == "reused" and x[1] >= 256 for x in info):
        missing.append("an insertion into a freed run at a slot >= 256")
    if not any(x is not None and x[0] == "fresh" and x[1] > 256 for x in info):
        missing.append("an insertion at a high-water mark > 256")
    seen = set().union(*[r.seen for ph in phases for r in ph])
    missing += [f"outcome {x}" for x in ((5, True), (5, False), (6, True), (6, False)) if x not in seen]
    if not any(k <= 4 and ok for k, _m, _n, ok, _i in ev):
        missing.append("an accepted displacement")
    return missing


def _across_sweeps(mcd, omcs, tabs, cand, device=None, after=None):
    """the filling and the emptying sweep on the oracle -> (Replays per phase, slot events per phase).  `device(phase, table)` runs the
    sweep on the device and returns its log (None: the prediction); `after(phase, replays)` is called when a sweep has been followed"""
    P = ACROSS
    K = len(P["T"])
    phis, dmax, thetamax, seed = cand[:2], cand[2], cand[3], cand[4]
    slots = []
    for _c in range(K):                   # the slots as ceg_mc_set_guests, the late insertions and the removals left them
        order = _initial_order(P["counts"], [(0, None)] * P["late"])
        sl = _Slots([len(ids) for ids in mcd.ffidx], order)
        for idx in P["holes"]:
            sl.remove(_remove_from_order(order, list(idx)), idx[0])
        slots.append(sl)
    phases, infos = [], []
    for ph in (0, 1):
        table = _species_table(mcd, ACROSS_MOVES, list(phis[ph]))
        log = device(ph, table) if device is not None else None
        reps = _on_oracle(mcd, omcs, tabs, table, P["T"], dmax, thetamax, [P["cap"]] * K, seed, P["first"] + ph * P["nsteps"], P["sid"],
                          P["nsteps"], log)
        tabs = [r.tab for r in reps]
        for s in slots:
            s.begin_sweep()
        infos.append([s.follow(r.events) for s, r in zip(slots, reps)])
        phases.append(reps)
        if after is not None:
            after(ph, reps)
    return phases, infos


_POPULATIONS = {}


def _across_population(mc):
    """[Na, CO2, X]: 101 CO2 + 155 X uploaded, 2 Na inserted by ceg_mc_insert (device indices 256, 257), then two X and two CO2 removed
    by ceg_mc_remove: 254 molecules (the Na now at 252, 253) and four freed runs at slots >= 256 in the handle's lists"""
    if "across" not in _POPULATIONS:
        P = ACROSS
        mcd = _three_kinds(mc)
        pos = _populate(mcd, [P["late"], P["counts"][1], P["counts"][2]], 7200)
        _POPULATIONS["across"] = (mcd, [[], pos[1], pos[2]], [(0, p) for p in pos[0]])
    return _POPULATIONS["across"]


def _across_oracle(mcd, positions, late):
    omc = _oracle(mcd, positions, late)
    order = _initial_order(ACROSS["counts"], late)
    for idx in ACROSS["holes"]:
        omc.remove(idx)
        _remove_from_order(order, list(idx))
    return omc, order


def _across_device(setup, mcd, positions, late, exact=False):
    dev = _device_chain(setup, mcd, positions, late, exact)
    for idx in ACROSS["holes"]:
        dev.remove(idx)
        i, j = idx
        dev.mc.positions[i][j] = dev.mc.positions[i][-1]
        dev.mc.positions[i].pop()
    return dev


def _choose_across(mcd, positions, late):
    P = ACROSS
    K = len(P["T"])
    base, order = _across_oracle(mcd, positions, late)
    for cand in P["candidates"]:
        phases, infos = _across_sweeps(mcd, [_clone(base) for _ in range(K)], [order] * K, cand)
        missing = _missing_across(phases, infos)
        for ph, reps in enumerate(phases):
            _summary(f"predicted, candidate {cand}, sweep {ph}", reps)
        print(f"  not reached: {missing}")
        if not missing:
            return cand
    raise AssertionError("no candidate reaches every branch on the oracle")


def test_gcmc_replay_across_256_molecules(setup):
    """2 chains of 2 Na + 99 CO2 + 153 X (254 molecules in 460 atom slots, four of them freed runs beyond slot 256 handed from the
    handle's lists to the device's stacks: the pair loop of every trial takes its second pass), max_molecules 270; a sweep of 150 steps
    whose phiPV_div_k (1e200: whatever the framework does not block and no overlap forbids is inserted) fills the box past 256
    molecules -- gcmc_select goes from one molecule per thread to two in the middle of the sweep -- and one of 150 steps that empties it
    below 256 again (1e-100: every deletion is accepted).  The X carry -0.35 e each, so the energies of a swap are of the order of
    1e4 K: the decisions of these two sweeps do not hang on the energies (those of the test above do); the rows do, at 1e-9.  Reached, on the prediction and
    on the device's log, per chain: nmol <= 256 and later >= 258, nmol < 256 again in the second sweep; over the chains: a displacement
    and an accepted deletion of a molecule of index >= 256 while nmol > 256, an accepted insertion into a freed run whose first slot is
    >= 256 and one into fresh slots at a high-water mark > 256, accepted and rejected insertions and deletions."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    P = ACROSS
    K, S, caps = len(P["T"]), P["nsteps"], [P["cap"]] * len(P["T"])
    mcd, positions, late = _across_population(mc)
    cand = _choose_across(mcd, positions, late)
    devs = [_across_device(setup, mcd, positions, late) for _ in range(K)]
    omcs, orders = zip(*[_across_oracle(mcd, positions, late) for _ in range(K)])
    tabs = [[list(x) for x in _device_order(d)] for d in devs]
    assert tabs[0] == orders[0] and len(tabs[0]) == 254
    stats = []
    with DeviceMonteCarloGroup(devs) as group:
        def device(ph, table):
            st, log = group.sweep_gcmc(S, cand[4], P["first"] + ph * S, temperature=P["T"], dmax=cand[2], thetamax=cand[3], species=table,
                                       max_molecules=caps, stream_id=P["sid"], log=True)
            assert log.shape == (S, K)
            stats.append(st)
            return log

        def after(ph, reps):             # (after the filling sweep: more than 256 molecules in the tables the wrapper rebuilt)
            _summary(f"across 256, device log, sweep {ph}", reps)
            _finish(reps, devs, stats[ph], ("across 256, sweep", ph))
            if ph == 0:
                assert all(st["nmol"] > 256 for st in stats[0]), stats[0]["nmol"]

        phases, infos = _across_sweeps(mcd, omcs, tabs, cand, device, after)
    missing = _missing_across(phases, infos)
    assert not missing, missing
    _close(devs)


# ------------------------------------------------------------------ shape 3: the other routes on a state of that size
ROUTES = dict(counts=(4, 104, 156), holes=((2, 150), (1, 90), (2, 3), (1, 40)), nsteps=60, T=400.0, dmax=0.4, thetamax=0.8, sid=6)


def _routes_state(setup, mc, k):
    """k chains of 4 Na + 104 CO2 + 156 X (264 molecules), then four molecules removed by ceg_mc_remove: 260 molecules with holes
    in the atom slots, two of them beyond slot 256, and the last molecules renumbered into the holes of the table"""
    P = ROUTES
    mcd = _three_kinds(mc)
    positions = _populate(mcd, list(P["counts"]), 7300)
    devs = [_device_chain(setup, mcd, positions) for _ in range(k)]
    omcs = [_oracle(mcd, positions) for _ in range(k)]
    for d, o in zip(devs, omcs):
        for idx in P["holes"]:
            assert d.remove(idx) == o.remove(idx)
        d.mc.positions = [[p.copy() for p in kind] for kind in o.positions]
    return mcd, devs, omcs


def _oracle_index(dev, d):
    """(kind, index in kind) of device molecule d"""
    return next((i, j) for i, kind in enumerate(dev._slot) for j, x in enumerate(kind) if x == d)


def test_plain_sweep_trial_and_accept_on_260_molecules(setup):
    """On chains of 260 molecules (about 470 atom slots with holes): a plain ceg_mc_group_sweep of 60 steps replayed as in
    test_sweep_replay_against_the_oracle (k_mcg_sweep_trial); one ceg_mc_group_trial + ceg_mc_group_accept round (k_mcg_trial) and
    batch-1 ceg_mc_trial calls on molecules of device index >= 64 and >= 256; every row against the oracle's movement_energy, the
    final state against the oracle's."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_chains import _displace
    mc, _owner = setup
    P = ROUTES
    K, S = 2, P["nsteps"]
    mcd, devs, omcs = _routes_state(setup, mc, K)
    nmol = sum(len(k) for k in devs[0]._slot)
    assert nmol == 260
    order = _device_order(devs[0])
    per_kind = mcrng.default_beads(mcd)
    beads = [per_kind[i] for i, _j in order]
    # the molecule of a step depends on the stream alone: the first seed whose 60 steps reach the indices wanted
    static = [omcs[0].positions[i][j] for i, j in order]
    for seed in range(SEED + 300, SEED + 320):
        picked = [mcrng.propose(seed, s, P["sid"], static, P["dmax"], P["thetamax"], 0.5, beads).molecule for s in range(S)]
        if sum(m >= 256 for m in picked) >= 2 and sum(64 <= m < 256 for m in picked) >= 10:
            break
    else:
        raise AssertionError("no seed selects molecules of index >= 256")
    T = [P["T"], 2 * P["T"]]
    with DeviceMonteCarloGroup(devs) as group:
        stats, log = group.sweep(S, seed, 0, temperature=T, dmax=P["dmax"], thetamax=P["thetamax"], p_rotation=0.5, stream_id=[P["sid"], P["sid"] + 1],
                                 log=True)
        exempt, seen, high = 0, set(), 0
        for c in range(K):
            omc, count, delta = omcs[c], np.zeros(5, dtype=np.int64), 0.0
            for s in range(S):
                rec = log[s, c]
                pr = mcrng.propose(seed, s, P["sid"] + c, [omc.positions[i][j] for i, j in order], P["dmax"], P["thetamax"], 0.5, beads)
                assert (rec["molecule"], rec["kind"]) == (pr.molecule, pr.kind) and rec["u"] == pr.u, (s, c)
                idx = order[pr.molecule]
                m = len(omc.ffidx[idx[0]])
                placed = rec["positions"][:m].copy()
                assert np.abs(placed - pr.positions).max() <= 1e-12 and not rec["positions"][m:].any(), (s, c)
                _check(rec["rows"][0], omc.movement_energy(idx), (s, c, "before"))
                _check(rec["rows"][1], omc.movement_energy(idx, placed), (s, c, "after"))
                ok, e = _rule(rec["rows"], rec["u"], T[c])
                if e is not None and abs(rec["u"] - e) <= 1e-12 * e:
                    exempt += 1
                else:
                    assert bool(rec["accepted"]) == ok, (s, c, rec)
                count[2 * pr.kind] += 1
                count[2 * pr.kind + 1] += rec["accepted"]
                count[4] += rec["rows"][1][0] >= 1e90
                seen.add((pr.kind, bool(rec["accepted"])))
                high += pr.molecule >= 256
                if rec["accepted"]:
                    delta += rec["rows"][1].sum() - rec["rows"][0].sum()
                    omc.update(idx, placed)
            st = stats[c]
            assert [st["translation_trials"], st["translation_accepted"], st["rotation_trials"], st["rotation_accepted"], st["blocked"]] == list(count), c
            assert abs(st["delta"] - delta) <= 1e-9 * max(1.0, np.abs(log["rows"][:, c]).clip(max=1e90).max()) , c
        assert exempt <= 0.01 * S * K and high >= 2 and {(0, True), (1, True)} <= seen, (exempt, high, seen)
        print(f"plain sweep on 260 molecules: {S * K} records, {exempt} exempt, {high} on molecules of index >= 256, outcomes {sorted(seen)}")
        # one group trial + accept round: chain 0 a molecule of index >= 256, chain 1 one of 64 ... 255 in waves 1 to 3; then the rows again
        rng = np.random.default_rng(7301)
        for picks in ((259, 70), (256, 200), (130, 258)):
            moves, want = [], []
            for c, d in enumerate(picks):
                idx = _oracle_index(devs[c], d)
                trials = _displace(rng, omcs[c].positions[idx[0]][idx[1]], 2)
                moves.append(("move", idx, trials))
                want.append((idx, trials))
            rows = group.trial(moves)
            for c, (idx, trials) in enumerate(want):
                _check(rows[c][0], omcs[c].movement_energy(idx), (picks, c, "before"))
                for t in range(len(trials)):
                    _check(rows[c][1 + t], omcs[c].movement_energy(idx, trials[t]), (picks, c, "after", t))
            group.accept([(idx, trials[0]) for idx, trials in want])
            for c, (idx, trials) in enumerate(want):
                omcs[c].update(idx, trials[0])
                devs[c].mc.positions[idx[0]][idx[1]] = trials[0].copy()
            rows = group.trial([("move", idx, np.empty((0, len(trials[0]), 3))) for idx, trials in want])
            for c, (idx, _t) in enumerate(want):
                _check(rows[c][0], omcs[c].movement_energy(idx), (picks, c, "accepted"))
        # batch-1 ceg_mc_trial on the member handles
        for c, d in ((0, 257), (1, 259), (0, 64), (1, 255), (0, 3)):
            idx = _oracle_index(devs[c], d)
            new = _displace(rng, omcs[c].positions[idx[0]][idx[1]], 1)
            got = devs[c].trial(idx, new)
            _check(got[0], omcs[c].movement_energy(idx), (c, d, "trial before"))
            _check(got[1], omcs[c].movement_energy(idx, new[0]), (c, d, "trial after"))
    for c, (d, o) in enumerate(zip(devs, omcs)):
        d.mc.positions = [[p.copy() for p in kind] for kind in o.positions]
        pos, sf = d.state()
        assert np.array_equal(pos, o.flat_positions()), c
        osf = o.total_structure_factor()
        assert np.abs(sf - osf).max() <= 1e-9 * np.abs(osf).max(), c
    _close(devs)


# ------------------------------------------------------------------ group composition
def test_a_large_chain_sweeps_the_same_alone_and_among_32_small_chains(setup):
    """A chain of 250 molecules swept alone in a group of one, and as member 17 of a group of 33 whose other members are small states
    (3 to 5 molecules) of both kernel classes, fast and exact pair functions in turn: log, statistics and final state of the large
    chain are the same bit for bit, for the plain sweep and for the GCMC sweep.  (The one comparison of the device with itself here.)"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = setup
    mcd, positions, late = _across_population(mc)
    S, at = 40, 17
    table = _species_table(mcd, ACROSS_MOVES, [1e12, 1e9, 1e9])
    results = []
    for others in (0, 32):
        big = _across_device(setup, mcd, positions, late)
        small = [_device_chain(setup, mcd, [positions[0][:1], positions[1][:1 + q % 2], positions[2][:1 + q % 3]], exact=q % 2 == 1) for q in range(others)]
        devs = small[:at] + [big] + small[at:] if others else [big]
        me = devs.index(big)
        sid = [100 + q for q in range(len(devs))]
        sid[me] = 7
        with DeviceMonteCarloGroup(devs) as group:
            s1, l1 = group.sweep(S, SEED + 400, 0, temperature=500.0, dmax=0.4, thetamax=0.8, p_rotation=0.5, stream_id=sid, log=True)
            s2, l2 = group.sweep_gcmc(S, SEED + 401, S, temperature=500.0, dmax=0.4, thetamax=0.8, species=table, max_molecules=270, stream_id=sid,
                                      log=True)
        results.append((s1[me].tobytes(), l1[:, me].tobytes(), s2[me].tobytes(), l2[:, me].tobytes(), copy.deepcopy(big._slot), big.state(),
                        l1[:, me]["accepted"].sum(), s2[me]["accepted"].copy()))
        _close(devs)
    a, b = results
    assert a[:5] == b[:5]
    assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1])
    assert a[6] > 0 and a[7][5:].sum() > 0, (a[6], a[7])                  # moves and swaps were accepted: the states did change
