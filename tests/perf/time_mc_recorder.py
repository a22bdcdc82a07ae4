"""The recorder of a chain group (ceg_mc_group_set_recorder): microseconds per chain-step at K = 16, 64 chains, medians of the windows
after a warm-up, routes alternated window by window in one process, in an order that rotates.  A window is C cycles of L = 64 steps of
translations and rotations.
  (n) one sweep_cycles call of C cycles with no recorder installed;
  (a) the same call with a frame at EVERY cycle end and track_min: one k_mcg_snapshot launch behind every cycle end;
  (t) the same call with a frame every 10 cycles and track_min (the launch at every cycle end, a frame body at every tenth);
  (h) the route a user had before: C calls of sweep_cycles of one cycle each, ceg_mc_get_state of every chain and the comparison with
      the minimum on the host in between.
After the windows: (r) the one-time recorder_read() of route (a)'s frames (all windows), in ms and per frame and chain.
The workload of tests/perf/time_mc_cycles.py: CHA + Na framework, 64 CO2 per chain, dmax 0.5 A, thetamax 30 degrees, both adapt bits,
every chain at its own temperature between 300 and 600 K.

    python tests/perf/time_mc_recorder.py > profiles/mc_recorder.txt
    python tests/perf/time_mc_recorder.py --only-n [--lib <libceg_hip.so of the parent commit>]   # route (n) alone, for the comparison with the parent
"""
import copy
import math
import os
import statistics
import sys
import tempfile
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
import ceg_hip as ceg
from ceg_hip import _abi, workloads as W

KS = tuple(int(x) for x in sys.argv[sys.argv.index("--ks") + 1].split(",")) if "--ks" in sys.argv else (16, 64)
ONLY_N = "--only-n" in sys.argv                  # route (n) alone: what the parent commit can run too
if "--lib" in sys.argv:                          # the parent's library does not export the five entry points
    for name in ("ceg_mc_group_set_recorder", "ceg_mc_group_snapshot", "ceg_mc_group_recorder_rebase", "ceg_mc_group_recorder_read", "ceg_mc_group_recorder_min"):
        _abi.PROTOTYPES.pop(name)
    os.environ["CEG_HIP_LIB"] = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

CYCLES, WINDOWS = 4, 8
L = 64
SEED = 20240611
COUNTERS = ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcr_")
os.makedirs(os.path.join(tmp, "raspa"))
for sub in ("forcefield", "molecules", "structures"):
    os.symlink(os.path.join(golden, sub), os.path.join(tmp, "raspa", sub))
ceg.setdir_RASPA(os.path.join(tmp, "raspa"))
FF = "BoulfelfelSholl2021"
co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", FF)
base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96_Na_11812", FF)
rng = np.random.default_rng(0)
centers = (W._random_atoms_min_sep(64, 1.0, 0.14, rng)) @ fw.mat.T
mc = M.setup_montecarlo("CHA_1.4_3b4eeb96_Na_11812", FF, [co2.with_positions(c + base) for c in centers])
NATOMS = sum(len(p) for kind in mc.positions for p in kind)
print(f"# {sum(len(k) for k in mc.positions)} CO2 per chain ({NATOMS} atoms), {len(mc.ewald.kfactors)} k-vectors; windows of {CYCLES} cycles of {L} steps")

owner = None
DMAX, THETAMAX = 0.5, math.radians(30.0)


def make_chains(n):
    global owner
    out = []
    for _ in range(n):
        mcc = copy.copy(mc)
        mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
        out.append(DeviceMonteCarlo(mcc, grids_from=owner))
        owner = owner or out[0]
    return out


class Caller:
    """what a caller keeps between its calls: step sizes, counters, cycle counter, and for route (h) energies, minimum and frames"""

    def __init__(self, k, energies):
        self.dm, self.th, self.total, self.cc = np.full(k, DMAX), np.full(k, THETAMAX), np.zeros((k, 4), dtype=np.int64), 1
        self.energy = np.array(energies, dtype=np.float64)
        self.mine, self.best, self.frames = self.energy.copy(), [None] * k, []

    def follow(self, rec, n):
        self.dm, self.th, self.cc = rec[-1]["dmax_next"].copy(), rec[-1]["thetamax_next"].copy(), self.cc + n
        self.total = np.stack([rec[-1][name] for name in COUNTERS], axis=1)


def window(route, group, T, first, caller):
    """seconds of one window of CYCLES cycles on `group`"""
    k = len(T)
    start = time.perf_counter()
    if route in "nat":
        _stats, rec = group.sweep_cycles(CYCLES, L, SEED, first, temperature=T, dmax=caller.dm, thetamax=caller.th, cycle0=caller.cc, prior=caller.total)
        caller.follow(rec, CYCLES)
    else:
        lib = group._lib
        for j in range(CYCLES):
            _stats, rec = group.sweep_cycles(1, L, SEED, first + j * L, temperature=T, dmax=caller.dm, thetamax=caller.th, cycle0=caller.cc, prior=caller.total)
            caller.energy = caller.energy + rec[0]["delta_moves"]
            frame = []
            for c, chain in enumerate(group.chains):
                pos = np.empty((NATOMS, 3))
                lib.ceg_mc_get_state(chain._h, _abi.dptr(pos.reshape(-1)), None, None)
                frame.append(pos)
                if caller.energy[c] < caller.mine[c]:
                    caller.mine[c], caller.best[c] = caller.energy[c], pos
            caller.frames.append(frame)
            caller.follow(rec, 1)
    return time.perf_counter() - start


routes = "n" if ONLY_N else "nath"
print(f"# us per chain-step, median of {WINDOWS} windows (range), routes alternated in one process")
print(f"# {'K':>3} | (n) no recorder, one call of {CYCLES} cycles | (a) a frame every cycle + min     | (t) a frame every 10 cycles + min | (h) {CYCLES} calls + get_state per chain | "
      f"(a)/(n) | (t)/(n) | (a)/(h) | (t)/(h) | (a)-(n), (t)-(n) per cycle, us | spread of (n) | (r) recorder_read of (a): frames, ms, us per frame and chain")
kmax = max(KS)
sets = {r: make_chains(kmax) for r in routes}
for k in KS:
    T = np.geomspace(300.0, 600.0, k)
    groups = {r: DeviceMonteCarloGroup(s[:k]) for r, s in sets.items()}
    energies = [float(r) for r in groups["n"].baseline_energies()]
    callers = {r: Caller(k, energies) for r in routes}
    ncyc = CYCLES * (WINDOWS + 1)
    if "a" in groups:
        groups["a"].set_recorder(1, capacity=ncyc, energies=energies, track_min=True)
        groups["t"].set_recorder(10, capacity=ncyc // 10 + 1, energies=energies, track_min=True)
    t = {r: [] for r in routes}
    steps = CYCLES * L
    for w in range(-1, WINDOWS):
        shift = (w + 1) % len(routes)                          # the order rotates: no route always runs behind the same one
        for r in routes[shift:] + routes[:shift]:
            dt = window(r, groups[r], T, (w + 1) * steps, callers[r])
            if w >= 0:
                t[r].append(dt / (k * steps) * 1e6)
    med = {r: statistics.median(v) for r, v in t.items()}
    cell = lambda r: f"{med[r]:7.3f} ({min(t[r]):6.3f}-{max(t[r]):6.3f})"
    if ONLY_N:
        print(f"  {k:3d} | {cell('n')}")
    else:
        start = time.perf_counter()
        records, frames = groups["a"].recorder_read()
        read = time.perf_counter() - start
        mink, mine, _rec, _bodies = groups["a"].recorder_minimum()
        assert records.shape == (ncyc, k) and np.allclose(mine, callers["h"].mine, rtol=1e-12, atol=0.0), "the device's minimum is the host route's (sums associated per call)"
        assert frames[-1][0][0].tobytes() == callers["h"].frames[-1][0].tobytes(), "the last frame is the host route's"
        spread = (max(t["n"]) - min(t["n"])) / med["n"]
        print(f"  {k:3d} | {cell('n')}            | {cell('a')}         | {cell('t')}          | {cell('h')}          | {med['a'] / med['n']:6.3f}  | {med['t'] / med['n']:6.3f}  | "
              f"{med['a'] / med['h']:6.3f}  | {med['t'] / med['h']:6.3f}  | {(med['a'] - med['n']) * k * L:14.2f}, {(med['t'] - med['n']) * k * L:14.2f} | {spread:13.3f} | "
              f"{len(records)} frames, {read * 1e3:.2f} ms, {read / (len(records) * k) * 1e6:.1f} us")
    for g in groups.values():
        g.close()
    for s in sets.values():                                    # every run starts from the same state
        for ch in s[:k]:
            ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
            ch.refresh()
for s in list(sets.values())[::-1]:
    for ch in s[::-1]:
        ch.close()
