"""Replica exchange at the cycle ends (ceg_mc_group_set_tempering): microseconds per chain-step at K = 16, 64 chains on a ladder of
temperatures, medians of the windows after a warm-up, routes alternated window by window in one process, in an order that rotates.  A
window is C cycles of L = 64 steps of translations and rotations.
  (a) one sweep_cycles call of C cycles with tempering installed, every = 1: one k_mcg_exchange launch behind every cycle end;
  (n) the same call on the same kind of group with no tempering installed (every chain at its own temperature of the ladder);
  (h) the route a user had before: C calls of sweep_cycles of one cycle each, mcrng.exchange_round on the host in between;
  (x) the call of (a) with `every` beyond the last cycle counter: the exchange launch, the ladder and the rungs' copy to the host at the
      end of the call, but no exchange, so the chains run the trajectories of (n) -- (x) - (n) is what the mechanism costs, (a) - (x)
      what the exchanged temperatures change.
The workload of tests/perf/time_mc_cycles.py: CHA + Na framework, 64 CO2 per chain, dmax 0.5 A, thetamax 30 degrees, both adapt bits;
the ladder is geometric from 300 to 600 K.

    python tests/perf/time_mc_tempering.py > profiles/mc_tempering.txt
    python tests/perf/time_mc_tempering.py --only-n [--lib <libceg_hip.so of the parent commit>]   # route (n) alone, for the comparison with the parent
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
from ceg_hip import _abi, mcrng, workloads as W

KS = tuple(int(x) for x in sys.argv[sys.argv.index("--ks") + 1].split(",")) if "--ks" in sys.argv else (16, 64)
ONLY_N = "--only-n" in sys.argv                  # route (n) alone: what the parent commit can run too
if "--lib" in sys.argv:                          # the parent's library does not export the two entry points
    for name in ("ceg_mc_group_set_tempering", "ceg_mc_group_tempering_read"):
        _abi.PROTOTYPES.pop(name)
    os.environ["CEG_HIP_LIB"] = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

CYCLES, WINDOWS = 4, 8
L = 64
SEED = 20240611
COUNTERS = ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mct_")
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
print(f"# {sum(len(k) for k in mc.positions)} CO2 per chain, {len(mc.ewald.kfactors)} k-vectors; windows of {CYCLES} cycles of {L} steps")

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
    """what a caller keeps between its calls: step sizes, counters, cycle counter, and for route (h) rungs and energies"""

    def __init__(self, k, energies):
        self.dm, self.th, self.total, self.cc = np.full(k, DMAX), np.full(k, THETAMAX), np.zeros((k, 4), dtype=np.int64), 1
        self.rung, self.energy = np.arange(k, dtype=np.int32), np.array(energies, dtype=np.float64)

    def follow(self, rec, n):
        self.dm, self.th, self.cc = rec[-1]["dmax_next"].copy(), rec[-1]["thetamax_next"].copy(), self.cc + n
        self.total = np.stack([rec[-1][name] for name in COUNTERS], axis=1)


def window(route, group, ladder, first, caller):
    """seconds of one window of CYCLES cycles on `group`"""
    k = len(ladder)
    start = time.perf_counter()
    if route in "anx":
        _stats, rec = group.sweep_cycles(CYCLES, L, SEED, first, temperature=ladder, dmax=caller.dm, thetamax=caller.th, cycle0=caller.cc, prior=caller.total)
        caller.follow(rec, CYCLES)
    else:
        sid = np.arange(k)
        for j in range(CYCLES):
            _stats, rec = group.sweep_cycles(1, L, SEED, first + j * L, temperature=ladder[caller.rung], dmax=caller.dm, thetamax=caller.th, cycle0=caller.cc,
                                             prior=caller.total)
            energy = caller.energy + rec[0]["delta_moves"]
            caller.rung, _x = mcrng.exchange_round(caller.rung, energy, ladder, [False] * k, SEED, first + (j + 1) * L - 1, sid, caller.cc, 1)
            caller.energy = energy
            caller.follow(rec, 1)
    return time.perf_counter() - start


routes = "n" if ONLY_N else "anhx"
print(f"# us per chain-step, median of {WINDOWS} windows (range), routes alternated in one process")
print(f"# {'K':>3} | (a) tempering, one call of {CYCLES} cycles | (n) no tempering, one call      | (h) {CYCLES} calls, host exchange     | (x) tempering, no round         | (a)/(n) | (a)/(h) | (x)/(n) | (a)-(n), (x)-(n) per cycle, us | spread of (n) | accepted / attempted")
kmax = max(KS)
sets = {r: make_chains(kmax) for r in routes}
for k in KS:
    ladder = np.geomspace(300.0, 600.0, k)
    groups = {r: DeviceMonteCarloGroup(s[:k]) for r, s in sets.items()}
    energies = [float(r) for r in groups["n"].baseline_energies()]
    callers = {r: Caller(k, energies) for r in routes}
    if "a" in groups:
        groups["a"].set_tempering(1, energies, capacity=CYCLES * (WINDOWS + 1))
        groups["x"].set_tempering(10 ** 9, energies, capacity=CYCLES * (WINDOWS + 1))
    t = {r: [] for r in routes}
    steps = CYCLES * L
    for w in range(-1, WINDOWS):
        shift = (w + 1) % len(routes)                          # the order rotates: no route always runs behind the same one
        for r in routes[shift:] + routes[:shift]:
            dt = window(r, groups[r], ladder, (w + 1) * steps, callers[r])
            if w >= 0:
                t[r].append(dt / (k * steps) * 1e6)
    med = {r: statistics.median(v) for r, v in t.items()}
    cell = lambda r: f"{med[r]:7.3f} ({min(t[r]):6.3f}-{max(t[r]):6.3f})"
    if ONLY_N:
        print(f"  {k:3d} | {cell('n')}")
    else:
        pairs = groups["a"].tempering_read()[2]
        spread = (max(t["n"]) - min(t["n"])) / med["n"]
        print(f"  {k:3d} | {cell('a')}         | {cell('n')}         | {cell('h')}         | {cell('x')}         | {med['a'] / med['n']:6.3f}  | {med['a'] / med['h']:6.3f}  | {med['x'] / med['n']:6.3f}  | "
              f"{(med['a'] - med['n']) * k * L:14.2f}, {(med['x'] - med['n']) * k * L:14.2f} | {spread:13.3f} | {int(pairs[:, 1].sum())} / {int(pairs[:, 0].sum())}")
    for g in groups.values():
        g.close()
    for s in sets.values():                                    # every run starts from the same state
        for ch in s[:k]:
            ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
            ch.refresh()
for s in list(sets.values())[::-1]:
    for ch in s[::-1]:
        ch.close()
