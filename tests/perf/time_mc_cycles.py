"""Whole cycles on the device (ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles): microseconds per chain-step at K = 16, 64,
256 chains, medians of the windows after a warm-up, routes alternated window by window in one process, in an order that rotates.  A window is C cycles of L
steps: L = 64 for the plain sweep (the molecules of a chain, the reference's numsteps), L = 50 for GCMC (its fixed 50 per swap species).
  (a) one sweep_cycles / sweep_gcmc_cycles call of C cycles: the cycle ends (adaptation of dmax / thetamax, both bits) on the device;
  (b) what a caller did without it: C calls of the existing sweep of one cycle each, mcrng.adapt_* on the host in between;
  (c) the existing sweep over the same C * L steps in one call with fixed parameters: the floor (a) is held against;
  (d) the call of (a) with adapt = 0: the steps of (c) move for move, plus the C cycle-end launches and the records -- what the
      feature itself costs, apart from the different moves that adapted step sizes make.
The workload of tests/perf/time_mc_sampler.py: CHA + Na framework, 64 CO2 per chain, T = 300 K, dmax 0.5 A, thetamax 30 degrees; GCMC
with a swap share of 0.2, max_molecules 96, positions=False.

    python tests/perf/time_mc_cycles.py > profiles/mc_cycles.txt
    python tests/perf/time_mc_cycles.py --only-c [--lib <libceg_hip.so of the parent commit>]      # route (c) alone, for the comparison with the parent
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

KS = tuple(int(x) for x in sys.argv[sys.argv.index("--ks") + 1].split(",")) if "--ks" in sys.argv else (16, 64, 256)
ONLY_C = "--only-c" in sys.argv                  # route (c) alone: what the parent commit can run too
if "--lib" in sys.argv:                          # the parent's library does not export the two entry points
    for name in ("ceg_mc_group_sweep_cycles", "ceg_mc_group_sweep_gcmc_cycles"):
        _abi.PROTOTYPES.pop(name)
    os.environ["CEG_HIP_LIB"] = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

CYCLES, WINDOWS = 4, 8
L_PLAIN, L_GCMC = 64, 50
SEED = 20240611
CAP = 96
PHI = 3.0e4

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcc_")
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
print(f"# {sum(len(k) for k in mc.positions)} CO2 per chain, {len(mc.ewald.kfactors)} k-vectors; windows of {CYCLES} cycles of {L_PLAIN} (plain) / {L_GCMC} (GCMC) steps")

owner = None
SWAPS = mcrng.MoveTable(translation=0.33 * 0.8, rotation=0.33 * 0.8, random_reinsertion=0.34 * 0.8, swap=0.2)
T, DMAX, THETAMAX = 300.0, 0.5, math.radians(30.0)


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
    """route (b): the step sizes and the cumulative counters a caller keeps between its one-cycle calls"""

    def __init__(self, k):
        self.dm, self.th, self.total, self.cc = np.full(k, DMAX), np.full(k, THETAMAX), np.zeros((k, 4), dtype=np.int64), 1

    def adapt(self, counters, nmol):
        self.total += counters
        for c, (tt, ta, rt, ra) in enumerate(self.total.tolist()):
            if nmol[c] > 0:
                self.dm[c] = mcrng.adapt_dmax(self.dm[c], ta, tt, self.cc)
                self.th[c] = mcrng.adapt_thetamax(self.th[c], ra, rt, self.cc)
        self.cc += 1


def window(route, gcmc, group, table, first, caller):
    """seconds of one window of CYCLES cycles on `group`"""
    steps = L_GCMC if gcmc else L_PLAIN
    extra = dict(species=table, max_molecules=CAP, positions=False) if gcmc else dict(p_rotation=0.5)
    start = time.perf_counter()
    if route == "a":
        call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
        _stats, rec = call(CYCLES, steps, SEED, first, temperature=T, dmax=caller.dm, thetamax=caller.th, cycle0=caller.cc, prior=caller.total, **extra)
        caller.dm, caller.th, caller.cc = rec[-1]["dmax_next"].copy(), rec[-1]["thetamax_next"].copy(), caller.cc + CYCLES
        caller.total = np.stack([rec[-1][n] for n in ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")], axis=1)
    elif route == "b":
        for j in range(CYCLES):
            if gcmc:
                st = group.sweep_gcmc(steps, SEED, first + j * steps, temperature=T, dmax=caller.dm, thetamax=caller.th, **extra)
                caller.adapt(np.stack([st["trials"][:, 0], st["accepted"][:, 0], st["trials"][:, 1], st["accepted"][:, 1]], axis=1), st["nmol"])
            else:
                st = group.sweep(steps, SEED, first + j * steps, temperature=T, dmax=caller.dm, thetamax=caller.th, **extra)
                caller.adapt(np.stack([st[n] for n in ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")], axis=1),
                             np.full(len(st), 1))
    elif route == "d":
        (group.sweep_gcmc_cycles if gcmc else group.sweep_cycles)(CYCLES, steps, SEED, first, temperature=T, dmax=DMAX, thetamax=THETAMAX, adapt=0, **extra)
    else:
        (group.sweep_gcmc if gcmc else group.sweep)(CYCLES * steps, SEED, first, temperature=T, dmax=DMAX, thetamax=THETAMAX, **extra)
    return time.perf_counter() - start


routes = "c" if ONLY_C else "abcd"
print(f"# us per chain-step, median of {WINDOWS} windows (range), routes alternated in one process")
print(f"# {'sweep':>5} {'K':>3} | (a) one call of {CYCLES} cycles      | (b) {CYCLES} calls, host adaptation | (c) one sweep, fixed parameters | (d) as (a), adapt = 0         | (a)/(b) | (a)/(c) | (d)/(c) | spread of (c)")
kmax = max(KS)
sets = {r: make_chains(kmax) for r in routes}
for k in KS:
    for gcmc in (False, True):
        groups = {r: DeviceMonteCarloGroup(s[:k]) for r, s in sets.items()}
        table = groups["c"].gcmc_species([SWAPS], [PHI]) if gcmc else None
        callers = {r: Caller(k) for r in routes}
        t = {r: [] for r in routes}
        steps = CYCLES * (L_GCMC if gcmc else L_PLAIN)
        for w in range(-1, WINDOWS):
            shift = (w + 1) % len(routes)                          # the order rotates: no route always runs behind the same one
            for r in routes[shift:] + routes[:shift]:
                dt = window(r, gcmc, groups[r], table, (w + 1) * steps, callers[r])
                if w >= 0:
                    t[r].append(dt / (k * steps) * 1e6)
        med = {r: statistics.median(v) for r, v in t.items()}
        cell = lambda r: f"{med[r]:7.2f} ({min(t[r]):6.2f}-{max(t[r]):6.2f})"
        name = "gcmc" if gcmc else "plain"
        if ONLY_C:
            print(f"  {name:>5} {k:3d} | {cell('c')}")
        else:
            spread = (max(t["c"]) - min(t["c"])) / med["c"]
            print(f"  {name:>5} {k:3d} | {cell('a')}       | {cell('b')}       | {cell('c')}         | {cell('d')}       | {med['a'] / med['b']:6.3f}  | {med['a'] / med['c']:6.3f}  | {med['d'] / med['c']:6.3f}  | {spread:6.3f}")
        for g in groups.values():
            g.close()
        for s in sets.values():                                    # every run starts from the same state
            for ch in s[:k]:
                ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
                ch.refresh()
for s in list(sets.values())[::-1]:
    for ch in s[::-1]:
        ch.close()
