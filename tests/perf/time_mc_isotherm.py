"""An isotherm on the device sweeps (ceg_mc_group_set_chain_plan): microseconds per chain-step at K = 16 and 64 chains, medians of the
windows after a warm-up, routes alternated window by window in one process, in an order that rotates.  A window is one
sweep_gcmc_cycles call of 4 cycles of 50 steps.
  (a) one group, one phiPV_div_k per chain in the plan, spread over three decades;
  (b) K one-chain groups, each with its own species table, swept one after another: the only device route to an isotherm without the plan;
  (c) the group of (a) with no plan and one shared value: what the plan is held against;
  (d) the group of (a) with stops as well: a third of the chains stop after a quarter of the window, a third after half, the rest
      run to its end -- reported per step of the CALL (all K chains), beside (a) in the same unit.
The workload of tests/perf/time_mc_cycles.py: CHA + Na framework, 64 CO2 per chain, T = 300 K, dmax 0.5 A, thetamax 30 degrees, a swap
share of 0.2, max_molecules 96, positions=False.

    python tests/perf/time_mc_isotherm.py > profiles/mc_isotherm.txt
    python tests/perf/time_mc_isotherm.py --only-c [--lib <libceg_hip.so of the parent commit>]      # route (c) alone, for the comparison with the parent
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
ONLY_C = "--only-c" in sys.argv                  # route (c) alone: what the parent commit can run too
if "--lib" in sys.argv:                          # the parent's library does not export the entry point
    _abi.PROTOTYPES.pop("ceg_mc_group_set_chain_plan")
    os.environ["CEG_HIP_LIB"] = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

CYCLES, L, WINDOWS = 4, 50, 8
STEPS = CYCLES * L
SEED = 20240611
CAP = 96
PHI = 3.0e4
T, DMAX, THETAMAX = 300.0, 0.5, math.radians(30.0)
SWAPS = mcrng.MoveTable(translation=0.33 * 0.8, rotation=0.33 * 0.8, random_reinsertion=0.34 * 0.8, swap=0.2)

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mci_")
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
print(f"# {sum(len(k) for k in mc.positions)} CO2 per chain, {len(mc.ewald.kfactors)} k-vectors; windows of {CYCLES} cycles of {L} steps, swap share {SWAPS.swap:.2f}")

owner = None


def make_chains(n):
    global owner
    out = []
    for _ in range(n):
        mcc = copy.copy(mc)
        mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
        out.append(DeviceMonteCarlo(mcc, grids_from=owner))
        owner = owner or out[0]
    return out


def spread(k):
    """one phiPV_div_k per chain over three decades about PHI"""
    return PHI * 10.0 ** np.linspace(-1.5, 1.5, k)


def window(groups, tables, first, sid):
    """seconds of one window: every group of the route swept once over the window's cycles"""
    start = time.perf_counter()
    for g, (group, table) in enumerate(zip(groups, tables)):
        ids = sid if len(groups) == 1 else sid[g:g + 1]
        group.sweep_gcmc_cycles(CYCLES, L, SEED, first, temperature=T, dmax=DMAX, thetamax=THETAMAX, adapt=0, species=table, max_molecules=CAP,
                                stream_id=ids, positions=False)
    return time.perf_counter() - start


routes = "c" if ONLY_C else "abcd"
print(f"# median of {WINDOWS} windows (range), routes alternated in one process; (a) (b) (c) in us per chain-step, (d) and (a) again in us per step of the call")
print(f"# {'K':>3} | (a) one group, plan            | (b) K one-chain groups          | (c) one group, no plan          | (a)/(b) | (a)/(c) | spread of (c) |"
      f" per step of the call: (a) no stops | (d) stops at 1/4, 1/2, end | (d)/(a)")
kmax = max(KS)
sets = {r: make_chains(kmax) for r in routes}
for k in KS:
    sid = np.arange(k, dtype=np.uint32)
    phi = spread(k)
    groups, tables = {}, {}
    for r, s in sets.items():
        if r == "b":
            groups[r] = [DeviceMonteCarloGroup([ch]) for ch in s[:k]]
            tables[r] = [groups[r][c].gcmc_species([SWAPS], [phi[c]]) for c in range(k)]
        else:
            groups[r] = [DeviceMonteCarloGroup(s[:k])]
            tables[r] = [groups[r][0].gcmc_species([SWAPS], [PHI])]
    t = {r: [] for r in routes}
    for w in range(-1, WINDOWS):
        first = (w + 1) * STEPS
        if "a" in groups:
            groups["a"][0].set_chain_plan(phi[:, None])
            stops = np.full(k, first + STEPS, dtype=np.int64)
            stops[:k // 3], stops[k // 3:2 * (k // 3)] = first + STEPS // 4, first + STEPS // 2
            groups["d"][0].set_chain_plan(phi[:, None], stops)      # (a chain that stopped early simply skips those steps of its stream)
        shift = (w + 1) % len(routes)                              # the order rotates: no route always runs behind the same one
        for r in routes[shift:] + routes[:shift]:
            dt = window(groups[r], tables[r], first, sid)
            if w >= 0:
                t[r].append(dt / STEPS * 1e6)                      # us per step of the call
    med = {r: statistics.median(v) for r, v in t.items()}
    per_chain = lambda r: f"{med[r] / k:7.2f} ({min(t[r]) / k:6.2f}-{max(t[r]) / k:6.2f})"
    per_call = lambda r: f"{med[r]:8.1f} ({min(t[r]):7.1f}-{max(t[r]):7.1f})"
    if ONLY_C:
        print(f"  {k:3d} | {med['c'] / k:8.3f} ({min(t['c']) / k:7.3f}-{max(t['c']) / k:7.3f})")
    else:
        print(f"  {k:3d} | {per_chain('a')}         | {per_chain('b')}         | {per_chain('c')}         | {med['a'] / med['b']:6.3f}  | {med['a'] / med['c']:6.3f}  |"
              f" {(max(t['c']) - min(t['c'])) / med['c']:6.3f}        | {per_call('a')}        | {per_call('d')}   | {med['d'] / med['a']:6.3f}")
    for gs in groups.values():
        for g in gs:
            g.close()
    for s in sets.values():                                        # every K starts from the same state
        for ch in s[:k]:
            ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
            ch.refresh()
for s in list(sets.values())[::-1]:
    for ch in s[::-1]:
        ch.close()
