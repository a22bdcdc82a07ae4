"""GCMC sweeps on the device with and without block pockets (ceg_mc_group_set_blocks): microseconds per chain-step at K = 16, 64, 256
chains, median (range) of the windows after a warm-up, the two routes alternated window by window in one process.
  (a) ceg_mc_group_sweep_gcmc with no masks installed: the path a group took before block pockets existed;
  (b) the same sweep on a second set of chains with the real atom masks of the workload, BlockFile(grid) of its VdW grids
      (montecarlo.jl:181-186), installed: mean attempt index per tested proposal, share of pocket-blocked steps and acceptance ratio
      per move kind beside those of (a).
The workload of time_mc_sweep_gcmc.py: CHA + Na framework, 64 CO2 per chain, the reference's default molecule table scaled to a swap
share of 0.2, T = 300 K, dmax 0.5 A, thetamax 30 degrees, max_molecules 96, no log, positions=False.

    python tests/perf/time_mc_sweep_gcmc_blocks.py >> profiles/mc_sweep_gcmc_blocks.txt

--tree DIR imports the package from DIR/crystalenergygrids.jl_amd instead of this checkout's: a checkout of another commit, built, to
compare the two in one session (a tree without set_blocks runs (a) alone); --repeats N windows (default 3).
"""
import copy
import os
import statistics
import sys
import tempfile
import time


def _option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


here = os.path.dirname(os.path.abspath(__file__))
tree = os.path.abspath(_option("--tree", os.path.join(here, '..', '..')))
sys.path[:0] = [os.path.join(tree, 'crystalenergygrids.jl_amd'), tree]
import numpy as np
import ceg_hip as ceg
from ceg_hip import mcrng, workloads as W
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

KS = (16, 64, 256)
STEPS, WINDOWS = 200, int(_option("--repeats", 3))
SEED = 20240611
CAP = 96
PHI = float(_option("--phi", 3.0e4))

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcg_")
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
HAS_BLOCKS = hasattr(DeviceMonteCarloGroup, "set_blocks")
print(f"# tree {os.path.basename(tree)}: {sum(len(k) for k in mc.positions)} CO2 per chain, {len(mc.ewald.kfactors)} k-vectors, phiPV_div_k {PHI:g} K, "
      f"max_molecules {CAP}, block pockets {'available' if HAS_BLOCKS else 'not in this tree'}")

owner = None
SWAPS = mcrng.MoveTable(translation=0.33 * 0.8, rotation=0.33 * 0.8, random_reinsertion=0.34 * 0.8, swap=0.2)
GEOM = dict(temperature=300.0, dmax=0.5, thetamax=30.0, degrees=True)
NAMES = ("tr", "rot", "rtr", "rrot", "rein", "ins", "del")


def make_chains(n):
    global owner
    out = []
    for _ in range(n):
        mcc = copy.copy(mc)
        mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
        out.append(DeviceMonteCarlo(mcc, grids_from=owner))
        owner = owner or out[0]
    return out


def timed(fn):
    start = time.perf_counter()
    out = fn()
    return time.perf_counter() - start, out


def ratios(trials, accepted):
    return " ".join(f"{n} {a / t:.3f}" for n, t, a in zip(NAMES, trials, accepted) if t > 0)


atom_blocks = None
if HAS_BLOCKS:
    from ceg_hip.grids import blockfile_from_grid_gpu
    atom_blocks = [None if g is None else blockfile_from_grid_gpu(g) for g in mc.grids]
    print("# atom masks: blocked share " + ", ".join(f"{b.block.mean():.3f}" for b in atom_blocks if b is not None))
print(f"# us per chain-step, median of {WINDOWS} windows of {STEPS} steps (range), routes alternated in one process")
kmax = max(KS)
sets = [make_chains(kmax) for _ in range(2 if HAS_BLOCKS else 1)]
for k in KS:
    groups = [DeviceMonteCarloGroup(s[:k]) for s in sets]
    table = groups[0].gcmc_species([SWAPS], [PHI])
    if HAS_BLOCKS:
        groups[1].set_blocks([None], atom_blocks)
    t = [[] for _ in groups]
    trials, accepted = [np.zeros(7, dtype=np.int64) for _ in groups], [np.zeros(7, dtype=np.int64) for _ in groups]
    pocket = attempts = capacity = 0
    for w in range(-1, WINDOWS):
        first = (w + 1) * STEPS
        for x, g in enumerate(groups):
            dt, st = timed(lambda: g.sweep_gcmc(STEPS, SEED, first, species=table, max_molecules=CAP, positions=False, **GEOM))
            if w < 0:
                continue
            t[x].append(dt / (k * STEPS) * 1e6)
            trials[x] += st["trials"].sum(axis=0)
            accepted[x] += st["accepted"].sum(axis=0)
            if x == 1:
                p, a = g.block_counts()
                pocket += int(p.sum())
                attempts += int(a.sum())
                capacity += int(st["capacity"].sum())
    cell = lambda v: f"{statistics.median(v):7.2f} ({min(v):6.2f}-{max(v):6.2f})"
    print(f"  K {k:3d} | (a) no masks {cell(t[0])} | acceptance {ratios(trials[0], accepted[0])}")
    if HAS_BLOCKS:
        tested = int(trials[1][:6].sum()) - capacity                  # every proposal that went through the resolve stage
        print(f"        | (b) atom masks {cell(t[1])}, (b)/(a) {statistics.median(t[1]) / statistics.median(t[0]):.2f} | mean attempt index "
              f"{attempts / max(tested, 1):.2f} | pocket-blocked {pocket / (k * STEPS * WINDOWS):.3f} of the steps | acceptance {ratios(trials[1], accepted[1])}")
    for g in groups:
        g.close()
    for s in sets:                                                 # every K starts from the same state
        for ch in s[:k]:
            ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
            ch.refresh()
for s in sets[::-1]:
    for ch in s[::-1]:
        ch.close()
