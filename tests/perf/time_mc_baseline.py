"""baseline_energy of K chains from the device state: ceg_mc_group_baseline against the rows route, milliseconds per call for all K
chains at K = 1, 16, 64, 256, medians of the repetitions after a warm-up, routes alternated repetition by repetition in one process.
  (a) DeviceMonteCarloGroup.baseline_energies(): two launches for the whole group, the reports composed on the host (the two Ewald
      constants of a chain are computed once per set of species counts, in the warm-up here);
  (a') DeviceMonteCarloGroup.baseline_records(): the call alone, the records as they come back;
  (b) the same with refresh=True: every structure factor recomputed from the positions first (four launches);
  (c) the route a caller had before: DeviceMonteCarlo.baseline_energy(route="rows") chain after chain -- one batch-1 ceg_mc_trial per
      molecule, the structure factor read back, the k-space sums in NumPy -- on the same chains in the same group.
CHA + Na framework, 64 CO2 per chain.  `--profile`: (a) and (b) alone, a few times at K = 256, for a kernel trace:

    python tests/perf/time_mc_baseline.py > profiles/mc_baseline.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tests/perf/time_mc_baseline.py --profile
"""
import copy
import os
import statistics
import sys
import tempfile
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
import ceg_hip as ceg
from ceg_hip import workloads as W
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

PROFILE = "--profile" in sys.argv
KS = (256,) if PROFILE else (1, 16, 64, 256)
REPS, ROWS_REPS = 9, 3

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcb_")
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
print(f"# {sum(len(k) for k in mc.positions)} CO2 per chain ({sum(len(p) for k in mc.positions for p in k)} atom slots), {len(mc.ewald.kfactors)} k-vectors")

chains = []
for _ in range(max(KS)):
    mcc = copy.copy(mc)
    mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
    chains.append(DeviceMonteCarlo(mcc, grids_from=chains[0] if chains else None))


def timed(fn):
    start = time.perf_counter()
    out = fn()
    return (time.perf_counter() - start) * 1e3, out


def cell(v):
    return f"{statistics.median(v):9.3f} ({min(v):8.3f}-{max(v):8.3f})"


print(f"# ms per call for all K chains, median of {REPS} repetitions ((c): {ROWS_REPS}) after a warm-up (range)")
print(f"# {'K':>3} | (a) baseline_energies()        | (b) with refresh               | (c) rows route, chain by chain | (c)/(a) | (c)/(b) | us per chain (a) | (a') baseline_records()")
for k in KS:
    with DeviceMonteCarloGroup(chains[:k]) as group:
        ta, tb, tc, tr = [], [], [], []
        for rep in range(-1, REPS):
            a, ra = timed(lambda: group.baseline_energies())
            b, rb = timed(lambda: group.baseline_energies(refresh=True))
            r, _ = timed(lambda: group.baseline_records())
            if rep >= 0:
                ta.append(a)
                tb.append(b)
                tr.append(r)
            if not PROFILE and rep < ROWS_REPS:
                c, rc = timed(lambda: [d.baseline_energy() for d in group.chains])
                if rep >= 0:
                    tc.append(c)
                for x, y in zip(ra, rc):                                # the routes agree (the tolerance of the tests)
                    assert abs(float(x) - float(y)) <= 1e-9 * abs(float(y)) + 1e-5, (float(x), float(y))
        if PROFILE:
            print(f"  {k:3d} | {cell(ta)} | {cell(tb)} | (a') {cell(tr)}")
        else:
            ma, mb, mcs = statistics.median(ta), statistics.median(tb), statistics.median(tc)
            print(f"  {k:3d} | {cell(ta)} | {cell(tb)} | {cell(tc)} | {mcs / ma:7.1f} | {mcs / mb:7.1f} | {ma / k * 1e3:8.2f}         | {cell(tr)}")
for ch in chains[::-1]:
    ch.close()
