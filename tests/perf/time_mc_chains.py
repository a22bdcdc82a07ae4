"""Many Markov chains, one step each (make_isotherm, parameterinputs.jl:316-329: one run_gcmc per pressure): microseconds per
chain-step for K = 1 ... 64 chains on one device, a step being one trial placement (movement_energy before + after) and, every
second step, an accept -- the convention of time_mc.py / profiles/r04_consumers_mc.txt.  Two routes, alternated window by window
in the same process after a warm-up, median of the windows:
  (a) K Python threads, each driving its own handle through ceg_mc_trial + ceg_mc_accept (ctypes releases the GIL in the call);
  (b) one chain group (ceg_mc_group_trial + ceg_mc_group_accept): one launch for every chain's trial, one for the accepts.
CHA + Na framework (0.15 A grids built by the HIP kernels, shared by every chain), 64 CO2 guests per chain.

    python tests/perf/time_mc_chains.py              # the table
    python tests/perf/time_mc_chains.py --group 16   # route (b) alone at K = 16, for a rocprofv3 --kernel-trace --stats run
"""
import copy
import os
import statistics
import sys
import tempfile
import threading
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
import ceg_hip as ceg
from ceg_hip import _abi, workloads as W
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

KS = (1, 2, 4, 8, 16, 32, 64)
STEPS, WINDOWS = 200, 7
only = int(sys.argv[sys.argv.index("--group") + 1]) if "--group" in sys.argv else 0

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
t0 = time.perf_counter()
mc = M.setup_montecarlo("CHA_1.4_3b4eeb96_Na_11812", FF, [co2.with_positions(c + base) for c in centers])
print(f"# setup_montecarlo: {time.perf_counter() - t0:.1f} s; {sum(len(k) for k in mc.positions)} molecules, "
      f"{len(mc.ewald.kfactors)} k-vectors per chain")

nchains = only or max(KS)
chains = []
for c in range(nchains):
    mcc = copy.copy(mc)
    mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
    chains.append(DeviceMonteCarlo(mcc, grids_from=chains[0] if chains else None))
lib = chains[0]._lib
idx = (0, 7)
mol = chains[0]._slot[idx[0]][idx[1]]
cur = mc.positions[idx[0]][idx[1]]
trial = np.ascontiguousarray((cur[None] + rng.uniform(-0.5, 0.5, (nchains, 1, 3)))[:, None], dtype=np.float64)   # [chain][1][3][3]


def route_threads(k, steps):
    """(a): k threads, one handle each; wall time from the common start to the last thread's end"""
    bar = threading.Barrier(k + 1)
    ends = [0.0] * k

    def run(c):
        h = chains[c]._h
        t = trial[c].reshape(-1)
        tp = _abi.dptr(t)
        out = np.empty(8)
        op = _abi.dptr(out)
        bar.wait()
        for s in range(steps):
            lib.ceg_mc_trial(h, mol, tp, 1, op)
            if s % 2 == 0:
                lib.ceg_mc_accept(h, mol, tp)
        ends[c] = time.perf_counter()

    ths = [threading.Thread(target=run, args=(c,)) for c in range(k)]
    for th in ths:
        th.start()
    bar.wait()
    start = time.perf_counter()
    for th in ths:
        th.join()
    for c in range(k):                                   # (the last accepts are asynchronous: drained outside the window)
        lib.ceg_mc_get_state(chains[c]._h, None, None, None)
    return max(ends) - start


def route_group(k, steps, group=None):
    """(b): one group of k chains; one ceg_mc_group_trial per step and one ceg_mc_group_accept every second step"""
    g = group or DeviceMonteCarloGroup(chains[:k])
    m = np.full(k, mol, dtype=np.int32)
    n = np.ones(k, dtype=np.int32)
    t = np.ascontiguousarray(trial[:k].reshape(-1))
    out = np.empty(8 * k)
    kinds = np.zeros(1, dtype=np.int32)
    args = (g._h, _abi.i32ptr(m), _abi.i32ptr(n), _abi.i32ptr(kinds), 0, _abi.dptr(t), _abi.dptr(out))
    acc = (g._h, _abi.i32ptr(m), _abi.dptr(t))
    start = time.perf_counter()
    for s in range(steps):
        rc = lib.ceg_mc_group_trial(*args)
        if s % 2 == 0:
            rc |= lib.ceg_mc_group_accept(*acc)
        assert rc == 0, lib.ceg_last_error()
    dt = time.perf_counter() - start
    if group is None:
        g.close()
    return dt


if only:
    with DeviceMonteCarloGroup(chains[:only]) as g:
        route_group(only, 50, g)
        dt = route_group(only, 2000, g)
    print(f"route (b), K = {only}: {dt / (2000 * only) * 1e6:.2f} us per chain-step over 2000 steps")
    for ch in chains[::-1]:
        ch.close()
    sys.exit(0)

# the rows of both routes agree (same kernel body; see tests/test_gpu_mc_chains.py)
with DeviceMonteCarloGroup(chains[:2]) as g:
    rows = g.trial([("move", idx, trial[0]), ("move", idx, trial[1])])
    for c in (0, 1):
        np.testing.assert_allclose(rows[c], chains[c].trial(idx, trial[c]), rtol=1e-10, atol=1e-7)

print(f"# us per chain-step (trial + an accept every second step), median of {WINDOWS} windows of {STEPS} steps, routes alternated")
print(f"# {'K':>3} | (a) K threads x ceg_mc_trial/accept   | (b) one group                | (a)/(b)")
for k in KS:
    route_threads(k, 20)                                 # warm-up
    route_group(k, 20)
    a, b = [], []
    for w in range(WINDOWS):
        a.append(route_threads(k, STEPS) / (k * STEPS) * 1e6)
        b.append(route_group(k, STEPS) / (k * STEPS) * 1e6)
    ma, mb = statistics.median(a), statistics.median(b)
    print(f"  {k:3d} | {ma:8.2f} (range {min(a):6.2f}-{max(a):6.2f})     | {mb:6.2f} (range {min(b):5.2f}-{max(b):5.2f}) | {ma / mb:5.1f}")
for ch in chains[::-1]:
    ch.close()
