"""Whole sweeps on the device against the host-driven group calls: microseconds per chain-step at K = 1, 16, 64, 256 chains, a step
being one Markov step of run_montecarlo! (src/simulation.jl:727-781): choose molecule and move, movement_energy before + after,
compute_accept_move, update_mc! when accepted.  Two routes, alternated window by window in the same process after a warm-up,
median of the windows:
  (a) ceg_mc_group_sweep: proposal, rows, decision and update on the device, one synchronisation per window (no log);
  (b) the route of the chain groups before sweeps existed: ceg_mc_group_trial + ceg_mc_group_accept per step, driven from NumPy
      with the SAME move stream and the SAME decisions -- both are taken from the log of a third, untimed group that runs the same
      sweep ahead of the window, and are packed into the call arguments BEFORE the clock starts, so route (b) is charged neither
      for producing proposals nor for deciding.
CHA + Na framework (0.15 A grids built by the HIP kernels, shared by every chain), 64 CO2 guests per chain, T = 300 K,
dmax = 0.5 A, thetamax = 30 degrees, p_rotation = 0.5.

    python tests/perf/time_mc_sweep.py              # the table
    python tests/perf/time_mc_sweep.py --sweep 16   # route (a) alone at K = 16, for a rocprofv3 --kernel-trace --stats run
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
from ceg_hip import _abi, workloads as W
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup

KS = (1, 16, 64, 256)
STEPS, WINDOWS = 200, 7
SEED = 20240607
only = int(sys.argv[sys.argv.index("--sweep") + 1]) if "--sweep" in sys.argv else 0

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcs_")
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


PARAMS = dict(temperature=300.0, dmax=0.5, thetamax=30.0, degrees=True, p_rotation=0.5)
lib = _abi.load_library()


def route_sweep(group, first, steps):
    """(a): one call, one synchronisation"""
    start = time.perf_counter()
    stats = group.sweep(steps, SEED, first, **PARAMS)
    return time.perf_counter() - start, stats


def pack(log):
    """the arguments of route (b)'s calls for every step of a log [steps, K] (every molecule here has three atoms)"""
    steps, k = log.shape
    n = np.ones(k, dtype=np.int32)
    kinds = np.zeros(1, dtype=np.int32)
    calls = []
    for s in range(steps):
        mol = np.ascontiguousarray(log["molecule"][s], dtype=np.int32)
        trial = np.ascontiguousarray(log["positions"][s, :, :3, :]).reshape(-1)
        acc = log["accepted"][s] != 0
        amol = np.where(acc, mol, -1).astype(np.int32)
        apos = np.ascontiguousarray(log["positions"][s, acc, :3, :]).reshape(-1) if acc.any() else np.zeros(1)
        calls.append((mol, n, kinds, trial, amol, apos, bool(acc.any())))
    return calls


def route_calls(group, calls, k):
    """(b): one ceg_mc_group_trial per step, one ceg_mc_group_accept where a chain accepted"""
    out = np.empty(8 * k)
    op = _abi.dptr(out)
    args = [((group._h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(kinds), 0, _abi.dptr(trial), op),
             (group._h, _abi.i32ptr(amol), _abi.dptr(apos)) if any_acc else None) for mol, n, kinds, trial, amol, apos, any_acc in calls]
    start = time.perf_counter()
    rc = 0
    for t, a in args:
        rc |= lib.ceg_mc_group_trial(*t)
        if a is not None:
            rc |= lib.ceg_mc_group_accept(*a)
    lib.ceg_mc_get_state(group.chains[0]._h, None, None, None)       # the last accept is asynchronous: drained inside the window,
    dt = time.perf_counter() - start                               # as the sweep's own synchronisation is
    assert rc == 0, lib.ceg_last_error()
    return dt


if only:
    chains = make_chains(only)
    with DeviceMonteCarloGroup(chains) as g:
        route_sweep(g, 0, 50)
        dt, stats = route_sweep(g, 50, 2000)
    acc = int((stats["translation_accepted"] + stats["rotation_accepted"]).sum())
    print(f"route (a), K = {only}: {dt / (2000 * only) * 1e6:.2f} us per chain-step over 2000 steps, {acc} of {2000 * only} moves accepted")
    for ch in chains[::-1]:
        ch.close()
    sys.exit(0)

print(f"# us per chain-step, median of {WINDOWS} windows of {STEPS} steps, routes alternated; T = 300 K, dmax 0.5 A, thetamax 30 deg, p_rotation 0.5")
print(f"# {'K':>3} | (a) ceg_mc_group_sweep         | (b) group trial + accept per step | (b)/(a) | accepted")
kmax = max(KS)
sets = [make_chains(kmax) for _ in range(3)]                       # scout (logs the moves ahead), route (a), route (b)
for k in KS:
    groups = [DeviceMonteCarloGroup(s[:k]) for s in sets]
    scout, ga, gb = groups
    a, b = [], []
    accepted = total = 0
    for w in range(-1, WINDOWS):                                    # window -1: warm-up
        first = (w + 1) * STEPS
        _stats, log = scout.sweep(STEPS, SEED, first, log=True, **PARAMS)
        calls = pack(log)
        ta, stats = route_sweep(ga, first, STEPS)
        tb = route_calls(gb, calls, k)
        assert np.array_equal(stats["translation_accepted"] + stats["rotation_accepted"], (log["accepted"] != 0).sum(axis=0))
        if w >= 0:
            a.append(ta / (k * STEPS) * 1e6)
            b.append(tb / (k * STEPS) * 1e6)
            accepted += int((log["accepted"] != 0).sum())
            total += log.size
    # the three groups went through the same moves: the same positions (route (b) applied the logged ones)
    for c in (0, k - 1):
        assert np.array_equal(sets[1][c].state()[0], sets[2][c].state()[0]) and np.array_equal(sets[0][c].state()[0], sets[1][c].state()[0])
    ma, mb = statistics.median(a), statistics.median(b)
    print(f"  {k:3d} | {ma:7.2f} (range {min(a):6.2f}-{max(a):6.2f})  | {mb:7.2f} (range {min(b):6.2f}-{max(b):6.2f})     | {mb / ma:6.1f}  | {accepted / total:.2f}")
    for g in groups:
        g.close()
    for s in sets:                                                 # every K starts from the same state
        for ch in s[:k]:
            ch.mc.positions = [[p.copy() for p in kind] for kind in mc.positions]
            ch.refresh()
for s in sets[::-1]:
    for ch in s[::-1]:
        ch.close()
