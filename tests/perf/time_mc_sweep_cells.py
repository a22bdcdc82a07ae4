"""Plain sweeps on chains that keep their guests in neighbour cells (ceg_mc_group_set_device_cells): microseconds per chain-step at
K = 16 and 64 chains of three routes, alternated window by window in one process in a rotating order after a warm-up window, median
of the windows with the window-to-window range:
  (1) ceg_mc_group_sweep with device cells: the cell walk in the trial rows, the cell lists kept on the device;
  (2) what such a chain had to use before: ceg_mc_group_trial + ceg_mc_group_accept per step from the host, with the moves and the
      decisions of a scout group's logged sweep, packed into the call arguments before the clock starts;
  (3) the same system created with CEG_HIP_MC_CELLS=0 in the existing sweep (the exhaustive pair loop).
Systems:
  a  the CHA + Na workload of time_mc_sweep.py (64 CO2, grids and Ewald sums) with cells forced on: where cells do not pay;
  b  the 72 x 66 x 84 A cell of time_mc_cells.py with 250 CO2 + 8 Na (no grids, no Ewald sums: the guest-guest term alone);
  c  the same cell with 1500 CO2 + 24 Na, route (1) and (3) only -- beyond the population sizes the sweeps are verified for.
Every sweep route ends with the drift check of run_montecarlo!: the energy of ceg_mc_group_baseline after the run against the energy
before it plus the accumulated `delta` of the statistics, rtol 1e-9 (the terms a displacement cannot change are left out of both).
Also printed: the cost per CALL of a one-step sweep with device cells (upload of the lists, the fill launch, and the read-back of
the lists when the step was accepted) against a one-step sweep without cells.

    python tests/perf/time_mc_sweep_cells.py a b        # the tables of systems a and b
    python tests/perf/time_mc_sweep_cells.py c          # system c (run it once, after b has passed its drift check)
    python tests/perf/time_mc_sweep_cells.py a --only 1 # route (1) alone at K = 16, for a rocprofv3 --kernel-trace --stats run
"""
import copy
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..'), os.path.join(here, '..')]
import numpy as np
import ceg_hip as ceg
from ceg_hip import _abi, workloads as W
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.hostmirror.constants import COULOMBIC_CONVERSION_FACTOR
from ceg_hip.energy import DeviceMonteCarlo
from test_gpu_consumers import _RawMc, _rotation

KS = (16, 64)
WINDOWS = 5
SEED = 20241019
FF = "BoulfelfelSholl2021"
systems = [a for a in sys.argv[1:] if a in ("a", "b", "c")] or ["a", "b"]
only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else 0
lib = _abi.load_library()

golden = os.path.join(here, '..', 'golden', 'raspa')
tmp = tempfile.mkdtemp(prefix="ceg_mcc_")
os.makedirs(os.path.join(tmp, "raspa"))
for sub in ("forcefield", "molecules", "structures"):
    os.symlink(os.path.join(golden, sub), os.path.join(tmp, "raspa", sub))
ceg.setdir_RASPA(os.path.join(tmp, "raspa"))
co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", FF)
base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)


class System:
    """make(cells) -> a new chain (an object with the handle in ._h or .h and close()); sizes: atoms per molecule in device order"""

    def handle(self, chain):
        return chain._h if hasattr(chain, "_h") else chain.h


class Cha(System):
    name, steps = "a: CHA + Na, 64 CO2, cells forced on", 100

    def __init__(self):
        fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96_Na_11812", FF)
        centers = (W._random_atoms_min_sep(64, 1.0, 0.14, np.random.default_rng(0))) @ fw.mat.T
        self.mc = M.setup_montecarlo("CHA_1.4_3b4eeb96_Na_11812", FF, [co2.with_positions(c + base) for c in centers])
        self.sizes = [3] * 64
        self.owner = None

    def make(self, cells):
        os.environ["CEG_HIP_MC_CELLS"] = "1" if cells else "0"
        mcc = copy.copy(self.mc)
        mcc.positions = [[p.copy() for p in kind] for kind in self.mc.positions]
        ch = DeviceMonteCarlo(mcc, grids_from=self.owner)
        self.owner = self.owner or ch
        del os.environ["CEG_HIP_MC_CELLS"]
        return ch


class Large(System):
    def __init__(self, nco2, nna, steps):
        self.name, self.steps = f"{'b' if nco2 < 1000 else 'c'}: 72 x 66 x 84 A, {nco2} CO2 + {nna} Na", steps
        ff = ceg.parse_forcefield_RASPA(FF)
        rng = np.random.default_rng(11)
        ids, na_id = [ff.sdict[a] - 1 for a in co2.atomic_symbol], [ff.sdict["Na"] - 1]
        mat = np.array([[72.0, 0, 0], [9.0, 66.0, 0], [-7.0, 11.0, 84.0]]).T
        rules, offsets = ff.pair_table()
        self.table = (mat, ff.cutoff ** 2, rules, offsets, ff.nkinds, COULOMBIC_CONVERSION_FACTOR)
        mols = [(ids, c + base @ _rotation(rng).T) for c in (rng.uniform(0, 1, (nco2, 3)) @ mat.T)] + \
               [(na_id, c[None].copy()) for c in (rng.uniform(0, 1, (nna, 3)) @ mat.T)]
        self.pos = np.concatenate([p for _k, p in mols])
        self.kinds = np.array([k for ks, _p in mols for k in ks], dtype=np.int32)
        self.first = np.concatenate([[0], np.cumsum([len(ks) for ks, _p in mols])]).astype(np.int32)
        self.sizes = [len(ks) for ks, _p in mols]

    def make(self, cells):
        os.environ["CEG_HIP_MC_CELLS"] = "1" if cells else "0"
        h = _RawMc(lib, *self.table)
        h.set_guests(self.pos, self.kinds, self.first)
        del os.environ["CEG_HIP_MC_CELLS"]
        assert (h.cells() is not None) == bool(cells)
        return h


class Group:
    def __init__(self, system, chains, device_cells=False):
        self.k = len(chains)
        hs = (C.c_void_p * self.k)(*[system.handle(c) for c in chains])
        self.h = C.c_void_p()
        _abi.check(lib, lib.ceg_mc_group_create(C.byref(self.h), hs, self.k))
        if device_cells:
            _abi.check(lib, lib.ceg_mc_group_set_device_cells(self.h, 1, 0))
        k = self.k
        self.sid = np.arange(k, dtype=np.uint32)
        self.par = [np.full(k, 300.0), np.full(k, 0.5), np.full(k, np.radians(30.0)), np.full(k, 0.5)]
        self.bead = np.ascontiguousarray([1 if m == 3 else 0 for m in system.sizes] * k, dtype=np.int32)
        self.delta = np.zeros(k)

    def sweep(self, first, steps, log=False):
        p = _abi.SweepParams(SEED, first, self.sid.ctypes.data, *[a.ctypes.data for a in self.par], self.bead.ctypes.data)
        stats = np.zeros(self.k, dtype=_abi.SWEEP_STATS_DTYPE)
        rec = np.zeros((steps, self.k), dtype=_abi.SWEEP_RECORD_DTYPE) if log else None
        start = time.perf_counter()
        rc = lib.ceg_mc_group_sweep(self.h, C.addressof(p), steps, stats.ctypes.data, rec.ctypes.data if log else None)
        dt = time.perf_counter() - start
        _abi.check(lib, rc)
        self.delta += stats["delta"]
        return dt, stats, rec

    def energy(self):
        """the terms of baseline_energy a displacement changes, per chain"""
        out = np.zeros(self.k, dtype=_abi.MC_BASELINE_DTYPE)
        _abi.check(lib, lib.ceg_mc_group_baseline(self.h, 0, out.ctypes.data))
        return out["framework_vdw"] + out["framework_direct"] + out["inter"] + 2.0 * out["recip_framework"] + out["recip_guests"]

    def close(self):
        lib.ceg_mc_group_destroy(self.h)


def pack(log, sizes):
    """the arguments of route (2)'s calls for every step of a log [steps, K]"""
    steps, k = log.shape
    n = np.ones(k, dtype=np.int32)
    kinds = np.zeros(1, dtype=np.int32)
    calls = []
    for s in range(steps):
        mol = np.ascontiguousarray(log["molecule"][s], dtype=np.int32)
        parts = [log["positions"][s, c, :sizes[mol[c]]].reshape(-1) for c in range(k)]
        acc = log["accepted"][s] != 0
        trial = np.ascontiguousarray(np.concatenate(parts))
        amol = np.where(acc, mol, -1).astype(np.int32)
        apos = np.ascontiguousarray(np.concatenate([p for p, a in zip(parts, acc) if a])) if acc.any() else np.zeros(1)
        calls.append((mol, n, kinds, trial, amol, apos, bool(acc.any())))
    return calls


def route_calls(group, system, chains, calls):
    out = np.empty(8 * group.k)
    op = _abi.dptr(out)
    args = [((group.h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(kinds), 0, _abi.dptr(trial), op),
             (group.h, _abi.i32ptr(amol), _abi.dptr(apos)) if any_acc else None) for mol, n, kinds, trial, amol, apos, any_acc in calls]
    start = time.perf_counter()
    rc = 0
    for t, a in args:
        rc |= lib.ceg_mc_group_trial(*t)
        if a is not None:
            rc |= lib.ceg_mc_group_accept(*a)
    lib.ceg_mc_get_state(system.handle(chains[0]), None, None, None)       # drains the last, asynchronous accept inside the window
    dt = time.perf_counter() - start
    assert rc == 0, lib.ceg_last_error()
    return dt


def drift(name, group, before):
    after = group.energy()
    err = np.abs((before + group.delta) - after) / np.abs(after)
    print(f"#   drift of {name}: max |recorded - actual| / |actual| = {err.max():.2e} over {group.k} chains (rtol 1e-9)", flush=True)
    assert (err <= 1e-9).all(), (name, err.max())


def spread(x):
    return f"{statistics.median(x):8.2f} (range {min(x):7.2f}-{max(x):7.2f})"


for which in systems:
    system = Cha() if which == "a" else (Large(250, 8, 100) if which == "b" else Large(1500, 24, 50))
    steps, host_route = system.steps, which != "c"
    print(f"# system {system.name}: us per chain-step, median of {WINDOWS} windows of {steps} steps, routes alternated in a rotating order", flush=True)
    if only:
        chains = [system.make(only == 1) for _ in range(16)]
        g = Group(system, chains, device_cells=only == 1)
        g.sweep(0, 50)
        dt, stats, _ = g.sweep(50, 1000)
        print(f"route ({only}), K = 16: {dt / 16000 * 1e6:.2f} us per chain-step over 1000 steps, "
              f"{int((stats['translation_accepted'] + stats['rotation_accepted']).sum())} of 16000 moves accepted")
        g.close()
        continue
    for k in KS:
        sets = [[system.make(True) for _ in range(k)] for _ in range(3 if host_route else 1)] + [[system.make(False) for _ in range(k)]]
        g1 = Group(system, sets[0], device_cells=True)
        scout, g2 = (Group(system, sets[1], device_cells=True), Group(system, sets[2])) if host_route else (None, None)
        g3 = Group(system, sets[-1])
        e1, e3 = g1.energy(), g3.energy()
        t = {1: [], 2: [], 3: []}
        accepted = 0
        for w in range(-1, WINDOWS):                                # window -1: warm-up
            first = (w + 1) * steps
            calls = pack(scout.sweep(first, steps, log=True)[2], system.sizes) if host_route else None
            for r in [(1, 2, 3), (2, 3, 1), (3, 1, 2)][(w + 1) % 3]:
                if r == 1:
                    dt, stats, _ = g1.sweep(first, steps)
                    accepted += int((stats["translation_accepted"] + stats["rotation_accepted"]).sum()) if w >= 0 else 0
                elif r == 2:
                    if not host_route:
                        continue
                    dt = route_calls(g2, system, sets[2], calls)
                else:
                    dt = g3.sweep(first, steps)[0]
                if w >= 0:
                    t[r].append(dt / (k * steps) * 1e6)
        print(f"  K = {k:3d} | (1) sweep, device cells {spread(t[1])} | (2) host trial + accept {spread(t[2]) if host_route else '       -'} | "
              f"(3) sweep, CEG_HIP_MC_CELLS=0 {spread(t[3])} | accepted {accepted / (k * steps * WINDOWS):.2f}", flush=True)
        drift("(1)", g1, e1)
        drift("(3)", g3, e3)
        # the cost per call: one-step sweeps (the lists are uploaded before and, after an accepted step, read back after the call)
        one = {1: [], 3: []}
        for i in range(20):
            one[1].append(g1.sweep((WINDOWS + 1) * steps + i, 1)[0] * 1e6)
            one[3].append(g3.sweep((WINDOWS + 1) * steps + i, 1)[0] * 1e6)
        print(f"#   one-step sweep calls, us per call: device cells {spread(one[1])}, without cells {spread(one[3])}", flush=True)
        for g in (g1, scout, g2, g3):
            if g is not None:
                g.close()
        for s in sets[::-1]:
            for ch in s[::-1]:
                if ch is not getattr(system, "owner", None):
                    ch.close()
    if getattr(system, "owner", None) is not None:
        system.owner.close()
