"""Site hopping on the device (ceg_site_group_*, ceg_site_tables): what the new entry points cost, compared against nothing but themselves.

  (s) chains: chain-steps per second and the latency of a step for n = 512 sites, m = 64 molecules at K = 1, 64, 1024, 8192 chains on
      synthetic tables (cycles of 64 steps, every chain at its own temperature), medians of the timed calls after a warm-up; beside
      it the useful bytes gathered per second (two rows of m doubles per chain-step).  Then the largest shape: n = 8192, m = 4096
      at K = 256, where the time of ONE launch of CEG_HIP_SITE_STEPS_PER_LAUNCH steps is what matters.
  (t) tables: ceg_site_tables for n = 256 and 2048 CO2 sites in the CHA + Na framework, beside the composed route a caller had
      before (n batch trials in the empty box, then per site an insertion, a batch trial against it and a removal) in the same process.

    python tests/perf/time_site_hopping.py > profiles/site_hopping.txt          # [--no-tables] [--no-chains]
"""
import os
import statistics
import sys
import tempfile
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
import ceg_hip as ceg
from ceg_hip import sitehopping as SH

SEED = 20240915


def tables(n, rng):
    fw = -1000.0 * rng.random(n)
    it = np.triu(600.0 * rng.random((n, n)) - 300.0, 1)
    it = it + it.T
    it[np.arange(n), np.arange(n)] = 1e100
    return fw, it


def time_chains(n, m, k, ncycles, repeats, spc=64):
    rng = np.random.default_rng(n + m + k)
    fw, it = tables(n, rng)
    pops = np.stack([rng.permutation(n)[:m] for _ in range(k)]).astype(np.uint16)
    T = 30.0 * 100.0 ** (np.arange(k) / max(k - 1, 1))
    with SH.DeviceSiteHoppingGroup(fw, it, pops) as g:
        g.sweep_cycles(max(ncycles // 4, 1), SEED, 0, temperature=T, steps_per_cycle=spc)          # warm-up
        first = max(ncycles // 4, 1) * spc
        times = []
        for r in range(repeats):
            t0 = time.perf_counter()
            stats, _recs, _log = g.sweep_cycles(ncycles, SEED, first, temperature=T, steps_per_cycle=spc, cycle0=r * ncycles)
            times.append(time.perf_counter() - t0)
            first += ncycles * spc
        drift = np.abs(stats["energy"] - g.baseline_energies()).max()
    t = statistics.median(times)
    steps = ncycles * spc
    rate = steps * k / t
    print(f"  n = {n:5d}  m = {m:5d}  K = {k:5d}: {steps:7d} steps per chain and call, {t * 1e3:9.2f} ms per call (spread {min(times) * 1e3:.2f} - {max(times) * 1e3:.2f}), "
          f"{t / steps * 1e6:8.3f} us per step of the call, {rate:12.4e} chain-steps/s, {rate * 2 * m * 8 / 1e9:9.3f} GB/s of gathered doubles, "
          f"acceptance {stats['accepted'].sum() / stats['attempted'].sum():.3f}, |energy - baseline| <= {drift:.2e}")
    return t / steps


def chains():
    print("(s) chains, synthetic tables, cycles of 64 steps")
    for k, ncycles in ((1, 512), (64, 512), (1024, 256), (8192, 64)):
        time_chains(512, 64, k, ncycles, 5)
    print("    MI355X_MICROARCH.md, gathered ROWS (1,152 B each): 16.8-18.8 TB/s from an XCD's L2, 8.6 TB/s from the Infinity Cache; an L2-hit load")
    print("    returns after 180-225 cycles, and a step here is a chain of dependent latencies (draws, LDS read, two 8-byte gathers per lane, butterfly, exp), not a stream")
    per_launch = int(os.environ.get("CEG_HIP_SITE_STEPS_PER_LAUNCH", "4096"))
    print(f"(s) the largest shape; a launch holds at most {per_launch} steps per chain")
    per_step = time_chains(8192, 4096, 256, 2, 3, spc=2048)
    print(f"    one launch of {per_launch} steps at this shape: {per_step * per_launch * 1e3:.1f} ms")


def time_tables():
    from ceg_hip.hostmirror import montecarlo as M
    from ceg_hip.energy import DeviceMonteCarlo
    golden = os.path.join(here, '..', 'golden', 'raspa')
    tmp = tempfile.mkdtemp(prefix="ceg_site_")
    os.makedirs(os.path.join(tmp, "raspa"))
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(os.path.join(golden, sub), os.path.join(tmp, "raspa", sub))
    ceg.setdir_RASPA(os.path.join(tmp, "raspa"))
    FF = "BoulfelfelSholl2021"
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", FF)
    base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
    fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96_Na_11812", FF)
    mc = M.setup_montecarlo("CHA_1.4_3b4eeb96_Na_11812", FF, [(co2.with_positions(base), 0)], blockfiles=[False])
    dev = DeviceMonteCarlo(mc, upload_guests=False)
    print(f"(t) tables, CO2 sites in CHA + Na, {len(mc.ewald.kfactors)} k-vectors")
    for n in (256, 2048):
        rng = np.random.default_rng(n)
        sites = (rng.random((n, 3)) @ fw.mat.T)[:, None, :] + base[None]
        SH.build_site_tables(dev, sites[:16])                                  # warm-up
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = SH.build_site_tables(dev, sites)
            times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        off1, off2 = SH.ewald_offsets(mc, 0, sites[0])
        rows = dev.trial_insert(0, sites)
        inter, pair = np.empty((n, n)), np.empty((n, n))
        for i in range(n):
            dev.insert(0, sites[i])
            r = dev.trial_insert(0, sites)
            dev.remove((0, 0))
            inter[i], pair[i] = r[:, 2], r[:, 3] - rows[:, 3]
        composed = time.perf_counter() - t0
        want = inter + pair + off2
        tol = 1e-9 * (np.abs(inter) + np.abs(pair) + np.abs(rows[:, 3])[:, None] + np.abs(rows[:, 3])[None, :]) + 1e-7      # the tests' tolerance
        fin = ~np.eye(n, dtype=bool) & (np.abs(want) < 1e90)
        worst = (np.abs(got[2] - want)[fin] / tol[fin]).max()
        print(f"  n = {n:5d}: ceg_site_tables {statistics.median(times) * 1e3:9.2f} ms (spread {min(times) * 1e3:.2f} - {max(times) * 1e3:.2f}; 3 launches), "
              f"composed route {composed * 1e3:10.1f} ms ({2 * n + 1} launches and more): {composed / statistics.median(times):8.1f} times; "
              f"{int((rows[:, 0] < 1e90).sum())} open sites, largest difference of a finite interaction {worst:.1e} of the tests' tolerance")
    dev.close()


if __name__ == "__main__":
    if "--no-chains" not in sys.argv:
        chains()
    if "--no-tables" not in sys.argv:
        time_tables()
