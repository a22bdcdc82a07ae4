"""Grouped cycles inside the site-hopping sweep (ceg_site_group_sweep_grouped, k_site_sweep_grouped): what they cost.

For n = 512 sites, m = 64 molecules, K = 1, 64, 1024 chains, groupcycles G = 1, 4 (cycles of G m steps), without and with a restart
per cycle, on synthetic tables, in ONE process and on one group per route:
  (a) the grouped sweep: us per step of a call (every chain makes one step in it);
  (b) the same chains swept by sweep_cycles over the same steps (k_site_sweep): the difference is the save, the decision and, with
      restart, the shuffle and the in-wave baseline, once per cycle;
  (c) the only route a caller had before: one sweep_cycles call per cycle, the populations read back, the decision on the host from
      the stats, a rejection through set_populations (which also rebases), a restart through a host randperm and another
      set_populations.  It is not the same trajectory; only its cost is compared.
(a) and (b) are timed in alternated windows (a, b, a, b, ...); the median of the windows and their spread are reported.  (c) runs
fewer cycles.  Every row runs at the same temperature.  (a) and (b) are still not the same trajectory: a restarted chain begins
every cycle from a random population and makes more downhill hops, which pay no exp, than the plain sweep beside it, so
(a) - (b) with restart is if anything a lower bound of what the restart costs.

    python tests/perf/time_site_grouped.py > profiles/site_grouped.txt
"""
import os
import statistics
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
from ceg_hip import sitehopping as SH

SEED = 20241020
N, M = 512, 64
STEPS, WINDOWS, HOST_CYCLES = 8192, 7, 40
TEMPERATURE = 3000.0      # one temperature for every row, so that rows with and without restart differ in the restart alone


def tables(n, rng):
    fw = -1000.0 * rng.random(n)
    it = np.triu(600.0 * rng.random((n, n)) - 300.0, 1)
    it = it + it.T
    it[np.arange(n), np.arange(n)] = 1e100
    return fw, it


def host_route(g, k, spc, restart, T, cycles, rng):
    """(c): `cycles` grouped cycles of every chain, one call per cycle, the decision, the restore and the restart on the host"""
    t0 = time.perf_counter()
    stats, pops = g.stats(), g.populations()
    rejected = 0
    for cyc in range(cycles):
        E0, P0 = stats["energy"].copy(), pops
        if restart:
            g.set_populations(np.stack([rng.permutation(N)[:M] for _ in range(k)]).astype(np.uint16))
        stats, _r, _l = g.sweep_cycles(1, SEED, cyc * spc, temperature=T, steps_per_cycle=spc, cycle0=cyc)
        pops = g.populations()
        E1 = stats["energy"]
        keep = (E1 < E0) | (rng.random(k) < np.exp(np.minimum((E0 - E1) / T, 0.0)))      # (vectorised: the cheapest host decision)
        if not keep.all():
            pops[~keep] = P0[~keep]
            g.set_populations(pops)          # (rebases: the accepted chains' energies move to their baselines' bits)
            stats = g.stats()
            rejected += int((~keep).sum())
    return (time.perf_counter() - t0) / (cycles * spc), rejected


def shape(k, G, restart):
    spc = G * M
    ncycles = STEPS // spc
    rng = np.random.default_rng(N + M + k)
    fw, it = tables(N, rng)
    pops = np.stack([rng.permutation(N)[:M] for _ in range(k)]).astype(np.uint16)
    T = TEMPERATURE
    with SH.DeviceSiteHoppingGroup(fw, it, pops) as ga, SH.DeviceSiteHoppingGroup(fw, it, pops) as gb, SH.DeviceSiteHoppingGroup(fw, it, pops) as gc:
        ga.sweep_grouped(ncycles // 4, SEED, 0, temperature=T, steps_per_cycle=spc, restart=restart)      # warm-up
        gb.sweep_cycles(ncycles // 4, SEED, 0, temperature=T, steps_per_cycle=spc)
        first = ncycles // 4 * spc
        ta, tb, acc, hops = [], [], 0, 0
        for w in range(WINDOWS):
            t0 = time.perf_counter()
            _s, _r, _l, gr = ga.sweep_grouped(ncycles, SEED, first, temperature=T, steps_per_cycle=spc, cycle0=w * ncycles, restart=restart)
            ta.append((time.perf_counter() - t0) / STEPS)
            t0 = time.perf_counter()
            gb.sweep_cycles(ncycles, SEED, first, temperature=T, steps_per_cycle=spc, cycle0=w * ncycles)
            tb.append((time.perf_counter() - t0) / STEPS)
            first += STEPS
            acc += int(gr["accepted"].sum())
            hops += int(gr["hops_accepted"].sum())
        drift = np.abs(ga.stats()["energy"] - ga.baseline_energies()).max()
        host_route(gc, k, spc, restart, T, 4, rng)                                                         # warm-up
        tc, rejected = host_route(gc, k, spc, restart, T, HOST_CYCLES, rng)
    a, b = statistics.median(ta), statistics.median(tb)
    ratios = [x / y for x, y in zip(ta, tb)]
    per_cycle = (a - b) * spc
    print(f"  K = {k:4d}  G = {G}  restart = {int(restart)}: (a) {a * 1e6:7.3f} us per step ({min(ta) * 1e6:.3f} - {max(ta) * 1e6:.3f});  "
          f"(b) {b * 1e6:7.3f} us ({min(tb) * 1e6:.3f} - {max(tb) * 1e6:.3f});  (a)/(b) {a / b:5.2f} (windows {min(ratios):.2f} - {max(ratios):.2f}), "
          f"{per_cycle * 1e6:7.2f} us more per cycle;  (c) {tc * 1e6:9.2f} us per step over {HOST_CYCLES} cycles, (c)/(a) {tc / a:7.1f};  "
          f"cycles accepted {acc} of {WINDOWS * ncycles * k}, hops accepted {hops}, |energy - baseline| <= {drift:.2e}; (c) rejected {rejected}")


if __name__ == "__main__":
    print(f"n = {N} sites, m = {M} molecules, T = {TEMPERATURE:g} K, {STEPS} steps per timed call, {WINDOWS} alternated windows")
    for k in (1, 64, 1024):
        for G in (1, 4):
            for restart in (False, True):
                shape(k, G, restart)
