"""Tempering ladders inside the site-hopping sweep (ceg_site_group_set_tempering, k_site_sweep_pt): what the exchange costs.

For n = 512 sites, m = 64 molecules, R = 4, 8, 16 rungs and L = 1, 16, 64 ladders on synthetic tables (geometric ladders 300 - 600 K,
the reference's p = 0.1, cycles of 64 steps), in ONE process and on one group per route:
  (a) the tempered sweep: us per step of a call (every ladder makes one step of its R rungs in it) and ladder-steps per second;
  (b) the same K = L R chains at the same temperatures swept untempered (k_site_sweep, one wave per workgroup): what the barrier and
      the exchange cost;
  (c) the only route a caller had before: one sweep_cycles call of ONE step per exchange opportunity, the pair and the decision drawn
      on the host from the stats, an accepted exchange through get_populations / set_populations (which rebases, so the trajectory
      is not the same one; only its cost is compared).
(a) and (b) are timed in alternated windows (a, b, a, b, ...), the median of the windows and their spread are reported; (c) runs
fewer steps, it is slower by orders of magnitude.

    python tests/perf/time_site_tempering.py > profiles/site_tempering.txt
"""
import os
import statistics
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, '..', '..', 'crystalenergygrids.jl_amd'), os.path.join(here, '..', '..')]
import numpy as np
from ceg_hip import mcrng
from ceg_hip import sitehopping as SH

SEED = 20240915
N, M, SPC = 512, 64, 64
NCYCLES, WINDOWS, HOST_STEPS = 128, 7, 300


def tables(n, rng):
    fw = -1000.0 * rng.random(n)
    it = np.triu(600.0 * rng.random((n, n)) - 300.0, 1)
    it = it + it.T
    it[np.arange(n), np.arange(n)] = 1e100
    return fw, it


def host_route(g, R, L, T, cdf, steps):
    """(c): `steps` steps of every ladder, one call per step, the exchange on the host"""
    t0 = time.perf_counter()
    stats = g.stats()
    accepted = 0
    for s in range(steps):
        pairs = [mcrng.site_exchange_draw(SEED, s, l, cdf) for l in range(L)]
        swaps = []
        for l, (j, u) in enumerate(pairs):
            if j < 0:
                continue
            a = l * R + j
            E_a, E_b = float(stats["energy"][a]), float(stats["energy"][a + 1])
            if E_b < E_a or u < mcrng.site_exchange_threshold(E_a, E_b, T[a], T[a + 1]):
                swaps.append(a)
        if swaps:
            pops = g.populations()
            for a in swaps:
                pops[[a, a + 1]] = pops[[a + 1, a]]
            g.set_populations(pops)
            accepted += len(swaps)
        # (the rungs of an attempted pair should sit this step out; they hop here, which only makes this route look cheaper)
        stats, _r, _l = g.sweep_cycles(1, SEED, s, temperature=T, steps_per_cycle=1, cycle0=s)
    return (time.perf_counter() - t0) / steps, accepted


def shape(R, L):
    k = R * L
    rng = np.random.default_rng(N + M + k)
    fw, it = tables(N, rng)
    pops = np.stack([rng.permutation(N)[:M] for _ in range(k)]).astype(np.uint16)
    T = np.tile(300.0 * 2.0 ** (np.arange(R) / (R - 1)), L)
    cdf = mcrng.site_exchange_cdf(R, 0.1)
    steps = NCYCLES * SPC
    with SH.DeviceSiteHoppingGroup(fw, it, pops) as ga, SH.DeviceSiteHoppingGroup(fw, it, pops) as gb, SH.DeviceSiteHoppingGroup(fw, it, pops) as gc:
        ga.set_tempering(R, pair_cdf=cdf)
        for g in (ga, gb):
            g.sweep_cycles(NCYCLES // 4, SEED, 0, temperature=T, steps_per_cycle=SPC)              # warm-up
        first = NCYCLES // 4 * SPC
        ta, tb = [], []
        for w in range(WINDOWS):
            for g, out in ((ga, ta), (gb, tb)):
                t0 = time.perf_counter()
                g.sweep_cycles(NCYCLES, SEED, first, temperature=T, steps_per_cycle=SPC, cycle0=w * NCYCLES)
                out.append((time.perf_counter() - t0) / steps)
            first += steps
        att, acc, _rep = ga.tempering_read()
        drift = np.abs(ga.stats()["energy"] - ga.baseline_energies()).max()
        host_route(gc, R, L, T, cdf, 20)                                                         # warm-up
        tc, host_acc = host_route(gc, R, L, T, cdf, HOST_STEPS)
    a, b = statistics.median(ta), statistics.median(tb)
    ratios = [x / y for x, y in zip(ta, tb)]
    print(f"  R = {R:2d}  L = {L:2d}  K = {k:4d}: (a) {a * 1e6:7.3f} us per step ({min(ta) * 1e6:.3f} - {max(ta) * 1e6:.3f}), {L / a:10.4e} ladder-steps/s;  "
          f"(b) {b * 1e6:7.3f} us ({min(tb) * 1e6:.3f} - {max(tb) * 1e6:.3f});  (a)/(b) {a / b:5.2f} (windows {min(ratios):.2f} - {max(ratios):.2f});  "
          f"(c) {tc * 1e6:9.1f} us per step over {HOST_STEPS} steps, (a)/(c) {a / tc:8.5f};  "
          f"exchanges accepted {int(acc.sum())} of {int(att.sum())}, |energy - baseline| <= {drift:.2e}")


if __name__ == "__main__":
    print(f"n = {N} sites, m = {M} molecules, cycles of {SPC} steps, {NCYCLES * SPC} steps per timed call, {WINDOWS} alternated windows; p = 0.1")
    for R in (4, 8, 16):
        for L in (1, 16, 64):
            shape(R, L)
