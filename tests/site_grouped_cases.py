"""Grouped cycles of site hopping (ceg_site_group_sweep_grouped) on the synthetic tables of tests/site_cases.py, shared by
tests/test_site_grouped_host.py (CPU) and tests/test_gpu_site_grouped.py (GPU).

A case is (n, m, K) x steps per cycle (m and 2 m: groupcycles 1 and 2) x restart (without, with).  The temperatures are one per
chain, geometric between the two ends that ``TEMPERATURES`` gives for the shape: the low end makes cycles that are rejected, the
high end cycles that are accepted by the draw.  The host replay of a case (``mcrng.site_grouped_replay`` from the extended-precision
baseline) is computed once and kept.

What a case must contain is listed by ``required``; ``coverage`` counts it over the host replay alone.  Some things cannot occur
by the rule itself and are therefore not asked:
  * a cut of 7 steps inside a cycle of ONE step ((2, 1, 1) at steps_per_cycle = 1);
  * an r_j that hits a displaced position when m = 1 (there is no earlier exchange);
  * a NEW minimum at the end of a rejected cycle: the restored energy E0 is the energy of the previous cycle end, which the strict <
    has already seen.  What is asked instead is a rejected cycle that comes after an update of the minimum (the kept population
    then differs from the start's and must survive the restore), and that no rejected cycle carries the flag.  The one chain of (2, 1, 1) starts
    on the lower of its two sites, so its minimum never moves at all, and this is not asked of it.
With n = m every site is occupied: a hop meets an occupied site or the own site, and a restart is a full permutation of the same
sites, so the energy never moves but for the rounding of the restart's baseline.  Such a case reaches accepted cycles only (E1 == E0
is accepted by the draw: u < exp(0) = 1); it is there for the full permutation and for the hops."""
import functools

import numpy as np

import site_cases as SC
from ceg_hip import mcrng

FULL = (40, 40, 3)                                # n = m
CASES = SC.CASES + (FULL,)


def ncycles(case) -> int:
    """12 cycles; 40 where a cycle is one or two steps, so that a cut of 7 steps falls inside several of them"""
    return 40 if case[1] <= 2 else 12


CUT = 7                                           # CEG_HIP_SITE_STEPS_PER_LAUNCH of the cut test
FRAME_EVERY, FRAME_ORIGIN = 2, 1                  # the recorder of the GPU tests: frames at the ends of cycles 1, 3, 5, ...
TAIL = 3.25
# (T of chain 0, T of chain K - 1) per (n, m, K), without and with restart
TEMPERATURES = {
    (2, 1, 1): ((15.0, 15.0), (15.0, 15.0)),          # the two sites lie 23.6 K apart
    (5, 2, 3): ((50.0, 500.0), (50.0, 500.0)),
    (70, 63, 5): ((30.0, 3000.0), (300.0, 30000.0)),
    (70, 64, 4): ((30.0, 3000.0), (300.0, 30000.0)),
    (200, 65, 5): ((30.0, 3000.0), (300.0, 30000.0)),
    (300, 130, 9): ((30.0, 3000.0), (300.0, 60000.0)),
    FULL: ((30.0, 3000.0), (30.0, 3000.0)),
}
VARIANTS = tuple((case, g, restart) for case in CASES for g in (1, 2) for restart in (False, True))


def variant_id(v) -> str:
    (n, m, k), g, restart = v
    return f"n{n}-m{m}-K{k}-G{g}-{'restart' if restart else 'plain'}"


def temperatures(case, restart: bool) -> np.ndarray:
    lo, hi = TEMPERATURES[case][1 if restart else 0]
    k = case[2]
    return lo * (hi / lo) ** (np.arange(k) / max(k - 1, 1))


def first_step(case, g: int) -> int:
    """the counter crosses 2^32 after about half of the run"""
    return 2 ** 32 - max((ncycles(case) * g * case[1]) // 2, 1)


def start_energy(case, c: int) -> float:
    n, m, k = case
    fw, it = SC.tables(n)
    return float(mcrng.site_baseline(fw, it, SC.populations(n, m, k)[c], TAIL))


def replay_chain(case, g: int, restart: bool, c: int, energy=None, log=None, grouped=None):
    n, m, k = case
    fw, it = SC.tables(n)
    e0 = start_energy(case, c) if energy is None else float(energy)
    T = np.full(ncycles(case), temperatures(case, restart)[c])
    return mcrng.site_grouped_replay(fw, it, SC.populations(n, m, k)[c], e0, SC.SEED, first_step(case, g), int(SC.stream_ids(k)[c]), T, g * m,
                                     restart=restart, tailcorrection=TAIL, log=log, grouped=grouped)


@functools.lru_cache(maxsize=None)
def host_replay(case, g: int, restart: bool):
    """[K] SiteGroupedReplay by the rule on the host alone, from the extended-precision baseline"""
    return tuple(replay_chain(case, g, restart, c) for c in range(case[2]))


def displaced_hits(n: int, m: int, draws) -> int:
    """exchanges j whose r_j is a position that an earlier exchange moved a foreign value into"""
    moved, hits = set(), 0
    for j, r in enumerate(draws):
        hits += r in moved
        if r != j:
            moved.update((j, r))
    return hits


def coverage(case, g: int, restart: bool, replays) -> dict:
    """counts over all chains of a case's host replay"""
    n, m, k = case
    spc = g * m
    out = dict(downhill=0, by_draw=0, rejected=0, rejected_with_hops=0, rejected_moved=0, displaced=0, rejected_cut=0, rejected_frame=0,
               rejected_after_minimum=0, rejected_new_minimum=0, near_ties=0)
    for c, rp in enumerate(replays):
        pop = SC.populations(n, m, k)[c].astype(np.int64)
        mine, updated = start_energy(case, c), False
        first = first_step(case, g)
        for cyc, cy in enumerate(rp.cycles):
            steps = rp.steps[cyc * spc:(cyc + 1) * spc]
            end = pop.copy() if cy.restart_population is None else cy.restart_population.astype(np.int64)
            for st in steps:
                if st.accepted:
                    end[st.molecule] = st.new_site
            if cy.restarted:
                out["displaced"] += displaced_hits(n, m, mcrng.site_restart_draws(SC.SEED, first + cyc * spc, int(SC.stream_ids(k)[c]), n, m))
            out["near_ties"] += (not cy.after < cy.before) and abs(cy.u - cy.threshold) < 1e-12
            if cy.accepted:
                out["downhill" if cy.after < cy.before else "by_draw"] += 1
                pop = end
            else:
                out["rejected"] += 1
                out["rejected_with_hops"] += cy.hops_accepted > 0
                out["rejected_moved"] += not np.array_equal(end, pop)
                out["rejected_cut"] += any(t % CUT == 0 for t in range(cyc * spc + 1, (cyc + 1) * spc))
                out["rejected_frame"] += mcrng.snapshot_due(cyc, FRAME_ORIGIN, FRAME_EVERY)
                out["rejected_after_minimum"] += updated
            if rp.cycle_energy[cyc] < mine:
                mine, updated = float(rp.cycle_energy[cyc]), True
                out["rejected_new_minimum"] += not cy.accepted
    return out


def required(case, g: int, restart: bool) -> tuple:
    """the counts of ``coverage`` that must be positive for the case (the module docstring gives the reasons for what is left out)"""
    n, m, k = case
    if n == m:
        return ("by_draw",) + (("displaced",) if restart else ())
    need = ["downhill", "by_draw", "rejected_with_hops", "rejected_moved", "rejected_frame"]
    if m > 1:
        need.append("rejected_after_minimum")
    if g * m > 1:
        need.append("rejected_cut")
    if restart and m > 1:
        need.append("displaced")
    return tuple(need)
