"""Grouped cycles of site hopping on the host alone: the restatement (mcrng.site_grouped_replay) against a literal transcription of
the reference's loop with its old_i / before / after cache and group_* copies; the restart's sparse shuffle against a plain
Fisher-Yates; the wave-order baseline against extended precision; and that the cases of tests/site_grouped_cases.py reach what
tests/test_gpu_site_grouped.py relies on."""
import math

import numpy as np
import pytest

import site_cases as SC
import site_grouped_cases as GC
from ceg_hip import mcrng


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _accept(before, after, u, T):
    """compute_accept_move (montecarlo.jl:702-712) with the draw given"""
    if after < before:
        return True
    with np.errstate(over="ignore", invalid="ignore"):
        x = float((np.float64(before) - np.float64(after)) / np.float64(T))
    try:
        e = math.exp(x)
    except OverflowError:
        e = math.inf
    return u < e


def transcription(case, g, restart, c):
    """simulation.jl:922-982 line by line for chain c of a case (0-based sites; ``old_i = -1`` is the reference's 0).  The draws are
    the restatement's: the hop's (i, newpos, u) of the absolute step, the restart's population and wave-order baseline, the
    decision's u.  -> per step (before, after, accepted), per cycle (energy, population), (attemptedhop, acceptedhop), the steps that
    took the cache's branch."""
    n, m, k = case
    fw, it = SC.tables(n)
    population = SC.populations(n, m, k)[c].astype(np.int64)
    stream = int(SC.stream_ids(k)[c])
    temperature = float(GC.temperatures(case, restart)[c])
    groupcycles = g
    energy = np.float64(GC.start_energy(case, c))
    movement_energy = lambda i, si=None: np.float64(mcrng.site_movement_energy(fw, it, population, i, si))      # noqa: E731
    old_i = -1
    accepted = False
    acceptedhop, attemptedhop = 0, 0
    before = movement_energy(0)
    after = movement_energy(0)
    group_populations = np.empty_like(population)
    step = GC.first_step(case, g)
    steps, cycles, cached = [], [], 0
    for _counter_cycle in range(GC.ncycles(case)):
        group_before = before
        group_after = after
        group_populations[:] = population
        group_energy = energy
        if restart:
            population[:] = mcrng.site_restart_population(SC.SEED, step, stream, n, m)
            energy = np.float64(mcrng.site_baseline_wave(fw, it, population, GC.TAIL))
            old_i = -1
            accepted = False
        for _idx_groupcycle in range(groupcycles):
            for _idx_step in range(m):
                i, newpos, u = mcrng.site_propose(SC.SEED, step, stream, m, n)
                if old_i == i:
                    cached += 1
                    if accepted:
                        before = after
                    after = movement_energy(i, newpos)
                else:
                    before, after = movement_energy(i), movement_energy(i, newpos)
                accepted = _accept(before, after, u, temperature)
                if accepted:
                    energy = energy + (after - before)
                    population[i] = newpos
                old_i = i
                steps.append((float(before), float(after), accepted))
                step += 1
        attemptedhop += 1
        w = mcrng.draw(SC.SEED, step - 1, stream, mcrng.SITE_GROUP)
        if _accept(group_energy, energy, mcrng.uniform(w[0], w[1]), temperature):
            acceptedhop += 1
        else:
            before = group_before
            after = group_after
            population[:] = group_populations
            energy = group_energy
            old_i = -1
            accepted = False
        cycles.append((float(energy), population.astype(np.uint16)))
    return steps, cycles, (attemptedhop, acceptedhop), cached


@pytest.mark.parametrize("variant", GC.VARIANTS, ids=GC.variant_id)
def test_restatement_equals_the_reference_loop_with_its_cache(variant):
    case, g, restart = variant
    hits = 0
    for c, rp in enumerate(GC.host_replay(case, g, restart)):
        steps, cycles, (att, acc), cached = transcription(case, g, restart, c)
        hits += cached
        assert len(steps) == len(rp.steps) and len(cycles) == len(rp.cycles)
        for t, (st, (before, after, ok)) in enumerate(zip(rp.steps, steps)):
            assert _bits(st.before) == _bits(before) and _bits(st.after) == _bits(after) and st.accepted == ok, (c, t)
        for cyc, (e, pop) in enumerate(cycles):
            assert _bits(rp.cycle_energy[cyc]) == _bits(e) and np.array_equal(rp.cycle_population[cyc], pop), (c, cyc)
        assert (rp.attempted, rp.accepted) == (att, acc)
        # delta follows the energy: energy - delta stays the baseline the chain began from, to rounding
        assert abs((rp.energy - rp.delta) - GC.start_energy(case, c)) <= 1e-9 * max(abs(GC.start_energy(case, c)), 1.0)
    if case[1] <= 2 and (g * case[1] > 1 or not restart):
        assert hits       # the cache's branch was taken: the same molecule twice in a row with no reset between


@pytest.mark.parametrize("variant", GC.VARIANTS, ids=GC.variant_id)
def test_cases_reach_what_the_gpu_tests_rely_on(variant):
    case, g, restart = variant
    cov = GC.coverage(case, g, restart, GC.host_replay(case, g, restart))
    for key in GC.required(case, g, restart):
        assert cov[key] > 0, (key, cov)
    assert cov["rejected_new_minimum"] == 0 and cov["near_ties"] == 0, cov
    for rp in GC.host_replay(case, g, restart):
        for cy in rp.cycles:
            assert cy.restarted == restart and (restart or _bits(cy.restart_energy) == _bits(cy.before))


def test_a_nan_energy_is_rejected_by_the_rule():
    fw, it = SC.tables(5)
    rp = mcrng.site_grouped_replay(fw, it, [0, 1], math.nan, 3, 0, 0, [1000.0] * 6, 4)        # E0 is NaN, and so is every E1
    assert not any(cy.accepted for cy in rp.cycles) and sum(cy.hops_accepted for cy in rp.cycles) > 0
    assert math.isnan(rp.energy) and rp.population.tolist() == [0, 1] and (rp.attempted, rp.accepted) == (6, 0)


@pytest.mark.parametrize("n,m", [(2, 1), (5, 2), (5, 5), (40, 40), (70, 64), (300, 130), (65535, 3)], ids=str)
def test_restart_population_is_a_plain_fisher_yates(n, m):
    displaced = 0
    for step in (0, 2 ** 32 - 1, 2 ** 40 + 5):
        for stream in (0, 7):
            r = mcrng.site_restart_draws(SC.SEED, step, stream, n, m)
            assert all(j <= r[j] < n for j in range(m))
            perm = list(range(n))
            for j in range(m):
                perm[j], perm[r[j]] = perm[r[j]], perm[j]
            got = mcrng.site_restart_population(SC.SEED, step, stream, n, m)
            assert got.dtype == np.uint16 and got.tolist() == perm[:m]
            assert len(set(got.tolist())) == m and (got < n).all()
            displaced += GC.displaced_hits(n, m, r)
    if n == m and m > 2:
        assert displaced
    # the key: counter word 3 = 14 | (j << 8) of the cycle's first step
    w = mcrng.draw(SC.SEED, 5, 3, 14 | ((m - 1) << 8))
    want = (m - 1) + min(int(math.floor(mcrng.uniform(w[0], w[1]) * float(n - m + 1))), n - m)
    assert mcrng.site_restart_draws(SC.SEED, 5, 3, n, m)[m - 1] == want and (mcrng.SITE_GROUP, mcrng.SITE_RESTART) == (13, 14)


@pytest.mark.parametrize("case", GC.CASES, ids=str)
def test_baseline_wave_against_extended_precision(case):
    n, m, k = case
    fw, it = SC.tables(n)
    pops = list(SC.populations(n, m, k)) + [mcrng.site_restart_population(SC.SEED, 11, c, n, m) for c in range(2)]
    for pop in pops:
        p = pop.astype(np.int64)
        got = mcrng.site_baseline_wave(fw, it, p, GC.TAIL)
        want = mcrng.site_baseline(fw, it, p, GC.TAIL)
        terms = abs(GC.TAIL) + np.abs(fw[p]).sum() + np.abs(np.triu(it[np.ix_(p, p)], 1)).sum()
        N = m + m * (m - 1) // 2
        assert abs(np.longdouble(got) - want) <= N * 2.0 ** -53 * terms, (case, got, want)
