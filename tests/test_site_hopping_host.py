"""Site hopping, host side (no device): the random stream's purpose 10, the row sum in the device's order, the replay against a literal
transcription of the reference's loop, the random start populations, and a CPU assertion for every claim that
tests/test_gpu_site_sweep.py makes about what its cases reach."""
import math

import numpy as np
import pytest

import site_cases as SC
from ceg_hip import mcrng


def test_purpose_10_known_answers():
    assert (mcrng.SITE_SELECT, mcrng.SITE_POPULATE, mcrng.ACCEPT) == (10, 11, 3)
    # the block itself, then what site_propose makes of it
    assert mcrng.draw(1, 2, 3, mcrng.SITE_SELECT) == KNOWN_BLOCK
    assert mcrng.site_propose(1, 2, 3, 5, 7) == KNOWN_PROPOSE
    # a step beyond the low counter word, a 64-bit seed
    assert mcrng.site_propose(0xDEADBEEFCAFEF00D, 2 ** 32 + 5, 9, 130, 300) == KNOWN_PROPOSE_HIGH
    w = mcrng.draw(1, 2, 3, mcrng.SITE_SELECT)
    assert mcrng.site_propose(1, 2, 3, 5, 7)[0] == min(int(math.floor(mcrng.uniform(w[0], w[1]) * 5)), 4)
    assert mcrng.site_propose(1, 2, 3, 5, 7)[1] == min(int(math.floor(mcrng.uniform(w[2], w[3]) * 7)), 6)
    assert mcrng.site_propose(1, 2, 3, 5, 7)[2] == mcrng.acceptance_draw(1, 2, 3)
    # m = 1 and n = 1 leave no choice
    assert mcrng.site_propose(4, 5, 6, 1, 1)[:2] == (0, 0)


KNOWN_BLOCK = (452563290, 3519468950, 1184276683, 1567020319)
KNOWN_PROPOSE = (0, 1, 0.23122102575920878)
KNOWN_PROPOSE_HIGH = (64, 193, 0.14835309028976562)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_row_sum_against_fsum(m):
    rng = np.random.default_rng(m)
    for scale in (1.0, 1e6):
        t = scale * (rng.random(m) - 0.5) * 10.0 ** rng.integers(-3, 4, m)
        got = mcrng.site_row_sum(t)
        assert abs(got - math.fsum(t)) <= (m + 6) * 2.0 ** -53 * math.fsum(np.abs(t))
    # the order is the device's: lanes first, then the butterfly
    t = rng.random(m)
    lanes = [0.0] * 64
    for j in range(m):
        lanes[j % 64] = lanes[j % 64] + float(t[j])
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
    assert mcrng.site_row_sum(t) == lanes[0]
    # +0.0 in the place of a term is the same as leaving it out
    skipped = [0.0] * 64
    for j in range(1, m):
        skipped[j % 64] = skipped[j % 64] + float(t[j])
    for o in (32, 16, 8, 4, 2, 1):
        skipped = [skipped[l] + skipped[l ^ o] for l in range(64)]
    assert mcrng.site_row_sum(np.concatenate([[0.0], t[1:]])) == skipped[0]
    assert mcrng.site_row_sum([]) == 0.0 and math.copysign(1.0, mcrng.site_row_sum([-0.0])) == 1.0


def _reference_loop(fw, it, population, energy, seed, first, stream, temperatures, m):
    """simulation.jl:943-966 transcribed literally (0-based), the old_i cache included, fed the draws of the Philox stream;
    movement_energy (sitehopping.jl:114-121) sums in the reference's order, molecule by molecule."""
    pop = [int(x) for x in population]
    n = len(fw)

    def movement_energy(i, si):
        inter = 0.0
        for j, sj in enumerate(pop):
            if i == j:
                continue
            inter += float(it[si, sj])
        return float(fw[si]) + inter

    old_i, accepted = -1, False
    before = after = movement_energy(0, pop[0])
    out, t = [], 0
    for T in temperatures:
        for _ in range(m):
            i, newpos, u = mcrng.site_propose(seed, first + t, stream, m, n)
            if old_i == i:
                if accepted:
                    before = after
                after = movement_energy(i, newpos)
            else:
                before, after = movement_energy(i, pop[i]), movement_energy(i, newpos)
            e = math.exp((before - after) / T) if (before - after) / T < 700 else math.inf
            accepted = after < before or u < e            # compute_accept_move, montecarlo.jl:702-712
            if accepted:
                energy += after - before
                pop[i] = newpos
            out.append((i, newpos, before, after, u, e, accepted))
            old_i = i
            t += 1
    return out, pop, energy


@pytest.mark.parametrize("case", SC.CASES, ids=str)
def test_replay_against_the_reference_loop(case):
    n, m, k = case
    fw, it = SC.tables(n)
    pops = SC.populations(n, m, k)
    eps = 2.0 ** -53
    for c, rp in enumerate(SC.host_replay(n, m, k)):
        e0 = float(mcrng.site_baseline(fw, it, pops[c]))
        T = [float(SC.temperatures(k)[c])] * SC.NCYCLES
        ref, ref_pop, ref_energy = _reference_loop(fw, it, pops[c], e0, SC.SEED, SC.first_step(m), int(SC.stream_ids(k)[c]), T, m)
        assert len(ref) == len(rp.steps) == SC.NCYCLES * m
        pop = [int(x) for x in pops[c]]
        bound = 0.0
        for (i, new, before, after, u, e, acc), st in zip(ref, rp.steps):
            assert (st.molecule, st.new_site, st.u) == (i, new, u)
            mag = lambda s: abs(float(fw[s])) + sum(abs(float(it[s, pop[j]])) for j in range(m) if j != i)
            bb, ba = 2 * (m + 6) * eps * mag(pop[i]), 2 * (m + 6) * eps * mag(new)
            assert abs(st.before - before) <= bb and abs(st.after - after) <= ba
            if abs(u - e) >= 1e-12 and abs(u - st.threshold) >= 1e-12:
                assert st.accepted == acc
            assert st.accepted == acc, "the two runs part at a near tie: pick another seed"
            if acc:
                pop[i] = new
                bound += bb + ba
        assert [int(x) for x in rp.population] == ref_pop == pop
        assert abs(rp.energy - ref_energy) <= bound + len(ref) * 2 * eps * max(abs(e0), abs(ref_energy))


def test_replay_follows_a_log_and_keeps_cycle_ends():
    n, m, k = 5, 2, 3
    fw, it = SC.tables(n)
    rp = SC.host_replay(n, m, k)[1]
    log = np.zeros(len(rp.steps), dtype=[("accepted", "<i4")])
    log["accepted"] = [not st.accepted for st in rp.steps]          # a log that decides the opposite is followed, too
    p = SC.populations(n, m, k)[1]
    forced = SC.replay_chain(n, m, k, 1, SC.NCYCLES, log=log)
    assert [st.accepted for st in forced.steps] == [bool(x) for x in log["accepted"]]
    assert rp.cycle_population.shape == (SC.NCYCLES, m) and rp.cycle_energy.shape == (SC.NCYCLES,)
    assert np.array_equal(rp.cycle_population[-1], rp.population) and rp.cycle_energy[-1] == rp.energy
    assert rp.accepted == sum(st.accepted for st in rp.steps)
    assert np.array_equal(SC.populations(n, m, k)[1], p)            # the start is not written


def test_baseline_is_the_definition():
    fw, it = SC.tables(70)
    pop = SC.populations(70, 63, 5)[2]
    want = math.fsum([1.5] + [fw[s] for s in pop] + [it[pop[i], pop[j]] for i in range(63) for j in range(i + 1, 63)])
    assert abs(float(mcrng.site_baseline(fw, it, pop, 1.5)) - want) <= 1e-12 * abs(want)
    assert float(mcrng.site_baseline(fw, it, pop[:1])) == fw[pop[0]]


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (5, 2), (70, 63), (70, 70), (300, 130), (65535, 40), (9, 0)])
def test_random_population_is_duplicate_free(n, m):
    for stream in (0, 1, 77):
        p = mcrng.site_random_population(SC.SEED, stream, n, m)
        assert p.dtype == np.uint16 and p.shape == (m,)
        assert len(set(p.tolist())) == m and all(0 <= int(x) < n for x in p)
    if m >= 2 and n >= 5:
        assert not np.array_equal(mcrng.site_random_population(SC.SEED, 0, n, m), mcrng.site_random_population(SC.SEED, 1, n, m))
    with pytest.raises(ValueError):
        mcrng.site_random_population(1, 0, 3, 4)


# ---- what tests/test_gpu_site_sweep.py claims about its cases, shown on the host replay
def test_the_gpu_cases_reach_what_they_claim():
    total = dict(accepted=0, rejected=0, occupied=0, own=0, occupied_accepted=0, own_rejected=0)
    for n, m, k in SC.CASES:
        first = SC.first_step(m)
        assert first < 2 ** 32 <= first + SC.NCYCLES * m - 1, "the counter crosses its low word inside the run"
        T = SC.temperatures(k)
        assert k == 1 or abs(T[-1] / T[0] - 100.0) < 1e-9
        case = dict.fromkeys(total, 0)
        for c, rp in enumerate(SC.host_replay(n, m, k)):
            assert SC.near_ties(rp.steps) == 0          # about 2e-12 per step: the replay alone stays within the cap of one
            cov = SC.coverage(rp.steps, SC.populations(n, m, k)[c])
            for key in case:
                case[key] += cov[key]
        assert case["occupied_accepted"] == 0 and case["own_rejected"] == 0      # by the rule itself, no special case
        if m >= 2:
            assert case["accepted"] and case["rejected"] and case["occupied"] and case["own"], (n, m, k, case)
        for key in total:
            total[key] += case[key]
    assert total["accepted"] and total["rejected"] and total["occupied"] and total["own"]


def test_the_recorder_cases_reach_what_they_claim():
    n, m, k = SC.MINIMUM_CASE
    ties = 0
    for c, rp in enumerate(SC.host_replay(n, m, k, SC.MINIMUM_NCYCLES)):
        e0 = float(mcrng.site_baseline(*SC.tables(n), SC.populations(n, m, k)[c]))
        ties += SC.minimum_ties(rp.cycle_energy, e0)
        mink, mine = mcrng.track_minimum(rp.cycle_energy.reshape(-1, 1), [e0], cycle0=0)
        assert mine[0] == min([e0] + list(rp.cycle_energy))
    assert ties >= 1, "a cycle end that ties with the minimum"
    n, m, k = SC.FRAMES_CASE
    due1 = mcrng.snapshot_cycles(0, SC.FRAMES_NCYCLES, SC.FRAMES_ORIGIN, 1)
    due3 = mcrng.snapshot_cycles(0, SC.FRAMES_NCYCLES, SC.FRAMES_ORIGIN, 3)
    assert due1 == [2, 3, 4, 5, 6] and due3 == [2, 5]
    reps = SC.host_replay(n, m, k, SC.FRAMES_NCYCLES)
    assert any(not np.array_equal(rp.cycle_population[2], rp.cycle_population[5]) for rp in reps), "the frames differ"
