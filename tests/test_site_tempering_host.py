"""Tempering of site-hopping ladders on the host (no device): mcrng.site_ladder_replay alone shows that every case of
tests/site_tempering_cases.py reaches what tests/test_gpu_site_tempering.py claims of it, and the small pieces of the rule
(the pair table, the draw, the structure's layout) are what include/ceg_hip.h states."""
import ctypes as C
import math

import numpy as np
import pytest

import site_cases as SC
import site_tempering_cases as TC
from ceg_hip import _abi, mcrng


@pytest.mark.parametrize("case", TC.CASES, ids=str)
def test_every_case_reaches_every_kind_of_exchange(case):
    n, m, R, L = case
    total = dict(downhill=0, drawn=0, rejected=0, consecutive=0, first=0, last=0, near_ties=0)
    pairs, moved = set(), 0
    for rp in TC.host_replay(case):
        cov = TC.coverage(rp, m)
        for key in total:
            total[key] += int(cov[key])
        pairs |= cov["pairs"]
        moved += int((rp.replica != np.arange(R)).sum())
        assert sorted(rp.replica.tolist()) == list(range(R))                     # a permutation inside the ladder
        # the rungs of a pair make no hop at an exchange step: hops + exchange records = steps, per rung
        for r in range(R):
            assert len(rp.steps[r]) == TC.ncycles(case) * m
            assert int(rp.attempted[r]) == sum(1 for st in rp.steps[r] if st.molecule >= 0)
        assert rp.pt_attempted.sum() == len(TC.exchanges(rp, m)) and (rp.pt_accepted <= rp.pt_attempted).all()
    assert total["downhill"] >= 1 and total["drawn"] >= 1 and total["rejected"] >= 1, total
    assert total["consecutive"] >= 2, total                    # an exchange step directly after another
    assert total["first"] + total["last"] >= 1, total          # on a cycle's first or last step
    assert moved >= 1                                          # a configuration ends on a rung other than its own
    assert total["near_ties"] <= 1
    if R == 16:
        assert pairs == set(range(R - 1))                      # every pair of the full workgroup is attempted
    assert pairs                                               # (and at p = 0.1 / 0.3 at least the lower ones)


def test_exchanges_fall_on_first_and_last_steps_of_cycles():
    first = sum(int(TC.coverage(rp, c[1])["first"]) for c in TC.CASES for rp in TC.host_replay(c))
    last = sum(int(TC.coverage(rp, c[1])["last"]) for c in TC.CASES for rp in TC.host_replay(c))
    assert first >= 1 and last >= 1


def test_configuration_quantities_travel_with_the_configuration():
    """energy - delta stays the baseline a configuration started from, whichever rung it ends on"""
    case = (200, 65, 5, 3)
    n, m, R, L = case
    fw, it = SC.tables(n)
    pops = SC.populations(n, m, L * R)
    for l, rp in enumerate(TC.host_replay(case)):
        for r in range(R):
            origin = l * R + int(rp.replica[r])
            e0 = float(mcrng.site_baseline(fw, it, pops[origin]))
            assert abs((rp.energy[r] - rp.delta[r]) - e0) <= 1e-9 * abs(e0)
            want = mcrng.site_baseline(fw, it, rp.population[r])
            assert abs(np.longdouble(rp.energy[r]) - want) <= 1e-9 * abs(want)


def test_a_table_of_zeros_is_the_untempered_replay():
    case = (70, 63, 3, 2)
    n, m, R, L = case
    rp = TC.replay_ladder(case, 1, cdf=np.zeros(R - 1))
    assert not rp.pt_attempted.any() and rp.replica.tolist() == list(range(R))
    for r in range(R):
        c = R + r
        one = mcrng.site_replay(*SC.tables(n), SC.populations(n, m, L * R)[c], float(mcrng.site_baseline(*SC.tables(n), SC.populations(n, m, L * R)[c])),
                                SC.SEED, SC.first_step(m, TC.ncycles(case)), int(SC.stream_ids(L * R)[c]), np.full(TC.ncycles(case), TC.temperatures(case)[c]), m)
        assert one.steps == rp.steps[r] and one.energy == rp.energy[r] and np.array_equal(one.population, rp.population[r])


def test_pair_table_against_its_closed_form():
    for R in (2, 3, 5, 16):
        cdf = mcrng.site_exchange_cdf(R, 0.1)
        assert cdf.shape == (R - 1,) and cdf.dtype == np.float64
        want = 1.0 - 0.9 ** np.arange(1, R, dtype=np.longdouble)
        assert np.abs(cdf - want).max() <= 1e-15
        assert (np.diff(cdf) > 0).all() and 0.0 < cdf[0] and cdf[-1] < 1.0
    assert mcrng.site_exchange_cdf(4, 0.0).tolist() == [0.0, 0.0, 0.0] and mcrng.site_exchange_cdf(4, 1.0).tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        mcrng.site_exchange_cdf(1)


def test_exchange_draw_and_threshold():
    assert mcrng.SITE_EXCHANGE == 12
    cdf = mcrng.site_exchange_cdf(4, 0.3)
    seen = set()
    for s in range(200):
        w = mcrng.draw(SC.SEED, s, 9, mcrng.SITE_EXCHANGE)
        v = mcrng.uniform(w[0], w[1])
        j, u = mcrng.site_exchange_draw(SC.SEED, s, 9, cdf)
        assert u == mcrng.uniform(w[2], w[3])
        assert j == next((i for i in range(3) if v < cdf[i]), -1)
        seen.add(j)
    assert seen == {-1, 0, 1, 2}
    assert mcrng.site_exchange_draw(SC.SEED, 3, 9, np.zeros(3))[0] == -1 and mcrng.site_exchange_draw(SC.SEED, 3, 9, np.ones(3))[0] == 0
    # Tx = 1 / (1 / T_a - 1 / T_b), then exp((E_a - E_b) / Tx), every operation rounded in this order
    E_a, E_b, T_a, T_b = -1234.5, -1200.25, 300.0, 377.9
    Tx = np.float64(1.0) / (np.float64(1.0) / np.float64(T_a) - np.float64(1.0) / np.float64(T_b))
    assert mcrng.site_exchange_threshold(E_a, E_b, T_a, T_b) == math.exp(float((np.float64(E_a) - np.float64(E_b)) / Tx))
    assert 0.0 < mcrng.site_exchange_threshold(E_a, E_b, T_a, T_b) < 1.0 < mcrng.site_exchange_threshold(E_b, E_a, T_a, T_b)


def test_structure_layout_and_prototypes():
    assert C.sizeof(_abi.SiteTempering) == 32
    assert [(f, getattr(_abi.SiteTempering, f).offset) for f, _t in _abi.SiteTempering._fields_] == [
        ("rungs", 0), ("_pad", 4), ("pair_cdf", 8), ("ladder_stream", 16), ("_reserved", 24)]
    assert len(_abi.PROTOTYPES["ceg_site_group_set_tempering"][1]) == 2 and len(_abi.PROTOTYPES["ceg_site_group_tempering_read"][1]) == 4
    assert _abi.SITE_MAX_RUNGS == 16
