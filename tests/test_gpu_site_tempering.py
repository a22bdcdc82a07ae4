"""Tempering ladders inside the site-hopping sweep (ceg_site_group_set_tempering, k_site_sweep_pt of csrc/ceg_site.hip) on synthetic
tables: every log record of every rung against the host restatement (mcrng.site_ladder_replay), bit for bit; a table of zeros against
the untempered sweep; a run cut three ways; the recorder by rung; the refusals; run_parallel_tempering.
tests/test_site_tempering_host.py shows on the CPU that the cases reach what is claimed of them here."""
import math

import numpy as np
import pytest

import site_cases as SC
import site_tempering_cases as TC
from ceg_hip import _abi, mcrng
from ceg_hip.sitehopping import DeviceSiteHoppingGroup, SiteHopping, run_parallel_tempering

pytestmark = pytest.mark.gpu


def _group(case, hip_lib, tempered=True, cdf=None):
    n, m, R, L = case
    fw, it = SC.tables(n)
    g = DeviceSiteHoppingGroup(fw, it, SC.populations(n, m, L * R))
    if tempered:
        g.set_tempering(R, pair_cdf=TC.pair_cdf(case) if cdf is None else cdf, ladder_stream=TC.ladder_streams(case))
    return g


def _run(g, case, nc, first=None, cycle0=0, log=True):
    n, m, R, L = case
    first = SC.first_step(m, nc) if first is None else first
    return g.sweep_cycles(nc, SC.SEED, first, temperature=TC.temperatures(case), cycle0=cycle0, stream_id=SC.stream_ids(L * R), log=log)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same_bytes(xs, ys):
    for x, y in zip(xs, ys):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("case", TC.CASES, ids=str)
def test_log_replays_bit_for_bit(case, hip_lib):
    n, m, R, L = case
    nc = TC.ncycles(case)
    T = TC.temperatures(case)
    with _group(case, hip_lib) as g:
        start = g.stats()
        att0, acc0, rep0 = g.tempering_read()
        assert not att0.any() and not acc0.any() and rep0.tolist() == list(range(R)) * L
        stats, recs, log = _run(g, case, nc)
        final = g.populations()
        att, acc, rep = g.tempering_read()
    assert log.shape == (nc * m, L * R) and recs.shape == (nc, L * R) and att.shape == (L, R - 1)
    exempt = 0
    kinds = dict(downhill=0, drawn=0, rejected=0)
    for l in range(L):
        rows = slice(l * R, (l + 1) * R)
        rp = TC.replay_ladder(case, l, start_energy=start["energy"][rows], log=log[:, rows])      # follows the logged decisions
        for r in range(R):
            c = l * R + r
            col = log[:, c]
            assert len(rp.steps[r]) == nc * m
            for t, st in enumerate(rp.steps[r]):
                rec = col[t]
                assert (int(rec["molecule"]), int(rec["old_site"]), int(rec["new_site"])) == (st.molecule, st.old_site, st.new_site), (c, t)
                assert _bits(rec["u"]) == _bits(st.u) and _bits(rec["before"]) == _bits(st.before) and _bits(rec["after"]) == _bits(st.after), (c, t)
                # the rule in NumPy on the logged values: a hop at the rung's temperature, an exchange at Tx of the pair
                if st.molecule >= 0:
                    with np.errstate(over="ignore"):
                        e = float(np.exp((rec["before"] - rec["after"]) / np.float64(T[c])))
                else:
                    a = c if st.molecule == -1 else c - 1
                    Tx = np.float64(1.0) / (np.float64(1.0) / np.float64(T[a]) - np.float64(1.0) / np.float64(T[a + 1]))
                    with np.errstate(over="ignore"):
                        e = float(np.exp((rec["before"] - rec["after"]) / Tx))
                    if st.molecule == -1:
                        down = bool(rec["after"] < rec["before"])
                        kinds["downhill" if down else ("drawn" if rec["accepted"] else "rejected")] += 1
                        # both rungs of the pair carry the same record but for the marker
                        other = log[t, c + 1]
                        assert int(other["molecule"]) == -2 and all(other[f] == rec[f] for f in ("old_site", "new_site", "accepted"))
                        assert all(_bits(other[f]) == _bits(rec[f]) for f in ("before", "after", "u"))
                if not rec["after"] < rec["before"] and abs(float(rec["u"]) - e) < 1e-12:
                    exempt += st.molecule != -2
                    continue
                assert bool(rec["accepted"]) == bool(rec["after"] < rec["before"] or rec["u"] < e), (c, t)
            # at the end: populations by rung exact, energy and delta the replay's bits, the hop counters equal
            assert np.array_equal(final[c], rp.population[r])
            assert _bits(stats["energy"][c]) == _bits(rp.energy[r]) and _bits(stats["delta"][c]) == _bits(rp.delta[r])
            assert (int(stats["attempted"][c]), int(stats["accepted"][c])) == (int(rp.attempted[r]), int(rp.accepted[r]))
            hops = np.cumsum(col["molecule"] >= 0)
            for j in range(nc):
                assert _bits(recs[j, c]["energy"]) == _bits(rp.cycle_energy[j, r]) and int(recs[j, c]["cycle"]) == j
                assert recs[j, c]["temperature"] == T[c] and int(recs[j, c]["attempted"]) == hops[(j + 1) * m - 1] and int(recs[j, c]["flags"]) == 0
            assert _bits(recs[-1, c]["delta"]) == _bits(rp.delta[r]) and int(recs[-1, c]["accepted"]) == int(rp.accepted[r])
        assert att[l].tolist() == rp.pt_attempted.tolist() and acc[l].tolist() == rp.pt_accepted.tolist()
        assert rep[rows].tolist() == rp.replica.tolist() and sorted(rep[rows].tolist()) == list(range(R))
    assert exempt <= 1
    assert kinds["downhill"] and kinds["drawn"] and kinds["rejected"], kinds
    assert (rep != np.tile(np.arange(R), L)).any()


def test_a_table_of_zeros_is_the_untempered_run(hip_lib):
    case = (200, 65, 5, 3)
    nc = TC.ncycles(case)
    with _group(case, hip_lib, tempered=False) as g:
        plain = _run(g, case, nc) + (g.populations(),)
    with _group(case, hip_lib, cdf=np.zeros(case[2] - 1)) as g:
        zeros = _run(g, case, nc) + (g.populations(),)
        att, acc, rep = g.tempering_read()
    _same_bytes(plain, zeros)
    assert not att.any() and not acc.any() and rep.tolist() == list(range(case[2])) * case[3]


def test_a_tempered_run_does_not_depend_on_how_it_is_cut(hip_lib, monkeypatch):
    case = (200, 65, 5, 3)
    n, m, R, L = case
    nc, first = 4, SC.first_step(m, 4)

    def whole(env=None):
        if env is not None:
            monkeypatch.setenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", env)
        else:
            monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
        with _group(case, hip_lib) as g:
            return _run(g, case, nc, first=first) + (g.populations(),) + g.tempering_read()

    one = whole()
    seven = whole("7")            # 65 steps per cycle: launches end inside cycles, and between two exchange steps that follow each other
    monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
    with _group(case, hip_lib) as g:
        a = _run(g, case, 1, first=first)
        b = _run(g, case, 3, first=first + m, cycle0=1)
        two = (b[0], np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), g.populations()) + g.tempering_read()
    # the launches of 7 steps do cut between two exchange steps
    ex = [(one[2][:, l * R:(l + 1) * R]["molecule"] < 0).any(axis=1) for l in range(L)]
    assert all(any(x[t - 1] and x[t] for t in range(7, nc * m, 7)) for x in ex)
    assert any(x[m - 1] and x[m] for x in ex)                # and so does the cut into two calls, in one ladder at least
    assert one[4].any() and one[5].any()
    for other in (seven, two):
        _same_bytes(one, other)


def test_recorder_under_tempering(hip_lib):
    case = (200, 65, 5, 3)
    n, m, R, L = case
    nc, origin, every = 7, 2, 1
    due = mcrng.snapshot_cycles(0, nc, origin, every)
    first = SC.first_step(m, nc)
    with _group(case, hip_lib) as g:
        e0 = g.stats()["energy"].copy()
        p0 = g.populations()
        g.set_recorder(every, origin=origin, capacity=len(due), track_min=True)
        _s, recs, log = _run(g, case, nc, first=first)
        fr, fp = g.recorder_read()
        mink, mine, best = g.recorder_minimum()
    assert fr.shape == (len(due), L * R) and fp.shape == (len(due), L * R, m)
    want_k, want_e = mcrng.track_minimum(recs["energy"], e0, cycle0=0)             # strict <: a tie keeps the earlier cycle
    assert np.array_equal(mink, want_k) and _bits(mine).tolist() == _bits(want_e).tolist()
    moved = 0
    for l in range(L):
        rows = slice(l * R, (l + 1) * R)
        rp = TC.replay_ladder(case, l, nc=nc, start_energy=e0[rows], log=log[:, rows], first=first)
        for r in range(R):
            c = l * R + r
            for f, cc in enumerate(due):
                assert int(fr[f, c]["cycle"]) == cc and _bits(fr[f, c]["energy"]) == _bits(rp.cycle_energy[cc, r])
                assert np.array_equal(fp[f, c], rp.cycle_population[cc, r])
            assert np.array_equal(best[c], p0[c] if mink[c] < 0 else rp.cycle_population[mink[c], r])
            assert [cc for cc in range(nc) if recs[cc, c]["flags"] & _abi.SITE_FRAME_TAKEN] == due
        # frames whose last step was an exchange of the rung: the population came from the partner's slot
        last = log[m - 1::m, rows]["molecule"] < 0
        moved += int(last[origin:].sum())
    assert moved >= 1


def test_refusals_leave_the_state_untouched(hip_lib):
    case = (70, 63, 3, 2)
    n, m, R, L = case
    nc = 2
    with _group(case, hip_lib, tempered=False) as g:
        with pytest.raises(_abi.CegError) as e:
            g.tempering_read()                                   # nothing installed
        assert e.value.code == -1
        plain = _run(g, case, nc) + (g.populations(),)
    with _group(case, hip_lib) as g:
        _run(g, case, 1)
        before = (g.stats().tobytes(), g.populations().tobytes()) + tuple(x.tobytes() for x in g.tempering_read())
        good = TC.pair_cdf(case)
        for rungs, cdf in ((4, mcrng.site_exchange_cdf(4, 0.3)),       # K % R != 0
                           (1, np.zeros(0)), (17, np.linspace(0.0, 0.5, 16)),
                           (R, good[::-1].copy()),                      # decreasing
                           (R, np.array([-0.1, 0.5])), (R, np.array([0.1, 1.5])), (R, np.array([0.1, math.nan])), (R, np.array([math.inf, math.inf]))):
            with pytest.raises(_abi.CegError) as e:
                g.set_tempering(rungs, pair_cdf=cdf)
            assert e.value.code == -1, (rungs, cdf)
        T = np.tile(TC.temperatures(case), (2, 1))
        for c, value in ((1, T[0, 0]), (2, T[0, 1] - 1.0), (R + 1, T[0, R] / 2)):       # equal to, and below, the rung under it
            Tbad = T.copy(); Tbad[1, c] = value
            with pytest.raises(_abi.CegError) as e:
                g.sweep_cycles(2, SC.SEED, 9, temperature=Tbad)
            assert e.value.code == -1
        assert (g.stats().tobytes(), g.populations().tobytes()) + tuple(x.tobytes() for x in g.tempering_read()) == before
        # a ladder's first rung may lie below the last rung of the ladder before it
        g.sweep_cycles(1, SC.SEED, 9, temperature=T[:1])
        assert g.tempering_read()[0].sum() > np.frombuffer(before[2], dtype=np.int64).sum()
        # set_populations resets the replica map, rebase leaves it; installing again zeroes the counters
        assert g.tempering_read()[2].tolist() != list(range(R)) * L
        g.rebase()
        assert g.tempering_read()[2].tolist() != list(range(R)) * L
        g.set_populations(SC.populations(n, m, L * R))
        assert g.tempering_read()[2].tolist() == list(range(R)) * L and g.tempering_read()[0].any()
        g.set_tempering(R, pair_cdf=good)
        assert not g.tempering_read()[0].any()
        g.set_tempering(None)
        with pytest.raises(_abi.CegError):
            g.tempering_read()
    # removing the tempering restores the untempered bytes
    with _group(case, hip_lib) as g:
        g.set_tempering(None)
        _same_bytes(plain, _run(g, case, nc) + (g.populations(),))


@pytest.mark.parametrize("case", TC.CASES[:2], ids=str)
def test_run_parallel_tempering(case, hip_lib):
    n, m, R, L = case
    fw, it = SC.tables(n)
    sh = SiteHopping(fw, it, SC.populations(n, m, 1)[0])
    Ts = TC.temperatures(case)[:R]
    nc, ninit, every = 6, 2, 2
    out = run_parallel_tempering(sh, Ts[::-1], nc, ninit, printevery=every, seed=SC.SEED, ladders=L, p=0.3)      # the drift check passed
    nprint = 1 + nc // every
    assert out.temperatures.tolist() == sorted(Ts.tolist())                        # sorted: rung order
    assert out.energies.shape == (nprint, L * R) and out.populations.shape == (nprint, L * R, m) and out.cycles.tolist() == [0, 2, 4, 6]
    assert out.pairs_attempted.shape == (L, R - 1) and out.pairs_accepted.shape == (L, R - 1) and out.replica.shape == (L * R,)
    assert np.array_equal(out.run.records["temperature"], np.tile(np.sort(Ts), (ninit + nc, L)))
    assert out.pairs_attempted.sum() > 0 and (out.pairs_accepted <= out.pairs_attempted).all()
    # hops + the exchange steps of the rung = the steps of the run
    assert (out.hops_attempted <= (ninit + nc) * m).all() and out.hops_attempted.sum() == L * R * (ninit + nc) * m - 2 * out.pairs_attempted.sum()
    for f in range(nprint):
        for c in range(L * R):
            want = mcrng.site_baseline(fw, it, out.populations[f, c])
            assert abs(np.longdouble(out.energies[f, c]) - want) <= 1e-9 * max(abs(want), 1.0)
    # every rung started from sh's population and baseline
    assert _bits(out.run.initial_energy).tolist() == [_bits(out.run.initial_energy[0]).tolist()] * (L * R)
    for l in range(L):
        assert sorted(out.replica[l * R:(l + 1) * R].tolist()) == list(range(R))
