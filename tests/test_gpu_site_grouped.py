"""Grouped cycles of site hopping on the device (ceg_site_group_sweep_grouped, k_site_sweep_grouped) on the synthetic cases of
tests/site_grouped_cases.py: every hop, grouped and cycle record against the host restatement (mcrng.site_grouped_replay), bit for
bit; a run cut three ways; the recorder across rejected cycles; accepted cycles against the plain sweep; the two drivers; the
refusals.  tests/test_site_grouped_host.py shows on the CPU that the cases reach what is claimed of them here."""
import math

import numpy as np
import pytest

import site_cases as SC
import site_grouped_cases as GC
from ceg_hip import _abi, mcrng
from ceg_hip import sitehopping as SH
from ceg_hip.sitehopping import DeviceSiteHoppingGroup

pytestmark = pytest.mark.gpu


def _group(case):
    n, m, k = case
    fw, it = SC.tables(n)
    return DeviceSiteHoppingGroup(fw, it, SC.populations(n, m, k), tailcorrection=GC.TAIL)


def _run(g, case, G, restart, ncycles=None, done=0, log=True):
    """cycles [done, done + ncycles) of the case's run"""
    n, m, k = case
    ncycles = GC.ncycles(case) - done if ncycles is None else ncycles
    return g.sweep_grouped(ncycles, SC.SEED, GC.first_step(case, G) + done * G * m, temperature=GC.temperatures(case, restart), steps_per_cycle=G * m,
                           cycle0=done, stream_id=SC.stream_ids(k), restart=restart, log=log)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _rule(before, after, u, T):
    """-> (the rule's decision in NumPy on the logged values, whether it hangs on the last bits of exp)"""
    with np.errstate(over="ignore", invalid="ignore"):
        e = float(np.exp((np.float64(before) - np.float64(after)) / np.float64(T)))
    return bool(after < before or u < e), (not after < before) and abs(float(u) - e) < 1e-12


def _replay(case, G, restart, c, e0, log, grouped):
    """chain c by the restatement from the device's start energy, following the logged decisions"""
    return GC.replay_chain(case, G, restart, c, energy=e0, log=log[:, c], grouped=grouped[:, c])


@pytest.mark.parametrize("variant", GC.VARIANTS, ids=GC.variant_id)
def test_records_replay_bit_for_bit(variant, hip_lib):
    case, G, restart = variant
    n, m, k = case
    spc, ncycles = G * m, GC.ncycles(case)
    with _group(case) as g:
        start = g.stats()
        stats, recs, log, grouped = _run(g, case, G, restart)
        final = g.populations()
    assert log.shape == (ncycles * spc, k) and recs.shape == (ncycles, k) and grouped.shape == (ncycles, k)
    exempt = accepted = rejected = 0
    for c in range(k):
        rp = _replay(case, G, restart, c, start["energy"][c], log, grouped)
        T = float(GC.temperatures(case, restart)[c])
        for t, st in enumerate(rp.steps):
            r = log[t, c]
            assert (int(r["molecule"]), int(r["old_site"]), int(r["new_site"])) == (st.molecule, st.old_site, st.new_site), (c, t)
            assert _bits(r["u"]) == _bits(st.u) and _bits(r["before"]) == _bits(st.before) and _bits(r["after"]) == _bits(st.after), (c, t)
            ok, tie = _rule(r["before"], r["after"], r["u"], T)
            exempt += tie
            assert tie or bool(r["accepted"]) == ok, (c, t)
        acc = 0
        for cyc, cy in enumerate(rp.cycles):
            r = grouped[cyc, c]
            assert _bits(r["before"]) == _bits(cy.before) and _bits(r["restart_energy"]) == _bits(cy.restart_energy), (c, cyc)
            assert _bits(r["after"]) == _bits(cy.after) and _bits(r["u"]) == _bits(cy.u), (c, cyc)
            assert int(r["restarted"]) == int(restart) and int(r["hops_accepted"]) == cy.hops_accepted, (c, cyc)
            if cy.restart_population is not None:
                assert len(set(cy.restart_population.tolist())) == m
            ok, tie = _rule(r["before"], r["after"], r["u"], T)
            exempt += tie
            assert tie or bool(r["accepted"]) == ok, (c, cyc)
            acc += int(r["accepted"])
            q = recs[cyc, c]
            assert _bits(q["energy"]) == _bits(rp.cycle_energy[cyc]) and _bits(q["delta"]) == _bits(rp.cycle_delta[cyc]), (c, cyc)
            assert (int(q["cycle"]), int(q["attempted"]), int(q["accepted"])) == (cyc, cyc + 1, acc) and q["temperature"] == T
            assert int(q["flags"]) == (_abi.SITE_GROUP_ACCEPTED if r["accepted"] else 0) | (_abi.SITE_GROUP_RESTARTED if restart else 0)
            if not r["accepted"]:        # the restore: E0 and, in the next cycle's records, P0
                assert _bits(q["energy"]) == _bits(r["before"])
        accepted += acc
        rejected += ncycles - acc
        assert np.array_equal(final[c], rp.population)
        assert _bits(stats["energy"][c]) == _bits(rp.energy) and _bits(stats["delta"][c]) == _bits(rp.delta)
        assert (int(stats["attempted"][c]), int(stats["accepted"][c])) == (ncycles, acc) == (rp.attempted, rp.accepted)
        # energy - delta stays the baseline the chain began from
        assert abs((stats["energy"][c] - stats["delta"][c]) - start["energy"][c]) <= 1e-9 * max(abs(start["energy"][c]), 1.0)
    assert exempt <= 1
    assert accepted and (rejected or n == m)


@pytest.mark.parametrize("variant", GC.VARIANTS, ids=GC.variant_id)
def test_a_run_does_not_depend_on_how_it_is_cut(variant, hip_lib, monkeypatch):
    case, G, restart = variant
    ncycles = GC.ncycles(case)
    due = mcrng.snapshot_cycles(0, ncycles, GC.FRAME_ORIGIN, GC.FRAME_EVERY)

    def state(g, outs):
        return tuple(outs) + (g.populations(),) + g.recorder_read() + g.recorder_minimum()

    def whole(env):
        if env is not None:
            monkeypatch.setenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", env)
        else:
            monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
        with _group(case) as g:
            g.set_recorder(GC.FRAME_EVERY, origin=GC.FRAME_ORIGIN, capacity=len(due), track_min=True)
            return state(g, _run(g, case, G, restart))

    one = whole(None)
    seven = whole(str(GC.CUT))       # launches end inside cycles, rejected ones among them wherever a cycle has more than one step
    monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
    with _group(case) as g:
        g.set_recorder(GC.FRAME_EVERY, origin=GC.FRAME_ORIGIN, capacity=len(due), track_min=True)
        a = _run(g, case, G, restart, ncycles=5)
        b = _run(g, case, G, restart, done=5)
        two = state(g, (b[0],) + tuple(np.concatenate([x, y]) for x, y in zip(a[1:], b[1:])))
    acc = one[3]["accepted"]
    if "rejected_with_hops" in GC.required(case, G, restart):
        assert acc.any() and not acc.all() and one[3]["hops_accepted"][acc == 0].any()
    else:                            # n = m: the energy never moves, every cycle is accepted
        assert acc.all()
    for other in (seven, two):
        for x, y in zip(one, other):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("restart", (False, True), ids=("plain", "restart"))
def test_recorder_across_rejected_cycles(restart, hip_lib):
    case, G = (200, 65, 5), 1
    n, m, k = case
    ncycles = GC.ncycles(case)
    due = mcrng.snapshot_cycles(0, ncycles, GC.FRAME_ORIGIN, GC.FRAME_EVERY)
    with _group(case) as g:
        e0, p0 = g.stats()["energy"].copy(), g.populations()
        g.set_recorder(GC.FRAME_EVERY, origin=GC.FRAME_ORIGIN, capacity=len(due), track_min=True)
        _s, recs, log, grouped = _run(g, case, G, restart)
        fr, fp = g.recorder_read()
        mink, mine, best = g.recorder_minimum()
    assert fr.shape == (len(due), k)
    want_k, want_e = mcrng.track_minimum(recs["energy"], e0, cycle0=0)
    assert np.array_equal(mink, want_k) and _bits(mine).tolist() == _bits(want_e).tolist()
    rejected_frames = rejected_after_minimum = 0
    for c in range(k):
        rp = _replay(case, G, restart, c, e0[c], log, grouped)
        for f, cc in enumerate(due):
            assert int(fr[f, c]["cycle"]) == cc and _bits(fr[f, c]["energy"]) == _bits(rp.cycle_energy[cc])
            assert np.array_equal(fp[f, c], rp.cycle_population[cc])
            if not grouped[cc, c]["accepted"]:       # the frame holds the restored population and E0, not what the hops left
                rejected_frames += 1
                assert np.array_equal(fp[f, c], rp.cycle_population[cc - 1] if cc else p0[c])
                assert _bits(fr[f, c]["energy"]) == _bits(grouped[cc, c]["before"])
        assert np.array_equal(best[c], p0[c] if mink[c] < 0 else rp.cycle_population[mink[c]])
        new = [cc for cc in range(ncycles) if recs[cc, c]["flags"] & _abi.SITE_NEW_MINIMUM]
        assert (new[-1] if new else -1) == mink[c]
        assert all(grouped[cc, c]["accepted"] for cc in new)       # a rejected cycle ends on an energy the minimum has seen
        rejected_after_minimum += sum(1 for cc in range(ncycles) if new and cc > new[0] and not grouped[cc, c]["accepted"])
        taken = [cc for cc in range(ncycles) if recs[cc, c]["flags"] & _abi.SITE_FRAME_TAKEN]
        assert taken == due and not (recs[:, c]["flags"] & _abi.SITE_FRAME_DROPPED).any()
    assert rejected_frames and rejected_after_minimum


def test_recorder_store_one_frame_too_small(hip_lib):
    case, G, restart = (200, 65, 5), 1, True
    ncycles = GC.ncycles(case)
    due = mcrng.snapshot_cycles(0, ncycles, GC.FRAME_ORIGIN, GC.FRAME_EVERY)
    with _group(case) as g:
        g.set_recorder(GC.FRAME_EVERY, origin=GC.FRAME_ORIGIN, capacity=len(due))
        _s, full, _l, gfull = _run(g, case, G, restart, log=False)
        want_r, want_p = g.recorder_read()
    with _group(case) as g:
        g.set_recorder(GC.FRAME_EVERY, origin=GC.FRAME_ORIGIN, capacity=len(due) - 1)
        _s, recs, _l, grouped = _run(g, case, G, restart, log=False)
        fr, fp = g.recorder_read()
        with pytest.raises(_abi.CegError):
            g.recorder_read(0, len(due))          # the dropped frame has no body to read
    assert fr.shape[0] == len(due) - 1
    assert fr.tobytes() == want_r[:-1].tobytes() and fp.tobytes() == want_p[:-1].tobytes()
    assert (recs[due[-1]]["flags"] & _abi.SITE_FRAME_DROPPED).all() and not (recs[due[-1]]["flags"] & _abi.SITE_FRAME_TAKEN).any()
    assert (recs[due[:-1]]["flags"] & _abi.SITE_FRAME_TAKEN).all()
    a, b = full.copy(), recs.copy()
    a["flags"] = b["flags"] = 0
    assert a.tobytes() == b.tobytes() and gfull.tobytes() == grouped.tobytes()


def test_accepted_cycles_are_the_plain_sweep(hip_lib):
    case = (70, 64, 4)
    n, m, k = case
    ncycles, first, T = 6, SC.first_step(m, 6), 1e9       # every hop onto a free site and every cycle is accepted
    with _group(case) as g:
        ps, pr, plog = g.sweep_cycles(ncycles, SC.SEED, first, temperature=T, stream_id=SC.stream_ids(k), log=True)
        ppop = g.populations()
    with _group(case) as g:
        gs, gr, glog, grouped = g.sweep_grouped(ncycles, SC.SEED, first, temperature=T, stream_id=SC.stream_ids(k), restart=False, log=True)
        gpop = g.populations()
    assert grouped["accepted"].all() and (grouped["hops_accepted"] > 0).all()
    assert np.array_equal(ppop, gpop) and plog.tobytes() == glog.tobytes()
    assert pr["energy"].tobytes() == gr["energy"].tobytes() and ps["energy"].tobytes() == gs["energy"].tobytes()
    # delta: the sum of the hops' changes there, D0 + (E1 - E0) per cycle here; m + 1 roundings of values below |energy| + |delta|
    tol = (m + 1) * ncycles * 2.0 ** -53 * (np.abs(pr["energy"]).max() + np.abs(pr["delta"]).max())
    assert np.abs(pr["delta"] - gr["delta"]).max() <= tol
    assert (gs["attempted"] == ncycles).all() and (gs["accepted"] == ncycles).all() and (ps["attempted"] == ncycles * m).all()
    assert np.array_equal(grouped["hops_accepted"].sum(axis=0), ps["accepted"])


def test_run_montecarlo_with_group_cycles(hip_lib):
    case = (200, 65, 5)
    n, m, k = case
    fw, it = SC.tables(n)
    pops = SC.populations(n, m, k)
    ninit, ncycles, G, seed = 2, 6, 2, 77
    T = np.outer(np.array([3000.0] * ninit + [2000.0, 1500.0, 1000.0, 700.0, 500.0, 300.0]), np.linspace(1.0, 3.0, k))
    with _group(case) as g:
        run = SH.run_montecarlo(g, T, ncycles, ninit, printevery=2, seed=seed, track_min=True, groupcycles=G, restartgroupcycle=True)   # passes the drift check
        with pytest.raises(ValueError):
            SH.run_montecarlo(g, T, ncycles, ninit, restartgroupcycle=True)
        g.set_tempering(k)
        with pytest.raises(ValueError):
            SH.run_montecarlo(g, T, ncycles, ninit, groupcycles=G)
    assert run.cycles.tolist() == [0, 2, 4, 6] and run.grouped.shape == (ninit + ncycles, k) and run.grouped["restarted"].all()
    assert (run.stats["attempted"] == ninit + ncycles).all() and np.array_equal(run.stats["accepted"], run.grouped["accepted"].sum(axis=0))
    updates = 0
    for c in range(k):
        first = mcrng.site_grouped_replay(fw, it, pops[c], run.initial_energy[c], seed, 0, c, T[:ninit, c], G * m, restart=True, tailcorrection=GC.TAIL,
                                          grouped=run.grouped[:ninit, c])
        assert np.array_equal(run.populations[0, c], first.population)
        second = mcrng.site_grouped_replay(fw, it, first.population, run.energies[0, c], seed, ninit * G * m, c, T[ninit:, c], G * m, restart=True,
                                           tailcorrection=GC.TAIL, grouped=run.grouped[ninit:, c], delta=first.delta)
        assert run.records["energy"][ninit:, c].tobytes() == second.cycle_energy.tobytes()
        for f, idx in enumerate(run.cycles.tolist()[1:], start=1):
            assert np.array_equal(run.populations[f, c], second.cycle_population[idx - 1])
        mink, mine = mcrng.track_minimum(second.cycle_energy.reshape(-1, 1), [run.energies[0, c]], cycle0=1)
        assert int(run.minimum[0][c]) == max(int(mink[0]), 0) and _bits(run.minimum[1][c]) == _bits(mine[0])
        assert np.array_equal(run.minimum[2][c], run.populations[0, c] if mink[0] < 0 else second.cycle_population[mink[0] - 1])
        updates += mink[0] > 0
    assert updates


def test_run_random_quenching_with_group_cycles(hip_lib):
    n, m, N, seed = 70, 20, 4, 5
    fw, it = SC.tables(n)
    sh = SH.SiteHopping(fw, it, m, GC.TAIL, seed=seed)
    T = np.array([800.0, 500.0, 300.0, 200.0, 100.0, 50.0])
    for G, restart in ((1, False), (2, True)):
        q = SH.run_random_quenching(sh, N, T, len(T), seed=seed, groupcycles=G, restartgroupcycle=restart)       # passes the drift check
        assert q.run.grouped.shape == (len(T), N) and q.run.grouped["restarted"].all() == restart
        for c in range(N):
            assert np.array_equal(q.start[c], mcrng.site_random_population(seed, c, n, m))
            rp = mcrng.site_grouped_replay(fw, it, q.start[c], q.run.energies[0, c], seed, 0, c, T, G * m, restart=restart, tailcorrection=GC.TAIL,
                                           grouped=q.run.grouped[:, c])
            assert q.run.records["energy"][:, c].tobytes() == rp.cycle_energy.tobytes()
            mink, mine = mcrng.track_minimum(rp.cycle_energy.reshape(-1, 1), [q.run.energies[0, c]], cycle0=1)
            assert int(q.run.minimum[0][c]) == max(int(mink[0]), 0) and _bits(q.run.minimum[1][c]) == _bits(mine[0])
            assert np.array_equal(q.run.minimum[2][c], q.start[c] if mink[0] < 0 else rp.cycle_population[mink[0] - 1])
        assert (q.run.minimum[1] <= q.run.initial_energy).all()


def test_refusals_leave_the_state_untouched(hip_lib):
    case = (5, 2, 3)
    n, m, k = case
    with _group(case) as g:
        g.set_recorder(1, origin=0, capacity=8, track_min=True)
        _run(g, case, 1, True, ncycles=3)

        def state():
            return (g.stats().tobytes(), g.populations().tobytes()) + tuple(x.tobytes() for x in g.recorder_read() + g.recorder_minimum())

        before = state()
        kw = dict(temperature=GC.temperatures(case, True), stream_id=SC.stream_ids(k))
        with pytest.raises(_abi.CegError) as e:
            g.sweep_grouped(2, SC.SEED, 50, restart=2, **kw)
        assert e.value.code == -1
        with pytest.raises(_abi.CegError) as e:
            g.sweep_grouped(2, SC.SEED, 50, restart=-1, **kw)
        assert e.value.code == -1
        g.set_tempering(k)
        for restart in (0, 1):
            with pytest.raises(_abi.CegError) as e:
                g.sweep_grouped(2, SC.SEED, 50, restart=restart, temperature=np.array([100.0, 200.0, 300.0]))
            assert e.value.code == -5
        g.set_tempering(None)
        T = np.tile(GC.temperatures(case, True), (2, 1))
        for value in (0.0, -1.0, math.nan, math.inf):
            Tbad = T.copy(); Tbad[1, 2] = value
            with pytest.raises(_abi.CegError) as e:
                g.sweep_grouped(2, SC.SEED, 50, temperature=Tbad, restart=True)
            assert e.value.code == -1
        for a in (dict(ncycles=-1), dict(ncycles=1, steps_per_cycle=0), dict(ncycles=1, first_step=2 ** 63 - 1), dict(ncycles=2, cycle0=2 ** 63 - 2)):
            with pytest.raises(_abi.CegError) as e:
                g.sweep_grouped(a.pop("ncycles"), SC.SEED, a.pop("first_step", 0), temperature=100.0, restart=True, **a)
            assert e.value.code == -1
        assert state() == before
        # and the group still runs, grouped or not
        s, _r, _l, gr = g.sweep_grouped(1, SC.SEED, 50, temperature=100.0, restart=True)
        assert s["attempted"].tolist() == [4] * k and gr["restarted"].all()
        assert g.sweep_cycles(1, SC.SEED, 60, temperature=100.0)[0]["attempted"].tolist() == [4 + m] * k
