"""Site hopping on the device (ceg_site_group_*, csrc/ceg_site.hip) on synthetic tables: every record of the sweep's log against the
host restatement (mcrng.site_replay), bit for bit; a run cut three ways; the recorder; baseline and rebase; the refusals.
tests/test_site_hopping_host.py shows on the CPU that the cases reach what is claimed of them here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import site_cases as SC
from ceg_hip import _abi, mcrng
from ceg_hip.sitehopping import DeviceSiteHoppingGroup

pytestmark = pytest.mark.gpu


def _group(n, m, k, hip_lib, **kw):
    fw, it = SC.tables(n)
    return DeviceSiteHoppingGroup(fw, it, SC.populations(n, m, k), **kw)


def _run(g, n, m, k, ncycles, first=None, cycle0=0, log=True):
    first = SC.first_step(m, ncycles) if first is None else first
    return g.sweep_cycles(ncycles, SC.SEED, first, temperature=SC.temperatures(k), cycle0=cycle0, stream_id=SC.stream_ids(k), log=log)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", SC.CASES, ids=str)
def test_log_replays_bit_for_bit(case, hip_lib):
    n, m, k = case
    fw, it = SC.tables(n)
    pops = SC.populations(n, m, k)
    total = dict(accepted=0, rejected=0, occupied=0, own=0, occupied_accepted=0, own_rejected=0)
    with _group(n, m, k, hip_lib) as g:
        start = g.stats()
        assert np.array_equal(g.populations(), pops) and not start["attempted"].any() and not start["delta"].any()
        stats, recs, log = _run(g, n, m, k, SC.NCYCLES)
        final = g.populations()
    assert log.shape == (SC.NCYCLES * m, k) and recs.shape == (SC.NCYCLES, k)
    exempt = 0
    for c in range(k):
        col = log[:, c]
        rp = SC.replay_chain(n, m, k, c, SC.NCYCLES, start_energy=start["energy"][c], log=col)      # follows the logged decisions
        T = float(SC.temperatures(k)[c])
        for t, st in enumerate(rp.steps):
            r = col[t]
            assert (int(r["molecule"]), int(r["old_site"]), int(r["new_site"])) == (st.molecule, st.old_site, st.new_site), (c, t)
            assert _bits(r["u"]) == _bits(st.u) and _bits(r["before"]) == _bits(st.before) and _bits(r["after"]) == _bits(st.after), (c, t)
            # the rule in NumPy on the logged values
            with np.errstate(over="ignore"):
                e = float(np.exp((r["before"] - r["after"]) / np.float64(T)))
            if not r["after"] < r["before"] and abs(float(r["u"]) - e) < 1e-12:
                exempt += 1
                continue
            assert bool(r["accepted"]) == bool(r["after"] < r["before"] or r["u"] < e), (c, t)
        cov = SC.coverage(rp.steps, pops[c])
        for key in total:
            total[key] += cov[key]
        # at the end: populations exact, the running energy the replay's bits, the counters equal
        assert np.array_equal(final[c], rp.population)
        assert _bits(stats["energy"][c]) == _bits(rp.energy) and _bits(stats["delta"][c]) == _bits(rp.delta)
        assert (int(stats["attempted"][c]), int(stats["accepted"][c])) == (SC.NCYCLES * m, rp.accepted)
        for j in range(SC.NCYCLES):
            assert _bits(recs[j, c]["energy"]) == _bits(rp.cycle_energy[j]) and int(recs[j, c]["cycle"]) == j
            assert recs[j, c]["temperature"] == T and int(recs[j, c]["attempted"]) == (j + 1) * m and int(recs[j, c]["flags"]) == 0
        assert int(recs[-1, c]["accepted"]) == rp.accepted
    assert exempt <= 1
    assert total["occupied_accepted"] == 0 and total["own_rejected"] == 0
    if m >= 2:       # the run contains acceptances and rejections, a hop onto an occupied site and one onto the own site
        assert total["accepted"] and total["rejected"] and total["occupied"] and total["own"], total


def test_a_run_does_not_depend_on_how_it_is_cut(hip_lib, monkeypatch):
    n, m, k = 200, 65, 5
    ncycles, first = 4, SC.first_step(m, 4)

    def whole(env=None):
        if env is not None:
            monkeypatch.setenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", env)
        else:
            monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
        with _group(n, m, k, hip_lib) as g:
            out = g.sweep_cycles(ncycles, SC.SEED, first, temperature=SC.temperatures(k), stream_id=SC.stream_ids(k), log=True)
            return out + (g.populations(),)

    one = whole()
    seven = whole("7")            # 65 steps per cycle: launches end inside cycles
    monkeypatch.delenv("CEG_HIP_SITE_STEPS_PER_LAUNCH", raising=False)
    with _group(n, m, k, hip_lib) as g:
        a = g.sweep_cycles(1, SC.SEED, first, temperature=SC.temperatures(k), stream_id=SC.stream_ids(k), log=True)
        b = g.sweep_cycles(3, SC.SEED, first + m, temperature=SC.temperatures(k), cycle0=1, stream_id=SC.stream_ids(k), log=True)
        two = (b[0], np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), g.populations())
    assert one[0]["accepted"].all() and (one[0]["accepted"] < one[0]["attempted"]).all()
    for other in (seven, two):
        for x, y in zip(one, other):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_recorder_frames(hip_lib):
    n, m, k = SC.FRAMES_CASE
    ncycles, origin = SC.FRAMES_NCYCLES, SC.FRAMES_ORIGIN
    for every in (1, 3):
        due = mcrng.snapshot_cycles(0, ncycles, origin, every)
        with _group(n, m, k, hip_lib) as g:
            e0 = g.stats()["energy"]
            g.set_recorder(every, origin=origin, capacity=len(due) + 2)
            # two calls: the frames of the second go behind those of the first
            _s, r1, l1 = _run(g, n, m, k, 3, first=SC.first_step(m, ncycles))
            _s, r2, l2 = _run(g, n, m, k, ncycles - 3, first=SC.first_step(m, ncycles) + 3 * m, cycle0=3)
            recs, log = np.concatenate([r1, r2]), np.concatenate([l1, l2])
            fr, fp = g.recorder_read()
            with pytest.raises(_abi.CegError):
                g.recorder_read(len(due), 1)
            with pytest.raises(_abi.CegError):
                g.recorder_minimum()              # no track_min
        assert fr.shape == (len(due), k) and fp.shape == (len(due), k, m)
        for c in range(k):
            rp = SC.replay_chain(n, m, k, c, ncycles, start_energy=e0[c], log=log[:, c], first=SC.first_step(m, ncycles))
            for f, cc in enumerate(due):
                assert int(fr[f, c]["cycle"]) == cc and _bits(fr[f, c]["energy"]) == _bits(rp.cycle_energy[cc])
                assert np.array_equal(fp[f, c], rp.cycle_population[cc])
            taken = [cc for cc in range(ncycles) if recs[cc, c]["flags"] & _abi.SITE_FRAME_TAKEN]
            assert taken == due and not (recs[:, c]["flags"] & _abi.SITE_FRAME_DROPPED).any()


def test_recorder_store_one_frame_too_small(hip_lib):
    n, m, k = SC.FRAMES_CASE
    ncycles, origin = SC.FRAMES_NCYCLES, SC.FRAMES_ORIGIN
    due = mcrng.snapshot_cycles(0, ncycles, origin, 1)
    with _group(n, m, k, hip_lib) as g:
        g.set_recorder(1, origin=origin, capacity=len(due))
        _s, full, _l = _run(g, n, m, k, ncycles, log=False)
        want_r, want_p = g.recorder_read()
    with _group(n, m, k, hip_lib) as g:
        g.set_recorder(1, origin=origin, capacity=len(due) - 1)
        _s, recs, _l = _run(g, n, m, k, ncycles, log=False)
        fr, fp = g.recorder_read()
        with pytest.raises(_abi.CegError):
            g.recorder_read(0, len(due))          # the dropped frame has no body to read
        pops = g.populations()
    assert fr.shape[0] == len(due) - 1
    assert fr.tobytes() == want_r[:-1].tobytes() and fp.tobytes() == want_p[:-1].tobytes()
    assert (recs[due[-1]]["flags"] == _abi.SITE_FRAME_DROPPED).all()              # every chain is flagged at that cycle
    assert (recs[due[:-1]]["flags"] == _abi.SITE_FRAME_TAKEN).all() and not recs[:origin]["flags"].any()
    # the run itself is the same bytes but for the flags
    a, b = full.copy(), recs.copy()
    a["flags"] = b["flags"] = 0
    assert a.tobytes() == b.tobytes() and np.array_equal(pops, want_p[-1])


@pytest.mark.parametrize("case,ncycles", [(SC.MINIMUM_CASE, SC.MINIMUM_NCYCLES), (SC.FRAMES_CASE, SC.FRAMES_NCYCLES)], ids=str)
def test_recorder_minimum(case, ncycles, hip_lib):
    n, m, k = case
    with _group(n, m, k, hip_lib) as g:
        e0 = g.stats()["energy"].copy()
        p0 = g.populations()
        g.set_recorder(0, track_min=True)             # the minimum only
        mink, mine, best = g.recorder_minimum()
        assert (mink == -1).all() and _bits(mine).tolist() == _bits(e0).tolist() and np.array_equal(best, p0)
        _s, recs, log = _run(g, n, m, k, ncycles)
        mink, mine, best = g.recorder_minimum()
        with pytest.raises(_abi.CegError):
            g.recorder_read(0, 1)                     # no frames were taken
    want_k, want_e = mcrng.track_minimum(recs["energy"], e0, cycle0=0)
    assert np.array_equal(mink, want_k) and _bits(mine).tolist() == _bits(want_e).tolist()
    ties = 0
    for c in range(k):
        rp = SC.replay_chain(n, m, k, c, ncycles, start_energy=e0[c], log=log[:, c])
        assert np.array_equal(best[c], p0[c] if mink[c] < 0 else rp.cycle_population[mink[c]])
        ties += SC.minimum_ties(recs["energy"][:, c], e0[c])
        new = [cc for cc in range(ncycles) if recs[cc, c]["flags"] & _abi.SITE_NEW_MINIMUM]
        assert (new[-1] if new else -1) == mink[c]
    if case == SC.MINIMUM_CASE:
        assert ties >= 1          # a tie with the minimum did occur, and the earlier cycle was kept (mink above)


def test_baseline_and_rebase(hip_lib):
    n, m, k = 300, 130, 9
    fw, it = SC.tables(n)
    tail = 12.5
    with _group(n, m, k, hip_lib, tailcorrection=tail) as g:
        b0 = g.baseline_energies()
        for c, p in enumerate(SC.populations(n, m, k)):
            want = mcrng.site_baseline(fw, it, p, tail)
            assert abs(np.longdouble(b0[c]) - want) <= 1e-9 * abs(want)
        assert _bits(g.stats()["energy"]).tolist() == _bits(b0).tolist()          # a group starts at its baseline
        stats, _r, _l = g.sweep_cycles(50, SC.SEED, 0, temperature=SC.temperatures(k), stream_id=SC.stream_ids(k))
        pops = g.populations()
        base = g.baseline_energies()
        assert stats["accepted"].all()
        for c in range(k):
            want = mcrng.site_baseline(fw, it, pops[c], tail)
            assert abs(np.longdouble(base[c]) - want) <= 1e-9 * abs(want)
            assert abs(stats["energy"][c] - base[c]) <= 1e-9 * abs(base[c])       # the drift check of the reference
        assert _bits(g.baseline_energies()).tolist() == _bits(base).tolist()      # repeatable
        g.rebase()
        after = g.stats()
        assert _bits(after["energy"]).tolist() == _bits(base).tolist()
        assert np.array_equal(after["attempted"], stats["attempted"]) and _bits(after["delta"]).tolist() == _bits(stats["delta"]).tolist()
        # set_populations validates, replaces and rebases
        g.set_populations(SC.populations(n, m, k)[::-1])
        assert np.array_equal(g.populations(), SC.populations(n, m, k)[::-1])
        assert _bits(g.stats()["energy"]).tolist() == _bits(b0[::-1]).tolist()


def test_tables_read_in_place_from_device_memory(hip_lib):
    import torch
    n, m, k = 70, 64, 4
    fw, it = SC.tables(n)
    with _group(n, m, k, hip_lib) as g:
        want = _run(g, n, m, k, 2) + (g.populations(),)
    dfw, dit = torch.from_numpy(fw).cuda(), torch.from_numpy(it).cuda()
    with DeviceSiteHoppingGroup(dfw, dit, SC.populations(n, m, k)) as g:
        got = _run(g, n, m, k, 2) + (g.populations(),)
    for x, y in zip(want, got):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(dit.cpu().numpy(), it) and np.array_equal(dfw.cpu().numpy(), fw)      # never written


def test_refusals_leave_the_state_untouched(hip_lib):
    n, m, k = 5, 2, 3
    fw, it = SC.tables(n)
    pops = SC.populations(n, m, k)

    def refused(code, *args, **kw):
        with pytest.raises(_abi.CegError) as e:
            DeviceSiteHoppingGroup(*args, **kw)
        assert e.value.code == code, e.value

    refused(-1, fw, it, np.zeros((k, 0), dtype=np.uint16))                 # m = 0
    refused(-1, fw, it, np.zeros((0, m), dtype=np.uint16))                 # K = 0
    bad = pops.copy(); bad[1, 1] = n
    refused(-1, fw, it, bad)                                               # a site >= n
    bad = pops.copy(); bad[2, 1] = bad[2, 0]
    refused(-1, fw, it, bad)                                               # a site twice within a chain
    refused(-1, fw, it, pops, tailcorrection=math.nan)
    same = np.stack([pops[0]] * k)                                         # the same site in different chains is fine
    DeviceSiteHoppingGroup(fw, it, same).close()
    # n > 65535: refused on n alone, before a table is read
    h, dummy = C.c_void_p(), np.zeros(4)
    rc = hip_lib.ceg_site_group_create(0, 65536, 1, 1, dummy.ctypes.data, dummy.ctypes.data, 0, np.zeros(1, dtype=np.uint16).ctypes.data, 0.0, C.byref(h))
    assert rc == -1 and not h.value and b"65535" in hip_lib.ceg_last_error()
    # the table limit
    os.environ["CEG_HIP_SITE_TABLE_LIMIT_MB"] = "1"
    try:
        big = 400                                                          # 400 * 400 * 8 bytes > 1 MiB
        refused(-5, np.zeros(big), np.zeros((big, big)), np.arange(2, dtype=np.uint16).reshape(1, 2))
    finally:
        del os.environ["CEG_HIP_SITE_TABLE_LIMIT_MB"]
    with DeviceSiteHoppingGroup(fw, it, pops) as g:
        g.sweep_cycles(2, SC.SEED, 5, temperature=SC.temperatures(k))
        before = (g.stats().tobytes(), g.populations().tobytes())
        T = np.tile(SC.temperatures(k), (2, 1))
        for value in (0.0, -1.0, math.nan, math.inf):
            Tbad = T.copy(); Tbad[1, 2] = value
            with pytest.raises(_abi.CegError) as e:
                g.sweep_cycles(2, SC.SEED, 9, temperature=Tbad)
            assert e.value.code == -1
        for kw in (dict(ncycles=-1), dict(ncycles=1, steps_per_cycle=0), dict(ncycles=1, first_step=2 ** 63 - 1), dict(ncycles=2, cycle0=2 ** 63 - 2)):
            with pytest.raises(_abi.CegError) as e:
                g.sweep_cycles(kw.pop("ncycles"), SC.SEED, kw.pop("first_step", 0), temperature=100.0, **kw)
            assert e.value.code == -1
        bad = pops.copy(); bad[0, 0] = bad[0, 1]
        with pytest.raises(_abi.CegError):
            g.set_populations(bad)
        with pytest.raises(_abi.CegError):
            g.set_recorder(-1)
        with pytest.raises(_abi.CegError):
            g.recorder_read()                                              # no recorder
        assert (g.stats().tobytes(), g.populations().tobytes()) == before
        # and the group still runs
        g.sweep_cycles(1, SC.SEED, 9, temperature=100.0)
        assert g.stats()["attempted"].tolist() == [3 * m] * k
