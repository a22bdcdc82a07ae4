"""Sweeps of a chain group (ceg_mc_group_sweep): molecule, move, Metropolis decision and update of S steps of K chains on the
device.  The log of a sweep is checked record by record against ceg_hip.mcrng (the NumPy restatement of the proposal), against
the ORACLE's state of every chain (oracle/montecarlo.OracleMonteCarlo) and against the rule evaluated in NumPy; further: the rows
of the existing group path, determinism, the limits of the rule, the energy bookkeeping, small shapes and every refusal.
Run with `pytest -m gpu` on an MI355X."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi, mcrng
from test_gpu_consumers import _mc_setup
from test_gpu_mc_chains import _check, _displace

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def setup(hip_lib, tmp_path_factory):
    """the Na + 4 CO2 CIT-7 setup, built once for the module; the first chain owns the grid interpolators"""
    from ceg_hip.energy import DeviceMonteCarlo
    try:
        _M, mc = _mc_setup(tmp_path_factory.mktemp("mc_sweep"))
        owner = DeviceMonteCarlo(_copy(mc))
        yield mc, owner
        owner.close()
    finally:
        ceg.setdir_RASPA(Path(__file__).parent / "golden" / "raspa")


def _copy(mc, positions=None):
    out = copy.copy(mc)
    out.positions = [[np.array(p, dtype=np.float64) for p in kind] for kind in (mc.positions if positions is None else positions)]
    return out


def _chains(setup, k, positions=None, oracle=False):
    """k chains in the state of the setup (or in `positions`), sharing the owner's grids; with their oracles on request"""
    from ceg_hip.energy import DeviceMonteCarlo
    from oracle.montecarlo import OracleMonteCarlo
    mc, owner = setup
    devs = [DeviceMonteCarlo(_copy(mc, positions), grids_from=owner) for _ in range(k)]
    omcs = []
    for d in devs if oracle else []:
        omc = OracleMonteCarlo.from_setup(d.mc)
        omc.compute_ewald()
        omcs.append(omc)
    return devs, omcs


def _close(devs):
    for d in devs[::-1]:
        d.close()


def _device_order(dev):
    """device molecule index -> (kind, index in kind)"""
    order = {d: (i, j) for i, kind in enumerate(dev._slot) for j, d in enumerate(kind)}
    return [order[d] for d in sorted(order)]


def _rule(rows, u, T):
    """part 2 of the specification on two logged rows -> (accepted, exp((b - a) / T) or None where it is not needed)"""
    if rows[1][0] >= 1e90:
        return False, None
    b = ((rows[0][0] + rows[0][1]) + rows[0][2]) + rows[0][3]
    a = ((rows[1][0] + rows[1][1]) + rows[1][2]) + rows[1][3]
    if a < b:
        return True, None
    with np.errstate(under="ignore"):
        e = float(np.exp((b - a) / T))
    return u < e, e


def _same_state(a, b):
    pa, sa = a.state()
    pb, sb = b.state()
    return np.array_equal(pa, pb) and np.array_equal(sa, sb)


def _step_sizes(omc, beads, T):
    """(dmax, thetamax) from a short host-side run of mcrng + the oracle on a copy of one chain: the first candidate with which
    both move kinds are accepted and rejected at least once"""
    from oracle.montecarlo import OracleMonteCarlo
    for dmax, thetamax in ((0.5, 1.0), (1.0, 2.0), (0.25, 0.5), (2.0, 3.0)):
        o = copy.copy(omc)
        o.positions = [[p.copy() for p in kind] for kind in omc.positions]
        o.sums_re, o.sums_im = omc.sums_re.copy(), omc.sums_im.copy()
        order = [(i, j) for i, kind in enumerate(o.positions) for j in range(len(kind))]
        seen = set()
        for s in range(40):
            pr = mcrng.propose(SEED, s, 0, [o.positions[i][j] for i, j in order], dmax, thetamax, 0.5, beads)
            idx = order[pr.molecule]
            ok = mcrng.accept_rule(o.movement_energy(idx), o.movement_energy(idx, pr.positions), pr.u, T)
            seen.add((pr.kind, ok))
            if ok:
                o.update(idx, pr.positions)
        if len(seen) == 4:
            return dmax, thetamax
    raise AssertionError("no candidate step size gives acceptances and rejections of both move kinds")


def test_sweep_replay_against_the_oracle(setup):
    """8 chains in states of their own, 100 steps, p_rotation = 0.5, temperatures 100 ... 1000 K: every record against mcrng.propose
    (molecule, kind, u exactly; positions to 1e-12 A), both rows against the chain's oracle at the LOGGED placement, the accepted flag
    against the rule in NumPy on the logged rows and u (a record within 1e-12 of the threshold is exempt; at most 1 %), the oracle
    advanced by the logged accepted positions; at the end positions exactly and the structure factor to 1e-9."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 8, 100
    devs, omcs = _chains(setup, K, oracle=True)
    for c in range(K):                                           # distinct states before grouping
        rng = np.random.default_rng(500 + c)
        for s in range(6):
            kind = s % 2
            j = int(rng.integers(len(omcs[c].positions[kind])))
            new = _displace(rng, omcs[c].positions[kind][j], 1)[0]
            devs[c].accept((kind, j), new)
            omcs[c].update((kind, j), new)
    order = _device_order(devs[0])
    per_kind = mcrng.default_beads(devs[0].mc)
    beads = [per_kind[i] for i, _j in order]
    T = np.linspace(100.0, 1000.0, K)
    dmax, thetamax = _step_sizes(omcs[0], beads, 400.0)
    sid = np.arange(K, dtype=np.uint32) * 3 + 1
    first = 2 ** 32 - 50                                         # the step counter crosses its low word inside the run
    with DeviceMonteCarloGroup(devs) as group:
        stats, log = group.sweep(S, SEED, first, temperature=T, dmax=dmax, thetamax=thetamax, p_rotation=0.5, stream_id=sid, log=True)
    assert log.shape == (S, K)
    exempt, seen = 0, set()
    count = np.zeros((K, 5), dtype=np.int64)
    delta = np.zeros(K)
    for s in range(S):
        for c in range(K):
            rec, omc = log[s, c], omcs[c]
            pr = mcrng.propose(SEED, first + s, int(sid[c]), [omc.positions[i][j] for i, j in order], dmax, thetamax, 0.5, beads)
            assert (rec["molecule"], rec["kind"]) == (pr.molecule, pr.kind), (s, c)
            assert rec["u"] == pr.u, (s, c)
            idx = order[pr.molecule]
            m = len(omc.ffidx[idx[0]])
            placed = rec["positions"][:m].copy()
            assert np.abs(placed - pr.positions).max() <= 1e-12, (s, c, placed, pr.positions)
            assert not rec["positions"][m:].any()
            _check(rec["rows"][0], omc.movement_energy(idx), (s, c, "before"))
            _check(rec["rows"][1], omc.movement_energy(idx, placed), (s, c, "after"))
            ok, e = _rule(rec["rows"], rec["u"], T[c])
            if e is not None and abs(rec["u"] - e) < 1e-12:
                exempt += 1
            else:
                assert bool(rec["accepted"]) == ok, (s, c, rec)
            count[c, 2 * pr.kind] += 1
            count[c, 2 * pr.kind + 1] += rec["accepted"]
            count[c, 4] += rec["rows"][1][0] >= 1e90
            seen.add((pr.kind, bool(rec["accepted"])))
            if rec["accepted"]:
                delta[c] += rec["rows"][1].sum() - rec["rows"][0].sum()
                omc.update(idx, placed)
    assert exempt <= 0.01 * S * K, exempt
    assert len(seen) == 4, seen                                  # both move kinds accepted and rejected
    for c in range(K):
        st = stats[c]
        assert [st["translation_trials"], st["translation_accepted"], st["rotation_trials"], st["rotation_accepted"], st["blocked"]] == list(count[c]), c
        assert abs(st["delta"] - delta[c]) <= 1e-9 * max(1.0, np.abs(log["rows"][:, c]).clip(max=1e90).max()), c
        pos, sf = devs[c].state()
        assert np.array_equal(pos, omcs[c].flat_positions()), c
        osf = omcs[c].total_structure_factor()
        assert np.abs(sf - osf).max() <= 1e-9 * np.abs(osf).max(), c
    print(f"sweep replay: {K} chains x {S} steps, dmax {dmax} A, thetamax {thetamax} rad, exempt {exempt}, "
          f"accepted {int(count[:, 1].sum())} of {int(count[:, 0].sum())} translations, {int(count[:, 3].sum())} of {int(count[:, 2].sum())} rotations")
    _close(devs)


def test_sweep_rows_are_those_of_the_group_trial(setup):
    """20 logged records (4 chains x 5 single-step sweeps): ceg_mc_group_trial on a twin group at the logged placement gives the
    same two rows -- columns 0, 2, 3 bit for bit, column 1 to 1e-12 relative (the header's statement for the group rows).  After
    every step both groups are put into the state the sweep reached by ceg_mc_set_guests, so their structure factors are the same
    sums."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 4
    devs, _ = _chains(setup, K)
    twins, _ = _chains(setup, K)
    order = _device_order(devs[0])
    sizes = [len(devs[0].mc.ffidx[i]) for i, _j in order]
    records = 0
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(twins) as twin:
        for s in range(5):
            _stats, log = group.sweep(1, SEED + 1, s, temperature=500.0, dmax=0.6, thetamax=60.0, degrees=True, p_rotation=0.5, log=True)
            moves = []
            for c in range(K):
                rec = log[0, c]
                moves.append(("move", order[rec["molecule"]], rec["positions"][:sizes[rec["molecule"]]][None].copy()))
            rows = twin.trial(moves)
            for c in range(K):
                for col in (0, 2, 3):
                    assert np.array_equal(rows[c][:, col], log[0, c]["rows"][:, col]), (s, c, col, rows[c], log[0, c]["rows"])
                np.testing.assert_allclose(rows[c][:, 1], log[0, c]["rows"][:, 1], rtol=1e-12, atol=0.0)
                records += 1
            for c in range(K):                                   # both groups into the state the sweep reached
                pos, _sf = devs[c].state()
                split = np.split(pos, np.cumsum(sizes)[:-1])
                for d in (devs[c], twins[c]):
                    for (i, j), p in zip(order, split):
                        d.mc.positions[i][j] = p.copy()
                    d.refresh()
    assert records == 20
    _close(twins)
    _close(devs)


def test_sweep_is_deterministic(setup):
    """The same call from the same state twice: identical logs and states, bit for bit; 60 + 40 steps with first_step continued =
    100 steps; a chain's log depends on its stream id alone, not on K or its place in the group (a group of 1 against a group of 5)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 2, 100
    kw = dict(temperature=[250.0, 700.0], dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=[4, 9], log=True)
    a, _ = _chains(setup, K)
    b, _ = _chains(setup, K)
    c, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(a) as ga, DeviceMonteCarloGroup(b) as gb, DeviceMonteCarloGroup(c) as gc:
        sa, la = ga.sweep(S, SEED, 1000, **kw)
        sb, lb = gb.sweep(S, SEED, 1000, **kw)
        s1, l1 = gc.sweep(60, SEED, 1000, **kw)
        s2, l2 = gc.sweep(40, SEED, 1060, **kw)
        assert la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes()
        assert la.tobytes() == np.concatenate([l1, l2]).tobytes()
        for name in sa.dtype.names[:5]:
            assert np.array_equal(sa[name], s1[name] + s2[name]), name
        for x, y, z in zip(a, b, c):
            assert _same_state(x, y) and _same_state(x, z)
        assert la["accepted"].any() and not la["accepted"].all()
    _close(c); _close(b); _close(a)
    one, _ = _chains(setup, 1)
    five, _ = _chains(setup, 5)
    kw1 = dict(temperature=400.0, dmax=0.5, thetamax=1.0, p_rotation=0.5, log=True)
    with DeviceMonteCarloGroup(one) as g1, DeviceMonteCarloGroup(five) as g5:
        _s, lone = g1.sweep(40, SEED, 7, stream_id=[77], **kw1)
        _s, lfive = g5.sweep(40, SEED, 7, stream_id=[1, 2, 3, 77, 5], **kw1)
        assert lone[:, 0].tobytes() == lfive[:, 3].tobytes()
        assert lfive[:, 0].tobytes() != lfive[:, 3].tobytes()
        assert _same_state(one[0], five[3])
    _close(five); _close(one)


def test_sweep_limits_of_the_rule(setup):
    """T = 1e12 K: every trial that is not blocked is accepted.  T = 1e-9 K: no accepted move raises the chain's energy, and
    stats.delta <= 0."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 3, 60
    devs, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(devs) as group:
        stats, log = group.sweep(S, SEED + 2, 0, temperature=1e12, dmax=1.5, thetamax=3.0, p_rotation=0.5, log=True)
        blocked = log["rows"][:, :, 1, 0] >= 1e90
        assert np.array_equal(log["accepted"] != 0, ~blocked)
        for c in range(K):
            assert stats[c]["blocked"] == blocked[:, c].sum()
            assert stats[c]["translation_accepted"] + stats[c]["rotation_accepted"] == S - blocked[:, c].sum()
        stats, log = group.sweep(S, SEED + 2, S, temperature=1e-9, dmax=0.3, thetamax=0.5, p_rotation=0.5, log=True)
        acc = log["accepted"] != 0
        before, after = log["rows"][:, :, 0, :].sum(axis=2), log["rows"][:, :, 1, :].sum(axis=2)
        assert (after[acc] <= before[acc]).all()
        assert acc.any() and not acc.all()
        assert (stats["delta"] <= 0.0).all()
    _close(devs)


def test_sweep_energy_bookkeeping(setup):
    """baseline_energy() after - before = stats.delta within 1e-9 (|before| + |after|) + 1e-7 accepted (the per-row tolerance summed)"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S = 3, 60
    devs, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(devs) as group:
        # the setup's own state has blocked atoms (baseline 2e100, which no tolerance relative to it can test): a sweep of its own
        # first takes every chain to a state of finite energy
        group.sweep(300, SEED + 3, 0, temperature=300.0, dmax=1.0, thetamax=1.5, p_rotation=0.5)
        before = [float(d.baseline_energy()) for d in devs]
        assert all(abs(e) < 1e6 for e in before), before
        stats = group.sweep(S, SEED + 3, 300, temperature=[150.0, 300.0, 900.0], dmax=0.4, thetamax=0.8, p_rotation=0.5)
        after = [float(d.baseline_energy()) for d in devs]
    for c in range(K):
        accepted = int(stats[c]["translation_accepted"] + stats[c]["rotation_accepted"])
        assert accepted > 0
        err = abs((after[c] - before[c]) - stats[c]["delta"])
        print(f"chain {c}: baseline {before[c]:.6f} -> {after[c]:.6f}, delta {stats[c]['delta']:.6f}, accepted {accepted}, |difference| {err:.3e}")
        assert err <= 1e-9 * (abs(before[c]) + abs(after[c])) + 1e-7 * accepted, (c, before[c], after[c], stats[c])
    _close(devs)


def test_sweep_small_shapes(setup):
    """K = 1 with one step; nsteps = 0; an empty chain among three (idle: molecule and kind -1, nothing counted); a chain of Na alone
    (never rotates); log_out = NULL gives the statistics and the state of the call with a log."""
    from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup
    mc, owner = setup
    kw = dict(temperature=300.0, dmax=0.5, thetamax=1.0, p_rotation=0.5)
    one, omcs = _chains(setup, 1, oracle=True)
    with DeviceMonteCarloGroup(one) as g:
        p0, sf0 = one[0].state()
        stats, log = g.sweep(0, SEED, 0, log=True, **kw)
        assert log.shape == (0, 1) and stats.tobytes() == np.zeros(1, dtype=_abi.SWEEP_STATS_DTYPE).tobytes()
        stats = g.sweep(0, SEED, 0, **kw)
        assert not any(stats[0][n] for n in stats.dtype.names)
        p1, sf1 = one[0].state()
        assert np.array_equal(p0, p1) and np.array_equal(sf0, sf1)
        stats, log = g.sweep(1, SEED, 5, log=True, **kw)
        rec = log[0, 0]
        order = _device_order(one[0])
        idx = order[rec["molecule"]]
        _check(rec["rows"][0], omcs[0].movement_energy(idx), "before")
        _check(rec["rows"][1], omcs[0].movement_energy(idx, rec["positions"][:len(omcs[0].ffidx[idx[0]])]), "after")
        assert stats[0]["translation_trials"] + stats[0]["rotation_trials"] == 1
        assert bool(rec["accepted"]) == _rule(rec["rows"], rec["u"], 300.0)[0]
    _close(one)
    # [full, empty, Na alone]
    na_only = [[p.copy() for p in mc.positions[0]], []]
    devs = [DeviceMonteCarlo(_copy(mc), grids_from=owner), DeviceMonteCarlo(_copy(mc, [[], []]), grids_from=owner),
            DeviceMonteCarlo(_copy(mc, na_only), grids_from=owner)]
    twins = [DeviceMonteCarlo(_copy(mc), grids_from=owner), DeviceMonteCarlo(_copy(mc, [[], []]), grids_from=owner),
             DeviceMonteCarlo(_copy(mc, na_only), grids_from=owner)]
    S = 30
    with DeviceMonteCarloGroup(devs) as g, DeviceMonteCarloGroup(twins) as gt:
        stats, log = g.sweep(S, SEED + 4, 0, log=True, **{**kw, "p_rotation": 1.0})
        assert (log["molecule"][:, 1] == -1).all() and (log["kind"][:, 1] == -1).all() and not log["accepted"][:, 1].any()
        assert not log["rows"][:, 1].any() and not log["positions"][:, 1].any()
        assert [log["u"][s, 1] for s in range(S)] == [mcrng.acceptance_draw(SEED + 4, s, 1) for s in range(S)]
        assert not any(stats[1][n] for n in stats.dtype.names)
        assert (log["molecule"][:, 2] == 0).all() and (log["kind"][:, 2] == mcrng.TRANSLATION).all()
        assert stats[2]["translation_trials"] == S and stats[2]["rotation_trials"] == 0
        assert stats[0]["translation_trials"] + stats[0]["rotation_trials"] == S and stats[0]["rotation_trials"] > 0
        quiet = gt.sweep(S, SEED + 4, 0, **{**kw, "p_rotation": 1.0})                  # log_out = NULL
        assert quiet.tobytes() == stats.tobytes()
        for x, y in zip(devs, twins):
            assert _same_state(x, y)
        # the moved state serves the existing entry points: a group trial of every chain that has a molecule
        rows = g.trial([("move", (1, 0), np.empty((0, 3, 3))), None, ("move", (0, 0), np.empty((0, 1, 3)))])
        assert rows[0].shape == (1, 4) and rows[2].shape == (1, 4) and np.isfinite(rows[0]).all() and np.isfinite(rows[2]).all()
    _close(twins)
    _close(devs)


def test_sweep_refusals_leave_the_state_alone(setup, monkeypatch):
    """Every refusal of the header: CEG_ERR_INVALID for a temperature / dmax / thetamax that is not finite, a temperature <= 0, a
    negative dmax / thetamax, p_rotation outside [0, 1], a bead outside its molecule, nsteps < 0, duplicate stream ids, a missing
    argument; CEG_ERR_UNSUPPORTED for a member with neighbour cells; CEG_ERR_HIP for a member marked inconsistent.  The state is the
    same before and after, and a valid call follows."""
    from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup
    mc, owner = setup
    lib = owner._lib
    K = 2
    devs, _ = _chains(setup, K)
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0, p_rotation=0.5)
    nan, inf = float("nan"), float("inf")
    bad = [dict(temperature=[300.0, nan]), dict(temperature=[inf, 300.0]), dict(temperature=[300.0, 0.0]), dict(temperature=-5.0),
           dict(dmax=[0.5, nan]), dict(dmax=inf), dict(dmax=[-0.1, 0.5]), dict(thetamax=nan), dict(thetamax=[1.0, inf]),
           dict(thetamax=-1.0), dict(p_rotation=[0.5, -0.01]), dict(p_rotation=1.01), dict(p_rotation=nan),
           dict(bead=[[0, 1], [0, 3]]), dict(bead=[[1, 1], [0, 1]]), dict(bead=[[0, -1], [0, 1]]), dict(stream_id=[6, 6])]
    with DeviceMonteCarloGroup(devs) as group:
        before = [d.state() for d in devs]

        def unchanged():
            for d, (p, sf) in zip(devs, before):
                p2, sf2 = d.state()
                assert np.array_equal(p, p2) and np.array_equal(sf, sf2)

        for change in bad:
            with pytest.raises(_abi.CegError) as ei:
                group.sweep(5, SEED, 0, **{**good, **change})
            assert ei.value.code == -1, change
            unchanged()
        with pytest.raises(_abi.CegError) as ei:
            group.sweep(-1, SEED, 0, **good)
        assert ei.value.code == -1
        stats = np.zeros(K, dtype=_abi.SWEEP_STATS_DTYPE)
        assert lib.ceg_mc_group_sweep(group._h, None, 5, stats.ctypes.data, None) == -1
        params = _abi.SweepParams(1, 0, None, None, None, None, None, None)
        assert lib.ceg_mc_group_sweep(group._h, C.addressof(params), 5, stats.ctypes.data, None) == -1
        unchanged()
        # a member marked inconsistent by a failed per-handle accept
        monkeypatch.setenv("CEG_HIP_MC_INJECT_FAILURE", "accept")
        with pytest.raises(_abi.CegError):
            devs[1].accept((0, 0), mc.positions[0][0] + 0.1)
        monkeypatch.delenv("CEG_HIP_MC_INJECT_FAILURE")
        with pytest.raises(_abi.CegError) as ei:
            group.sweep(5, SEED, 0, **good)
        assert ei.value.code == -3 and "chain 1" in str(ei.value)
        devs[1].refresh()
        unchanged()
        stats = group.sweep(5, SEED, 0, **good)                     # a valid call follows
        assert all(s["translation_trials"] + s["rotation_trials"] == 5 for s in stats)
    _close(devs)
    # a member that keeps its guests in neighbour cells
    monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
    cells = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    monkeypatch.delenv("CEG_HIP_MC_CELLS")
    assert cells.neighbour_cells() is not None
    plain = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    with DeviceMonteCarloGroup([plain, cells]) as group:
        before = [d.state() for d in (plain, cells)]
        with pytest.raises(_abi.CegError) as ei:
            group.sweep(5, SEED, 0, **good)
        assert ei.value.code == -5 and "chain 1" in str(ei.value)
        for d, (p, sf) in zip((plain, cells), before):
            p2, sf2 = d.state()
            assert np.array_equal(p, p2) and np.array_equal(sf, sf2)
    with DeviceMonteCarloGroup([plain]) as group:
        st = group.sweep(3, SEED, 0, **good)[0]
        assert st["translation_trials"] + st["rotation_trials"] == 3
    cells.close()
    plain.close()


def test_of_two_faults_the_first_is_reported(setup):
    """The order of the refusals: the cycles before the chains, then chain by chain, and within a chain temperature / dmax / thetamax,
    p_rotation, stream id, beads.  Each call carries two faults; the one that the order puts first is the one reported, and nothing
    is launched or changed."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 2
    devs, _ = _chains(setup, K)
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0, p_rotation=0.5)
    nan = float("nan")
    two = [(dict(p_rotation=[1.01, 0.5], temperature=[300.0, nan]), "chain 0: p_rotation"),
           (dict(temperature=[300.0, 0.0], stream_id=[6, 6]), "chain 1: the temperature"),
           (dict(bead=[[1, 1], [0, 1]], dmax=[0.5, -0.1]), "chain 0: a bead lies outside")]
    with DeviceMonteCarloGroup(devs) as group:
        before = [d.state() for d in devs]

        def refused(call, what):
            with pytest.raises(_abi.CegError) as ei:
                call()
            assert ei.value.code == -1 and what in str(ei.value), (what, str(ei.value))
            for d, (p, sf) in zip(devs, before):
                p2, sf2 = d.state()
                assert np.array_equal(p, p2) and np.array_equal(sf, sf2)

        for change, what in two:
            refused(lambda: group.sweep(5, SEED, 0, **{**good, **change}), what)
        # a cycle description that cycles_check refuses (cycle0 < 1) together with a dmax that is not finite
        refused(lambda: group.sweep_cycles(2, 3, SEED, 0, cycle0=0, **{**good, "dmax": [nan, 0.5]}), "cycles: ncycles >= 0")
    _close(devs)
