"""Replica exchange at the cycle ends of ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles (ceg_mc_group_set_tempering, kernel
k_mcg_exchange).  The yardstick is the same entry point driven ONE CYCLE PER CALL on identical fresh chains WITHOUT tempering, the host
applying ceg_hip.mcrng.exchange_round (held to hand-computed values by tests/test_mc_tempering_host.py) and checking mcrng.adapt_*
between the calls: logs, statistics, cycle records, exchange records, rungs, energies and final states must be EQUAL, byte for byte;
only `threshold`, the device library's exp, may differ from the host's, by 4 ulp at the most.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_cycles import COUNTERS, DISPLACEMENTS, _adapted, _chains
from test_gpu_mc_sweep import SEED, _close, _copy, _device_order, setup  # noqa: F401  (setup: the CIT-7 fixture of the chains with cells)
from test_gpu_mc_sampler import SWAP_HEAVY, _kinds, _replayed_frames, _start, _state_bytes, cha  # noqa: F401  (cha: 6 CO2 in CHA + Na, grid step 0.3)

pytestmark = pytest.mark.gpu

K, L, NC = 5, 6, 24         # (24 cycles: the run then holds 18 / 8 / 22 attempts of the three sorts test_decisions asks for; 12 cycles held 11 / 1 / 12)
LADDER = np.array([200.0, 260.0, 340.0, 450.0, 600.0])
RAMP = LADDER[None, :] * np.linspace(1.0, 1.25, NC)[:, None]           # [NC, K]: every row non-decreasing in the rung
SID = np.array([3, 10, 17, 24, 31], dtype=np.uint32)
STEP_SIZES = dict(dmax=[0.5, 0.8, 1.0, 1.3, 2.0], thetamax=[0.5, 0.7, 1.0, 1.5, 2.0])
ULP = 2.0 ** -52
_CACHE = {}


def _energies(group):
    return np.array([float(r) for r in group.baseline_energies()])


def _rows(ladder, a, b):
    ladder = np.asarray(ladder, dtype=np.float64)
    return ladder[a:b] if ladder.ndim == 2 else ladder


def _row(ladder, j, n):
    ladder = np.asarray(ladder, dtype=np.float64)
    return ladder[min(j, n - 1)] if ladder.ndim == 2 else ladder


def _tempered(make, ladder, *, gcmc=False, ncycles=NC, steps=L, seed, first=5, every=1, dmax, thetamax, adapt=3, cycle0=1, rungs=None, parts=None,
              prepare=None, sampler=None, **kw):
    """The run under test: tempering installed, the cycles in one call (or in the calls `parts`, continued as the header says).
    -> dict of everything the run returned and left"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = make()
    k = len(devs)
    out = {}
    with DeviceMonteCarloGroup(devs) as group:
        if prepare is not None:
            prepare(group)
        if sampler is not None:
            group.set_sampler(**sampler)
        out["starts"] = [_start(d) for d in devs]
        out["E0"] = _energies(group)
        group.set_tempering(every, out["E0"], rungs, capacity=ncycles)
        call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
        extra = dict(positions=False) if gcmc else {}
        dm, th, prior, done = dmax, thetamax, None, 0
        stats, cycs, logs = [], [], []
        for n in parts or [ncycles]:
            s, c, l = call(n, steps, seed, first + done * steps, temperature=_rows(ladder, done, done + n), dmax=dm, thetamax=th, adapt=adapt,
                           cycle0=cycle0 + done, prior=prior, log=True, **extra, **kw)
            stats.append(s); cycs.append(c); logs.append(l)
            dm, th, prior = c[-1]["dmax_next"], c[-1]["thetamax_next"], np.stack([c[-1][n_] for n_ in COUNTERS], axis=1)
            done += n
        out["rung"], out["energy"], out["pairs"], out["xrec"] = group.tempering_read()
        out.update(stats=stats, cyc=np.concatenate(cycs), log=np.concatenate(logs), state=[_state_bytes(d) for d in devs], slot=[d._slot for d in devs])
        if sampler is not None:
            out["sampled"] = group.sampler_read()
            out["sampler"] = group.sampler
    _close(devs)
    assert out["xrec"].shape == (ncycles, k)
    return out


def _moved(rec):
    """after - before of an accepted displacement, in the device's order (displacement_decision)"""
    rows = rec["rows"]
    b = ((rows[0][0] + rows[0][1]) + rows[0][2]) + rows[0][3]
    a = ((rows[1][0] + rows[1][1]) + rows[1][2]) + rows[1][3]
    return a - b


def _yardstick(make, ladder, *, gcmc=False, ncycles=NC, steps=L, seed, first=5, every=1, dmax, thetamax, adapt=3, cycle0=1, rungs=None, stop=None,
               prepare=None, stream_id=None, tempered_off=False, **kw):
    """One cycle per call without tempering, mcrng.exchange_round on the host in between (tempered_off: no exchange at all, every chain
    stays on its rung).  -> what _tempered must have returned"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = make()
    k = len(devs)
    sid = np.arange(k, dtype=np.uint32) if stream_id is None else np.asarray(stream_id, dtype=np.uint32)
    with DeviceMonteCarloGroup(devs) as group:
        if prepare is not None:
            prepare(group)
        E0 = _energies(group)
        rung = np.arange(k, dtype=np.int32) if rungs is None else np.array(rungs, dtype=np.int32)
        dm, th = (np.broadcast_to(np.asarray(x, dtype=np.float64), (k,)).copy() for x in (dmax, thetamax))
        total = np.zeros((k, 4), dtype=np.int64)
        running = np.zeros(k)
        call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
        extra = dict(positions=False) if gcmc else {}
        logs, cycs, xrecs, calls = [], [], [], []
        E = E0.copy()
        for j in range(ncycles):
            row, nxt = _row(ladder, j, ncycles), _row(ladder, j + 1, ncycles)
            s, c, l = call(1, steps, seed, first + j * steps, temperature=row[rung], dmax=dm, thetamax=th, adapt=adapt, cycle0=cycle0 + j, prior=total,
                           log=True, stream_id=sid, **extra, **kw)
            last = first + (j + 1) * steps - 1
            stopped = [stop is not None and last >= int(stop[q]) for q in range(k)]
            for q in range(k):                   # the energy sum runs on through the cycles of the one call: accumulate it in step order
                for rec in l[:, q]:
                    if rec["accepted"]:
                        running[q] += _moved(rec)
                total[q] = [c[0, q][n] for n in COUNTERS]
                if not stopped[q]:               # the device's adaptation of this one-cycle call against the host's restatement
                    want = _adapted(dm[q], th[q], total[q], int(c[0, q]["nmol"]), cycle0 + j, adapt)
                    assert want == (c[0, q]["dmax_next"], c[0, q]["thetamax_next"]), (j, q)
            E = (E0 + running) + 0.0 if gcmc else E0 + running
            if tempered_off:
                new, xr = rung.copy(), None
            else:
                new, xr = mcrng.exchange_round(rung, E, row, stopped, seed, last, sid, cycle0 + j, every, nxt)
            expect = c[0].copy()
            expect["delta_moves"] = running
            logs.append(l); cycs.append(expect); xrecs.append(xr); calls.append(s)
            dm, th, rung = c[0]["dmax_next"].copy(), c[0]["thetamax_next"].copy(), new
        out = dict(E0=E0, rung=rung, energy=E, xrec=None if tempered_off else np.stack(xrecs), cyc=np.stack(cycs), log=np.concatenate(logs), calls=calls,
                   running=running.copy(), state=[_state_bytes(d) for d in devs], slot=[d._slot for d in devs])
    _close(devs)
    return out


def _same_but_threshold(got, want, what):
    """exchange records: every field equal in its bytes, `threshold` to 4 ulp; -> the worst threshold deviation in ulp"""
    assert got.shape == want.shape, what
    for name in got.dtype.names:
        if name != "threshold":
            assert got[name].tobytes() == want[name].tobytes(), (what, name, got[name], want[name])
    g, w = got["threshold"], want["threshold"]
    same = (g == w) | (np.isnan(g) & np.isnan(w))
    with np.errstate(invalid="ignore"):          # (inf - inf where both are inf: `same`)
        dev = np.where(same, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300)) / ULP
    print(f"{what}: worst threshold deviation {dev.max():.2f} ulp over {(got['accepted'] >= 0).sum() // 2} attempts")
    assert dev.max() <= 4.0, (what, dev.max())
    return float(dev.max())


def _hold(got, want, what, gcmc=False):
    """everything of the tempered run against the yardstick"""
    assert got["E0"].tobytes() == want["E0"].tobytes(), what
    assert got["log"].shape == want["log"].shape and got["log"].tobytes() == want["log"].tobytes(), what
    for name in got["cyc"].dtype.names:
        assert got["cyc"][name].tobytes() == want["cyc"][name].tobytes(), (what, name, got["cyc"][name], want["cyc"][name])
    if want["xrec"] is not None:
        _same_but_threshold(got["xrec"], want["xrec"], what)
        pairs = np.zeros_like(got["pairs"])
        for j in range(len(got["xrec"])):        # attempted and accepted per rung pair, counted at the pair's lower rung
            for rec in got["xrec"][j]:
                lower = rec["accepted"] >= 0 and got["xrec"][j][rec["partner"]]["rung"] == rec["rung"] + 1
                if lower:
                    pairs[rec["rung"]] += (1, rec["accepted"])
        assert np.array_equal(got["pairs"], pairs) and not got["pairs"][-1].any(), (what, got["pairs"], pairs)
    assert np.array_equal(got["rung"], want["rung"]) and got["energy"].tobytes() == want["energy"].tobytes(), (what, got["rung"], want["rung"])
    assert got["state"] == want["state"] and got["slot"] == want["slot"], what
    # the statistics of the last (or only) call of the tempered run: counters summed over the yardstick's calls, the sum as accumulated
    if len(got["stats"]) == 1:
        stats, calls = got["stats"][0], want["calls"]
        names = ("trials", "accepted", "blocked", "capacity", "spent") if gcmc else COUNTERS + ("blocked",)
        for name in names:
            assert np.array_equal(stats[name], sum(c[name] for c in calls)), (what, name)
        assert stats["delta_moves" if gcmc else "delta"].tobytes() == want["running"].tobytes(), what
        if gcmc:
            assert not stats["delta_swaps"].any() and np.array_equal(stats["nmol"], calls[-1]["nmol"]) and np.array_equal(stats["count"], calls[-1]["count"])


def _cha_chains(cha, k=K):
    return lambda: _chains(cha, [None] * k)


def _main(cha):
    """the run every = 1 on the table ramp, and its yardstick, once for the module"""
    if "main" not in _CACHE:
        args = dict(seed=SEED + 1301, every=1, p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        _CACHE["main"] = (_tempered(_cha_chains(cha), RAMP, **args), _yardstick(_cha_chains(cha), RAMP, **args), args)
    return _CACHE["main"]


def test_every_cycle_on_a_table_ramp_equals_one_cycle_per_call(cha):
    """K = 5, 24 cycles of 6 steps, every = 1, a [24, 5] table whose rows rise by 25 % over the run"""
    got, want, _args = _main(cha)
    _hold(got, want, "every 1, ramp")
    x = got["xrec"]
    assert (x["rung"] != np.arange(K)[None, :]).any() and (x["accepted"] >= 0).sum() > 0
    assert np.array_equal(x["rung"][1:], x["rung_next"][:-1]) and np.array_equal(x["rung"][0], np.arange(K))
    for j in range(NC):                          # a chain runs at its rung's entry of the row; the record names the next row's
        assert np.array_equal(got["cyc"]["temperature"][j], RAMP[j][x["rung"][j]])
        assert np.array_equal(x["temperature_next"][j], RAMP[min(j + 1, NC - 1)][x["rung_next"][j]])
        assert sorted(x["rung_next"][j]) == list(range(K))
    assert np.array_equal(x["energy"], got["E0"][None, :] + got["cyc"]["delta_moves"])


def test_every_third_cycle_without_a_table(cha):
    """every = 3 from cycle0 = 2 without a table: rounds at cc = 3, 6, ..., 24 with alternating parity; no attempt in the other cycles"""
    args = dict(seed=SEED + 1302, every=3, cycle0=2, p_rotation=0.5, stream_id=SID, **STEP_SIZES)
    got = _tempered(_cha_chains(cha), LADDER, **args)
    _hold(got, _yardstick(_cha_chains(cha), LADDER, **args), "every 3, no table")
    x = got["xrec"]
    for j in range(NC):
        pairs = mcrng.exchange_pairs(K, 2 + j, 3)
        assert ((x["accepted"][j] >= 0).sum() == 2 * len(pairs)), j
        assert sorted(r for r in x["rung"][j][x["accepted"][j] >= 0]) == sorted(r for p in pairs for r in p)
        assert np.array_equal(x["temperature_next"][j], LADDER[x["rung_next"][j]])
    assert (x["accepted"] >= 0).sum() == 2 * 2 * (NC // 3) and NC % 3 == 0


def test_decisions(cha):
    """Every record's `accepted` is the rule on the stored values and the host's decision; no draw lies within 4 ulp of a threshold;
    the run holds at least two attempts accepted with E_b < E_a, two accepted by the draw and two rejected."""
    got, want, _args = _main(cha)
    x, cyc = got["xrec"], got["cyc"]
    downhill = by_draw = rejected = 0
    for j in range(NC):
        for c in range(K):
            rec = x[j, c]
            if rec["accepted"] < 0 or x[j, rec["partner"]]["rung"] != rec["rung"] + 1:
                continue
            b = rec["partner"]
            Ea, Eb, u, e = float(rec["energy"]), float(x[j, b]["energy"]), float(rec["u"]), float(rec["threshold"])
            assert rec["accepted"] == int(Eb < Ea or u < e) == want["xrec"][j, c]["accepted"] == x[j, b]["accepted"], (j, c, rec)
            host = mcrng.exchange_threshold(Ea, Eb, float(cyc[j, c]["temperature"]), float(cyc[j, b]["temperature"]))
            assert abs(e - host) <= 4 * ULP * host and abs(u - e) > 4 * ULP * max(e, u), (j, c, u, e, host)
            w = mcrng.draw(_args["seed"], 5 + (j + 1) * L - 1, int(SID[c]), mcrng.EXCHANGE)
            assert u == mcrng.uniform(w[0], w[1]) and x[j, b]["partner"] == c and x[j, b]["u"] == u and x[j, b]["threshold"] == e
            downhill += int(Eb < Ea)
            by_draw += int(not Eb < Ea and u < e)
            rejected += int(not rec["accepted"])
    print(f"decisions: accepted with E_b < E_a {downhill}, accepted by the draw {by_draw}, rejected {rejected}")
    assert downhill >= 2 and by_draw >= 2 and rejected >= 2, (downhill, by_draw, rejected)


def test_a_run_continued_in_a_second_call(cha):
    """24 cycles in one call == 5 + 19 cycles: the rungs and energies persist on the device, the records run on.  Logs, states, rungs,
    partners, decisions, draws and pair counts are equal in every byte, without a table and with the ramp.  Two things cannot be, by
    the header's own definitions, and are held to what those definitions give instead:
      energy: a chain's energy is (energy at the call's start) + (the call's delta_moves); the second call starts from the ROUNDED sum
        of the first and its delta_moves starts at zero, so from cycle 5 on the same terms are added in another association.  Measured:
        1 ulp on one record of the run without a table.  Bound: one rounding of at most ulp/2 of the largest partial sum per step of
        the run in either association, NC * L * 2^-52 * max|E|.  (The cycle records' delta_moves differs likewise, as in
        test_gpu_mc_cycles.py.)  `threshold`, a function of the energies, follows them: 4 ulp of exp beside the energies' share.
      temperature_next of the first call's last cycle, with a table: that call cannot know the row that follows, so it is the ENDED
        cycle's row at the chain's next rung; the second call starts every chain at its rung's entry of its own first row, so every
        temperature a chain RUNS at is the one-call run's."""
    def same(two, one, what):
        assert two["log"].tobytes() == one["log"].tobytes() and two["state"] == one["state"], what
        assert np.array_equal(two["rung"], one["rung"]) and np.array_equal(two["pairs"], one["pairs"]), what
        for n in one["xrec"].dtype.names:
            if n not in ("energy", "threshold", "temperature_next"):
                assert two["xrec"][n].tobytes() == one["xrec"][n].tobytes(), (what, n)
        assert two["xrec"]["energy"][:5].tobytes() == one["xrec"]["energy"][:5].tobytes() and two["xrec"]["threshold"][:5].tobytes() == one["xrec"]["threshold"][:5].tobytes()
        bound = NC * L * ULP * float(np.abs(one["xrec"]["energy"]).max())
        worst = float(np.abs(two["xrec"]["energy"] - one["xrec"]["energy"]).max())
        print(f"{what}: energies of the split run within {worst:.3e} K of the one-call run's (bound {bound:.3e} K)")
        assert worst <= bound and float(np.abs(two["energy"] - one["energy"]).max()) <= bound, (what, worst, bound)
        # x = (E_a - E_b) / Tp moves by at most 2 bound / Tp with Tp >= the ladder's smallest 1 / (1 / T_r - 1 / T_{r+1}) = 866 K
        e1, e2 = one["xrec"]["threshold"], two["xrec"]["threshold"]
        finite = np.isfinite(e1) & (e1 > 0)
        assert np.array_equal(finite, np.isfinite(e2) & (e2 > 0)) and (np.abs(e2[finite] - e1[finite]) <= (4 * ULP + 2 * bound / 866.0) * e1[finite]).all(), what

    flat = dict(seed=SEED + 1312, every=1, p_rotation=0.5, stream_id=SID, **STEP_SIZES)
    one, two = _tempered(_cha_chains(cha), LADDER, **flat), _tempered(_cha_chains(cha), LADDER, parts=[5, NC - 5], **flat)
    same(two, one, "continued, no table")
    assert two["xrec"]["temperature_next"].tobytes() == one["xrec"]["temperature_next"].tobytes() and (one["xrec"]["accepted"] == 1).any()
    got, _want, args = _main(cha)
    two = _tempered(_cha_chains(cha), RAMP, parts=[5, NC - 5], **args)
    same(two, got, "continued, ramp")
    rest = np.arange(NC) != 4
    assert two["xrec"]["temperature_next"][rest].tobytes() == got["xrec"]["temperature_next"][rest].tobytes()
    assert np.array_equal(two["xrec"]["temperature_next"][4], RAMP[4][got["xrec"]["rung_next"][4]])
    for n in got["cyc"].dtype.names:
        if n != "delta_moves":                   # (a call's sum starts at zero: the second call's records hold its own)
            assert two["cyc"][n].tobytes() == got["cyc"][n].tobytes(), n
    assert two["cyc"]["delta_moves"][:5].tobytes() == got["cyc"]["delta_moves"][:5].tobytes()


def test_no_attempts_is_the_run_without_tempering(cha):
    """every beyond the last cycle counter, and K = 1: no attempt, and log, statistics, cycle records and states of the run without
    tempering, byte for byte.  K = 2 has attempts at even rounds only."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    for k, every in ((K, NC + 1), (1, 1)):
        args = dict(seed=SEED + 1303, ncycles=6, p_rotation=0.5, stream_id=SID[:k], dmax=STEP_SIZES["dmax"][:k], thetamax=STEP_SIZES["thetamax"][:k])
        got = _tempered(_cha_chains(cha, k), RAMP[:6, :k], every=every, **args)
        assert (got["xrec"]["accepted"] == -1).all() and (got["xrec"]["partner"] == -1).all() and not got["pairs"].any()
        assert np.array_equal(got["xrec"]["rung"], np.broadcast_to(np.arange(k), (6, k))) and np.array_equal(got["rung"], np.arange(k))
        devs = _chains(cha, [None] * k)
        with DeviceMonteCarloGroup(devs) as group:
            stats, cyc, log = group.sweep_cycles(6, L, args["seed"], 5, temperature=RAMP[:6, :k], dmax=args["dmax"], thetamax=args["thetamax"],
                                                 p_rotation=0.5, stream_id=SID[:k], log=True)
            state = [_state_bytes(d) for d in devs]
        _close(devs)
        assert log.tobytes() == got["log"].tobytes() and stats.tobytes() == got["stats"][0].tobytes() and cyc.tobytes() == got["cyc"].tobytes()
        assert state == got["state"], k
        assert got["energy"].tobytes() == (got["E0"] + stats["delta"]).tobytes()
    args = dict(seed=SEED + 1304, ncycles=6, p_rotation=0.5, stream_id=SID[:2], dmax=0.8, thetamax=1.0)
    got = _tempered(_cha_chains(cha, 2), LADDER[:2], every=1, **args)
    _hold(got, _yardstick(_cha_chains(cha, 2), LADDER[:2], every=1, **args), "K = 2")
    assert [(got["xrec"]["accepted"][j] >= 0).all() for j in range(6)] == [(1 + j) % 2 == 0 for j in range(6)]


def test_equal_temperatures(cha):
    """one temperature on all rungs: every attempt is accepted (e = 1), the rungs permute, and log and states are those of the run
    without tempering"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    flat = np.full(K, 400.0)
    args = dict(seed=SEED + 1305, ncycles=8, p_rotation=0.5, stream_id=SID, **STEP_SIZES)
    got = _tempered(_cha_chains(cha), flat, every=1, **args)
    x = got["xrec"]
    tried = x["accepted"] >= 0
    assert tried.sum() == 2 * sum(len(mcrng.exchange_pairs(K, 1 + j, 1)) for j in range(8)) and (x["accepted"][tried] == 1).all()
    assert (x["threshold"][tried] == 1.0).all() or (np.abs(x["threshold"][tried] - 1.0) <= 4 * ULP).all()
    assert sorted(got["rung"]) == list(range(K)) and not np.array_equal(got["rung"], np.arange(K))
    assert np.array_equal(got["pairs"][:, 0], got["pairs"][:, 1])
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        _s, _c, log = group.sweep_cycles(8, L, args["seed"], 5, temperature=flat, p_rotation=0.5, stream_id=SID, log=True, **STEP_SIZES)
        state = [_state_bytes(d) for d in devs]
    _close(devs)
    assert log.tobytes() == got["log"].tobytes() and state == got["state"]


def test_a_stopped_chain_is_in_no_pair(cha):
    """chain 2 (rung 2 at the start) stops in the middle of cycle 4 of the call: from that cycle end on it has partner = -1 in every
    record and keeps its rung, and the chains on the rungs beside it are not paired with each other across it"""
    stop = np.array([2 ** 62, 2 ** 62, 5 + 3 * L + 2, 2 ** 62, 2 ** 62], dtype=np.int64)
    plan = lambda group: group.set_chain_plan(stop_step=stop)
    args = dict(seed=SEED + 1306, every=1, p_rotation=0.5, stream_id=SID, prepare=plan, **STEP_SIZES)
    got = _tempered(_cha_chains(cha), LADDER, **args)
    _hold(got, _yardstick(_cha_chains(cha), LADDER, stop=stop, **args), "a stopped chain")
    x = got["xrec"]
    assert (x["partner"][:3, 2] >= 0).any(), "the chain took part before it stopped"
    held = int(x["rung"][3, 2])
    assert (x["partner"][3:, 2] == -1).all() and (x["accepted"][3:, 2] == -1).all() and (x["rung"][3:, 2] == held).all() and (x["rung_next"][3:, 2] == held).all()
    for j in range(3, NC):
        assert not (x["partner"][j] == 2).any()
        for c in range(K):
            if x["partner"][j, c] >= 0:
                assert abs(int(x["rung"][j, c]) - int(x["rung"][j, x["partner"][j, c]])) == 1, (j, c)
    assert (got["log"]["molecule"][3 * L + 2:, 2] == _abi.MC_STOPPED).all()


def test_gcmc_cycles_with_displacements_only(cha):
    """sweep_gcmc_cycles with a displacement-only MoveTable (random_reinsertion included) against the same yardstick; with a swap
    probability > 0 the call is refused and nothing changes"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        still = group.gcmc_species([DISPLACEMENTS], [3e4])
        swaps = group.gcmc_species([SWAP_HEAVY], [3e4])
        group.set_tempering(1, capacity=4)
        before = [_state_bytes(d) for d in devs], [a.tobytes() for a in group.tempering_read()]
        with pytest.raises(_abi.CegError) as e:
            group.sweep_gcmc_cycles(2, L, SEED, 0, temperature=np.full(K, 300.0), dmax=0.5, thetamax=1.0, species=swaps, max_molecules=16, stream_id=SID)
        assert e.value.code == -1 and "swap" in str(e.value)
        assert before == ([_state_bytes(d) for d in devs], [a.tobytes() for a in group.tempering_read()])
    _close(devs)
    args = dict(gcmc=True, ncycles=8, seed=SEED + 1307, every=1, species=still, max_molecules=16, stream_id=SID, **STEP_SIZES)
    got = _tempered(_cha_chains(cha), RAMP[:8], **args)
    _hold(got, _yardstick(_cha_chains(cha), RAMP[:8], **args), "gcmc, displacements only", gcmc=True)
    assert got["log"]["kind"].max() == 4 and (got["xrec"]["accepted"] >= 0).any() and (got["log"]["accepted"] != 0).any()


def test_a_chain_with_neighbour_cells(setup, monkeypatch):
    """the Na + 4 CO2 CIT-7 chains, one of the five with its guests in 4 A neighbour cells and device cells on"""
    from test_gpu_mc_sweep_cells import _make
    bins = (None, 4, None, None, None)
    make = lambda: _make(setup, monkeypatch, bins)
    cells = lambda group: group.device_cells()
    args = dict(ncycles=8, seed=SEED + 1308, every=1, p_rotation=0.5, stream_id=SID, prepare=cells, **STEP_SIZES)
    ladder = np.array([400.0, 500.0, 650.0, 800.0, 1000.0])
    got = _tempered(make, ladder, **args)
    _hold(got, _yardstick(make, ladder, **args), "a chain with cells")
    assert (got["xrec"]["partner"][:, 1] >= 0).any() and (got["log"]["accepted"][:, 1] != 0).any()


def test_sampler_maps_belong_to_rungs(cha):
    """one density map per RUNG (chain_map = 0..K-1) and a frame at every cycle end: the bins are mcrng.bin_positions over the replayed
    log with chain c routed into the map of the rung the exchange records name for that cycle; the series stays per chain"""
    mc = cha[0]
    kinds = _kinds(mc)
    first = 2 * L
    samp = dict(every=L, step=2.0, channels={kinds[0][0]: 0, kinds[0][1]: 1}, chain_map=np.arange(K), series_capacity=NC)
    got = _tempered(_cha_chains(cha), LADDER, seed=SEED + 1309, first=first, every=1, p_rotation=0.5, stream_id=SID, sampler=samp, **STEP_SIZES)
    bins, series, _total = got["sampled"]
    s, x = got["sampler"], got["xrec"]
    frames = mcrng.sampler_frames(first, NC * L, L)
    assert frames == [first + (j + 1) * L - 1 for j in range(NC)] and series.shape == (NC, K)
    states = _replayed_frames(got["starts"], got["log"], first, frames, None)
    na, nb, nc = s["dims"]
    want = np.zeros((K, s["nchannels"], nc, nb, na), dtype=np.int64)
    by_chain = np.zeros_like(want)
    for c in range(K):
        for f, (spec, mols) in enumerate(states[c]):
            for route, m in ((want, int(x[f, c]["rung"])), (by_chain, c)):
                for sp, p in zip(spec, mols):
                    for a, kind in enumerate(kinds[sp]):
                        ch = int(s["channels"][kind])
                        if ch >= 0:
                            mcrng.bin_positions(route[m, ch], s["unit_invmat"], p[a:a + 1], s["symmetries"])
    assert (x["rung"] != np.arange(K)[None, :]).any() and not np.array_equal(want, by_chain)
    assert np.array_equal(bins, want)
    assert bins.sum() == NC * K * 18
    for c in range(K):                           # the series records stay with the chain
        assert series[:, c]["delta_moves"].tobytes() == got["cyc"]["delta_moves"][:, c].tobytes() and (series[:, c]["nmol"] == 6).all()


def test_a_standalone_frame_is_binned_by_rung(cha):
    """ceg_mc_group_sample with a tempering state installed: chain c goes into the map of rungs[c]; without the state, into map c"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    kinds = _kinds(cha[0])
    shift = [[p + 0.37 * c for p in cha[0].positions[0]] for c in range(K)]          # every chain somewhere else
    devs = _chains(cha, [[s] for s in shift])
    rungs = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    out = {}
    with DeviceMonteCarloGroup(devs) as group:
        for mode in ("by rung", "by chain"):
            group.set_sampler(L, step=2.0, channels={kinds[0][0]: 0, kinds[0][1]: 1}, chain_map=np.arange(K), series_capacity=1)
            group.set_tempering(1 if mode == "by rung" else None, np.zeros(K), rungs, capacity=1)
            group.sample()
            out[mode] = group.sampler_read()[0]
        s = group.sampler
        starts = [_start(d) for d in devs]
    _close(devs)
    na, nb, nc = s["dims"]
    want = {mode: np.zeros((K, s["nchannels"], nc, nb, na), dtype=np.int64) for mode in out}
    for c, (spec, mols) in enumerate(starts):
        for sp, p in zip(spec, mols):
            for a, kind in enumerate(kinds[sp]):
                for mode, m in (("by rung", int(rungs[c])), ("by chain", c)):
                    mcrng.bin_positions(want[mode][m, int(s["channels"][kind])], s["unit_invmat"], p[a:a + 1], s["symmetries"])
    assert not np.array_equal(want["by rung"], want["by chain"])
    assert np.array_equal(out["by rung"], want["by rung"]) and np.array_equal(out["by chain"], want["by chain"])


def _raw_set(group, every, capacity, rung, energy):
    spec = _abi.McTempering(every, capacity, None if rung is None else rung.ctypes.data, None if energy is None else energy.ctypes.data)
    return group._lib.ceg_mc_group_set_tempering(group._h, C.addressof(spec))


def test_refusals_leave_everything_alone(cha):
    """every refusal of the header gives CEG_ERR_INVALID with rungs, energies, pair counts, records, chains and sampler untouched; a
    valid call follows"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = _chains(cha, [None] * K)
    run = dict(dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=SID)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(L, series_capacity=8)
        rungs0 = np.array([1, 0, 2, 4, 3], dtype=np.int32)
        group.set_tempering(2, rungs=rungs0, capacity=4)
        group.sweep_cycles(2, L, SEED + 1310, 0, temperature=LADDER, **run)

        def snapshot():
            return ([a.tobytes() for a in group.tempering_read()], [_state_bytes(d) for d in devs], len(group.sampler_read()[1]))

        before = snapshot()
        assert len(group.tempering_read()[3]) == 2 and before[2] == 2
        E = np.full(K, -1000.0)
        nan, inf = E.copy(), E.copy()
        nan[3], inf[0] = np.nan, np.inf
        twice, outside, negative = (np.arange(K, dtype=np.int32) for _ in range(3))
        twice[4], outside[2], negative[0] = 0, K, -1
        for name, a in {"every 0": (0, 4, None, E), "every < 0": (-2, 4, None, E), "capacity < 0": (1, -1, None, E), "a rung twice": (1, 4, twice, E),
                        "a rung beyond K - 1": (1, 4, outside, E), "a rung < 0": (1, 4, negative, E), "energy nan": (1, 4, None, nan),
                        "energy inf": (1, 4, None, inf), "no energy": (1, 4, None, None)}.items():
            assert _raw_set(group, *a) == -1 and b"tempering" in group._lib.ceg_last_error(), name
            assert snapshot() == before, name
        down = LADDER.copy()
        down[3] = 300.0
        table = np.broadcast_to(LADDER, (2, K)).copy()
        table[1, 1] = 100.0
        swaps = group.gcmc_species([SWAP_HEAVY], [3e4])
        for name, call in {"more cycles than record slots": lambda: group.sweep_cycles(3, L, SEED, 2 * L, temperature=LADDER, cycle0=3, **run),
                           "a decreasing ladder": lambda: group.sweep_cycles(2, L, SEED, 2 * L, temperature=down, cycle0=3, **run),
                           "a decreasing row": lambda: group.sweep_cycles(2, L, SEED, 2 * L, temperature=table, cycle0=3, **run),
                           "swaps": lambda: group.sweep_gcmc_cycles(2, L, SEED, 2 * L, temperature=LADDER, dmax=0.5, thetamax=1.0, species=swaps,
                                                                    max_molecules=16, stream_id=SID, cycle0=3)}.items():
            with pytest.raises(_abi.CegError) as e:
                call()
            assert e.value.code == -1 and "tempering" in str(e.value), name
            assert snapshot() == before, name
        # the plain sweeps ignore the state (and make its energies stale, which is the caller's to mend); a valid call follows
        stats, cyc = group.sweep_cycles(2, L, SEED + 1310, 2 * L, temperature=LADDER, cycle0=3, **run)
        rung, energy, pairs, rec = group.tempering_read()
        assert rec.shape == (4, K) and rec[:2].tobytes() == np.frombuffer(before[0][3], dtype=_abi.MC_EXCHANGE_RECORD_DTYPE).tobytes()
        assert np.array_equal(rec["rung"][0], rungs0) and (rec["accepted"][0] >= 0).sum() == 0 and (rec["accepted"][1] >= 0).sum() == 4
        assert len(group.sampler_read()[1]) == 4
        group.set_tempering(None)
        with pytest.raises(RuntimeError):
            group.tempering_read()
        assert group._lib.ceg_mc_group_tempering_read(group._h, None, None, None, None, None) == -1
    _close(devs)


def test_run_parallel_tempering(cha):
    """ninit = 2, ncycles = 8: the drift check passes at rtol 1e-9, every chain's final recorded energy matches the baseline of
    oracle/montecarlo.py on the final state at 1e-9, and the output is sorted by rung."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from oracle.montecarlo import OracleMonteCarlo
    from test_gpu_mc_baseline import _oracle_constants, _reference
    mc = cha[0]
    ninit, ncycles = 2, 8
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        run = group.run_parallel_tempering(LADDER, ncycles, ninit, every=1, seed=SEED + 1311, stream_id=SID)
        assert group.tempering is None
        finals = [d.state()[0].reshape(-1, 3, 3) for d in devs]
        actual = np.array([float(r) for r in run.baselines[2]])
    orders = [_device_order(d) for d in devs]
    _close(devs)
    n = ninit + ncycles
    assert run.exchanges.shape == run.cycles_by_rung.shape == run.exchanges_by_rung.shape == run.chain_of_rung.shape == (n, K)
    assert (run.exchanges_by_rung["rung"] == np.arange(K)[None, :]).all()
    assert np.array_equal(run.cycles_by_rung["temperature"], np.broadcast_to(LADDER, (n, K)))
    for j in range(n):
        for r in range(K):
            c = int(run.chain_of_rung[j, r])
            assert run.exchanges[j, c]["rung"] == r and run.exchanges_by_rung[j, r].tobytes() == run.exchanges[j, c].tobytes()
    assert np.array_equal(run.exchanges["rung"][ninit], run.exchanges["rung_next"][ninit - 1]), "the rungs carry over into the production cycles"
    assert np.array_equal(run.rungs, run.exchanges["rung_next"][-1]) and (run.exchanges["rung"] != np.arange(K)[None, :]).any()
    tried = run.pair_counts[:-1, 0] > 0
    assert tried.all() and np.array_equal(run.acceptance, run.pair_counts[:-1, 1] / run.pair_counts[:-1, 0]) and not run.pair_counts[-1].any()
    drift = np.abs(run.recorded - actual) / np.maximum(np.abs(run.recorded), np.abs(actual))
    print(f"run_parallel_tempering: recorded {run.recorded.tolist()}, device baseline {actual.tolist()}, relative deviation {drift.tolist()}, "
          f"acceptance {run.acceptance.tolist()}")
    assert (drift <= 1e-9).all()
    assert run.recorded.tobytes() == run.exchanges["energy"][-1].tobytes()
    for c in range(K):                           # the oracle's baseline_energy of the final state
        positions = [[None] * len(kind) for kind in mc.positions]
        for d, (i, j) in enumerate(orders[c]):
            positions[i][j] = finals[c][d]
        omc = OracleMonteCarlo.from_setup(_copy(mc, positions))
        omc.compute_ewald()
        v = _reference(omc)["value"]
        enc, static = _oracle_constants(omc)
        oracle = v["framework_vdw"] + v["framework_direct"] + v["inter"] + (2 * (v["recip_framework"] + enc) + v["recip_guests"] + static) + mc.tailcorrection
        dev = abs(run.recorded[c] - oracle) / max(abs(run.recorded[c]), abs(oracle))
        print(f"  chain {c}: recorded {run.recorded[c]!r}, oracle {oracle!r}, relative deviation {dev:.3e}")
        assert dev <= 1e-9, (c, run.recorded[c], oracle)
