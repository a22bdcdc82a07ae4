"""Whole cycles of run_montecarlo! on the device (ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles, kernel k_mcg_cycle_end):
the temperature schedule and the adaptation of dmax / thetamax at every cycle end.  The yardstick is the existing sweep entry point
driven ONE CYCLE PER CALL on identical fresh chains, the parameters adapted between the calls with ceg_hip.mcrng.adapt_* (held to
hand-computed values by tests/test_mc_cycles_host.py): logs, statistics, cycle records and final states must be EQUAL, byte for byte.
The running energy sums, which the one-call run accumulates across the cycles, are recomputed from the log in the device's operation
order.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_sweep import SEED, _close, _copy, setup  # noqa: F401  (setup: the CIT-7 fixture of the block masks)
from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES
from test_gpu_mc_sweep_gcmc_blocks import masks  # noqa: F401  (the module's fixture)
from test_gpu_mc_sampler import GCMC_CASE, SWAP_HEAVY, _state_bytes, cha  # noqa: F401  (cha: 6 CO2 in CHA + Na, grid step 0.3)

pytestmark = pytest.mark.gpu

K, L, NC = 3, 6, 8
COUNTERS = ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")
RAMPS = np.stack([np.linspace(300.0, 600.0, NC), np.linspace(600.0, 300.0, NC), np.full(NC, 450.0)], axis=1)       # [NC, K]
SID = np.array([3, 10, 17], dtype=np.uint32)
DISPLACEMENTS = mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_reinsertion=1)


def _chains(fixture, positions_of_chain):
    """one fresh chain per entry (None: the fixture's start state), sharing the owner's grids"""
    from ceg_hip.energy import DeviceMonteCarlo
    mc, owner = fixture
    return [DeviceMonteCarlo(_copy(mc, p), grids_from=owner) for p in positions_of_chain]


def _table(temperature, ncycles, k):
    """[ncycles, k] from a scalar, one value per chain or a table"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (ncycles, k)))


def _deltas(log, T, species=None):
    """(delta_moves, delta_swaps) [steps, K]: the running sums of the statistics after every step, accumulated from the log's rows in
    the device's order (a - b of compute_accept_move, diff of compute_accept_move_swap); T [steps, K]"""
    S, k = log.shape
    out = np.zeros((2, S, k))
    for c in range(k):
        moves = swaps = 0.0
        for s in range(S):
            rec = log[s, c]
            if rec["accepted"]:
                rows = rec["rows"]
                if species is None or rec["kind"] <= 4:
                    b = ((rows[0][0] + rows[0][1]) + rows[0][2]) + rows[0][3]
                    a = ((rows[1][0] + rows[1][1]) + rows[1][2]) + rows[1][3]
                    moves += a - b
                else:
                    t, ins = species[int(rec["species"])], rec["kind"] == 5
                    swaps += mcrng.swap_threshold(rows[1] if ins else rows[0], float(T[s, c]), int(rec["n_species"]), float(t["phiPV_div_k"]),
                                                  float(t["self_reciprocal"]), float(rec["tc"]), bool(ins))[0]
            out[0, s, c], out[1, s, c] = moves, swaps
    return out[0], out[1]


def _adapted(d, t, counters, nmol, cc, adapt):
    """what the caller of the one-cycle-per-call run does between two calls"""
    tt, ta, rt, ra = (int(x) for x in counters)
    if nmol > 0 and adapt & 1:
        d = mcrng.adapt_dmax(d, ta, tt, cc)
    if nmol > 0 and adapt & 2:
        t = mcrng.adapt_thetamax(t, ra, rt, cc)
    return d, t


def _one_cycle_per_call(group, gcmc, ncycles, steps, seed, first, temperature, dmax, thetamax, adapt, cycle0=1, prior=None, **kw):
    """The yardstick: `ncycles` calls of the existing sweep on `group`, adapted on the host in between.
    -> (log [ncycles * steps, K], the call-by-call statistics, the cumulative counters [ncycles, K, 4] with `prior`, nmol [ncycles, K])"""
    k = len(group.chains)
    T = _table(temperature, ncycles, k)
    dm, th = np.broadcast_to(np.asarray(dmax, dtype=np.float64), (k,)).copy(), np.broadcast_to(np.asarray(thetamax, dtype=np.float64), (k,)).copy()
    total = np.zeros((k, 4), dtype=np.int64) if prior is None else np.array(prior, dtype=np.int64)
    logs, calls, counters, nmols = [], [], [], []
    for j in range(ncycles):
        if gcmc:
            stats, log = group.sweep_gcmc(steps, seed, first + j * steps, temperature=T[j], dmax=dm, thetamax=th, log=True, positions=False, **kw)
            total += np.stack([stats["trials"][:, 0], stats["accepted"][:, 0], stats["trials"][:, 1], stats["accepted"][:, 1]], axis=1)
            nmol = stats["nmol"].copy()
        else:
            stats, log = group.sweep(steps, seed, first + j * steps, temperature=T[j], dmax=dm, thetamax=th, log=True, **kw)
            total += np.stack([stats[n] for n in COUNTERS], axis=1)
            nmol = np.array([sum(len(kind) for kind in d._slot) for d in group.chains])
        logs.append(log); calls.append(stats); counters.append(total.copy()); nmols.append(nmol)
        for c in range(k):
            dm[c], th[c] = _adapted(dm[c], th[c], total[c], nmol[c], cycle0 + j, adapt)
    return np.concatenate(logs), calls, np.array(counters), np.array(nmols)


def _expected(gcmc, log, calls, counters, nmols, steps, temperature, dmax, thetamax, adapt, cycle0=1, prior=None, species=None):
    """(statistics, cycle records [ncycles, K]) the one-call run must return, from the yardstick's results and mcrng.cycle_records"""
    ncycles, k = nmols.shape
    T = _table(temperature, ncycles, k)
    moves, swaps = _deltas(log, np.repeat(T, steps, axis=0), species)
    ends = np.arange(1, ncycles + 1) * steps - 1
    stats = calls[-1].copy()                     # (count, nmol of a GCMC run: the last call's)
    for name in stats.dtype.names:
        if stats.dtype[name].base.kind == "i" and name not in ("count", "nmol", "_pad"):
            stats[name] = sum(call[name] for call in calls)
    stats["delta_moves" if gcmc else "delta"] = moves[-1]
    if gcmc:
        stats["delta_swaps"] = swaps[-1]
    dm, th = np.broadcast_to(np.asarray(dmax, dtype=np.float64), (k,)), np.broadcast_to(np.asarray(thetamax, dtype=np.float64), (k,))
    pr = np.zeros((k, 4), dtype=np.int64) if prior is None else np.asarray(prior, dtype=np.int64)
    records = np.stack([mcrng.cycle_records(T[:, c], dm[c], th[c], counters[:, c] - pr[c], nmols[:, c], moves[ends, c], swaps[ends, c],
                                            cycle0=cycle0, adapt=adapt, prior=pr[c]) for c in range(k)], axis=1)
    return stats, records


def _compare(fixture, positions_of_chain, *, gcmc=False, ncycles=NC, steps=L, seed=SEED + 1201, first=5, temperature, dmax, thetamax, adapt=3,
             cycle0=1, prior=None, blocks=None, what="", **kw):
    """The one-call run against the one-cycle-per-call run on identical fresh chains.  -> (stats, records, log, state bytes) of the one call"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    results = []
    for one_call in (False, True):
        devs = _chains(fixture, positions_of_chain)
        with DeviceMonteCarloGroup(devs) as group:
            if blocks is not None:
                group.set_blocks(*blocks)
            if one_call:
                call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
                extra = dict(positions=False) if gcmc else {}
                stats, records, log = call(ncycles, steps, seed, first, temperature=temperature, dmax=dmax, thetamax=thetamax, adapt=adapt, cycle0=cycle0,
                                           prior=prior, log=True, **extra, **kw)
                pockets = group.block_counts() if gcmc else None
            else:
                log, calls, counters, nmols = _one_cycle_per_call(group, gcmc, ncycles, steps, seed, first, temperature, dmax, thetamax, adapt, cycle0, prior, **kw)
                stats, records = _expected(gcmc, log, calls, counters, nmols, steps, temperature, dmax, thetamax, adapt, cycle0, prior, kw.get("species"))
                pockets = None
            results.append((stats, records, log, [_state_bytes(d) for d in devs], [d._slot for d in devs], pockets))
        _close(devs)
    (ws, wr, wl, wstate, wslot, _), (gs, gr, gl, gstate, gslot, pockets) = results
    assert gl.shape == wl.shape == (ncycles * steps, len(positions_of_chain)) and gl.tobytes() == wl.tobytes(), what
    for name in gs.dtype.names:
        assert np.array_equal(gs[name], ws[name]), (what, name, gs[name], ws[name])
    assert gs.tobytes() == ws.tobytes(), what
    for name in gr.dtype.names:                  # field by field first: a failure names what differs
        assert gr[name].tobytes() == wr[name].tobytes(), (what, name, gr[name], wr[name])
    assert gr.tobytes() == wr.tobytes(), what
    assert gstate == wstate and gslot == wslot, what
    return gs, gr, gl, gstate, pockets


def test_plain_run_with_a_ramp_per_chain_equals_one_cycle_per_call(cha):
    """K = 3, 8 cycles of 6 steps, both adapt bits, a [8, 3] table (300 -> 600 K, 600 -> 300 K, constant 450 K): log, statistics, records
    and states equal to 8 calls of ceg_mc_group_sweep with mcrng.adapt_* in between; every record equal to mcrng.cycle_records."""
    stats, records, log, _state, _p = _compare(cha, [None] * K, temperature=RAMPS, dmax=[0.5, 1.3, 2.0], thetamax=[0.5235987755982988, 1.0, 2.0],
                                               p_rotation=0.5, stream_id=SID, what="ramps")
    assert np.array_equal(records["temperature"], RAMPS) and (records["nmol"] == 6).all() and not records["delta_swaps"].any()
    assert (stats["translation_trials"] + stats["rotation_trials"] == NC * L).all()
    assert (log["accepted"] != 0).sum() > 0 and (records["dmax_next"] != records["dmax"]).any() and (records["thetamax_next"] != records["thetamax"]).any()
    assert np.array_equal(records["dmax"][1:], records["dmax_next"][:-1]) and np.array_equal(records["thetamax"][1:], records["thetamax_next"][:-1])
    print("dmax after every cycle:", records["dmax_next"].T.tolist(), "\nthetamax:", records["thetamax_next"].T.tolist())


EDGE_T = [1.0, 1e7, 400.0, 400.0]
EDGE_DMAX, EDGE_THETAMAX = [0.12, 2.8, 1.3, 1.3], [0.2, 3.0, 0.7, 0.7]
# what the chains did before the call: the acceptance ratio of 48 steps from a start state is set by that state (at 1 K every downhill
# proposal is accepted, about one half); the long history makes the cumulative ratios ~0 and ~1, as the cases ask
EDGE_PRIOR = [[4000, 0, 4000, 0], [4000, 4000, 4000, 4000], [0, 0, 0, 0], [0, 0, 0, 0]]


@pytest.mark.parametrize("adapt", [3, 0, 1, 2])
def test_edges_of_the_adaptation(cha, adapt):
    """Four chains: 1 K from dmax 0.12 / thetamax 0.2 with ratios near 0 (both lower clamps), 1e7 K from 2.8 / 3.0 with ratios near 1
    (both upper clamps), p_rotation = 0 (no rotation trial: thetamax carried over), an empty chain (both carried over, nmol 0); with
    both adapt bits, none, and each alone.  The device's records equal the restatement exactly -- this is the check of the device's
    division and square root."""
    mc = cha[0]
    _stats, rec, _log, _state, _p = _compare(cha, [None, None, None, [[] for _ in mc.positions]], temperature=EDGE_T, dmax=EDGE_DMAX, thetamax=EDGE_THETAMAX,
                                             adapt=adapt, prior=EDGE_PRIOR, p_rotation=[0.5, 0.5, 0.0, 0.5], stream_id=[1, 2, 3, 4], seed=SEED + 1202,
                                             what=f"edges, adapt {adapt}")
    assert (rec["translation_trials"][-1, :2] > 4000).all() and (rec["rotation_trials"][-1, :2] > 4000).all()        # both kinds were tried
    if adapt & 1:
        assert rec["dmax_next"][-1, 0] == 0.1 and rec["dmax_next"][-1, 1] == 3.0 and rec["dmax_next"][0, 0] > 0.1
        assert (rec["dmax_next"][:, 2] != 1.3).all()
    else:
        assert np.array_equal(rec["dmax_next"], np.broadcast_to(EDGE_DMAX, (NC, 4)))
    if adapt & 2:
        assert rec["thetamax_next"][-1, 0] == 0.17453292519943295 and rec["thetamax_next"][-1, 1] == 3.141592653589793
    else:
        assert np.array_equal(rec["thetamax_next"][:, :2], np.broadcast_to(EDGE_THETAMAX[:2], (NC, 2)))
    assert not rec["rotation_trials"][:, 2].any() and (rec["thetamax_next"][:, 2] == 0.7).all()
    assert not rec["nmol"][:, 3].any() and not rec["translation_trials"][:, 3].any()
    assert (rec["dmax_next"][:, 3] == 1.3).all() and (rec["thetamax_next"][:, 3] == 0.7).all()


def test_a_run_continued_in_a_second_call(cha):
    """8 cycles in one call == 3 + 5 cycles with first_step and cycle0 advanced, prior = the third record's counters, dmax / thetamax =
    its *_next: logs, records, statistics' counters and states."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    args = dict(p_rotation=0.5, stream_id=SID)
    seed, first, d0, t0 = SEED + 1203, 11, [0.5, 1.3, 2.0], [0.6, 1.0, 2.0]
    out = []
    for split in (False, True):
        devs = _chains(cha, [None] * K)
        with DeviceMonteCarloGroup(devs) as group:
            if not split:
                stats, rec, log = group.sweep_cycles(NC, L, seed, first, temperature=RAMPS, dmax=d0, thetamax=t0, log=True, **args)
            else:
                s1, r1, l1 = group.sweep_cycles(3, L, seed, first, temperature=RAMPS[:3], dmax=d0, thetamax=t0, log=True, **args)
                prior = np.stack([r1[-1][n] for n in COUNTERS], axis=1)
                s2, r2, l2 = group.sweep_cycles(5, L, seed, first + 3 * L, temperature=RAMPS[3:], dmax=r1[-1]["dmax_next"], thetamax=r1[-1]["thetamax_next"],
                                                cycle0=4, prior=prior, log=True, **args)
                rec, log = np.concatenate([r1, r2]), np.concatenate([l1, l2])
                stats = s2.copy()
                for n in COUNTERS + ("blocked",):
                    stats[n] = s1[n] + s2[n]
            out.append((rec, log, [_state_bytes(d) for d in devs], stats))
        _close(devs)
    (r_one, l_one, st_one, s_one), (r_two, l_two, st_two, s_two) = out
    assert l_one.tobytes() == l_two.tobytes() and st_one == st_two
    for n in COUNTERS + ("blocked",):
        assert np.array_equal(s_one[n], s_two[n]), n
    for n in r_one.dtype.names:
        if n != "delta_moves":                   # (a call's sum starts at zero: the second call's records hold its own)
            assert r_one[n].tobytes() == r_two[n].tobytes(), n
    assert r_one["delta_moves"][:3].tobytes() == r_two["delta_moves"][:3].tobytes()


def test_one_cycle_without_adaptation_is_the_sweep_and_no_cycle_is_nothing(cha):
    """ncycles = 1, adapt = 0, no table: statistics, log and states of ceg_mc_group_sweep over the same steps.  ncycles = 0: zero
    statistics, no record, the state untouched."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    args = dict(temperature=[300.0, 500.0, 900.0], dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=SID, log=True)
    out = []
    for cycles in (False, True):
        devs = _chains(cha, [None] * K)
        with DeviceMonteCarloGroup(devs) as group:
            if cycles:
                before = [_state_bytes(d) for d in devs]
                s0, r0, l0 = group.sweep_cycles(0, L, SEED + 1204, 7, **args)
                assert s0.tobytes() == bytes(s0.nbytes) and r0.shape == (0, K) and l0.shape == (0, K) and [_state_bytes(d) for d in devs] == before
                stats, rec, log = group.sweep_cycles(1, 4 * L, SEED + 1204, 7, adapt=0, **args)
                assert rec.shape == (1, K) and np.array_equal(rec["dmax_next"], rec["dmax"]) and np.array_equal(rec["thetamax_next"], rec["thetamax"])
                assert rec["delta_moves"].tobytes() == stats["delta"].tobytes() and list(rec["temperature"][0]) == [300.0, 500.0, 900.0]
            else:
                stats, log = group.sweep(4 * L, SEED + 1204, 7, **args)
            out.append((stats.tobytes(), log.tobytes(), [_state_bytes(d) for d in devs]))
        _close(devs)
    assert out[0] == out[1]


def test_gcmc_cycles_equal_one_cycle_per_call(cha):
    """6 cycles of 10 steps with the swap-heavy move table and the (phiPV_div_k, seed) of the sampler's GCMC test: logs, statistics,
    the final molecule table and states equal to six sweep_gcmc(..., positions=False) calls with host adaptation.  A temperature
    column that varies is refused where a species swaps, and accepted -- equal to its restatement -- with a displacement-only table."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    phi, seed = GCMC_CASE
    T = np.array([300.0, 800.0, 1200.0])
    devs = _chains(cha, [None])
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species([SWAP_HEAVY], [phi])
        still = group.gcmc_species([DISPLACEMENTS], [phi])
        before = _state_bytes(devs[0])
        with pytest.raises(_abi.CegError) as e:
            group.sweep_gcmc_cycles(6, 10, seed, 5, temperature=RAMPS[:6, :1], dmax=0.5, thetamax=1.0, species=table, max_molecules=16)
        assert e.value.code == -1 and "constant" in str(e.value) and _state_bytes(devs[0]) == before
    _close(devs)
    common = dict(gcmc=True, ncycles=6, steps=10, seed=seed, dmax=0.5, thetamax=1.0, max_molecules=16, stream_id=np.arange(K, dtype=np.uint32) * 7 + 3)
    stats, rec, log, _state, _p = _compare(cha, [None] * K, temperature=T, species=table, what="gcmc", **common)
    ins, dele = int(stats["accepted"][:, 5].sum()), int(stats["accepted"][:, 6].sum())
    print(f"gcmc cycles: accepted insertions {ins}, deletions {dele}, molecules per cycle {rec['nmol'].T.tolist()}")
    assert ins > 0 and (rec["nmol"][-1] == stats["nmol"]).all() and (rec["nmol"] != 6).any() and rec["delta_swaps"].any()
    assert np.array_equal(rec["translation_trials"][-1], stats["trials"][:, 0]) and np.array_equal(rec["rotation_accepted"][-1], stats["accepted"][:, 1])
    # a constant table is the scalar; a varying one runs where nothing swaps
    again, rec2, log2, _s, _p = _compare(cha, [None] * K, temperature=np.broadcast_to(T, (6, K)), species=table, what="gcmc, constant table", **common)
    assert log2.tobytes() == log.tobytes() and rec2.tobytes() == rec.tobytes() and again.tobytes() == stats.tobytes()
    s3, rec3, _l, _s, _p = _compare(cha, [None] * K, temperature=RAMPS[:6], species=still, what="gcmc, displacements only", **common)
    assert np.array_equal(rec3["temperature"], RAMPS[:6]) and not s3["trials"][:, 5:].any() and s3["trials"][:, 2].sum() > 0


def test_gcmc_cycles_with_block_masks(setup, masks):
    """The CIT-7 chains (Na + 4 CO2) with the species mask and the atom masks installed: the one-call run resolves the pockets as the
    six calls do; the pocket counters of the call are the sums of theirs."""
    species_blocks, atom_blocks = masks
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = _chains(setup, [None])
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species([NA_MOVES, CO2_MOVES], [3e5, 3e5])
    _close(devs)
    stats, rec, log, _state, pockets = _compare(setup, [None] * K, gcmc=True, ncycles=6, steps=10, seed=SEED + 1205, first=2 ** 32 - 30,
                                                temperature=[300.0, 600.0, 900.0], dmax=0.5, thetamax=1.0, species=table, max_molecules=12,
                                                stream_id=SID, blocks=(species_blocks, atom_blocks), what="gcmc, masks")
    pocket_steps = ((log["flags"] & 8) != 0).sum(axis=0)
    print(f"gcmc cycles with masks: pocket-blocked steps {pocket_steps.tolist()}, attempts {pockets[1].tolist()}")
    assert pocket_steps.sum() > 0 and np.array_equal(pockets[0], pocket_steps) and np.array_equal(pockets[1], (log["flags"] >> 16).sum(axis=0))


def test_cycles_and_the_sampler(cha):
    """A sampler with every = 6, series only: series and frame count of the one-call run equal those of the one-cycle-per-call run; the
    one-call run's log and states are identical with and without the sampler."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    args = dict(dmax=[0.5, 1.3, 2.0], thetamax=[0.6, 1.0, 2.0], p_rotation=0.5, stream_id=SID)
    seed, first = SEED + 1206, 6
    out = {}
    for mode in ("calls", "cycles", "cycles, no sampler"):
        devs = _chains(cha, [None] * K)
        with DeviceMonteCarloGroup(devs) as group:
            if mode != "cycles, no sampler":
                group.set_sampler(L, series_capacity=NC)
            if mode == "calls":
                log, _calls, _counters, _nmols = _one_cycle_per_call(group, False, NC, L, seed, first, RAMPS, args["dmax"], args["thetamax"], 3,
                                                                      p_rotation=0.5, stream_id=SID)
            else:
                _stats, _rec, log = group.sweep_cycles(NC, L, seed, first, temperature=RAMPS, log=True, **args)
            series = group.sampler_read()[1] if mode != "cycles, no sampler" else None
            out[mode] = (log.tobytes(), [_state_bytes(d) for d in devs], series)
        _close(devs)
    assert out["calls"][:2] == out["cycles"][:2] == out["cycles, no sampler"][:2]
    got, want = out["cycles"][2], out["calls"][2]
    assert got.shape == (NC, K) and list(got[:, 0]["step"]) == mcrng.sampler_frames(first, NC * L, L)
    for n in got.dtype.names:
        if n != "delta_moves":                   # (a call's sum starts at zero: each of the eight calls holds its own)
            assert got[n].tobytes() == want[n].tobytes(), n
    assert got["delta_moves"][0].tobytes() == want["delta_moves"][0].tobytes()


def _raw_plain(group, cyc, *, temperature=(300.0, 500.0, 900.0), out=True, first_step=0):
    """ceg_mc_group_sweep_cycles straight through the C ABI -> (code, the statistics buffer, which was filled with a pattern)"""
    k = len(group.chains)
    sid, T = np.arange(k, dtype=np.uint32), np.ascontiguousarray(temperature, dtype=np.float64)
    dm, th, pr = np.full(k, 0.5), np.full(k, 1.0), np.full(k, 0.5)
    beads = np.zeros(sum(len(kind) for d in group.chains for kind in d._slot), dtype=np.int32) + 0
    params = _abi.SweepParams(SEED, first_step, sid.ctypes.data, T.ctypes.data, dm.ctypes.data, th.ctypes.data, pr.ctypes.data, beads.ctypes.data)
    stats = np.full(k * _abi.SWEEP_STATS_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    n = cyc.ncycles if cyc is not None and 0 <= cyc.ncycles <= 64 else 1
    records = np.zeros((n, k), dtype=_abi.MC_CYCLE_RECORD_DTYPE)
    code = group._lib.ceg_mc_group_sweep_cycles(group._h, C.addressof(params), C.addressof(cyc) if cyc is not None else None, stats.ctypes.data,
                                                records.ctypes.data if out else None, None)
    return code, stats


def test_refusals_leave_everything_alone(cha, setup, masks, monkeypatch):
    """Every refusal of the header gives CEG_ERR_INVALID with the states, the statistics buffer and the sampler's frame count unchanged;
    masks on the plain entry point and a member with neighbour cells give CEG_ERR_UNSUPPORTED; a valid call follows."""
    from ceg_hip.energy import DeviceMonteCarlo, DeviceMonteCarloGroup
    big = 2 ** 63 - 1
    nan_table, zero_table, neg_table, inf_table = (np.full((2, K), 300.0) for _ in range(4))
    nan_table[1, 2], zero_table[0, 0], neg_table[1, 1], inf_table[0, 2] = np.nan, 0.0, -5.0, np.inf
    neg_prior, over_prior, over_rot = (np.zeros((K, 4), dtype=np.int64) for _ in range(3))
    neg_prior[1, 0], over_prior[2, :2], over_rot[0, 2:] = -1, (3, 4), (0, 1)
    keep = [nan_table, zero_table, neg_table, inf_table, neg_prior, over_prior, over_rot]

    def cyc(ncycles=2, steps=L, cycle0=1, adapt=3, table=None, prior=None):
        return _abi.McCycles(ncycles, steps, cycle0, adapt, 0, None if table is None else table.ctypes.data, None if prior is None else prior.ctypes.data)

    bad = {"no cycles": (None, {}), "ncycles < 0": (cyc(ncycles=-1), {}), "steps_per_cycle 0": (cyc(steps=0), {}), "steps_per_cycle < 0": (cyc(steps=-3), {}),
           "cycle0 0": (cyc(cycle0=0), {}), "adapt bit 2": (cyc(adapt=4), {}), "adapt negative": (cyc(adapt=-1), {}),
           "table nan": (cyc(table=nan_table), {}), "table zero": (cyc(table=zero_table), {}), "table negative": (cyc(table=neg_table), {}),
           "table inf": (cyc(table=inf_table), {}), "prior negative": (cyc(prior=neg_prior), {}), "prior accepted > trials": (cyc(prior=over_prior), {}),
           "prior rotation accepted > trials": (cyc(prior=over_rot), {}), "no cycles_out": (cyc(), dict(out=False)),
           "ncycles * steps_per_cycle": (cyc(ncycles=2 ** 40, steps=2 ** 30), {}), "first_step + steps": (cyc(ncycles=4, steps=2 ** 60), dict(first_step=2 ** 62)),
           "first_step beyond 2^63": (cyc(), dict(first_step=2 ** 63 + 5)), "99 + cycle0 + ncycles": (cyc(cycle0=big - 100), {}),
           "too many records": (cyc(ncycles=_abi.MC_CYCLES_MAX_RECORDS // K + 1, steps=1), {}), "temperature of the sweep": (cyc(), dict(temperature=(300.0, -1.0, 900.0)))}
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(L, series_capacity=4)
        group.sweep_cycles(1, L, SEED, 0, temperature=300.0, dmax=0.5, thetamax=1.0)
        before, frames = [_state_bytes(d) for d in devs], len(group.sampler_read()[1])
        assert frames == 1
        for name, (c, kw) in bad.items():
            code, stats = _raw_plain(group, c, **kw)
            assert code == -1, name
            assert (stats == 0xA5).all() and [_state_bytes(d) for d in devs] == before and len(group.sampler_read()[1]) == frames, name
        code, stats = _raw_plain(group, cyc(ncycles=4), first_step=L)          # the sampler's series holds 4 frames: one is taken
        assert code == -1 and b"frames" in group._lib.ceg_last_error() and (stats == 0xA5).all() and [_state_bytes(d) for d in devs] == before
        # the GCMC entry point: its own refusals and those of the cycles
        table = group.gcmc_species([SWAP_HEAVY], [3e4])
        g = dict(dmax=0.5, thetamax=1.0, species=table, max_molecules=16)
        for name, kw in {"adapt": dict(adapt=8, temperature=300.0), "cycle0": dict(cycle0=0, temperature=300.0), "steps": dict(steps_per_cycle=0, temperature=300.0),
                         "varying column": dict(temperature=RAMPS[:2]), "table nan": dict(temperature=nan_table), "prior": dict(prior=over_prior, temperature=300.0),
                         "max_molecules": dict(temperature=300.0, max_molecules=2)}.items():
            with pytest.raises(_abi.CegError) as e:
                group.sweep_gcmc_cycles(2, kw.pop("steps_per_cycle", L), SEED, L, **{**g, **kw})
            assert e.value.code == -1 and [_state_bytes(d) for d in devs] == before and len(group.sampler_read()[1]) == frames, name
        stats, rec = group.sweep_cycles(3, L, SEED, L, temperature=300.0, dmax=0.5, thetamax=1.0)      # a valid call follows
        assert (stats["translation_trials"] + stats["rotation_trials"] == 3 * L).all() and len(group.sampler_read()[1]) == 4
    _close(devs)
    # masks: the plain entry point refuses the group as the plain sweep does
    devs = _chains(setup, [None] * 2)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_blocks(*masks)
        before = [_state_bytes(d) for d in devs]
        for call in (lambda: group.sweep(L, SEED, 0, temperature=300.0, dmax=0.5, thetamax=1.0),
                     lambda: group.sweep_cycles(2, L, SEED, 0, temperature=300.0, dmax=0.5, thetamax=1.0)):
            with pytest.raises(_abi.CegError) as e:
                call()
            assert e.value.code == -5 and "masks" in str(e.value) and [_state_bytes(d) for d in devs] == before
    _close(devs)
    # a member that keeps its guests in neighbour cells
    mc, owner = setup
    monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
    cells = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    monkeypatch.delenv("CEG_HIP_MC_CELLS")
    assert cells.neighbour_cells() is not None
    plain = DeviceMonteCarlo(_copy(mc), grids_from=owner)
    with DeviceMonteCarloGroup([plain, cells]) as group:
        before = [_state_bytes(d) for d in (plain, cells)]
        table = group.gcmc_species([NA_MOVES, CO2_MOVES], [3e5, 3e5])
        for call in (lambda: group.sweep_cycles(2, L, SEED, 0, temperature=300.0, dmax=0.5, thetamax=1.0),
                     lambda: group.sweep_gcmc_cycles(2, L, SEED, 0, temperature=300.0, dmax=0.5, thetamax=1.0, species=table, max_molecules=12)):
            with pytest.raises(_abi.CegError) as e:
                call()
            assert e.value.code == -5 and "chain 1" in str(e.value) and [_state_bytes(d) for d in (plain, cells)] == before
    _close([plain, cells])


def _follow_tail(devs, before):
    """modify_species!(mc.tailcorrection, i, +-1) (montecarlo.jl:814,858) for the molecules a GCMC call added to or took from the chains:
    the sweeps leave mc.tailcorrection alone, and baseline_energy reports it"""
    from ceg_hip.hostmirror.montecarlo import modify_species_dryrun
    for d, old in zip(devs, before):
        counts = list(old)
        for i, kind in enumerate(d._slot):
            while d.mc.tail_cross is not None and counts[i] != len(kind):
                num = 1 if counts[i] < len(kind) else -1
                d.mc.tailcorrection += modify_species_dryrun(d.mc.tail_framework, d.mc.tail_cross, counts, i, num)
                counts[i] += num


@pytest.mark.parametrize("kind", ["plain", "gcmc"])
def test_run_montecarlo(cha, kind):
    """ninit = 2, ncycles = 6: the returned energies are baseline + record deltas, the drift check passes at the reference's rtol 1e-9,
    and the result equals the same run composed by hand from sweep_cycles and baseline_energies.  GCMC: what the drift check compares
    is energies[-1] plus the bookkeeping of the accepted swaps (delta_swaps sums the rule's `diff`, which leaves out the self term and
    the Ewald constants of the changed counts: without it this run deviates by 1.1e5 K, 75 %, on the first chain)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    ninit, ncycles, seed = 2, 6, SEED + 1207
    phi = GCMC_CASE[0]
    T = RAMPS if kind == "plain" else np.array([300.0, 800.0, 1200.0])
    out = []
    for by_hand in (False, True):
        devs = _chains(cha, [None] * K)
        with DeviceMonteCarloGroup(devs) as group:
            gcmc = None if kind == "plain" else dict(species=group.gcmc_species([SWAP_HEAVY], [phi]), max_molecules=16)
            steps = 6 if kind == "plain" else 50
            assert group.numsteps(None if kind == "plain" else [SWAP_HEAVY]) == [steps] * K
            if not by_hand:
                run = group.run_montecarlo(T, ncycles, ninit, seed=seed, gcmc=gcmc, stream_id=SID, positions=False)
                assert run.initial_energies.shape == (ninit, K) and run.energies.shape == (ncycles, K) and run.cycles.shape == (ninit + ncycles, K)
                b0, b1, b2 = (np.array([float(r) for r in b]) for b in run.baselines)
                c = run.cycles
                assert np.array_equal(run.initial_energies, b0 + c["delta_moves"][:ninit] + c["delta_swaps"][:ninit])
                assert np.array_equal(run.energies, b1 + c["delta_moves"][ninit:] + c["delta_swaps"][ninit:])
                drift = np.abs(run.recorded - b2) / np.maximum(np.abs(run.recorded), np.abs(b2))
                print(f"run_montecarlo ({kind}): recorded {run.recorded.tolist()}, actual {b2.tolist()}, relative deviation {drift.tolist()}, "
                      f"energies[-1] {run.energies[-1].tolist()}, molecules {c['nmol'][-1].tolist()}")
                assert (drift <= 1e-9).all()
                if kind == "plain":
                    assert np.array_equal(run.recorded, run.energies[-1])
                else:                            # the run must put the swaps' bookkeeping to work
                    assert (c["nmol"][-1] != c["nmol"][ninit - 1]).any() and not np.array_equal(run.recorded, run.energies[-1])
                assert c["dmax"][0].tolist() == [1.3] * K and c["thetamax"][0].tolist() == [math.radians(30.0)] * K
                if kind == "plain":              # the counters run on through both calls
                    assert list(c["translation_trials"][-1] + c["rotation_trials"][-1]) == [(ninit + ncycles) * steps] * K
                out.append((run.initial_energies, run.energies, run.cycles, run.stats, [_state_bytes(d) for d in devs]))
                continue
            call = group.sweep_cycles if kind == "plain" else group.sweep_gcmc_cycles
            extra = {} if kind == "plain" else dict(positions=False, **gcmc)
            rows = (lambda a, b: T[a:b]) if kind == "plain" else (lambda a, b: T)
            e0 = np.array([float(r) for r in group.baseline_energies()])
            counts = [[len(kind) for kind in d._slot] for d in devs]
            s1, c1 = call(ninit, steps, seed, 0, temperature=rows(0, ninit), dmax=1.3, thetamax=math.radians(30.0), stream_id=SID, **extra)
            _follow_tail(devs, counts)
            e1 = np.array([float(r) for r in group.baseline_energies()])
            s2, c2 = call(ncycles, steps, seed, ninit * steps, temperature=rows(ninit, ninit + ncycles), dmax=c1[-1]["dmax_next"], thetamax=c1[-1]["thetamax_next"],
                          cycle0=1 + ninit, prior=np.stack([c1[-1][n] for n in COUNTERS], axis=1), stream_id=SID, **extra)
            out.append((e0 + c1["delta_moves"] + c1["delta_swaps"], e1 + c2["delta_moves"] + c2["delta_swaps"], np.concatenate([c1, c2]), (s1, s2),
                        [_state_bytes(d) for d in devs]))
        _close(devs)
    got, want = out
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes() and got[4] == want[4]
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got[3], want[3]))
