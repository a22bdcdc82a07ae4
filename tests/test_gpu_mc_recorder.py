"""The recorder of a chain group (ceg_mc_group_set_recorder / _snapshot / _recorder_rebase / _recorder_read / _recorder_min, kernel
k_mcg_snapshot): position snapshots at cycle ends and the minimum-energy record, taken on the device inside
ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles.  The yardstick is the same entry point driven ONE CYCLE PER CALL on
identical fresh chains with NO recorder, ceg_mc_get_state and the host mirror read after every call: frames must equal it byte for
byte (positions, kinds, mol_first, species, nmol, natoms, cycle, step), and the energy must equal E0 + delta, the deltas accumulated
from the yardstick's log in step order, bit for bit.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_cycles import COUNTERS, _chains, _deltas
from test_gpu_mc_sweep import SEED, _close, _device_order, setup  # noqa: F401  (setup: the CIT-7 fixture of the chains with cells)
from test_gpu_mc_sampler import GCMC_CASE, SWAP_HEAVY, _start, _state_bytes, cha  # noqa: F401  (cha: 6 CO2 in CHA + Na, grid step 0.3)

pytestmark = pytest.mark.gpu

K, L, NC = 5, 6, 12
LADDER = np.array([200.0, 260.0, 340.0, 450.0, 600.0])
RAMP = LADDER[None, :] * np.linspace(1.0, 1.25, 24)[:, None]            # [24, K]: every row non-decreasing in the chain (rung)
SID = np.array([3, 10, 17, 24, 31], dtype=np.uint32)
STEP_SIZES = dict(dmax=[0.5, 0.8, 1.0, 1.3, 2.0], thetamax=[0.5, 0.7, 1.0, 1.5, 2.0])
FIRST = 5
_CACHE = {}


def _energies(group):
    return np.array([float(r) for r in group.baseline_energies()])


def _frame_of(dev):
    """(positions [natoms, 3], kinds, mol_first, species) of a chain in device molecule order: ceg_mc_get_state and the host mirror"""
    spec = [i for i, _j in _device_order(dev)]
    sizes = [len(dev.mc.ffidx[i]) for i in spec]
    pos = np.zeros((sum(sizes), 3))
    _abi.check(dev._lib, dev._lib.ceg_mc_get_state(dev._h, _abi.dptr(pos.reshape(-1)) if len(pos) else None, None, None))
    kinds = np.array([q - 1 for i in spec for q in dev.mc.ffidx[i]], dtype=np.int32)
    return pos, kinds, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), np.array(spec, dtype=np.int32)


def _rows(T, a, b):
    T = np.asarray(T, dtype=np.float64)
    return T[a:b] if T.ndim == 2 else T


def _yard(make, T, *, gcmc=False, ncycles=NC, steps=L, seed, dmax, thetamax, adapt=3, cycle0=1, stop=None, prepare=None, parts=None, **kw):
    """One cycle per call with no recorder, the state read after every call.  -> E0, E [ncycles, K] (per call of `parts`: the energy at
    the call's start + the deltas accumulated over the call's log), frames0 / frames [ncycles][K], log, stopped [ncycles, K]"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = make()
    k = len(devs)
    with DeviceMonteCarloGroup(devs) as group:
        if prepare is not None:
            prepare(group)
        if stop is not None:
            group.set_chain_plan(stop_step=stop)
        E0 = _energies(group)
        dm, th = (np.broadcast_to(np.asarray(x, dtype=np.float64), (k,)).copy() for x in (dmax, thetamax))
        total = np.zeros((k, 4), dtype=np.int64)
        call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
        extra = dict(positions=False) if gcmc else {}
        frames0 = [_frame_of(d) for d in devs]
        frames, logs = [], []
        for j in range(ncycles):
            _s, c, l = call(1, steps, seed, FIRST + j * steps, temperature=_rows(T, j, j + 1), dmax=dm, thetamax=th, adapt=adapt, cycle0=cycle0 + j,
                            prior=total, log=True, **extra, **kw)
            total = np.stack([c[0][n] for n in COUNTERS], axis=1)
            dm, th = c[0]["dmax_next"].copy(), c[0]["thetamax_next"].copy()
            frames.append([_frame_of(d) for d in devs])
            logs.append(l)
        state, slot = [_state_bytes(d) for d in devs], [d._slot for d in devs]
    _close(devs)
    log = np.concatenate(logs)
    table = np.broadcast_to(np.asarray(T, dtype=np.float64), (ncycles, k)) if np.ndim(T) < 2 else np.asarray(T, dtype=np.float64)[:ncycles]
    E = np.zeros((ncycles, k))
    base, a = E0, 0
    for n in parts or [ncycles]:
        moves, swaps = _deltas(log[a * steps:(a + n) * steps], np.repeat(table[a:a + n], steps, axis=0), kw.get("species"))
        ends = np.arange(1, n + 1) * steps - 1
        E[a:a + n] = (base + moves[ends]) + swaps[ends] if gcmc else base + moves[ends]
        base, a = E[a + n - 1], a + n
    last = FIRST + np.arange(1, ncycles + 1) * steps - 1
    stopped = np.zeros((ncycles, k), dtype=bool) if stop is None else last[:, None] >= np.asarray(stop)[None, :]
    return dict(E0=E0, E=E, frames0=frames0, frames=frames, log=log, state=state, slot=slot, stopped=stopped)


def _recorded(make, T, *, rec, gcmc=False, ncycles=NC, steps=L, seed, dmax, thetamax, adapt=3, cycle0=1, stop=None, prepare=None, parts=None,
              tempering=None, snap=False, **kw):
    """The run under test: the cycles in one call (or in the calls `parts`), with the recorder `rec` (None: without one); snap: one
    ceg_mc_group_snapshot behind the calls, the last frame, and the chains' states then in out["final"]"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = make()
    out = {}
    with DeviceMonteCarloGroup(devs) as group:
        if prepare is not None:
            prepare(group)
        if stop is not None:
            group.set_chain_plan(stop_step=stop)
        out["E0"] = _energies(group)
        if tempering is not None:
            group.set_tempering(tempering, out["E0"], capacity=ncycles)
        if rec is not None:
            group.set_recorder(energies=out["E0"], **rec)
        call = group.sweep_gcmc_cycles if gcmc else group.sweep_cycles
        extra = dict(positions=False) if gcmc else {}
        dm, th, prior, done = dmax, thetamax, None, 0
        stats, cycs, logs = [], [], []
        for n in parts or [ncycles]:
            s, c, l = call(n, steps, seed, FIRST + done * steps, temperature=_rows(T, done, done + n), dmax=dm, thetamax=th, adapt=adapt,
                           cycle0=cycle0 + done, prior=prior, log=True, **extra, **kw)
            stats.append(s); cycs.append(c); logs.append(l)
            dm, th, prior = c[-1]["dmax_next"], c[-1]["thetamax_next"], np.stack([c[-1][n_] for n_ in COUNTERS], axis=1)
            done += n
        out.update(stats=[s.tobytes() for s in stats], cyc=np.concatenate(cycs), log=np.concatenate(logs), state=[_state_bytes(d) for d in devs],
                   slot=[d._slot for d in devs])
        if tempering is not None:
            out["tempering"] = group.tempering_read()
        if snap:
            group.snapshot()
            out["final"] = [_frame_of(d) for d in devs]
        if rec is not None:
            out["records"], out["frames"] = group.recorder_read()
            out["window"] = group.recorder_read(1, 2) if len(out["records"]) >= 3 else None
            if rec.get("track_min"):
                out["min"] = group.recorder_minimum()
    _close(devs)
    return out


def _same_frame(got, want, gcmc, what):
    (gp, gk, gf, gs), (wp, wk, wf, ws) = got, want
    assert gp.shape == wp.shape and gp.tobytes() == wp.tobytes(), (what, "positions")
    assert np.array_equal(gk, wk) and gk.dtype == np.int32, (what, "kinds", gk, wk)
    assert np.array_equal(gf, wf), (what, "mol_first", gf, wf)
    assert np.array_equal(gs, ws if gcmc else np.full(len(ws), -1)), (what, "species", gs, ws)


def _hold(got, want, due, *, gcmc=False, steps=L, cycle0=1, what=""):
    """the frames of the recorded run at the cycles `due` against the yardstick"""
    records, frames = got["records"], got["frames"]
    k = len(want["E0"])
    assert records.shape == (len(due), k) and len(frames) == len(due), (what, records.shape, due)
    assert got["E0"].tobytes() == want["E0"].tobytes(), what
    for f, cc in enumerate(due):
        j = cc - cycle0
        for c in range(k):
            r, w = records[f, c], want["frames"][j][c]
            where = (what, "cycle", cc, "chain", c)
            assert (r["cycle"], r["step"]) == (cc, FIRST + (j + 1) * steps - 1), where
            assert (r["nmol"], r["natoms"]) == (len(w[2]) - 1, len(w[1])), where
            assert r["flags"] == (2 if want["stopped"][j, c] else 0), where
            assert r["energy"].tobytes() == want["E"][j, c].tobytes(), (where, r["energy"], want["E"][j, c])
            _same_frame(frames[f][c], w, gcmc, where)


def _untouched(got, plain, what):
    """log, statistics, cycle records and states of the run with a recorder against the same run without one"""
    assert got["log"].tobytes() == plain["log"].tobytes() and got["stats"] == plain["stats"], what
    assert got["cyc"].tobytes() == plain["cyc"].tobytes() and got["state"] == plain["state"] and got["slot"] == plain["slot"], what


def _cha_chains(cha, k=K):
    return lambda: _chains(cha, [None] * k)


def _main(cha):
    """the plain run on the ramp: the yardstick, the run without a recorder and the run with every = 1 and track_min, once for the module"""
    if "main" not in _CACHE:
        args = dict(seed=SEED + 1401, p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        _CACHE["main"] = (_yard(_cha_chains(cha), RAMP, **args), _recorded(_cha_chains(cha), RAMP, rec=None, **args),
                          _recorded(_cha_chains(cha), RAMP, rec=dict(every=1, capacity=NC, track_min=True), **args), args)
    return _CACHE["main"]


def test_a_frame_at_every_cycle_end_on_a_ramp(cha):
    """cases 1, 9, 12: every = 1 under a temperature ramp; the sweep is untouched; windows of recorder_read"""
    want, plain, got, _args = _main(cha)
    assert (want["log"]["accepted"] != 0).sum() > 10
    _hold(got, want, list(range(1, NC + 1)), what="every 1")
    _untouched(got, plain, "every 1")
    records, frames = got["window"]
    assert records.tobytes() == got["records"][1:3].tobytes()
    for f in range(2):
        for c in range(K):
            _same_frame(frames[f][c], got["frames"][1 + f][c], True, ("window", f, c))


def test_every_third_cycle_from_an_origin(cha):
    """case 1: every = 3, origin = 4: frames at the ends of cycles 4, 7, 10; no track_min: no launch at the other cycle ends"""
    want, plain, _got, args = _main(cha)
    due = mcrng.snapshot_cycles(1, NC, 4, 3)
    assert due == [4, 7, 10]
    got = _recorded(_cha_chains(cha), RAMP, rec=dict(every=3, origin=4, capacity=3), **args)
    _hold(got, want, due, what="every 3, origin 4")
    _untouched(got, plain, "every 3, origin 4")


def test_the_minimum(cha):
    """case 6: recorder_minimum() is mcrng.track_minimum over the yardstick's energies, its body the yardstick's state at that cycle"""
    want, _plain, got, _args = _main(cha)
    mink, mine, records, bodies = got["min"]
    wk, we = mcrng.track_minimum(want["E"], want["E0"])
    print(f"minimum: mink {mink.tolist()} (yardstick {wk.tolist()}), mine {mine.tolist()}")
    assert np.array_equal(mink, wk) and mine.tobytes() == we.tobytes()
    assert (mink >= 1).any()
    for c in range(K):
        w = want["frames0"][c] if mink[c] < 0 else want["frames"][mink[c] - 1][c]
        _same_frame(bodies[c], w, False, ("minimum", c))
        assert records[c]["energy"] == mine[c] and records[c]["cycle"] == mink[c] and records[c]["flags"] == 0
        assert records[c]["step"] == (-1 if mink[c] < 0 else FIRST + mink[c] * L - 1)


def test_restore_and_run_montecarlo(cha):
    """case 6: after restore(c, best) the baseline energy agrees with mine[c] at the reference's drift tolerance, rtol 1e-9
    (simulation.jl:851); run_montecarlo with ninit > 0 rebases an installed recorder at both baselines, so mine is the minimum over
    initial_energies and energies from the start baseline"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_recorder(0, capacity=0, track_min=True)
        group.sweep_cycles(NC, L, SEED + 1402, FIRST, temperature=RAMP[:NC], p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        mink, mine, records, bodies = group.recorder_minimum()
        assert group.recorder_read()[0].shape == (0, K)
        for c in range(K):
            group.restore(c, bodies[c])
        actual = _energies(group)
        dev = np.abs(actual - mine) / np.maximum(np.abs(actual), np.abs(mine))
        print(f"restore: mink {mink.tolist()}, mine {mine.tolist()}, baseline after restore {actual.tolist()}, relative deviation {dev.tolist()}")
        assert (mink >= 1).any() and (dev <= 1e-9).all()
        for c, d in enumerate(devs):             # (a frame of the plain entry point carries species -1: restore took them from the kinds)
            now = _frame_of(d)
            assert all(np.array_equal(a, b) for a, b in zip(now[:3], bodies[c][:3])) and not now[3].any(), c
    _close(devs)
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_recorder(0, capacity=0, track_min=True)
        run = group.run_montecarlo(RAMP[:8], 6, 2, seed=SEED + 1403, stream_id=SID, positions=False)
        mink, mine, _records, _bodies = group.recorder_minimum()
    _close(devs)
    start = np.array([float(r) for r in run.baselines[0]])
    wk, we = mcrng.track_minimum(np.concatenate([run.initial_energies, run.energies]), start)
    print(f"run_montecarlo: mink {mink.tolist()} (expected {wk.tolist()}), mine {mine.tolist()}")
    assert np.array_equal(mink, wk) and mine.tobytes() == we.tobytes() and (mink >= 1).any()


def test_gcmc_frames_under_swaps(cha):
    """case 2: SWAP_HEAVY, the molecule count changes between frames and freed atom slots are reused (molecule order != slot order).
    The yardstick's log must itself hold an accepted insertion and an accepted deletion; track_min is refused under swaps."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    phi, seed = GCMC_CASE
    nc = 24
    devs = _chains(cha, [None])
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species([SWAP_HEAVY], [phi])
    _close(devs)
    T = np.array([300.0, 800.0, 1200.0, 1000.0, 600.0])
    args = dict(gcmc=True, ncycles=nc, seed=seed, dmax=0.5, thetamax=1.0, adapt=0, species=table, max_molecules=16, stream_id=np.arange(K, dtype=np.uint32) * 7 + 3)
    want = _yard(_cha_chains(cha), T, **args)
    log = want["log"]
    ins = (log["kind"] == 5) & (log["accepted"] != 0)
    dele = (log["kind"] == 6) & (log["accepted"] != 0)
    print(f"gcmc: accepted insertions {int(ins.sum())}, deletions {int(dele.sum())} per chain {ins.sum(axis=0).tolist()} / {dele.sum(axis=0).tolist()}")
    assert ins.sum() > 0 and dele.sum() > 0
    # a chain that deleted and later inserted: the insertion took the freed slots, so its molecules are no longer in slot order
    reused = [c for c in range(K) if dele[:, c].any() and ins[np.argmax(dele[:, c]):, c].any()]
    print(f"gcmc: chains with an insertion after a deletion {reused}; molecules at the end {[len(f[2]) - 1 for f in want['frames'][-1]]}")
    assert reused                                # (24 cycles: chain 0 deletes once and inserts afterwards; 16 cycles held no insertion behind the deletion)
    got = _recorded(_cha_chains(cha), T, rec=dict(every=1, capacity=nc + 1, max_molecules=16), snap=True, **args)
    # the snapshot behind the call: the views' counts are current again (the molecule counts changed), the species are not known
    last = got["records"][-1]
    assert (last["cycle"] == -1).all() and (last["step"] == -1).all() and last["energy"].tobytes() == want["E"][-1].tobytes()
    assert list(last["nmol"]) == [len(f[2]) - 1 for f in got["final"]] and (last["nmol"] != 6).any()
    for c in range(K):
        _same_frame(got["frames"][-1][c], got["final"][c], False, ("snapshot after gcmc", c))
        _same_frame(got["final"][c], want["frames"][-1][c], True, ("final state", c))
    got["records"], got["frames"] = got["records"][:-1], got["frames"][:-1]
    _hold(got, want, list(range(1, nc + 1)), gcmc=True, what="gcmc")
    assert got["state"] == want["state"] and got["slot"] == want["slot"]
    counts = got["records"]["nmol"]
    assert (counts != counts[0]).any()
    plain = _recorded(_cha_chains(cha), T, rec=None, **args)
    _untouched(got, plain, "gcmc")


def test_a_chain_with_neighbour_cells(setup, monkeypatch):
    """case 3: the Na + 4 CO2 CIT-7 chains, one of the five with its guests in 4 A neighbour cells, after device_cells()"""
    from test_gpu_mc_sweep_cells import _make
    make = lambda: _make(setup, monkeypatch, (None, 4, None, None, None))
    args = dict(seed=SEED + 1404, p_rotation=0.5, stream_id=SID, prepare=lambda group: group.device_cells(), **STEP_SIZES)
    T = np.array([400.0, 500.0, 650.0, 800.0, 1000.0])
    want = _yard(make, T, **args)
    got = _recorded(make, T, rec=dict(every=2, origin=1, capacity=NC, track_min=True), **args)
    assert (want["log"]["accepted"][:, 1] != 0).any()
    _hold(got, want, mcrng.snapshot_cycles(1, NC, 1, 2), what="cells")
    mink, mine, _records, _bodies = got["min"]
    wk, we = mcrng.track_minimum(want["E"], want["E0"])
    assert np.array_equal(mink, wk) and mine.tobytes() == we.tobytes()
    assert got["state"] == want["state"]


def test_two_calls_and_a_stopped_chain(cha):
    """case 4: 12 cycles as 5 + 7 with chain 2 stopped by the chain plan in the middle of cycle 7: its frames repeat the frozen state
    with flag 2 from that cycle end on, and its minimum stops updating.  The second call starts from the rounded energies of the first."""
    stop = np.array([2 ** 62, 2 ** 62, FIRST + 6 * L + 2, 2 ** 62, 2 ** 62], dtype=np.int64)
    args = dict(seed=SEED + 1405, p_rotation=0.5, stream_id=SID, stop=stop, parts=[5, 7], **STEP_SIZES)
    want = _yard(_cha_chains(cha), RAMP, **args)
    got = _recorded(_cha_chains(cha), RAMP, rec=dict(every=1, capacity=NC, track_min=True), **args)
    assert want["stopped"][:, 2].tolist() == [False] * 6 + [True] * 6 and not want["stopped"][:, [0, 1, 3, 4]].any()
    _hold(got, want, list(range(1, NC + 1)), what="two calls, a stop")
    assert (got["records"]["flags"][:, 2] == [0] * 6 + [2] * 6).all()
    for f in range(7, NC):                       # frozen: the frames repeat
        _same_frame(got["frames"][f][2], got["frames"][6][2], True, ("frozen", f))
    mink, mine, _records, _bodies = got["min"]
    wk, we = mcrng.track_minimum(want["E"], want["E0"], want["stopped"])
    assert np.array_equal(mink, wk) and mine.tobytes() == we.tobytes() and mink[2] <= 6
    assert got["state"] == want["state"]


def test_with_tempering(cha):
    """case 5: tempering installed: exchange records, rungs, energies, log and final states equal those of the same run without the
    recorder; the frames carry the energies of the exchange records, and the states of the untempered definition of a frame"""
    args = dict(seed=SEED + 1406, p_rotation=0.5, stream_id=SID, tempering=1, **STEP_SIZES)
    plain = _recorded(_cha_chains(cha), RAMP, rec=None, **args)
    got = _recorded(_cha_chains(cha), RAMP, rec=dict(every=1, capacity=NC, track_min=True), **args)
    _untouched(got, plain, "tempering")
    for a, b in zip(got["tempering"], plain["tempering"]):
        assert a.tobytes() == b.tobytes()
    xrec = got["tempering"][3]
    assert (xrec["accepted"] == 1).any() and got["records"].shape == xrec.shape
    assert got["records"]["energy"].tobytes() == xrec["energy"].tobytes()
    assert list(got["records"]["cycle"][:, 0]) == list(range(1, NC + 1))
    wk, we = mcrng.track_minimum(xrec["energy"], got["E0"])
    assert np.array_equal(got["min"][0], wk) and got["min"][1].tobytes() == we.tobytes()
    for c in range(K):                           # the last frame is the final state
        pos = got["frames"][-1][c][0]
        assert got["state"][c].startswith(pos.tobytes())


def test_chains_of_more_molecules_than_a_workgroup_has_lanes(setup, monkeypatch):
    """case 7: 257 and 513 molecules of 1- and 3-atom species (two and three chunks of the prefix sum, the 3-atom molecules first, two
    molecules removed from each so that molecule order != slot order) beside an EMPTY chain: one snapshot and one cycle"""
    import test_gpu_mc_many_molecules as mm
    from ceg_hip.energy import DeviceMonteCarloGroup
    monkeypatch.setattr(mm, "MIN_SEP", 2.0)      # (513 molecules do not fit the cell 2.4 A apart; the copy does not care)
    mc, _owner = setup
    mcd = mm._three_kinds(mc)
    devs = []
    for counts, seed in (((0, 61, 198), 7400), ((0, 15, 500), 7401)):
        dev = mm._device_chain(setup, mcd, mm._populate(mcd, list(counts), seed))
        for i, j in ((1, 5), (2, 100)):          # the last molecule of the kind takes index j (montecarlo.jl:798-808)
            dev.remove((i, j))
            dev.mc.positions[i][j] = dev.mc.positions[i][-1]
            dev.mc.positions[i].pop()
        devs.append(dev)
    devs.append(mm._device_chain(setup, mcd, [[], [], []]))
    assert [sum(len(kind) for kind in d._slot) for d in devs] == [257, 513, 0]
    with DeviceMonteCarloGroup(devs) as group:
        E0 = _energies(group)
        assert np.isfinite(E0).all()
        group.set_recorder(1, capacity=2, energies=E0, track_min=True)
        assert (group.recorder["max_molecules"], group.recorder["max_atoms"]) == (513, 14 * 3 + 499)
        before = [_frame_of(d) for d in devs]
        group.snapshot()
        stats, _cyc = group.sweep_cycles(1, L, SEED + 1407, 0, temperature=[500.0] * 3, dmax=0.4, thetamax=0.8, p_rotation=0.5, stream_id=[6, 7, 8])
        after = [_frame_of(d) for d in devs]
        records, frames = group.recorder_read()
        mink, mine, mrec, bodies = group.recorder_minimum()
    assert records.shape == (2, 3) and list(records["cycle"][:, 0]) == [-1, 1] and list(records["step"][:, 0]) == [-1, L - 1]
    assert stats["translation_accepted"].sum() + stats["rotation_accepted"].sum() > 0
    E1 = E0 + stats["delta"]
    for c in range(3):
        _same_frame(frames[0][c], before[c], False, ("snapshot", c))
        _same_frame(frames[1][c], after[c], False, ("cycle", c))
        assert records[0, c]["energy"] == E0[c] and records[1, c]["energy"].tobytes() == E1[c].tobytes() and not records["flags"][:, c].any()
        assert (records[0, c]["nmol"], records[0, c]["natoms"]) == (len(before[c][2]) - 1, len(before[c][1]))
        _same_frame(bodies[c], after[c] if E1[c] < E0[c] else before[c], False, ("minimum", c))
        assert mink[c] == (1 if E1[c] < E0[c] else -1) and mine[c] == min(E0[c], E1[c])
    assert records[1, 2]["nmol"] == 0 == records[1, 2]["natoms"] and list(frames[1][2][2]) == [0]
    _close(devs)


def _raw_read(group, nframes):
    """the padded arrays of recorder_read, straight from the C call"""
    s, k = group.recorder, len(group.chains)
    xyz, kind = np.full((nframes, k, s["max_atoms"], 3), 7.0), np.full((nframes, k, s["max_atoms"]), 7, dtype=np.int32)
    first, species = np.full((nframes, k, s["max_molecules"] + 1), 7, dtype=np.int32), np.full((nframes, k, s["max_molecules"]), 7, dtype=np.int32)
    _abi.check(group._lib, group._lib.ceg_mc_group_recorder_read(group._h, 0, nframes, None, _abi.dptr(xyz.reshape(-1)), _abi.i32ptr(kind.reshape(-1)),
                                                                 _abi.i32ptr(first.reshape(-1)), _abi.i32ptr(species.reshape(-1)), None))
    return xyz, kind, first, species


def test_a_chain_that_does_not_fit(cha):
    """case 8: max_atoms one below chain 0's atom count: flag 1, the true counts, a zero body and CEG_OK; the other chains' frames intact
    and zero beyond their counts"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc = cha[0]
    fewer = [[p.copy() for p in mc.positions[0][:5]]]
    devs = _chains(cha, [None, fewer, fewer])
    with DeviceMonteCarloGroup(devs) as group:
        group.set_recorder(1, capacity=3, max_atoms=17, max_molecules=6, track_min=True)
        group.sweep_cycles(2, L, SEED + 1408, FIRST, temperature=[300.0, 500.0, 900.0], dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=[3, 10, 17])
        group.snapshot()
        want = [_frame_of(d) for d in devs]
        records, frames = group.recorder_read()
        xyz, kind, first, species = _raw_read(group, 3)
        _mink, _mine, mrec, bodies = group.recorder_minimum()
    assert records.shape == (3, 3)
    assert (records["flags"][:, 0] == 1).all() and (records["nmol"][:, 0] == 6).all() and (records["natoms"][:, 0] == 18).all()
    assert not xyz[:, 0].any() and not kind[:, 0].any() and not first[:, 0].any() and not species[:, 0].any()
    assert all(len(frames[f][0][0]) == 0 for f in range(3)) and mrec[0]["flags"] == 1 and len(bodies[0][0]) == 0
    for c in (1, 2):
        assert not records["flags"][:, c].any() and (records["natoms"][:, c] == 15).all()
        for f in (1, 2):                         # the end of cycle 2 and the snapshot after the call
            _same_frame(frames[f][c], want[c], False, ("fits", f, c))
        assert not xyz[:, c, 15:].any() and not kind[:, c, 15:].any() and not first[:, c, 6:].any() and (species[:, c, :5] == -1).all() and not species[:, c, 5:].any()
    _close(devs)


def test_refusals_leave_everything_alone(cha):
    """cases 10, 11: every refusal of the header gives CEG_ERR_INVALID before anything changed -- states equal to the start -- and the
    earlier recorder still works afterwards"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs = _chains(cha, [None] * K)
    with DeviceMonteCarloGroup(devs) as group:
        E0 = _energies(group)
        group.set_recorder(1, capacity=2, energies=E0)
        earlier = dict(group.recorder)
        start = [_state_bytes(d) for d in devs]

        def refused(fn, word):
            with pytest.raises(_abi.CegError) as e:
                fn()
            assert e.value.code == -1 and word in str(e.value), (word, str(e.value))
            assert group.recorder == earlier     # (the Python side notes a recorder only after the C call succeeded)
            assert [_state_bytes(d) for d in devs] == start

        for bad, word in ((dict(every=-1), "every"), (dict(every=1, origin=-1), "origin"), (dict(every=1, capacity=-1), "frame_capacity"),
                          (dict(every=1, max_atoms=0, max_molecules=6), "max_atoms"), (dict(every=1, max_atoms=18, max_molecules=0), "max_atoms"),
                          (dict(every=1, energies=[np.nan] + [0.0] * (K - 1)), "finite"), (dict(every=1, energies=[np.inf] * K), "finite"),
                          (dict(every=1, capacity=2 ** 40), "too large")):
            kw = dict(energies=E0)
            kw.update(bad)
            if "max_atoms" in bad:               # (set_recorder clamps the room to >= 1 for the defaults: go to the C call for a zero)
                spec = _abi.McRecorder(1, 0, 2, bad["max_atoms"], bad["max_molecules"], 0, 0, E0.ctypes.data)
                refused(lambda: _abi.check(group._lib, group._lib.ceg_mc_group_set_recorder(group._h, C.addressof(spec))), word)
            else:
                refused(lambda: group.set_recorder(**kw), word)
        spec = _abi.McRecorder(1, 0, 2, 18, 6, 0, 0, None)
        refused(lambda: _abi.check(group._lib, group._lib.ceg_mc_group_set_recorder(group._h, C.addressof(spec))), "missing")
        refused(lambda: group.recorder_rebase([np.nan] * K), "finite")
        refused(lambda: group.recorder_minimum(), "track_min")
        refused(lambda: group.recorder_read(1, 1), "window")
        sweep = dict(temperature=RAMP[:3], p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        # case 11: three frames due, room for two
        refused(lambda: group.sweep_cycles(3, L, SEED + 1409, FIRST, **sweep), "frames")
        assert group.recorder_read()[0].shape == (0, K)
        # the earlier recorder works: a snapshot, a call of one cycle, then the store is full
        group.snapshot()
        group.sweep_cycles(1, L, SEED + 1409, FIRST, temperature=RAMP[:1], p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        records, _frames = group.recorder_read()
        assert records.shape == (2, K) and list(records["cycle"][:, 0]) == [-1, 1] and records["energy"][0].tobytes() == E0.tobytes()
        start = [_state_bytes(d) for d in devs]
        refused(lambda: group.snapshot(), "full")
        refused(lambda: group.sweep_cycles(1, L, SEED + 1409, FIRST + L, cycle0=2, temperature=RAMP[:1], p_rotation=0.5, stream_id=SID, **STEP_SIZES), "frames")
        # a call with no frame due (origin beyond it would be another recorder; here: the plain sweep ignores the recorder) still runs
        group.sweep(L, SEED + 1409, FIRST + L, temperature=RAMP[0], p_rotation=0.5, stream_id=SID, **STEP_SIZES)
        assert group.recorder_read()[0].shape == (2, K)
        # track_min under swaps
        start = [_state_bytes(d) for d in devs]
        group.set_recorder(0, capacity=0, track_min=True, max_molecules=16)
        earlier = dict(group.recorder)
        swaps = group.gcmc_species([SWAP_HEAVY], [GCMC_CASE[0]])
        refused(lambda: group.sweep_gcmc_cycles(2, L, SEED, 0, temperature=np.full(K, 300.0), dmax=0.5, thetamax=1.0, species=swaps, max_molecules=16,
                                                stream_id=SID, positions=False), "swap")
        mink, mine, _r, _b = group.recorder_minimum()
        assert (mink == -1).all() and np.isfinite(mine).all()
        group.set_recorder(None)
        with pytest.raises(RuntimeError):
            group.snapshot()
        with pytest.raises(_abi.CegError) as e:
            _abi.check(group._lib, group._lib.ceg_mc_group_snapshot(group._h))
        assert e.value.code == -1
    _close(devs)


def test_a_poisoned_member_is_refused(cha, monkeypatch):
    """case 10: a member marked inconsistent by a failed ceg_mc_accept (the test hook of the library: no kernel is launched on bad data)
    makes ceg_mc_group_snapshot, ceg_mc_group_set_recorder with track_min and a *_cycles call fail with CEG_ERR_HIP and the chain's
    index; frames, store, minimum and the other chains' states stay as they were, and after ceg_mc_set_guests on the member the
    earlier recorder takes its next frame"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    k = 3
    devs = _chains(cha, [None] * k)
    with DeviceMonteCarloGroup(devs) as group:
        E0 = _energies(group)
        group.set_recorder(1, capacity=3, energies=E0, track_min=True)
        earlier = dict(group.recorder)
        group.snapshot()

        def store():
            records, frames = group.recorder_read()
            mink, mine, mrec, bodies = group.recorder_minimum()
            flat = [a.tobytes() for row in frames for body in row for a in body] + [a.tobytes() for body in bodies for a in body]
            return records.tobytes(), mink.tobytes(), mine.tobytes(), mrec.tobytes(), flat

        before = store()
        states = {c: _state_bytes(devs[c]) for c in (0, 2)}
        monkeypatch.setenv("CEG_HIP_MC_INJECT_FAILURE", "accept")
        with pytest.raises(_abi.CegError) as e:
            devs[1].accept((0, 0), devs[1].mc.positions[0][0] + 0.1)
        assert e.value.code == -3
        monkeypatch.delenv("CEG_HIP_MC_INJECT_FAILURE")
        sweep = dict(temperature=[300.0, 500.0, 900.0], dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=[3, 10, 17])
        for name, call in (("snapshot", lambda: group.snapshot()),
                           ("set_recorder", lambda: group.set_recorder(1, capacity=5, energies=E0, track_min=True)),
                           ("sweep_cycles", lambda: group.sweep_cycles(1, L, SEED + 1410, FIRST, **sweep))):
            with pytest.raises(_abi.CegError) as e:
                call()
            assert e.value.code == -3 and "chain 1" in str(e.value), (name, str(e.value))
            assert group.recorder == earlier and store() == before, name
            assert {c: _state_bytes(devs[c]) for c in (0, 2)} == states, name
        devs[1].refresh()
        group.snapshot()
        group.sweep_cycles(1, L, SEED + 1410, FIRST, **sweep)
        records, frames = group.recorder_read()
        assert records.shape == (3, k) and list(records["cycle"][:, 1]) == [-1, -1, 1] and records[:2].tobytes() == before[0] * 2
        for c in range(k):
            _same_frame(frames[1][c], frames[0][c], True, ("after refresh", c))
            _same_frame(frames[2][c], _frame_of(devs[c]), False, ("the next cycle", c))
    _close(devs)
