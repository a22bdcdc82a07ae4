"""The chain plan of a group (ceg_mc_group_set_chain_plan): one phiPV_div_k per chain in the swap rules of the GCMC sweeps and a last
step per chain in all four sweep entry points -- what make_isotherm (parameterinputs.jl:305-334) varies between its chains -- and
DeviceMonteCarloGroup.make_isotherm composed from them.  Against the oracle replay of test_gpu_mc_sweep_gcmc, against the same chain
swept alone, and against the sweeps without a plan, byte for byte.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import math
from unittest import mock

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_sweep import SEED, _chains, _close, _device_order, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES, Replay, _clone, _distinct_states, _follow, _tail
from test_gpu_mc_sweep_gcmc_blocks import masks  # noqa: F401  (the module's fixture)
from test_gpu_mc_sampler import GCMC_CASE, SWAP_HEAVY, _check_counts, _host_bins, _kinds, _new_chains, _start, _state_bytes, cha  # noqa: F401

pytestmark = pytest.mark.gpu

K = 4
NEVER = 2 ** 62
SID = np.arange(K, dtype=np.uint32) * 5 + 2
TEMPS = np.linspace(100.0, 1000.0, K)


class PlanReplay(Replay):
    """Replay whose table carries its own chain's phiPV_div_k; counts the swaps whose decision under that value differs from the
    decision under `shared`, the single value of the group's species table (the last swap_rule call of a step is its decision)."""

    def __init__(self, *args, shared):
        super().__init__(*args)
        self.shared, self.plan_flips = float(shared), 0

    def step(self, seed, step, sid, rec=None, what=None):
        calls, rule = [], mcrng.swap_rule
        with mock.patch.object(mcrng, "swap_rule", lambda *a: (calls.append(a), rule(*a))[1]):
            super().step(seed, step, sid, rec, what)
        if calls:
            row, u, T, n, _phi, sr, tc, ins = calls[-1]
            self.plan_flips += rule(row, u, T, n, float(self.table["phiPV_div_k"][0]), sr, tc, ins) != rule(row, u, T, n, self.shared, sr, tc, ins)


def _own(table, phi):
    t = table.copy()
    t["phiPV_div_k"][:] = phi
    return t


def _whole(rep):
    rep.tab = [[i, j] for i, kind in enumerate(rep.omc.positions) for j in range(len(kind))]
    return rep


def test_pressures_per_chain_against_the_oracle(setup):
    """4 chains in states of their own, 150 steps, Na: translation + random_translation, CO2: all six kinds with a swap share of 0.4,
    the tail correction of _tail; phiPV_div_k[c] = base * (1, 10, 100, 1000) in the plan, `base` in the species table.  The candidate
    (base, step sizes, seed) is the first whose PREDICTED run (mcrng + the oracle, every chain under its own value) holds accepted and
    rejected insertions and deletions and a swap that the table's value would have decided the other way.  Every record, the
    statistics and the final state against each chain's Replay with its own value; the flips counted again from the real log."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S = 150
    devs, omcs = _chains(setup, K, oracle=True)
    _distinct_states(devs, omcs)
    first = 2 ** 32 - 70
    caps = [12] * K
    decades = 10.0 ** np.arange(K)
    assert decades[-1] / decades[0] == 1e3

    def replays(os_, table, dmax, thetamax):
        return [PlanReplay(d.mc, o, _device_order(d), _own(table, table["phiPV_div_k"][1] * decades[c]), TEMPS[c], dmax, thetamax, caps[c],
                           shared=table["phiPV_div_k"][1]) for c, (d, o) in enumerate(zip(devs, os_))]

    with DeviceMonteCarloGroup(devs) as group:
        chosen = None
        for base, dmax, thetamax, seed in ((300.0, 0.5, 1.0, SEED + 100), (30.0, 1.0, 2.0, SEED + 101), (3000.0, 0.25, 0.5, SEED + 102),
                                           (100.0, 0.5, 1.0, SEED + 103), (1000.0, 0.5, 1.0, SEED + 104), (10.0, 0.5, 1.0, SEED + 105)):
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [base, base]))
            pred = replays([_clone(o) for o in omcs], table, dmax, thetamax)
            for s in range(S):
                for c, rep in enumerate(pred):
                    rep.step(seed, first + s, int(SID[c]))
            seen = set().union(*[rep.seen for rep in pred])
            flips = sum(rep.plan_flips for rep in pred)
            print(f"candidate base {base}, dmax {dmax}, thetamax {thetamax}: predicted swaps {sorted(x for x in seen if x[0] >= 5)}, flips {flips}")
            if {(5, True), (5, False), (6, True), (6, False)} <= seen and flips > 0:
                chosen = (dmax, thetamax, seed, table)
                break
        assert chosen is not None, "no candidate holds accepted and rejected swaps and a flipped decision on the oracle"
        dmax, thetamax, seed, table = chosen
        phi = np.outer(decades, table["phiPV_div_k"])
        group.set_chain_plan(phi)
        stats, log = group.sweep_gcmc(S, seed, first, temperature=TEMPS, dmax=dmax, thetamax=thetamax, species=table, max_molecules=caps,
                                      stream_id=SID, log=True)
    reps = [_whole(rep) for rep in replays(omcs, table, dmax, thetamax)]
    _follow(reps, log, seed, first, SID)
    exempt = sum(rep.exempt for rep in reps)
    assert exempt <= 0.01 * S * K, exempt
    seen = set().union(*[rep.seen for rep in reps])
    assert {(5, True), (5, False), (6, True), (6, False)} <= seen, seen
    flips = [rep.plan_flips for rep in reps]
    print(f"per-chain phiPV_div_k {phi[:, 1].tolist()}: exempt {exempt}, swaps decided otherwise than under the table's value, per chain: {flips}")
    assert flips[0] == 0 and sum(flips) > 0, flips                  # (chain 0 carries the table's value)
    for c, rep in enumerate(reps):
        rep.check_stats(stats[c], c)
        rep.check_state(devs[c], c)
    _close(devs)


def _gcmc_kw(table, chains=slice(None), **more):
    return dict(temperature=TEMPS[chains], dmax=0.4, thetamax=0.8, species=table, max_molecules=[10] * len(SID[chains]), stream_id=SID[chains], log=True, **more)


def test_a_member_equals_the_chain_alone_byte_for_byte(setup):
    """Every chain of a group of 4 against a one-chain group around an identical fresh chain (same stream id, seed, steps): log,
    statistics and ceg_mc_get_state as bytes -- first with no plan and one table (the property the comparison rests on), then with
    per-chain values in the plan against a table carrying the chain's own."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S, seed, first = 60, SEED + 110, 11
    base = 3000.0
    own = base * 10.0 ** np.array([-100.0, -3.0, 0.0, 100.0])       # (the ends: no insertion / no deletion is accepted, unlike at `base`)
    logs = []
    for planned in (False, True):
        devs, _ = _chains(setup, K)
        with DeviceMonteCarloGroup(devs) as group:
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [base, base]))
            if planned:
                group.set_chain_plan(np.stack([own, own], axis=1))
            stats, log = group.sweep_gcmc(S, seed, first, **_gcmc_kw(table))
        states = [_state_bytes(d) for d in devs]
        _close(devs)
        assert ((log["accepted"] != 0) & (log["kind"] >= 5)).any(), "no accepted swap in the run"
        logs.append(log.tobytes())
        for c in range(K):
            solo, _ = _chains(setup, 1)
            with DeviceMonteCarloGroup(solo) as one:
                s1, l1 = one.sweep_gcmc(S, seed, first, **_gcmc_kw(_own(table, own[c]) if planned else table, slice(c, c + 1)))
            what = ("plan" if planned else "no plan", c)
            assert log[:, c].tobytes() == l1[:, 0].tobytes(), what
            assert stats[c].tobytes() == s1[0].tobytes(), what
            assert states[c] == _state_bytes(solo[0]), what
            _close(solo)
    assert logs[0] != logs[1], "no swap was decided otherwise than under the table's value"


@pytest.mark.parametrize("with_masks", [False, True])
def test_no_plan_a_cleared_plan_and_a_uniform_plan_give_the_same_bytes(setup, masks, with_masks):
    """A GCMC sweep with no plan ever installed, after set_chain_plan(None, None) following a real plan, and with every chain's value
    equal to the table's and no stops: log, statistics, states and block_counts identical; once more with the block masks installed."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S = 60
    runs = []
    for variant in ("never", "cleared", "uniform"):
        devs, _ = _chains(setup, K)
        with DeviceMonteCarloGroup(devs) as group:
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [5000.0, 5000.0]))
            if with_masks:
                group.set_blocks(*masks)
            if variant == "cleared":
                group.set_chain_plan(np.full((K, 2), 7.0), np.array([3, 0, NEVER, 40]))
                group.set_chain_plan(None, None)
                assert group.chain_plan is None
            elif variant == "uniform":
                group.set_chain_plan(np.full((K, 2), 5000.0))
            stats, log = group.sweep_gcmc(S, SEED + 120, 7, **_gcmc_kw(table))
            runs.append((stats.tobytes(), log.tobytes(), [_state_bytes(d) for d in devs], [x.tobytes() for x in group.block_counts()]))
            pocket = group.block_counts()[0]
        _close(devs)
    assert runs[0] == runs[1], "a cleared plan changed the sweep"
    assert runs[0] == runs[2], "a uniform plan changed the sweep"
    log = np.frombuffer(runs[0][1], dtype=_abi.GCMC_RECORD_DTYPE)
    assert ((log["accepted"] != 0) & (log["kind"] >= 5)).any() and (log["molecule"] > -2).all()
    assert bool(pocket.sum() > 0) == with_masks


def _stopped_record(dtype):
    rec = np.zeros((), dtype=dtype)
    rec["molecule"], rec["kind"] = -2, -1
    if "species" in dtype.names:
        rec["species"] = -1
    return rec.tobytes()


@pytest.mark.parametrize("gcmc", [False, True], ids=["plain", "gcmc"])
def test_stops(setup, gcmc):
    """S = 120, stop_step = first + (0, 37, 120, 2^62).  A chain stopped at t equals the same chain swept alone for t - first steps
    (state and statistics as bytes); its records from t on are the stopped record; the stopped chain continued without a plan from
    first_step = t over the remaining steps reaches the bytes of an unstopped clone, log included."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S, seed, first = 120, SEED + 130, 2 ** 32 - 50
    stop = first + np.array([0, 37, 120, NEVER - first], dtype=np.int64)
    ran = [0, 37, 120, 120]

    def sweep(group, nsteps, at, chains=slice(None)):
        if gcmc:
            table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [3000.0, 3000.0]))
            return group.sweep_gcmc(nsteps, seed, at, **_gcmc_kw(table, chains))
        return group.sweep(nsteps, seed, at, temperature=TEMPS[chains], dmax=0.5, thetamax=1.0, p_rotation=0.5, stream_id=SID[chains], log=True)

    a, _ = _chains(setup, K)
    b, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(a) as ga, DeviceMonteCarloGroup(b) as gb:
        ga.set_chain_plan(None, stop)
        sa, la = sweep(ga, S, first)
        sb, lb = sweep(gb, S, first)
    assert la.shape == (S, K) and (lb["molecule"] > -2).all() and (lb["accepted"] != 0).sum() > 0
    stopped = _stopped_record(la.dtype)
    for c in range(K):
        t = ran[c]
        assert la[:t, c].tobytes() == lb[:t, c].tobytes(), c
        assert la[t:, c].tobytes() == stopped * (S - t), c
        solo, _ = _chains(setup, 1)
        with DeviceMonteCarloGroup(solo) as one:
            s1, l1 = sweep(one, t, first, slice(c, c + 1))
        assert sa[c].tobytes() == s1[0].tobytes(), (c, sa[c], s1[0])
        assert _state_bytes(a[c]) == _state_bytes(solo[0]), c
        assert l1[:, 0].tobytes() == la[:t, c].tobytes(), c
        _close(solo)
        with DeviceMonteCarloGroup([a[c]]) as rest:                  # the stopped chain, continued without a plan
            s2, l2 = sweep(rest, S - t, first + t, slice(c, c + 1))
        assert np.concatenate([la[:t, c], l2[:, 0]]).tobytes() == lb[:, c].tobytes(), c
        assert _state_bytes(a[c]) == _state_bytes(b[c]), c
        for name in (("trials", "accepted", "blocked", "capacity", "spent") if gcmc else
                     ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted", "blocked")):
            assert np.array_equal(sa[c][name] + s2[0][name], sb[c][name]), (c, name)
    assert not any(sa[0][n].any() for n in (("trials", "accepted", "spent") if gcmc else ("translation_trials", "rotation_trials")))
    _close(b)
    _close(a)


def test_stops_with_cycles_and_a_sampler(cha):
    """sweep_gcmc_cycles over 4 cycles of 30 steps from step 10, stops at cycle 0 (step 10), at cycle 2 (step 70), mid-cycle (step
    57) and never; a pooled two-channel map and the series with a frame every 10 steps.  Cycle records before a chain's stop equal
    those of the chain run alone; from the cycle of the stop on the counters are frozen and the step sizes carried over; the map equals
    bin_positions over replay_positions of the log restricted to the frames each chain had not stopped at; K records per frame."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    mc, _owner = cha
    NC, L, first, every = 4, 30, 10, 10
    stop = np.array([first, first + 2 * L, first + 47, NEVER], dtype=np.int64)
    whole = [0, 2, 1, NC]                                            # whole cycles before the stop
    frames = mcrng.sampler_frames(first, NC * L, every)
    assert len(frames) == 12 and frames[-1] == first + NC * L - 1
    phi, seed = GCMC_CASE
    T = np.array([300.0, 800.0, 1200.0, 1000.0])
    kinds = _kinds(mc)
    counters = ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")

    def run(group, ncycles, chains=slice(None)):
        table = group.gcmc_species([SWAP_HEAVY], [phi])
        return group.sweep_gcmc_cycles(ncycles, L, seed, first, temperature=T[chains], dmax=0.5, thetamax=1.0, species=table,
                                       max_molecules=16, stream_id=SID[chains], log=True)

    devs = _new_chains(cha, K)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_chain_plan(None, stop)
        group.set_sampler(every, step=1.0, channels={"C_co2": 0, "O_co2": 1, "Na": -1}, chain_map=[0] * K, series_capacity=len(frames))
        samp = group.sampler
        starts = [_start(d) for d in devs]
        stats, rec, log = run(group, NC)
        bins, series, _total = group.sampler_read()
    assert rec.shape == (NC, K) and series.shape == (len(frames), K)
    states, binned = [], []
    for c, (spec, pos) in enumerate(starts):
        every_step = list(mcrng.replay_positions(pos, log[:, c], [len(k) for k in kinds], start_species=spec))
        states.append([every_step[s - first] for s in frames])
        binned.append([every_step[s - first] for s in frames if s < stop[c]])
    assert [len(x) for x in binned] == [0, 6, 4, 12]
    _check_counts(series, states, frames, 1, "stops")               # the frozen chains still give their records
    want = _host_bins(samp, binned, kinds)
    print(f"bins: {int(bins.sum())} counts, {int((bins != want).sum())} bins differ; all frames of all chains would be {int(_host_bins(samp, states, kinds).sum())}")
    assert np.array_equal(bins, want) and bins.sum() < _host_bins(samp, states, kinds).sum()
    for c in range(K):
        n = whole[c]
        if n > 0:
            solo = _new_chains(cha, 1)
            with DeviceMonteCarloGroup(solo) as one:
                _s1, r1, _l1 = run(one, n, slice(c, c + 1))
            assert rec[:n, c].tobytes() == r1[:, 0].tobytes(), c
            _close(solo)
        for j in range(n, NC):                                       # the cycle that holds the stop and every later one
            assert rec[j, c]["dmax_next"] == rec[j, c]["dmax"] and rec[j, c]["thetamax_next"] == rec[j, c]["thetamax"], (c, j)
            assert rec[j, c]["dmax"] == (rec[j - 1, c]["dmax_next"] if j else 0.5), (c, j)
            for name in counters + ("delta_moves", "delta_swaps", "nmol"):
                assert rec[j, c][name] == rec[NC - 1, c][name], (c, j, name)
        assert [rec[NC - 1, c][x] for x in counters] == [stats[c]["trials"][0], stats[c]["accepted"][0], stats[c]["trials"][1], stats[c]["accepted"][1]], c
        assert stats[c]["trials"].sum() + stats[c]["spent"] == min(int(stop[c]) - first, NC * L), c
    assert (rec[:, 3]["dmax_next"] != rec[:, 3]["dmax"]).any()        # the chain that never stops does adapt
    _close(devs)


def test_refusals(setup):
    """Refused before anything is launched or changed: a plan whose nspecies differs from the sweep's; 0, a negative value, NaN and Inf
    for a swapping species; a negative stop, which leaves the earlier plan installed.  Garbage in the entry of a species that does not
    swap is accepted.  The sweep after all of them gives the bytes of a group that never saw a refusal.  A plain sweep ignores a
    phiPV_div_k-only plan."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S, seed = 40, SEED + 150
    own = 3000.0 * 10.0 ** np.arange(K)
    stop = np.array([NEVER, 25, NEVER, 10], dtype=np.int64)
    ref, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(ref) as group:
        table = _tail(group.gcmc_species([NA_MOVES, CO2_MOVES], [1.0, 1.0]))
        group.set_chain_plan(np.stack([own, own], axis=1), stop)
        want = group.sweep_gcmc(S, seed, 0, **_gcmc_kw(table))
    want = (want[0].tobytes(), want[1].tobytes(), [_state_bytes(d) for d in ref])
    _close(ref)
    devs, _ = _chains(setup, K)
    with DeviceMonteCarloGroup(devs) as group:
        before = [_state_bytes(d) for d in devs]

        def refused(**kw):
            with pytest.raises(_abi.CegError) as ei:
                group.sweep_gcmc(S, seed, 0, **{**_gcmc_kw(table), **kw})
            assert ei.value.code == -1, ei.value
            assert [_state_bytes(d) for d in devs] == before

        group.set_chain_plan(np.ones((K, 3)))
        refused()
        for bad in (0.0, -5.0, float("nan"), float("inf")):
            phi = np.stack([own, own], axis=1)
            phi[2, 1] = bad
            group.set_chain_plan(phi, stop)
            refused()
            assert "chain 2" in (group._lib.ceg_last_error() or b"").decode()
        garbage = np.stack([np.array([float("nan"), -1.0, 0.0, float("inf")]), own], axis=1)          # Na does not swap: not read
        group.set_chain_plan(garbage, stop)
        with pytest.raises(_abi.CegError) as ei:
            group.set_chain_plan(np.ones((K, 2)), np.array([5, -1, 5, 5]))
        assert ei.value.code == -1
        lib, ones = group._lib, np.ones((K, 2))
        for plan in (_abi.McChainPlan(_abi.GCMC_MAX_SPECIES + 1, 0, None, None), _abi.McChainPlan(-1, 0, None, None), _abi.McChainPlan(0, 0, ones.ctypes.data, None)):
            assert lib.ceg_mc_group_set_chain_plan(group._h, C.addressof(plan)) == -1
        assert [_state_bytes(d) for d in devs] == before
        got = group.sweep_gcmc(S, seed, 0, **_gcmc_kw(table))        # the earlier plan -- garbage for Na, the stops -- is still the one installed
        assert (got[0].tobytes(), got[1].tobytes(), [_state_bytes(d) for d in devs]) == want
        assert (got[1]["molecule"][:, 1] == -2).sum() == S - 25 and (got[1]["molecule"][:, 3] == -2).sum() == S - 10
    _close(devs)
    runs = []
    for planned in (False, True):
        plain, _ = _chains(setup, 2)
        with DeviceMonteCarloGroup(plain) as group:
            if planned:
                group.set_chain_plan(np.array([[float("nan")] * 5, [-1.0] * 5]))
            st, lg = group.sweep(S, seed, 3, temperature=[300.0, 700.0], dmax=0.5, thetamax=1.0, p_rotation=0.5, log=True)
            runs.append((st.tobytes(), lg.tobytes(), [_state_bytes(d) for d in plain]))
        _close(plain)
    assert runs[0] == runs[1]


def test_make_isotherm_small(cha):
    """Three chains with ncycles = isotherm_ncycles(3, P) = 9, 6, 4 for P = 500, 1000, 1e5 Pa, ninit = 1, 10 steps per cycle: loadings and
    means equal the composition written out here from sweep_gcmc_cycles + plan + baseline_energies on clones; every drift check passes
    at rtol 1e-9; a chain's loadings and final state are those of the same chain run alone for its own length."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    pressures = (500.0, 1000.0, 1e5)
    n = np.array([mcrng.isotherm_ncycles(3, p) for p in pressures])
    assert n.tolist() == [9, 6, 4]
    L, ninit, seed, k, supercell = 10, 1, GCMC_CASE[1], 3, (1, 1, 2)
    phi = GCMC_CASE[0] * np.array([[0.3], [1.0], [10.0]])
    T, sid = np.array([300.0, 300.0, 300.0]), SID[:3]
    moves = [SWAP_HEAVY]
    kw = dict(temperature=T, max_molecules=16, moves=moves, seed=seed, steps_per_cycle=L, supercell=supercell, stream_id=sid)
    devs = _new_chains(cha, k)
    with DeviceMonteCarloGroup(devs) as group:
        group.set_sampler(5, series_capacity=1)
        with pytest.raises(RuntimeError):
            group.make_isotherm(phi, n, ninit, **kw)
        group.set_sampler(None)
        iso = group.make_isotherm(phi, n, ninit, **kw)
        assert group.sampler is None and group.chain_plan is None
    states = [_state_bytes(d) for d in devs]
    _close(devs)
    assert iso.drift_ok.all(), (iso.recorded, iso.actual)
    assert [len(x) for x in iso.loadings] == n.tolist() == [len(x) for x in iso.energies]
    # by hand, on clones
    devs = _new_chains(cha, k)
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species(moves, [phi[0, 0]])
        group.set_chain_plan(phi, (ninit + n) * L)
        group.set_sampler(L, from_step=ninit * L, series_capacity=int(n.max()))
        group.baseline_energies()
        common = dict(temperature=T, species=table, max_molecules=16, stream_id=sid)
        _s, c0 = group.sweep_gcmc_cycles(ninit, L, seed, 0, dmax=1.3, thetamax=math.radians(30.0), cycle0=1, **common)
        group.baseline_energies()
        prior = np.stack([c0[-1][x] for x in ("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")], axis=1)
        group.sweep_gcmc_cycles(int(n.max()), L, seed, ninit * L, dmax=c0[-1]["dmax_next"], thetamax=c0[-1]["thetamax_next"], cycle0=1 + ninit,
                                prior=prior, **common)
        series = group.sampler_read()[1]
    assert series.shape == (9, k)
    assert [_state_bytes(d) for d in devs] == states
    _close(devs)
    for c in range(k):
        hand = series["count"][:n[c], c, 0] / 2
        assert np.array_equal(iso.loadings[c], hand) and iso.isotherm[c] == hand.mean(), (c, iso.loadings[c], hand)
    assert len({tuple(x) for x in iso.loadings}) > 1 and any(x.max() != x.min() for x in iso.loadings)
    for c in range(k):                                               # the chain alone, for its own length
        solo = _new_chains(cha, 1)
        with DeviceMonteCarloGroup(solo) as one:
            alone = one.make_isotherm(phi[c:c + 1], n[c:c + 1], ninit, **{**kw, "temperature": T[c:c + 1], "stream_id": sid[c:c + 1]})
        assert np.array_equal(alone.loadings[0], iso.loadings[c]) and alone.energies[0].tobytes() == iso.energies[c].tobytes(), c
        assert _state_bytes(solo[0]) == states[c], c
        assert alone.recorded[0] == iso.recorded[c] and alone.actual[0] == iso.actual[c], c
        _close(solo)
