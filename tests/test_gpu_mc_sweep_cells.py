"""Device cells (ceg_mc_group_set_device_cells): the plain and the GCMC sweeps on chains that keep their guests in neighbour cells, the
cell lists kept on the device during a sweep.  The yardstick is the host-driven route on identical clones -- group.trial + group.accept at the logged
placements, where the host's CellMirror works out the cell operations -- which must give the same rows (the pair sum bit for bit: its
order is the order of the entries of the cells), the same final bytes and the same cell lists; further ceg_hip.mcrng (proposals, and
CellBook for the lists) and the oracle's state.  The logged placements agree with mcrng.propose to 1e-12 A as in test_gpu_mc_sweep.py,
so the clones are driven with the logged ones.  Cells are forced on with CEG_HIP_MC_CELLS=1 on the Na + 4 CO2 CIT-7 fixture of the
sweep tests.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_chains import _check
from test_gpu_mc_sweep import SEED, _close, _copy, _device_order, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc_blocks import masks  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

KW = dict(temperature=700.0, dmax=1.0, thetamax=2.0, p_rotation=0.5)


def _make(setup, monkeypatch, bins, positions=None, oracle=False):
    """one chain per entry of `bins`: None without cells, else the bin width in A (CEG_HIP_MC_BIN) with cells forced on"""
    from ceg_hip.energy import DeviceMonteCarlo
    from oracle.montecarlo import OracleMonteCarlo
    mc, owner = setup
    devs, omcs = [], []
    for b in bins:
        if b is not None:
            monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
            monkeypatch.setenv("CEG_HIP_MC_BIN", str(b))
        devs.append(DeviceMonteCarlo(_copy(mc, positions), grids_from=owner))
        monkeypatch.delenv("CEG_HIP_MC_CELLS", raising=False)
        monkeypatch.delenv("CEG_HIP_MC_BIN", raising=False)
        assert (devs[-1].neighbour_cells() is not None) == (b is not None)
        if oracle:
            omc = OracleMonteCarlo.from_setup(devs[-1].mc)
            omc.compute_ewald()
            omcs.append(omc)
    return (devs, omcs) if oracle else devs


def _layout(dev):
    """device molecule order -> (kind, index), atoms per molecule, first atom slot per molecule (no swap has happened: slots are packed)"""
    order = _device_order(dev)
    sizes = [len(dev.mc.ffidx[i]) for i, _j in order]
    return order, sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)


def _book(dev):
    """mcrng.CellBook of a chain's present state"""
    nb, _cap = dev.neighbour_cells()
    return mcrng.CellBook(dev.mc.invmat, nb).set_atoms(dev.state()[0])


def _bytes(dev):
    pos, sf = dev.state()
    return pos.tobytes() + sf.tobytes()


def _follow(group, log, layouts, omcs=None):
    """drive the clones' group through the log of a sweep on the host route: per step one group.trial at the logged placements --
    columns 0, 2, 3 of both rows bit for bit, column 1 to 1e-12 relative (the header's statement for the group rows) -- and one
    group.accept of the accepted ones"""
    S, K = log.shape
    for s in range(S):
        moves, acc = [], []
        for c in range(K):
            rec = log[s, c]
            if rec["molecule"] < 0:
                moves.append(None)
                acc.append(None)
                continue
            order, sizes, _first = layouts[c]
            placed = rec["positions"][:sizes[rec["molecule"]]].copy()
            moves.append(("move", order[rec["molecule"]], placed[None]))
            acc.append((order[rec["molecule"]], placed) if rec["accepted"] else None)
        rows = group.trial(moves)
        for c in range(K):
            if moves[c] is None:
                continue
            for col in (0, 2, 3):
                assert np.array_equal(rows[c][:, col], log[s, c]["rows"][:, col]), (s, c, col, rows[c], log[s, c]["rows"])
            np.testing.assert_allclose(rows[c][:, 1], log[s, c]["rows"][:, 1], rtol=1e-12, atol=0.0)
            if omcs is not None and acc[c] is not None:
                omcs[c].update(*acc[c])
        if any(a is not None for a in acc):
            group.accept(acc)


def _same_lists(a, b):
    la, lb = a.cell_lists(), b.cell_lists()
    if la is None or lb is None:
        return la is None and lb is None
    return np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and a.neighbour_cells() == b.neighbour_cells()


BINS = (4, 4, 1.0, None)          # two chains with 4 A bins, one with 1 A bins (the atoms of a molecule in different cells), one without cells


def test_plain_sweep_against_the_host_route(setup, monkeypatch):
    """60 steps of 4 chains.  Every record against mcrng.propose (molecule, kind, u exactly; placement to 1e-12 A); the statistics
    against the log; rows, final bytes and cell lists against clones on the host route; cell_lists() against the CellBook replay of
    the log; the rows of a following trial against the clones' bit for bit and against the oracle; at least 10 accepted moves change
    a cell."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S, first = len(BINS), 60, 2 ** 32 - 20
    devs = _make(setup, monkeypatch, BINS)
    clones, omcs = _make(setup, monkeypatch, BINS, oracle=True)
    layouts = [_layout(d) for d in devs]
    books = [_book(d) if b is not None else None for d, b in zip(devs, BINS)]
    beads = [[mcrng.default_beads(d.mc)[i] for i, _j in lay[0]] for d, lay in zip(devs, layouts)]
    sid = np.array([5, 2, 11, 7], dtype=np.uint32)
    starts = [d.state()[0].copy() for d in devs]
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(clones) as twin:
        group.device_cells()
        stats, log = group.sweep(S, SEED, first, stream_id=sid, log=True, **KW)
        assert (group.halted() == -1).all()
        count = np.zeros((K, 4), dtype=np.int64)
        _follow(twin, log, layouts, omcs)
        crossing = 0
        for c in range(K):
            order, sizes, firsts = layouts[c]
            mols = [np.array(p) for p in np.split(starts[c], np.cumsum(sizes)[:-1])]
            for s in range(S):
                rec = log[s, c]
                pr = mcrng.propose(SEED, first + s, int(sid[c]), mols, KW["dmax"], KW["thetamax"], KW["p_rotation"], beads[c])
                assert (rec["molecule"], rec["kind"], rec["u"]) == (pr.molecule, pr.kind, pr.u), (s, c)
                placed = rec["positions"][:sizes[pr.molecule]]
                assert np.abs(placed - pr.positions).max() <= 1e-12, (s, c)
                count[c, 2 * pr.kind] += 1
                count[c, 2 * pr.kind + 1] += rec["accepted"]
                if rec["accepted"]:
                    mols[pr.molecule] = placed.copy()
                    if books[c] is not None:
                        crossing += books[c].move(int(firsts[pr.molecule]), placed) > 0
            st = stats[c]
            assert [st["translation_trials"], st["translation_accepted"], st["rotation_trials"], st["rotation_accepted"]] == list(count[c]), c
            assert _bytes(devs[c]) == _bytes(clones[c]), c
            assert np.array_equal(devs[c].state()[0], np.concatenate(mols)), c
            assert _same_lists(devs[c], clones[c]), c
            if books[c] is not None:
                lists = devs[c].cell_lists()
                want = books[c].lists(len(lists[0]))
                assert np.array_equal(lists[0], want[0]) and np.array_equal(lists[1], want[1]), c
            else:
                assert devs[c].cell_lists() is None
        print(f"plain sweep with device cells: accepted {int(count[:, 1].sum() + count[:, 3].sum())} of {S * K}, {crossing} of them change a cell")
        assert crossing >= 10, crossing
        # a following trial of every chain: the clones' rows bit for bit, the oracle's to 1e-9
        moves = [("move", lay[0][1], np.empty((0, lay[1][1], 3))) for lay in layouts]
        got, want = group.trial(moves), twin.trial(moves)
        for c in range(K):
            assert got[c].tobytes() == want[c].tobytes(), c
            _check(got[c][0], omcs[c].movement_energy(layouts[c][0][1]), (c, "after the sweep"))
    _close(clones)
    _close(devs)


def test_a_member_gets_the_bytes_it_gets_alone(setup, monkeypatch):
    """the chain with 1 A bins in a mixed group of 5 against the same chain in a group of its own: log, statistics, state, lists"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S = 40
    five = _make(setup, monkeypatch, (None, 4, 1.0, None, 4))
    alone = _make(setup, monkeypatch, (1.0,))
    sid = np.array([1, 2, 3, 4, 5], dtype=np.uint32)
    T = np.array([300.0, 500.0, 700.0, 900.0, 400.0])
    kw = dict(dmax=1.0, thetamax=2.0, p_rotation=0.5, log=True)
    with DeviceMonteCarloGroup(five) as g5, DeviceMonteCarloGroup(alone) as g1:
        g5.device_cells()
        g1.device_cells()
        s5, l5 = g5.sweep(S, SEED + 2, 7, temperature=T, stream_id=sid, **kw)
        s1, l1 = g1.sweep(S, SEED + 2, 7, temperature=T[2:3], stream_id=sid[2:3], **kw)
        assert l5[:, 2].tobytes() == l1[:, 0].tobytes() and s5[2:3].tobytes() == s1.tobytes()
        assert _bytes(five[2]) == _bytes(alone[0]) and _same_lists(five[2], alone[0])
        assert s1[0]["translation_accepted"] + s1[0]["rotation_accepted"] > 0
    _close(alone)
    _close(five)


def test_device_cells_are_opt_in(setup, monkeypatch):
    """Without device_cells(), and after device_cells(False), all four sweep entry points refuse the chain with cells (-5, naming it)
    and leave the states alone; device_cells() on a group without a cells chain changes no byte;
    host-driven accepts between two sweeps are picked up by the second."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES
    good = dict(temperature=300.0, dmax=0.5, thetamax=1.0)
    devs = _make(setup, monkeypatch, (None, 4))
    with DeviceMonteCarloGroup(devs) as group:
        table = group.gcmc_species([NA_MOVES, CO2_MOVES], [3e5, 3e5])
        plain_calls = (lambda: group.sweep(5, SEED, 0, **good), lambda: group.sweep_cycles(2, 3, SEED, 0, **good))
        gcmc_calls = (lambda: group.sweep_gcmc(5, SEED, 0, species=table, max_molecules=12, **good),
                      lambda: group.sweep_gcmc_cycles(2, 3, SEED, 0, species=table, max_molecules=12, **good))
        before = [_bytes(d) for d in devs]
        lists = devs[1].cell_lists()

        def refused(calls):
            for call in calls:
                with pytest.raises(_abi.CegError) as e:
                    call()
                assert e.value.code == -5 and "chain 1" in str(e.value) and "neighbour cells" in str(e.value)
                assert [_bytes(d) for d in devs] == before
                assert np.array_equal(devs[1].cell_lists()[0], lists[0]) and np.array_equal(devs[1].cell_lists()[1], lists[1])

        refused(plain_calls + gcmc_calls)
        group.device_cells()
        group.device_cells(False)
        refused(plain_calls + gcmc_calls)
        assert (group.halted() == -1).all()
    _close(devs)
    # no chain with cells: a no-op
    a, b = _make(setup, monkeypatch, (None, None)), _make(setup, monkeypatch, (None, None))
    with DeviceMonteCarloGroup(a) as ga, DeviceMonteCarloGroup(b) as gb:
        gb.device_cells(capacity=32)
        sa, la = ga.sweep(30, SEED + 3, 0, log=True, **KW)
        sb, lb = gb.sweep(30, SEED + 3, 0, log=True, **KW)
        assert la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes() and [_bytes(d) for d in a] == [_bytes(d) for d in b]
        assert (gb.halted() == -1).all() and b[0].cell_lists() is None
    _close(b)
    _close(a)
    # host-driven accepts between two sweeps
    devs, clones = _make(setup, monkeypatch, (1.0, 4)), _make(setup, monkeypatch, (1.0, 4))
    layouts = [_layout(d) for d in devs]
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(clones) as twin:
        group.device_cells()
        _s, log = group.sweep(20, SEED + 4, 0, log=True, **KW)
        _follow(twin, log, layouts)
        for d, t in zip(devs, clones):                                # one molecule each moved by the host, across cells
            new = d.state()[0][1:4] + np.array([2.5, -1.5, 3.0])
            d.accept((1, 0), new)
            t.accept((1, 0), new)
        far = devs[0].state()[0][4:7] + np.array([-6.0, 4.0, 5.0])
        group.accept([((1, 1), far), None])
        twin.accept([((1, 1), far), None])
        assert all(_same_lists(d, t) for d, t in zip(devs, clones))
        _s, log = group.sweep(20, SEED + 4, 20, log=True, **KW)
        _follow(twin, log, layouts)
        for c, (d, t) in enumerate(zip(devs, clones)):
            assert _bytes(d) == _bytes(t) and _same_lists(d, t), c
        assert log["accepted"].sum() > 0
    _close(clones)
    _close(devs)


# ---- halting: a full cell.  12 A bins (few cells, capacity 8).  The chains are staged by host-driven accepts so that the cell of the Na
# holds exactly 8 atoms: the Na, two CO2 wholly inside and one CO2 with a single atom inside.  At 1e9 K every proposal outside the
# framework's hard core is accepted, so the next atom to enter that cell overfills it.
HOT = dict(temperature=1e9, dmax=1.5, thetamax=3.0, p_rotation=0.5)
HALT_STEPS = 40
HALT_SID = 5                      # the stream whose chain halts well inside the sweep (chosen on the host route's replay, asserted below)


def _stage(devs, seed=7):
    """fill the Na's cell of every chain (identical chains) to its capacity of 8; -> the cell"""
    dev = devs[0]
    nb, cap = dev.neighbour_cells()
    assert cap == 8, (nb, cap)
    book = _book(dev)
    mat = np.asarray(dev.mc.mat, dtype=np.float64)
    pos = dev.state()[0]
    target = book.bin_of(pos[0])
    b = np.array([target // (nb[1] * nb[2]), (target // nb[2]) % nb[1], target % nb[2]])
    rng = np.random.default_rng(seed)
    now = {-1: pos[0:1]}
    now.update({j: pos[1 + 3 * j:4 + 3 * j] for j in range(4)})
    # every CO2 out of the target cell first, then CO2 0 and 1 wholly into it and CO2 2 with one atom: the cell never holds more than 8
    for j, inside in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 3), (1, 3), (2, 1)):
        cur = now[j]
        if inside == 0 and not any(book.bin_of(a) == target for a in cur):
            continue
        centres = (mat @ ((b[:, None] + rng.uniform(-0.3, 1.3, (3, 400))) / np.array(nb)[:, None])).T
        cands = np.array([cur - cur[1] + c for c in centres])
        others = np.concatenate([p for q, p in now.items() if q != j])
        keep = [t for t, p in enumerate(cands)
                if sum(book.bin_of(a) == target for a in p) == inside and np.linalg.norm(p[:, None] - others[None], axis=2).min() > 3.0]
        assert keep, (j, inside)
        rows = dev.trial((1, j), cands[keep])
        free = [t for t, r in zip(keep, rows[1:]) if np.isfinite(r).all() and r[0] < 1e90]
        assert free, (j, inside)
        now[j] = cands[free[0]]
        for d in devs:
            d.accept((1, j), now[j])
    for d in devs:
        assert d.neighbour_cells() == (nb, 8) and (d.cell_lists()[0] == target).sum() == 8
    return target


def _halting_run(setup, monkeypatch, sids):
    """small: chains with capacity 8 swept HALT_STEPS steps; big: the same with capacity 32 from the start; clones: the host route
    driven with big's log, watched for the step at which a chain's capacity grows -> per chain (halted step, step the host grew at)
    after all the assertions of the halting test on that chain"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K, S, first = len(sids), HALT_STEPS, 1000
    small, big, clones = (_make(setup, monkeypatch, (12,) * K) for _ in range(3))
    _stage(small + big + clones)
    layouts = [_layout(d) for d in small]
    sid = np.asarray(sids, dtype=np.uint32)
    out = []
    with DeviceMonteCarloGroup(small) as gs, DeviceMonteCarloGroup(big) as gb, DeviceMonteCarloGroup(clones) as gc:
        gb.device_cells(capacity=32)
        assert all(d.neighbour_cells()[1] == 32 for d in big)
        sb, lb = gb.sweep(S, SEED + 5, first, stream_id=sid, log=True, **HOT)
        assert (gb.halted() == -1).all()
        # the host route, step by step; before[c]: bytes and lists of clone c before the step at which its capacity grew
        grew, before = [-1] * K, [None] * K
        for s in range(S):
            snap = [(_bytes(d), d.cell_lists()) for d in clones]
            _follow(gc, lb[s:s + 1], layouts)
            for c, d in enumerate(clones):
                if grew[c] < 0 and d.neighbour_cells()[1] > 8:
                    grew[c], before[c] = s, snap[c]
        gs.device_cells()
        ss, ls = gs.sweep(S, SEED + 5, first, stream_id=sid, log=True, **HOT)
        halted = gs.halted()
        print("halting: host route grew at", grew, "device halted at", (halted - first).tolist())
        for c in range(K):
            h = grew[c]
            assert halted[c] == (first + h if h >= 0 else -1), (c, halted[c], h)
            if h < 0:
                assert ls[:, c].tobytes() == lb[:, c].tobytes() and _bytes(small[c]) == _bytes(big[c])
                continue
            assert ls[:h, c].tobytes() == lb[:h, c].tobytes()
            assert (ls["molecule"][h:, c] == -2).all() and (ls["kind"][h:, c] == -1).all() and not ls["accepted"][h:, c].any()
            assert not ls["rows"][h:, c].any() and not ls["positions"][h:, c].any()
            assert ss[c]["translation_trials"] + ss[c]["rotation_trials"] == h
            assert ss[c]["translation_accepted"] + ss[c]["rotation_accepted"] == ls["accepted"][:h, c].sum()
            assert _bytes(small[c]) == before[c][0]
            lists = small[c].cell_lists()
            assert np.array_equal(lists[0], before[c][1][0]) and np.array_equal(lists[1], before[c][1][1]) and small[c].neighbour_cells()[1] == 8
        # a larger capacity, and on from the halted steps: chain c sits out the steps before its own (a chain plan's stop would do the
        # same from the other end), one call per distinct halted step
        gs.device_cells(capacity=32)
        assert all(d.neighbour_cells()[1] == 32 for d in small)
        full = ls.copy()
        for h in sorted({g for g in grew if g >= 0}):
            members = [c for c in range(K) if grew[c] == h]
            idle = np.array([first + S if c not in members else 0 for c in range(K)])
            # (chains that are not continued in this call are stopped from its first step on)
            gs.set_chain_plan(None, np.where(idle > 0, 0, first + S))
            s2, l2 = gs.sweep(S - h, SEED + 5, first + h, stream_id=sid, log=True, **HOT)
            assert (gs.halted() == -1).all()
            for c in members:
                full[h:, c] = l2[:, c]
                assert s2[c]["translation_trials"] + s2[c]["rotation_trials"] + ss[c]["translation_trials"] + ss[c]["rotation_trials"] == S
        gs.set_chain_plan(None, None)
        for c in range(K):
            assert full[:, c].tobytes() == lb[:, c].tobytes(), c
            assert _bytes(small[c]) == _bytes(big[c]) and _bytes(small[c]) == _bytes(clones[c]), c
            la, lb_ = small[c].cell_lists(), big[c].cell_lists()
            assert np.array_equal(la[0], lb_[0]) and np.array_equal(la[1], lb_[1]), c
            out.append((int(halted[c]) - first if halted[c] >= 0 else -1, grew[c]))
    _close(clones)
    _close(big)
    _close(small)
    return out


def test_a_full_cell_halts_the_chain_and_the_run_continues(setup, monkeypatch):
    """The host route on a clone first: the step at which its capacity grows lies at least 5 steps from either end of the sweep.  The
    device sweep halts exactly there: halted() names the step, state, lists and counts are the clone's before that step, the later
    records carry molecule = -2, the statistics count the steps before it.  With device_cells(capacity=32) and a continuation from the
    halted step, the final bytes, the lists and the concatenated log are those of a group that had the capacity from the start."""
    (halted, grew), = _halting_run(setup, monkeypatch, [HALT_SID])
    assert halted == grew and 5 <= halted <= HALT_STEPS - 6, (halted, grew)


def _oracles(devs):
    from oracle.montecarlo import OracleMonteCarlo
    out = []
    for d in devs:
        omc = OracleMonteCarlo.from_setup(d.mc)
        omc.compute_ewald()
        out.append(omc)
    return out


def test_cycles_on_chains_with_cells(setup, monkeypatch):
    """sweep_cycles over 3 cycles equals three one-cycle calls whose step sizes come from mcrng.adapt_*: logs, cycle records, final
    bytes and cell lists, byte for byte; the oracle's baseline_energy of the final state to 1e-9."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_baseline import _check_record, _reference
    bins, L, NC = (4, 1.0), 7, 3
    K = len(bins)
    a, b = _make(setup, monkeypatch, bins), _make(setup, monkeypatch, bins)
    omcs = _oracles(a)
    layouts = [_layout(d) for d in a]
    T = np.array([500.0, 900.0])
    with DeviceMonteCarloGroup(a) as ga, DeviceMonteCarloGroup(b) as gb:
        ga.device_cells()
        gb.device_cells()
        sa, ca, la = ga.sweep_cycles(NC, L, SEED + 6, 0, temperature=T, dmax=0.8, thetamax=1.5, log=True)
        dm, th, prior = np.full(K, 0.8), np.full(K, 1.5), np.zeros((K, 4), dtype=np.int64)
        running = np.zeros(K)
        for j in range(NC):
            _s, c1, l1 = gb.sweep_cycles(1, L, SEED + 6, j * L, temperature=T, dmax=dm, thetamax=th, cycle0=1 + j, prior=prior, log=True)
            assert l1.tobytes() == la[j * L:(j + 1) * L].tobytes(), j
            for name in ca.dtype.names:                          # (the energy sum runs on through the cycles of one call: compared below)
                assert name == "delta_moves" or c1[0][name].tobytes() == ca[j][name].tobytes(), (j, name)
            running += c1[0]["delta_moves"]
            scale = max(1.0, float(np.abs(la["rows"][:(j + 1) * L]).clip(max=1e90).max()))
            assert np.abs(ca[j]["delta_moves"] - running).max() <= 1e-12 * scale * (j + 1) * L, j
            for c in range(K):
                rec = c1[0, c]
                prior[c] = [rec["translation_trials"], rec["translation_accepted"], rec["rotation_trials"], rec["rotation_accepted"]]
                dm[c] = mcrng.adapt_dmax(dm[c], int(prior[c, 1]), int(prior[c, 0]), 1 + j)
                th[c] = mcrng.adapt_thetamax(th[c], int(prior[c, 3]), int(prior[c, 2]), 1 + j)
                assert (dm[c], th[c]) == (rec["dmax_next"], rec["thetamax_next"]), (j, c)
        assert la["accepted"].sum() > 0 and not np.array_equal(ca["dmax_next"][-1], [0.8, 0.8])
        for c in range(K):
            assert _bytes(a[c]) == _bytes(b[c]) and _same_lists(a[c], b[c]), c
            order, sizes, _f = layouts[c]
            for rec in la[:, c]:
                if rec["accepted"]:
                    omcs[c].update(order[rec["molecule"]], rec["positions"][:sizes[rec["molecule"]]].copy())
        for c, rec in enumerate(ga.baseline_records()):
            _check_record(rec, _reference(omcs[c]), ("baseline after the cycles", c))
    _close(b)
    _close(a)


def test_sampler_and_chain_plan_on_chains_with_cells(setup, monkeypatch):
    """A sampler map of a sweep with device cells equals mcrng.bin_positions over the replay of the log; a chain plan that stops the
    chains inside the sweep, continued from the stops, gives the bytes of the unstopped clones."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_sampler import _host_bins, _kinds, _replayed_frames, _start
    mc, _owner = setup
    bins, S, first, every = (1.0, 4), 30, 3, 6
    frames = mcrng.sampler_frames(first, S, every, 0)
    devs, free = _make(setup, monkeypatch, bins), _make(setup, monkeypatch, bins)
    kinds = _kinds(mc)
    kw = dict(stream_id=[8, 1], log=True, **KW)
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(free) as other:
        group.device_cells()
        other.device_cells()
        other.set_sampler(every, step=1.5, supercell=(2, 3, 3), channels={kinds[0][0]: 0, kinds[1][0]: 1, kinds[1][1]: 1}, chain_map=[0, 1],
                          series_capacity=len(frames))
        samp = other.sampler
        starts = [_start(d) for d in free]
        s0, l0 = other.sweep(S, SEED + 8, first, **kw)
        got, series, _total = other.sampler_read()
        states = _replayed_frames(starts, l0, first, frames, None)
        assert np.array_equal(got, _host_bins(samp, states, kinds)) and got.sum() == 2 * len(frames) * 13 and l0["accepted"].sum() > 0
        assert [int(r["step"]) for r in series[:, 0]] == frames
        # stops at steps 12 and 20 of the stream, then each chain on from its stop
        stops = np.array([first + 9, first + 17])
        group.set_chain_plan(None, stops)
        s1, l1 = group.sweep(S, SEED + 8, first, **kw)
        for c in range(2):
            n = int(stops[c]) - first
            assert l1[:n, c].tobytes() == l0[:n, c].tobytes() and (l1["molecule"][n:, c] == -2).all()
        group.set_chain_plan(None, [first + S, 0])
        _s, l2 = group.sweep(S - 9, SEED + 8, int(stops[0]), **kw)
        group.set_chain_plan(None, [0, first + S])
        _s, l3 = group.sweep(S - 17, SEED + 8, int(stops[1]), **kw)
        assert l2[:, 0].tobytes() == l0[9:, 0].tobytes() and l3[:, 1].tobytes() == l0[17:, 1].tobytes()
        for c in range(2):
            assert _bytes(devs[c]) == _bytes(free[c]) and _same_lists(devs[c], free[c]), c
    _close(free)
    _close(devs)


def test_host_driven_insert_and_remove_between_two_sweeps(setup, monkeypatch):
    """Between two sweeps the host removes a middle molecule (the last one is renumbered), inserts one into the freed atom slots,
    inserts another beyond the high-water mark (the device's lists grow) and removes one more (a run of free slots stays: -1 in the
    lists, the slots no longer packed).  The second sweep picks all of it up: rows, bytes and lists equal the clones' on the host route."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    bins = (1.0, 4)
    devs, clones = _make(setup, monkeypatch, bins), _make(setup, monkeypatch, bins)
    unit = np.asarray(devs[0].mc.mat, dtype=np.float64) / np.array([2.0, 3.0, 3.0])[None, :]
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(clones) as twin:
        group.device_cells()
        _s, log = group.sweep(15, SEED + 9, 0, log=True, **KW)
        _follow(twin, log, [_layout(d) for d in devs])
        for d, t in zip(devs, clones):
            pos = d.state()[0]
            a, b = pos[4:7] + unit[:, 0], pos[7:10] + unit[:, 1]
            for x in (d, t):
                x.remove((1, 1))
                x.insert(1, a)
                x.insert(1, b)
                x.remove((1, 0))
        nslots = 16
        for d, t in zip(devs, clones):
            assert _device_bytes(d) == _device_bytes(t)
            ld, lt = d.cell_lists(nslots), t.cell_lists(nslots)
            assert np.array_equal(ld[0], lt[0]) and np.array_equal(ld[1], lt[1]) and (ld[0] == -1).sum() == 3
        _s, log = group.sweep(25, SEED + 9, 15, log=True, **KW)
        assert (group.halted() == -1).all() and log["accepted"].sum() > 0
        _follow(twin, log, [_layout(d) for d in devs])
        for c, (d, t) in enumerate(zip(devs, clones)):
            assert _device_bytes(d) == _device_bytes(t) and d.neighbour_cells() == t.neighbour_cells(), c
            ld, lt = d.cell_lists(nslots), t.cell_lists(nslots)
            assert np.array_equal(ld[0], lt[0]) and np.array_equal(ld[1], lt[1]) and (ld[0] == -1).sum() == 3, c
    _close(clones)
    _close(devs)


def test_run_montecarlo_raises_where_a_chain_halts(setup, monkeypatch):
    """run_montecarlo on chains staged to a full cell: MonteCarloHalted names the chain and the step halted() reports, and the halted
    chain still has its capacity of 8."""
    from ceg_hip.energy import DeviceMonteCarloGroup, MonteCarloHalted
    devs = _make(setup, monkeypatch, (12, 12, 12))
    _stage(devs)
    with DeviceMonteCarloGroup(devs) as group:
        group.device_cells()
        with pytest.raises(MonteCarloHalted) as e:
            group.run_montecarlo(1e9, 30, 0, seed=SEED + 5, steps_per_cycle=10, dmax=1.5, thetamax=3.0, adapt=(), stream_id=[5, 1, 9], check_drift=False)
        halted = group.halted()
        assert 0 <= e.value.step < 300 and halted[e.value.chain] == e.value.step and e.value.chain == int(np.nonzero(halted >= 0)[0][0])
        assert devs[e.value.chain].neighbour_cells()[1] == 8
    _close(devs)


# ---- GCMC sweeps on chains with cells
def _index_of(dev, d):
    """(kind, index) of device molecule d"""
    for i, kind in enumerate(dev._slot):
        if d in kind:
            return i, kind.index(d)
    raise AssertionError((d, dev._slot))


def _follow_gcmc(group, clones, log, sizes, books=None):
    """drive the clones through the log of a GCMC sweep on the host route -- group.trial at the logged placement (columns 0, 2, 3 of the
    rows bit for bit, column 1 to 1e-12 relative), then accept / insert / remove per handle -- and, with `books`, a mcrng.CellBook per
    chain beside it, with the device's rule for the atom slots (an insertion takes the run freed last, else fresh slots at the
    high-water mark; a deletion moves the last molecule to the index).  -> accepted (insertions, deletions, deletions that renumber,
    insertions into a freed run)"""
    S, K = log.shape
    counts = np.zeros(4, dtype=np.int64)
    for s in range(S):
        for c in range(K):
            rec, dev = log[s, c], clones[c]
            if rec["molecule"] < 0 or rec["flags"] & (1 | 4 | 8):
                continue
            i, kind = int(rec["species"]), int(rec["kind"])
            m = sizes[i]
            placed = rec["positions"][:m].copy()
            moves = [None] * K
            if kind == 5:
                moves[c] = ("insert", i, placed[None])
                want = rec["rows"][1:2]
            else:
                idx = _index_of(dev, int(rec["molecule"]))
                moves[c] = ("move", idx, placed[None] if kind != 6 else np.empty((0, m, 3)))
                want = rec["rows"][:1] if kind == 6 else rec["rows"]
            rows = group.trial(moves)[c]
            for col in (0, 2, 3):
                assert np.array_equal(rows[:, col], want[:, col]), (s, c, kind, col, rows, want)
            np.testing.assert_allclose(rows[:, 1], want[:, 1], rtol=1e-12, atol=0.0)
            if not rec["accepted"]:
                continue
            book = books[c] if books is not None else None
            if kind == 5:
                dev.insert(i, placed)
                counts[0] += 1
                if book is not None:
                    reused = bool(book.free.get(m))
                    first = book.free[m].pop() if reused else book.natoms
                    book.natoms += 0 if reused else m
                    counts[3] += reused
                    book.first.append(first)
                    book.size.append(m)
                    book.insert(first, placed)
            elif kind == 6:
                d = int(rec["molecule"])
                nmol = sum(len(k) for k in dev._slot)
                dev.remove(idx)
                counts[1] += 1
                counts[2] += d != nmol - 1
                if book is not None:
                    last = len(book.first) - 1
                    book.remove(book.first[d], book.size[d], book.first[last], book.size[last] if last != d else 0)
                    book.free.setdefault(book.size[d], []).append(book.first[d])
                    book.first[d], book.size[d] = book.first[last], book.size[last]
                    book.first.pop()
                    book.size.pop()
            else:
                dev.accept(idx, placed)
                if book is not None:
                    book.move(book.first[int(rec["molecule"])], placed)
    return counts


def _device_bytes(dev):
    """positions in the device's molecule order and the structure factor, as bytes, read with the molecule count of the handle's
    own table (DeviceMonteCarlo.state() counts the molecules of the host-side setup, which insert / remove do not touch)"""
    natoms = sum(len(dev.mc.ffidx[i]) * len(kind) for i, kind in enumerate(dev._slot))
    nk = len(dev.mc.ewald.kfactors) if dev.mc.ewald.alpha != 0.0 else 0
    pos, re, im = np.empty((natoms, 3)), np.empty(max(nk, 1)), np.empty(max(nk, 1))
    _abi.check(dev._lib, dev._lib.ceg_mc_get_state(dev._h, _abi.dptr(pos.reshape(-1)) if natoms else None, _abi.dptr(re), _abi.dptr(im)))
    return pos.tobytes() + re[:nk].tobytes() + im[:nk].tobytes()


def _empty_book(dev):
    book = mcrng.CellBook(dev.mc.invmat, dev.neighbour_cells()[0])
    book.free, book.natoms, book.first, book.size = {}, 0, [], []          # free: atoms per molecule -> stack of freed runs
    return book


def _lists_equal(a, b, nslots):
    la, lb = a.cell_lists(nslots), b.cell_lists(nslots)
    return np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and a.neighbour_cells() == b.neighbour_cells()


def test_gcmc_sweep_from_an_empty_box_and_back(setup, monkeypatch):
    """Chains with cells (4 A and 1 A bins) created empty: a large phiPV_div_k fills the box to at least 6 molecules, a second species
    table with a tiny one empties it (deletions of a molecule that is not the last: renumbering), a third fills it again (freed atom
    slots reused).  After every phase: rows, bytes and cell lists of clones on the host route (trial_insert / insert / remove / accept
    through the same calls a host-driven caller makes), cell_lists() against the CellBook replay, statistics and state against the
    oracle replay of test_gpu_mc_sweep_gcmc at 1e-9."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_sweep_gcmc import _follow as _oracle_follow, _replays, _tail
    bins, S, caps, nslots = (4, 1.0), 120, [12, 12], 36
    na_moves = mcrng.MoveTable(translation=1, swap=3)
    co2_moves = mcrng.MoveTable(translation=1, rotation=1, random_reinsertion=1, swap=6)
    devs = _make(setup, monkeypatch, bins, positions=[[], []])
    clones = _make(setup, monkeypatch, bins, positions=[[], []])
    omcs = _oracles(devs)
    books = [_empty_book(d) for d in devs]
    sizes = [len(ids) for ids in devs[0].mc.ffidx]
    sid = np.array([3, 8], dtype=np.uint32)
    T = [300.0, 600.0]
    total = np.zeros(4, dtype=np.int64)
    tabs = None
    with DeviceMonteCarloGroup(devs) as group, DeviceMonteCarloGroup(clones) as twin:
        group.device_cells()
        for phase, phi in enumerate((1e12, 1e-100, 1e12)):
            table = _tail(group.gcmc_species([na_moves, co2_moves], [phi, phi]))
            stats, log = group.sweep_gcmc(S, SEED + 10, phase * S, temperature=T, dmax=0.8, thetamax=1.5, species=table, max_molecules=caps,
                                          stream_id=sid, log=True)
            assert (group.halted() == -1).all()
            total += _follow_gcmc(twin, clones, log, sizes, books)
            reps = _replays(devs, omcs, table, T, 0.8, 1.5, caps)
            for c, rep in enumerate(reps):
                rep.tab = [] if tabs is None else tabs[c]
            _oracle_follow(reps, log, SEED + 10, phase * S, sid)
            tabs = [rep.tab for rep in reps]
            for c, rep in enumerate(reps):
                rep.sf_scale = 1.0
                rep.check_stats(stats[c], (phase, c))
                rep.check_state(devs[c], (phase, c))
                assert _device_bytes(devs[c]) == _device_bytes(clones[c]), (phase, c)
                assert _lists_equal(devs[c], clones[c], nslots), (phase, c)
                got, want = devs[c].cell_lists(nslots), books[c].lists(nslots)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (phase, c)
            nmol = [int(s["nmol"]) for s in stats]
            print(f"gcmc with device cells, phase {phase}: nmol {nmol}, accepted ins / del / renumbering del / ins into freed slots so far {total.tolist()}")
            if phase == 0:
                assert min(nmol) >= 6, nmol
            if phase == 1:
                assert max(nmol) < 6 and total[2] > 0, (nmol, total)
        assert total[3] > 0 and total[0] > total[1] > 0, total
    _close(clones)
    _close(devs)


def test_gcmc_sweep_with_block_masks_on_chains_with_cells(setup, monkeypatch, masks):
    """block pockets with sweep_gcmc on a chain with cells: the log and the pocket counters are those of the same chain without cells
    wherever no pair sum enters (species, molecule, kind, attempt and pocket flags of every record up to the first decision that the
    summation order of the pair term could turn), and rows, bytes and lists equal the clone's on the host route"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    from test_gpu_mc_sweep_gcmc import CO2_MOVES, NA_MOVES
    S, caps, nslots = 50, [14], 42
    dev, clone = _make(setup, monkeypatch, (4,)), _make(setup, monkeypatch, (4,))
    sizes = [len(ids) for ids in dev[0].mc.ffidx]
    with DeviceMonteCarloGroup(dev) as group, DeviceMonteCarloGroup(clone) as twin:
        group.device_cells()
        group.set_blocks(*masks)
        table = group.gcmc_species([NA_MOVES, CO2_MOVES], [3e5, 3e5])
        stats, log = group.sweep_gcmc(S, SEED + 12, 0, temperature=[500.0], dmax=0.8, thetamax=1.5, species=table, max_molecules=caps, log=True)
        pocket, attempts = group.block_counts()
        _follow_gcmc(twin, clone, log, sizes)
        assert _device_bytes(dev[0]) == _device_bytes(clone[0]) and _lists_equal(dev[0], clone[0], nslots)
        flagged = (log["flags"][:, 0] & 8) != 0
        assert pocket[0] == flagged.sum() > 0 and attempts[0] == (log["flags"][:, 0] >> 16).sum() > 0, (pocket, attempts)
        assert stats[0]["blocked"] >= pocket[0] and log["accepted"].sum() > 0
    _close(clone)
    _close(dev)


def test_gcmc_sweep_halts_on_a_full_cell_and_continues(setup, monkeypatch):
    """12 A bins, capacity 8, an empty box and a high phiPV_div_k: the cells fill by insertions.  The host route on a clone (driven with
    the log of a group that had capacity 64 from the start) grows its capacity at some step; the device sweep with capacity 8 halts
    exactly there with the clone's state before that step, later records carry molecule = -2 and the statistics count only the steps
    before it; with device_cells(capacity=64) the continuation gives the bytes, lists and log of the group with the large capacity."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    S, first, caps, nslots = 300, 200, [40], 120
    swaps = mcrng.MoveTable(translation=1, swap=6)
    small, big, clone = (_make(setup, monkeypatch, (12,), positions=[[], []]) for _ in range(3))
    sizes = [len(ids) for ids in small[0].mc.ffidx]
    assert small[0].neighbour_cells()[1] == 8
    kw = dict(temperature=[600.0], dmax=0.8, thetamax=1.5, max_molecules=caps, log=True)
    with DeviceMonteCarloGroup(small) as gs, DeviceMonteCarloGroup(big) as gb, DeviceMonteCarloGroup(clone) as gc:
        gb.device_cells(capacity=64)
        table = gb.gcmc_species([swaps, swaps], [1e12, 1e12])
        sb, lb = gb.sweep_gcmc(S, SEED + 14, first, species=table, **kw)
        assert (gb.halted() == -1).all() and big[0].neighbour_cells()[1] == 64
        grew, before = -1, None
        for s in range(S):
            snap = (_device_bytes(clone[0]), clone[0].cell_lists(nslots))
            _follow_gcmc(gc, clone, lb[s:s + 1], sizes)
            if grew < 0 and clone[0].neighbour_cells()[1] > 8:
                grew, before = s, snap
        print(f"gcmc halting: the host route grew its capacity at step {grew} of {S}, {int(sb[0]['nmol'])} molecules at the end")
        assert 5 <= grew <= S - 6, grew
        gs.device_cells()
        ss, ls = gs.sweep_gcmc(S, SEED + 14, first, species=table, **kw)
        assert gs.halted()[0] == first + grew
        assert ls[:grew, 0].tobytes() == lb[:grew, 0].tobytes()
        assert (ls["molecule"][grew:, 0] == -2).all() and (ls["species"][grew:, 0] == -1).all() and not ls["accepted"][grew:, 0].any()
        assert ss[0]["trials"].sum() + ss[0]["spent"] == grew and ss[0]["accepted"].sum() == ls["accepted"][:grew, 0].sum()
        assert _device_bytes(small[0]) == before[0] and small[0].neighbour_cells()[1] == 8
        got = small[0].cell_lists(nslots)
        assert np.array_equal(got[0], before[1][0]) and np.array_equal(got[1], before[1][1])
        gs.device_cells(capacity=64)
        s2, l2 = gs.sweep_gcmc(S - grew, SEED + 14, first + grew, species=table, **kw)
        assert (gs.halted() == -1).all()
        assert np.concatenate([ls[:grew], l2]).tobytes() == lb.tobytes()
        assert _device_bytes(small[0]) == _device_bytes(big[0]) == _device_bytes(clone[0])
        lists = [d.cell_lists(nslots) for d in (small[0], big[0], clone[0])]
        assert all(np.array_equal(lists[0][q], l[q]) for l in lists[1:] for q in (0, 1))
    _close(clone)
    _close(big)
    _close(small)
