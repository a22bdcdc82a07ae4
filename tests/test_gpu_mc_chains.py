"""Chain groups of the device-resident MC state (ceg_mc_group_*): K Markov chains stepped in lockstep, one launch for all their
trials and one for all their accepts -- the way make_isotherm (parameterinputs.jl:316-329) runs one run_gcmc per pressure.
Checked against the ORACLE's state chain by chain (oracle/montecarlo.OracleMonteCarlo), against the single-handle
entry points, and for every refusal of the C ABI.  Run with `pytest -m gpu` on an MI355X."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from test_gpu_consumers import _mc_setup, _rotation

pytestmark = pytest.mark.gpu

GROUP_MAX = 256


def _check(row, r, what):
    """the tolerance of test_mc_replay_1000_moves: 1e-9 relative + 1e-7, blocked (>= 1e90) where the oracle is blocked"""
    ok = np.isfinite(r) & (np.abs(r) < 1e90)
    assert np.array_equal(row[~ok] >= 1e90, r[~ok] >= 1e90), (what, row, r)
    err = np.abs(row[ok] - r[ok]) / (1e-9 * np.abs(r[ok]) + 1e-7)
    assert (err <= 1.0).all(), (what, row, r)


def _chains(tmp_path, k, monkeypatch=None, cells=()):
    """k DeviceMonteCarlo chains of the Na + 4 CO2 CIT-7 setup sharing one set of grid interpolators, each with its own host copy of
    the setup and its own OracleMonteCarlo; chains in `cells` are created with CEG_HIP_MC_CELLS=1 (neighbour cells forced on)."""
    from ceg_hip.energy import DeviceMonteCarlo
    from oracle.montecarlo import OracleMonteCarlo
    M, mc = _mc_setup(tmp_path)
    devs, omcs, mcs = [], [], []
    for c in range(k):
        mcc = copy.copy(mc)
        mcc.positions = [[p.copy() for p in kind] for kind in mc.positions]
        if c in cells:
            monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
        devs.append(DeviceMonteCarlo(mcc, grids_from=devs[0] if devs else None))
        if c in cells:
            monkeypatch.delenv("CEG_HIP_MC_CELLS")
            assert devs[-1].neighbour_cells() is not None
        omc = OracleMonteCarlo.from_setup(mcc)
        omc.compute_ewald()
        omcs.append(omc)
        mcs.append(mcc)
    return mc, devs, omcs, mcs


def _displace(rng, cur, n, jump=False):
    """n trial placements of a molecule now at `cur`: small translations, rigid rotations about the centre atom, an occasional jump"""
    out = []
    for _ in range(n):
        new = cur + (rng.uniform(-6.0, 6.0, 3) if jump else rng.uniform(-0.35, 0.35, 3))
        if len(cur) > 1 and rng.random() < 0.5:
            c = new[len(cur) // 2]
            new = c + (new - c) @ _rotation(rng).T
        out.append(new)
    return np.array(out).reshape(n, len(cur), 3)


def _close(devs):
    for d in devs:
        d.close()


def test_group_lockstep_replay_against_the_oracle(hip_lib, tmp_path):
    """8 chains, each moved to a state of its own by 20 per-handle accepts, then 200 lockstep steps: Na and CO2 displacements and
    rotations in the same call, idle chains, insertion trials (accepted by a per-handle ceg_mc_insert while grouped), deletions
    (n = 0, accepted by ceg_mc_remove), some chains with several placements; one group accept per step with an energy-independent
    acceptance pattern.  Every row against the chain's oracle; at the end every chain's positions (exactly) and total structure
    factor (1e-9)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 8
    try:
        mc, devs, omcs, mcs = _chains(tmp_path, K)
        rngs = [np.random.default_rng(1000 + c) for c in range(K)]
        for c in range(K):                                       # distinct states before grouping
            rng, omc = rngs[c], omcs[c]
            for s in range(20):
                kind = s % 2
                j = int(rng.integers(len(omc.positions[kind])))
                new = _displace(rng, omc.positions[kind][j], 1)[0]
                devs[c].accept((kind, j), new)
                omc.update((kind, j), new)
        base = mc.positions[1][0] - mc.positions[1][0][1]       # CO2 geometry about its carbon
        seen = dict(idle=0, insert=0, inserted=0, delete=0, deleted=0, multi=0, na=0, co2=0, accepted=0)
        with DeviceMonteCarloGroup(devs) as group:
            for step in range(200):
                ins_kind = step % 2                              # one inserted species per call
                moves, plan = [], []
                for c in range(K):
                    rng, omc = rngs[c], omcs[c]
                    u = rng.random()
                    kind = int(rng.integers(2))
                    if u < 0.1:
                        moves.append(None); plan.append(None)
                        seen["idle"] += 1
                    elif u < 0.22:
                        shape = np.zeros((1, 3)) if ins_kind == 0 else base @ _rotation(rng).T
                        nt = int(rng.integers(1, 4))
                        trials = (mc.mat @ rng.uniform(0, 1, (nt, 3)).T).T[:, None, :] + shape[None]
                        moves.append(("insert", ins_kind, trials)); plan.append(("insert", ins_kind, trials))
                        seen["insert"] += 1
                    elif u < 0.32 and len(omc.positions[kind]) > 1:
                        j = int(rng.integers(len(omc.positions[kind])))
                        m = len(omc.ffidx[kind])
                        moves.append(("move", (kind, j), np.empty((0, m, 3)))); plan.append(("delete", (kind, j), None))
                        seen["delete"] += 1
                    else:
                        if not omc.positions[kind]:
                            kind = 1 - kind
                        j = int(rng.integers(len(omc.positions[kind])))
                        n = 1 if rng.random() < 0.75 else int(rng.integers(2, 5))
                        trials = _displace(rng, omc.positions[kind][j], n, jump=rng.random() < 0.1)
                        moves.append(("move", (kind, j), trials)); plan.append(("move", (kind, j), trials))
                        seen["multi"] += n > 1
                        seen["na" if kind == 0 else "co2"] += 1
                rows = group.trial(moves)
                accepted = [None] * K
                for c in range(K):
                    p, r, omc, rng = plan[c], rows[c], omcs[c], rngs[c]
                    if p is None:
                        assert r is None
                        continue
                    what, idx, trials = p
                    if what == "insert":
                        assert r.shape == (len(trials), 4)
                        for t in range(len(trials)):
                            _check(r[t], omc.insertion_energy(idx, trials[t]), (step, c, "insert", t))
                        if rng.random() < 0.5:
                            assert devs[c].insert(idx, trials[0]) == omc.add(idx, trials[0])
                            seen["inserted"] += 1
                    elif what == "delete":
                        assert r.shape == (1, 4)
                        _check(r[0], omc.movement_energy(idx), (step, c, "delete"))
                        if rng.random() < 0.7:
                            assert devs[c].remove(idx) == omc.remove(idx)
                            seen["deleted"] += 1
                    else:
                        assert r.shape == (len(trials) + 1, 4)
                        _check(r[0], omc.movement_energy(idx), (step, c, "before"))
                        for t in range(len(trials)):
                            _check(r[1 + t], omc.movement_energy(idx, trials[t]), (step, c, "after", t))
                        if rng.random() < 0.6:                   # energy-independent acceptance pattern
                            accepted[c] = (idx, trials[0])
                            omc.update(idx, trials[0])
                            seen["accepted"] += 1
                group.accept(accepted)
        assert all(v > 0 for v in seen.values()), seen
        for c in range(K):
            mcs[c].positions = [[p.copy() for p in kind] for kind in omcs[c].positions]     # (DeviceMonteCarlo.state counts atoms there)
            pos, sf = devs[c].state()
            assert np.array_equal(pos, omcs[c].flat_positions()), c
            osf = omcs[c].total_structure_factor()
            assert np.abs(sf - osf).max() <= 1e-9 * np.abs(osf).max(), c
        print(f"group replay: {K} chains x 200 steps, {seen}")
        _close(devs[::-1])
    finally:
        ceg.setdir_RASPA(Path(__file__).parent / "golden" / "raspa")


def test_group_rows_match_the_single_handle_rows(hip_lib, tmp_path, monkeypatch):
    """At several states, each chain's group rows against ceg_mc_trial / ceg_mc_trial_insert on the same handle: the same body and the
    same three-workgroup term split, hence the same sums in the same order.  The two instantiations of the body are compiled apart,
    and the backend pairs some multiply-adds of the framework Coulomb interpolation differently (seen: 1e-12 relative in column 1 of
    some Na placements); every other column must be bit-identical, column 1 agree to 1e-10 relative (+ 1e-7 K), the bound that
    test_mc_large_batches_take_the_wave_kernels sets for the same terms summed in another order.  One chain keeps its guests in neighbour cells
    (CEG_HIP_MC_CELLS=1), so the calls mix kernel classes and take two launches (three with an insertion)."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 4
    try:
        mc, devs, omcs, _mcs = _chains(tmp_path, K, monkeypatch, cells=(3,))
        rng = np.random.default_rng(31)
        base = mc.positions[1][0] - mc.positions[1][0][1]
        with DeviceMonteCarloGroup(devs) as group:
            for state in range(6):
                ins_kind = state % 2
                shape = np.zeros((1, 3)) if ins_kind == 0 else base @ _rotation(rng).T
                ins = (mc.mat @ rng.uniform(0, 1, (3, 3)).T).T[:, None, :] + shape[None]
                moves = []
                for c in range(K):
                    omc = omcs[c]
                    kind = (c + state) % 2
                    j = int(rng.integers(len(omc.positions[kind])))
                    if c == 2 and state % 3 == 0:
                        moves.append(("insert", ins_kind, ins))
                    elif c == 1 and state == 4:
                        moves.append(("move", (kind, j), np.empty((0, len(omc.ffidx[kind]), 3))))        # deletion energy
                    else:
                        n = 255 if (c == 3 and state == 2) else 1 + (c + state) % 4                     # 256 rows: the split's last size
                        moves.append(("move", (kind, j), _displace(rng, omc.positions[kind][j], n)))
                rows = group.trial(moves)
                accepted = [None] * K
                for c, (mv, r) in enumerate(zip(moves, rows)):
                    what, idx, trials = mv
                    single = devs[c].trial_insert(idx, trials) if what == "insert" else devs[c].trial(idx, trials)
                    assert r.shape == single.shape
                    for col in (0, 2, 3):
                        assert np.array_equal(r[:, col], single[:, col]), (state, c, what, col, r, single)
                    np.testing.assert_allclose(r[:, 1], single[:, 1], rtol=1e-10, atol=1e-7)
                    if what == "move" and len(trials):
                        accepted[c] = (idx, trials[0])
                        omcs[c].update(idx, trials[0])
                group.accept(accepted)
        _close(devs[::-1])
    finally:
        ceg.setdir_RASPA(Path(__file__).parent / "golden" / "raspa")


def _raw_handle(lib, dev, device):
    """ceg_mc_create through the C ABI without grids or Ewald sums (the pair table of `dev`'s force field)"""
    ff, mc = dev.mc.ff, dev.mc
    rules, offsets = ff.pair_table()
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    matT = np.ascontiguousarray(np.asarray(mc.mat, dtype=np.float64).T.reshape(9))
    invT = np.ascontiguousarray(np.asarray(mc.invmat, dtype=np.float64).T.reshape(9))
    charge = np.zeros(ff.nkinds)
    h = C.c_void_p()
    _abi.check(lib, lib.ceg_mc_create(C.byref(h), device, None, None, _abi.dptr(charge), ff.nkinds, _abi.dptr(matT), _abi.dptr(invT),
                                      ff.cutoff ** 2, rules.ctypes.data, _abi.i32ptr(offsets), 1.0, None, None, None, None, 0, None, None))
    return h, (rules, offsets)


def test_group_refusals_poison_and_release(hip_lib, tmp_path, monkeypatch):
    """Every refusal of ceg_mc_group_create (k out of range, a handle twice, a handle already grouped, a handle whose guests were never
    set, handles on two devices), ceg_mc_destroy of a grouped handle, a bad molecule index, insertion kinds outside the pair table, a
    call larger than the group's staging (CEG_ERR_UNSUPPORTED); a member poisoned by a failed per-handle accept makes the next group
    calls fail with its index until ceg_mc_set_guests; after destroy the members run alone and give the same rows.  Nothing here
    launches a kernel on a bad argument."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    lib = hip_lib
    K = 3
    try:
        mc, devs, omcs, _mcs = _chains(tmp_path, K)
        hs = [d._h for d in devs]

        def create(handles, k=None):
            arr = (C.c_void_p * max(len(handles), 1))(*handles)
            g = C.c_void_p()
            rc = lib.ceg_mc_group_create(C.byref(g), arr, len(handles) if k is None else k)
            return rc, g

        assert create(hs, 0)[0] == -1
        assert create(hs * (GROUP_MAX // K + 1), GROUP_MAX + 1)[0] == -1
        assert create([hs[0], hs[1], hs[0]])[0] == -1                        # a handle twice
        assert b"twice" in lib.ceg_last_error()
        raw, keep = _raw_handle(lib, devs[0], 0)
        assert create([hs[0], raw.value])[0] == -1                         # guests never set
        assert b"ceg_mc_set_guests" in lib.ceg_last_error()
        if lib.ceg_device_count() > 1:                                     # handles on two devices
            other, keep2 = _raw_handle(lib, devs[0], 1)
            p = np.zeros(3)
            _abi.check(lib, lib.ceg_mc_set_guests(other, _abi.dptr(p), _abi.i32ptr(np.zeros(1, dtype=np.int32)),
                                                  _abi.i32ptr(np.array([0, 1], dtype=np.int32)), 1))
            assert create([hs[0], other.value])[0] == -1
            assert b"one device" in lib.ceg_last_error()
            lib.ceg_mc_destroy(other)
        with DeviceMonteCarloGroup(devs[:1]) as g1:                       # already in a group
            assert create([hs[1], hs[0]])[0] == -1
            assert b"already in a group" in lib.ceg_last_error()
            assert lib.ceg_mc_destroy(hs[0]) == -1                         # ceg_mc_destroy of a grouped handle
            with pytest.raises(RuntimeError, match="DeviceMonteCarloGroup"):
                devs[0].close()
        lib.ceg_mc_destroy(raw)
        del keep

        group = DeviceMonteCarloGroup(devs)
        moves = [("move", (1, 0), _displace(np.random.default_rng(1), mc.positions[1][0], 2)), None, ("insert", 0, np.zeros((1, 1, 3)))]
        before = [r.copy() if r is not None else None for r in group.trial(moves)]
        mol = np.array([10 ** 6, -2, -2], dtype=np.int32)
        n = np.zeros(3, dtype=np.int32)
        out = np.empty((8, 4))
        kinds = np.zeros(1, dtype=np.int32)
        assert lib.ceg_mc_group_trial(group._h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(kinds), 1, None, _abi.dptr(out.reshape(-1))) == -1
        assert lib.ceg_mc_group_accept(group._h, _abi.i32ptr(mol), _abi.dptr(np.zeros(3))) == -1
        mol = np.array([-1, -2, -2], dtype=np.int32)
        n[0] = 1
        bad = np.array([10 ** 6], dtype=np.int32)
        assert lib.ceg_mc_group_trial(group._h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(bad), 1, _abi.dptr(np.zeros(3)),
                                      _abi.dptr(out.reshape(-1))) == -1
        big = 20000                                                        # 2 x 20 001 rows > the 32 768 rows of the staging
        mol = np.array([0, 0, -2], dtype=np.int32)
        n = np.array([big, big, 0], dtype=np.int32)
        t = np.zeros(2 * big * 3)
        huge = np.empty((2 * (big + 1), 4))
        assert lib.ceg_mc_group_trial(group._h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(kinds), 1, _abi.dptr(t), _abi.dptr(huge.reshape(-1))) == -5
        # a failed per-handle accept poisons member 1: every group call that uses it fails with its index, until ceg_mc_set_guests
        monkeypatch.setenv("CEG_HIP_MC_INJECT_FAILURE", "accept")
        with pytest.raises(_abi.CegError) as ei:
            devs[1].accept((0, 0), mc.positions[0][0] + 0.1)
        assert ei.value.code == -3
        monkeypatch.delenv("CEG_HIP_MC_INJECT_FAILURE")
        use1 = [None, ("move", (0, 0), np.empty((0, 1, 3))), None]
        for call in (lambda: group.trial(use1), lambda: group.accept([None, ((0, 0), mc.positions[0][0]), None])):
            with pytest.raises(_abi.CegError) as ei:
                call()
            assert ei.value.code == -3 and "chain 1" in str(ei.value)
        after = group.trial(moves)                                         # chain 1 idle: unaffected
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
        devs[1].refresh()                                                  # ceg_mc_set_guests rebuilds host and device state
        r1 = group.trial(use1)[1]
        _check(r1[0], omcs[1].movement_energy((0, 0)), "after set_guests")
        group.close()
        # the members alone again: the same rows from their own streams (to the tolerance of the test above)
        np.testing.assert_allclose(devs[0].trial((1, 0), moves[0][2]), before[0], rtol=1e-10, atol=1e-7)
        np.testing.assert_allclose(devs[2].trial_insert(0, np.zeros((1, 1, 3))), before[2], rtol=1e-10, atol=1e-7)
        np.testing.assert_allclose(devs[1].trial((0, 0), np.empty((0, 1, 3))), r1, rtol=1e-10, atol=1e-7)
        _close(devs[::-1])
    finally:
        ceg.setdir_RASPA(Path(__file__).parent / "golden" / "raspa")
