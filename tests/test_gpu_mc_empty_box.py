"""The device-resident Monte-Carlo state (ceg_mc_*) with NO guest: a handle straight out of ceg_mc_create, after
ceg_mc_set_guests(nmol = 0), drained molecule by molecule, and as a member of a chain group -- where a GCMC isotherm starts
(make_isotherm -> run_gcmc from an empty box).  Every row against the ORACLE's state (oracle/montecarlo.OracleMonteCarlo, itself checked
at zero guests by tests/test_oracle_empty_box.py) with the tolerance of the replay tests (_check: 1e-9 relative + 1e-7 K, blocked rows
blocked), with the guest-guest sum on the exhaustive loop and on neighbour cells (CEG_HIP_MC_CELLS).  No row is skipped; insertion
placements are drawn so that a fifth of them is blocked on the oracle (draw_placements).  Run with `pytest -m gpu` on an MI355X."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from test_gpu_consumers import _mc_setup
from test_gpu_mc_chains import _check, _displace, _raw_handle
from test_oracle_empty_box import draw_placements

pytestmark = pytest.mark.gpu

GOLDEN_RASPA = Path(__file__).parent / "golden" / "raspa"
WAVE_ROWS = 1100          # from 1024 rows on a batch takes the wave-per-placement kernels (test_mc_large_batches_take_the_wave_kernels)
CELLS = pytest.mark.parametrize("cells", ["0", "1"])


def _setups(tmp_path):
    """(M, the Na + 4 CO2 setup, a setup of the same species, grids and Ewald tables without any molecule, CO2 geometry about its carbon)"""
    M, mc = _mc_setup(tmp_path)
    ff = "BoulfelfelSholl2021"
    na = ceg.load_molecule_RASPA("Na", "TraPPE", ff).with_positions(mc.positions[0][0])
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", ff).with_positions(mc.positions[1][0])
    empty = M.setup_montecarlo("CIT-7", ff, [(na, 0), (co2, 0)])           # (the grid files of the first setup are read back)
    assert [len(k) for k in empty.positions] == [0, 0] and empty.ffidx == mc.ffidx
    return M, mc, empty, mc.positions[1][0] - mc.positions[1][0][1]


def _copy_setup(mc):
    out = copy.copy(mc)
    out.positions = [[p.copy() for p in kind] for kind in mc.positions]
    return out


def _device(mc, monkeypatch, cells, **kw):
    from ceg_hip.energy import DeviceMonteCarlo
    monkeypatch.setenv("CEG_HIP_MC_CELLS", cells)
    dev = DeviceMonteCarlo(mc, **kw)
    monkeypatch.delenv("CEG_HIP_MC_CELLS")
    assert (dev.neighbour_cells() is not None) == (cells == "1")
    return dev


def _oracle(mc):
    from oracle.montecarlo import OracleMonteCarlo
    omc = OracleMonteCarlo.from_setup(mc)
    omc.compute_ewald()
    return omc


def _empty_box_batches(omc, base):
    """the insertion batches of B1 / B2: Na and CO2, 1, 5 and WAVE_ROWS placements each"""
    rng = np.random.default_rng(9001)
    return [(kind, draw_placements(omc, base, kind, n, rng)) for kind in (0, 1) for n in (1, 5, WAVE_ROWS)]


def _insertion_rows(dev, omc, batches, what, against_oracle=True):
    """ceg_mc_trial_insert and ceg_mc_trial_insert_device on every batch: every row against the oracle's insertion_energy, the
    guest-guest column exactly 0.0 (there is no guest), the device-entry rows against the host-entry rows as the large-batch test
    relates them (1e-10 relative + 1e-7)"""
    import torch
    out = []
    for kind, trials in batches:
        rows = dev.trial_insert(kind, trials)
        assert rows.shape == (len(trials), 4)
        nblocked = 0
        for t in range(len(trials) if against_oracle else 0):
            ref = omc.insertion_energy(kind, trials[t])
            nblocked += bool(ref[0] >= 1e90)
            _check(rows[t], ref, (what, kind, len(trials), t))
        assert 4 * nblocked <= len(trials), (nblocked, len(trials))         # at most a quarter blocked on the oracle
        assert (rows[:, 2] == 0.0).all(), (what, kind, rows[:, 2][rows[:, 2] != 0.0][:4])
        d_trial = torch.tensor(trials, dtype=torch.float64, device="cuda")
        d_rows = torch.full((len(trials), 4), float("nan"), dtype=torch.float64, device="cuda")
        dev.trial_insert_device(kind, d_trial.data_ptr(), len(trials), d_rows.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_allclose(d_rows.cpu().numpy(), rows, rtol=1e-10, atol=1e-7)
        assert bool((d_rows[:, 2] == 0.0).all())
        out.append(rows)
    return out


def _final_state(dev, omc, scale, what):
    """positions exactly, total structure factor to 1e-9 of the largest component the chain has had"""
    dev.mc.positions = [[p.copy() for p in kind] for kind in omc.positions]          # (DeviceMonteCarlo.state counts atoms there)
    pos, sf = dev.state()
    assert np.array_equal(pos, omc.flat_positions()), what
    osf = omc.total_structure_factor()
    assert np.abs(sf - osf).max() <= 1e-9 * scale, (what, float(np.abs(sf - osf).max()), scale)


@CELLS
def test_fresh_handle_is_an_empty_box(hip_lib, tmp_path, monkeypatch, cells):
    """B1.  ceg_mc_create and NO ceg_mc_set_guests: insertion trials of Na and CO2 (1, 5 and 1100 placements: the workgroup-per-row
    kernel with its three-way split and the wave kernels; host and device entry points) against the oracle's empty box;
    ceg_mc_get_state gives no atoms and a total structure factor of exact zeros; ceg_mc_trial / ceg_mc_accept of molecule 0 and
    a chain group holding the handle are refused with CEG_ERR_INVALID.  Also a handle without grids and k-space tables
    (_raw_handle): every column of an insertion row is exactly 0.0 there."""
    lib = hip_lib
    try:
        M, mc, empty, base = _setups(tmp_path)
        dev = _device(empty, monkeypatch, cells, upload_guests=False)
        omc = _oracle(empty)
        _insertion_rows(dev, omc, _empty_box_batches(omc, base), "fresh")
        pos, sf = dev.state()
        assert pos.shape == (0, 3) and sf.shape == (len(empty.ewald.kfactors),) and not sf.real.any() and not sf.imag.any()
        out = np.full((2, 4), np.nan)
        p = np.ascontiguousarray(mc.positions[0][0].reshape(-1))
        assert lib.ceg_mc_trial(dev._h, 0, _abi.dptr(p), 1, _abi.dptr(out.reshape(-1))) == -1
        assert lib.ceg_mc_accept(dev._h, 0, _abi.dptr(p)) == -1
        assert np.isnan(out).all()
        g = C.c_void_p()
        assert lib.ceg_mc_group_create(C.byref(g), (C.c_void_p * 1)(dev._h), 1) == -1
        assert b"ceg_mc_set_guests" in lib.ceg_last_error()
        monkeypatch.setenv("CEG_HIP_MC_CELLS", cells)
        raw, keep = _raw_handle(lib, dev, 0)
        monkeypatch.delenv("CEG_HIP_MC_CELLS")
        kinds = np.ascontiguousarray([ix - 1 for ix in empty.ffidx[1]], dtype=np.int32)
        trials = draw_placements(omc, base, 1, 5, np.random.default_rng(3))
        rows = np.full((5, 4), np.nan)
        _abi.check(lib, lib.ceg_mc_trial_insert(raw, _abi.i32ptr(kinds), len(kinds), _abi.dptr(trials.reshape(-1)), 5, _abi.dptr(rows.reshape(-1))))
        assert (rows == 0.0).all(), rows
        assert lib.ceg_mc_get_state(raw, None, None, None) == 0
        lib.ceg_mc_destroy(raw)
        del keep
        dev.close()
    finally:
        ceg.setdir_RASPA(GOLDEN_RASPA)


@CELLS
def test_set_guests_with_no_molecule_then_the_first_insertions(hip_lib, tmp_path, monkeypatch, cells):
    """B2.  ceg_mc_set_guests(nmol = 0): the rows of B1's batches bit-identical to those of a fresh handle.  Then the first
    ceg_mc_insert ever (no free slot, minimum capacity), a displacement trial of that single molecule (pair column exactly 0.0, the
    reciprocal term against rest = framework alone), its accept, the first molecule of the other species, and 40 mixed steps
    (insertion trials and insertions, deletion rows and removals down to zero, displacements) against the oracle; final positions
    exactly, total structure factor to 1e-9 of its scale."""
    try:
        M, mc, empty, base = _setups(tmp_path)
        fresh = _device(_copy_setup(empty), monkeypatch, cells, upload_guests=False)
        dev = _device(empty, monkeypatch, cells, grids_from=fresh)
        omc = _oracle(empty)
        batches = _empty_box_batches(omc, base)
        # (the second set of rows is held to the first bit for bit, which the oracle has checked row by row)
        for a, b in zip(_insertion_rows(fresh, omc, batches, "fresh"), _insertion_rows(dev, omc, batches, "set_guests(0)", against_oracle=False)):
            assert np.array_equal(a, b)
        rng = np.random.default_rng(9002)
        t = draw_placements(omc, base, 0, 1, rng, blocked_share=0.0)[0]
        assert dev.insert(0, t) == omc.add(0, t) == 0
        new = _displace(rng, t, 1)[0]
        rows = dev.trial((0, 0), new[None])
        _check(rows[0], omc.movement_energy((0, 0)), "the only molecule, where it is")
        _check(rows[1], omc.movement_energy((0, 0), new), "the only molecule, displaced")
        assert rows[0, 2] == 0.0 and rows[1, 2] == 0.0
        dev.accept((0, 0), new)
        omc.update((0, 0), new)
        t = draw_placements(omc, base, 1, 1, rng, blocked_share=0.0)[0]
        assert dev.insert(1, t) == omc.add(1, t) == 0
        scale = float(np.abs(omc.total_structure_factor()).max())
        seen = dict(insert=0, inserted=0, delete=0, removed=0, emptied=0, move=0, accepted=0)
        for step in range(40):
            kind = int(rng.integers(2))
            u = rng.random()
            if u < 0.3 or not any(omc.positions):
                trials = draw_placements(omc, base, kind, 5, rng)
                rows = dev.trial_insert(kind, trials)
                for i in range(5):
                    _check(rows[i], omc.insertion_energy(kind, trials[i]), (step, "insert", i))
                seen["insert"] += 1
                if rng.random() < 0.6:
                    assert dev.insert(kind, trials[4]) == omc.add(kind, trials[4])
                    seen["inserted"] += 1
            else:
                if not omc.positions[kind]:
                    kind = 1 - kind
                j = int(rng.integers(len(omc.positions[kind])))
                if u < 0.6:
                    row = dev.trial((kind, j), np.empty((0, len(omc.ffidx[kind]), 3)))
                    assert row.shape == (1, 4)
                    _check(row[0], omc.movement_energy((kind, j)), (step, "delete"))
                    seen["delete"] += 1
                    if rng.random() < 0.8:
                        assert dev.remove((kind, j)) == omc.remove((kind, j))
                        seen["removed"] += 1
                        seen["emptied"] += not any(omc.positions)
                else:
                    trials = _displace(rng, omc.positions[kind][j], 2)
                    rows = dev.trial((kind, j), trials)
                    _check(rows[0], omc.movement_energy((kind, j)), (step, "before"))
                    for i in range(2):
                        _check(rows[1 + i], omc.movement_energy((kind, j), trials[i]), (step, "after", i))
                    seen["move"] += 1
                    if rng.random() < 0.6:
                        dev.accept((kind, j), trials[0])
                        omc.update((kind, j), trials[0])
                        seen["accepted"] += 1
            scale = max(scale, float(np.abs(omc.total_structure_factor()).max()))
        assert all(v > 0 for v in seen.values()), seen
        _final_state(dev, omc, scale, "after 40 steps")
        print(f"empty box, cells {cells}: {seen}, {sum(len(k) for k in omc.positions)} molecules at the end")
        dev.close()
        fresh.close()
    finally:
        ceg.setdir_RASPA(GOLDEN_RASPA)


@CELLS
def test_drain_and_refill(hip_lib, tmp_path, monkeypatch, cells):
    """B3.  The Na + 4 CO2 state emptied one molecule per step in a seeded order (the deletion row and the index ceg_mc_remove reports
    against the oracle's each time); with nothing left ceg_mc_get_state gives no atoms and a total structure factor within 1e-9 of
    the largest component it had at the start (of zero, and of the oracle's residue of the same subtractions); six insertions
    (the freed atom slots are taken again; the molecule indices are the oracle's), 30 displacements, final state."""
    try:
        M, mc, empty, base = _setups(tmp_path)
        dev = _device(mc, monkeypatch, cells)
        omc = _oracle(mc)
        scale = float(np.abs(omc.total_structure_factor()).max())
        rng = np.random.default_rng(9003)
        while any(omc.positions):
            kind = int(rng.integers(2))
            if not omc.positions[kind]:
                kind = 1 - kind
            j = int(rng.integers(len(omc.positions[kind])))
            row = dev.trial((kind, j), np.empty((0, len(omc.ffidx[kind]), 3)))
            _check(row[0], omc.movement_energy((kind, j)), ("delete", kind, j))
            assert dev.remove((kind, j)) == omc.remove((kind, j))
        dev.mc.positions = [[], []]
        pos, sf = dev.state()
        assert pos.shape == (0, 3)
        assert np.abs(sf).max() <= 1e-9 * scale and np.abs(sf - omc.total_structure_factor()).max() <= 1e-9 * scale
        for kind in (1, 0, 1, 1, 0, 1):
            trials = draw_placements(omc, base, kind, 5, rng)
            rows = dev.trial_insert(kind, trials)
            for i in range(5):
                _check(rows[i], omc.insertion_energy(kind, trials[i]), ("refill", kind, i))
            assert dev.insert(kind, trials[4]) == omc.add(kind, trials[4])
            scale = max(scale, float(np.abs(omc.total_structure_factor()).max()))
        assert [len(k) for k in omc.positions] == [2, 4]
        for step in range(30):
            kind = step % 2
            j = int(rng.integers(len(omc.positions[kind])))
            new = _displace(rng, omc.positions[kind][j], 1, jump=step % 7 == 0)[0]
            rows = dev.trial((kind, j), new[None])
            _check(rows[0], omc.movement_energy((kind, j)), (step, "before"))
            _check(rows[1], omc.movement_energy((kind, j), new), (step, "after"))
            if step % 3:
                dev.accept((kind, j), new)
                omc.update((kind, j), new)
            scale = max(scale, float(np.abs(omc.total_structure_factor()).max()))
        _final_state(dev, omc, scale, "drained and refilled")
        dev.close()
    finally:
        ceg.setdir_RASPA(GOLDEN_RASPA)


@CELLS
def test_group_with_empty_chains(hip_lib, tmp_path, monkeypatch, cells):
    """B4.  Four chains in lockstep, chains 1 and 3 without a molecule: 60 steps with insertion trials into the empty chains in the
    same call as displacements in the populated ones, idle empty chains, insertions by per-handle ceg_mc_insert while grouped, and
    chain 2 drained to zero by per-handle removes and refilled; every row against its chain's oracle, every branch counted."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    K = 4
    try:
        M, mc, empty, base = _setups(tmp_path)
        mcs = [_copy_setup(empty if c % 2 else mc) for c in range(K)]
        devs = []
        for c in range(K):
            devs.append(_device(mcs[c], monkeypatch, cells, grids_from=devs[0] if devs else None))
        omcs = [_oracle(m) for m in mcs]
        rngs = [np.random.default_rng(9100 + c) for c in range(K)]
        scales = [max(float(np.abs(o.total_structure_factor()).max()), 0.0) for o in omcs]
        seen = dict(idle_empty=0, insert_empty=0, inserted_into_empty=0, mixed_call=0, drain=0, drained=0, refilled=0, move=0, accepted=0, delete=0)
        with DeviceMonteCarloGroup(devs) as group:
            for step in range(60):
                ins_kind = step % 2
                moves = []
                for c in range(K):
                    rng, omc = rngs[c], omcs[c]
                    was_empty = not any(omc.positions)
                    u = rng.random()
                    if was_empty:
                        if u < 0.25:
                            moves.append(None)
                            seen["idle_empty"] += 1
                        else:
                            moves.append(("insert", ins_kind, draw_placements(omc, base, ins_kind, int(rng.integers(1, 4)), rng)))
                            seen["insert_empty"] += 1
                    elif c == 2 and step < 30:
                        kind = 0 if omc.positions[0] and (not omc.positions[1] or u < 0.5) else 1
                        j = int(rng.integers(len(omc.positions[kind])))
                        moves.append(("move", (kind, j), np.empty((0, len(omc.ffidx[kind]), 3))))
                        seen["drain"] += 1
                    elif u < 0.1:
                        moves.append(None)
                    elif u < 0.25:
                        moves.append(("insert", ins_kind, draw_placements(omc, base, ins_kind, 2, rng)))
                    else:
                        kind = int(rng.integers(2))
                        if not omc.positions[kind]:
                            kind = 1 - kind
                        j = int(rng.integers(len(omc.positions[kind])))
                        n = 0 if u < 0.35 else int(rng.integers(1, 4))
                        moves.append(("move", (kind, j), _displace(rng, omc.positions[kind][j], n) if n else np.empty((0, len(omc.ffidx[kind]), 3))))
                seen["mixed_call"] += (any(m and m[0] == "insert" and not any(omcs[c].positions) for c, m in enumerate(moves))
                                       and any(m and m[0] == "move" and len(m[2]) for m in moves))
                rows = group.trial(moves)
                accepted = [None] * K
                for c in range(K):
                    mv, r, omc, rng = moves[c], rows[c], omcs[c], rngs[c]
                    if mv is None:
                        assert r is None
                        continue
                    what, idx, trials = mv
                    was_empty = not any(omc.positions)
                    if what == "insert":
                        assert r.shape == (len(trials), 4)
                        for t in range(len(trials)):
                            _check(r[t], omc.insertion_energy(idx, trials[t]), (step, c, "insert", t))
                        if was_empty:
                            assert (r[:, 2] == 0.0).all()
                        if rng.random() < 0.5 and not (c == 2 and step < 30):
                            assert devs[c].insert(idx, trials[-1]) == omc.add(idx, trials[-1])
                            seen["inserted_into_empty"] += was_empty
                            seen["refilled"] += c == 2 and was_empty
                    elif len(trials) == 0:
                        assert r.shape == (1, 4)
                        _check(r[0], omc.movement_energy(idx), (step, c, "delete"))
                        seen["delete"] += 1
                        if c == 2 or rng.random() < 0.5:
                            assert devs[c].remove(idx) == omc.remove(idx)
                            seen["drained"] += c == 2 and not any(omc.positions)
                    else:
                        assert r.shape == (len(trials) + 1, 4)
                        _check(r[0], omc.movement_energy(idx), (step, c, "before"))
                        for t in range(len(trials)):
                            _check(r[1 + t], omc.movement_energy(idx, trials[t]), (step, c, "after", t))
                        seen["move"] += 1
                        if rng.random() < 0.6:
                            accepted[c] = (idx, trials[0])
                            omc.update(idx, trials[0])
                            seen["accepted"] += 1
                    scales[c] = max(scales[c], float(np.abs(omc.total_structure_factor()).max()))
                group.accept(accepted)
        assert all(v > 0 for v in seen.values()), seen
        for c in range(K):
            _final_state(devs[c], omcs[c], scales[c], c)
        print(f"group with empty chains, cells {cells}: {seen}; molecules at the end {[sum(len(k) for k in o.positions) for o in omcs]}")
        for d in devs[::-1]:
            d.close()
    finally:
        ceg.setdir_RASPA(GOLDEN_RASPA)
