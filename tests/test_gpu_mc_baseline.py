"""ceg_mc_baseline / ceg_mc_group_baseline: baseline_energy (montecarlo.jl:530-542) of one chain or of all chains of a group from
the device-resident state.  Run with `pytest -m gpu` on an MI355X.

Reference.  Composed here from oracle/montecarlo.OracleMonteCarlo, nothing of the product in it: framework terms = the sum of
framework_interactions over the molecules, inter = 1/2 the sum of single_contribution_vdw(i, j, current positions), the two k-space
sums from total_structure_factor() with the setup's kfactors and framework structure factor.  hostmirror.montecarlo.baseline_energy
is a second assert, DeviceMonteCarlo.baseline_energy(route="rows") a third.

Tolerance per term: |device - oracle| <= 1e-9 * sum over the molecules of |that molecule's oracle term| + 1e-7 * max(nmol, 1) (the
per-row tolerance of the project, summed as test_sweep_energy_bookkeeping sums it); a term >= 1e90 on the oracle (blocked atoms)
must be >= 1e90 on the device.  The per-molecule terms of the k-space sums are sum_k kf Re(conj(S_fw) S_m) and
sum_k kf Re(conj(S) S_m), whose sums over the molecules are the two quantities.  The composed reciprocal energy
2 (recip_framework + energy_net_charges) + recip_guests + static_contribution carries the tolerances of its two sums (the first
twice) plus 1e-9 of |2 energy_net_charges + static_contribution|, the two constants being computed by two implementations.

Populations: 85 CO2 + 2 Na at open sites of the CIT-7 2x3x3 cell (the _populate of test_gpu_mc_many_molecules), built once; every
smaller population is a prefix of it, so that the occupied atom-slot counts are 1, 3, 63, 64, 65, 129 and 257: the smallest that
fill, cross and leave one short the 64-slot tiles of the kernel, with one, two, three and five tiles."""
import ctypes as C

import numpy as np
import pytest

from ceg_hip import _abi, mcrng
from test_gpu_mc_chains import _check, _displace
from test_gpu_mc_many_molecules import _device_chain, _oracle, _populate, _two_kinds
from test_gpu_mc_sweep import SEED, _chains, _close, _copy, _device_order, setup  # noqa: F401  (setup: the module's fixture)
from test_gpu_mc_sweep_gcmc import Replay, _tail

pytestmark = pytest.mark.gpu

TERMS = ("framework_vdw", "framework_direct", "inter", "recip_framework", "recip_guests")
_CACHE = {}


def _population(mc, n_na, n_co2):
    """(setup with the kinds [Na, CO2] and no molecules, positions of the first n_na Na and n_co2 CO2 of the one population)"""
    if "pop" not in _CACHE:
        mcd = _two_kinds(mc)
        _CACHE["pop"] = (mcd, _populate(mcd, (2, 85), 20261))
    mcd, full = _CACHE["pop"]
    return mcd, [full[0][:n_na], full[1][:n_co2]]


def _reference(omc):
    """the oracle's terms: value and sum of |per-molecule term| of each, nmol, natoms"""
    mols = list(omc.molecules())
    n = len(mols)
    fv, fd, inter = np.zeros(n), np.zeros(n), np.zeros(n)
    for m, (i, j, pos) in enumerate(mols):
        fv[m], fd[m] = omc.framework_interactions(i, pos)
        inter[m] = omc.single_contribution_vdw(i, j, pos)
    value = {"framework_vdw": float(fv.sum()), "framework_direct": float(fd.sum()), "inter": 0.5 * float(inter.sum()),
             "recip_framework": 0.0, "recip_guests": 0.0}
    scale = {"framework_vdw": float(np.abs(fv).sum()), "framework_direct": float(np.abs(fd).sum()), "inter": float(np.abs(inter).sum()),
             "recip_framework": 0.0, "recip_guests": 0.0}
    if omc.has_ewald:
        assert omc.sums_re is not None and omc.sums_re.shape[1] == 1 + n
        kf = np.asarray(omc.ef.kfactors, dtype=np.float64)
        fr, fi = np.asarray(omc.ef.sf_re, dtype=np.float64), np.asarray(omc.ef.sf_im, dtype=np.float64)
        s = omc.total_structure_factor()
        mr, mi = omc.sums_re[:, 1:], omc.sums_im[:, 1:]
        value["recip_framework"] = float((kf * (fr * s.real + fi * s.imag)).sum())
        value["recip_guests"] = float((kf * (s.real ** 2 + s.imag ** 2)).sum())
        scale["recip_framework"] = float(np.abs((kf[:, None] * (fr[:, None] * mr + fi[:, None] * mi)).sum(axis=0)).sum())
        scale["recip_guests"] = float(np.abs((kf[:, None] * (s.real[:, None] * mr + s.imag[:, None] * mi)).sum(axis=0)).sum())
    return {"value": value, "scale": scale, "nmol": n, "natoms": sum(len(p) for _i, _j, p in mols)}


def _tol(ref, name):
    return 1e-9 * ref["scale"][name] + 1e-7 * max(ref["nmol"], 1)


def _close_enough(got, want, tol, what):
    print(f"  {what}: device {got!r}, reference {want!r}, |difference| {abs(got - want) if abs(want) < 1e90 else float('nan'):.3e}, tolerance {tol:.3e}")
    if not np.isfinite(want) or abs(want) >= 1e90:
        assert got >= 1e90 and want >= 1e90, (what, got, want)
    else:
        assert abs(got - want) <= tol, (what, got, want, tol)


def _check_record(rec, ref, what):
    assert (int(rec["nmol"]), int(rec["natoms"])) == (ref["nmol"], ref["natoms"]), (what, rec, ref["nmol"], ref["natoms"])
    for name in TERMS:
        _close_enough(float(rec[name]), ref["value"][name], _tol(ref, name), (what, name))


def _oracle_constants(omc):
    from oracle import hostlogic as H
    if not omc.has_ewald:
        return 0.0, 0.0
    kinds = [(omc._mol_charges(i), kind[0], len(kind)) for i, kind in enumerate(omc.positions) if kind]
    return H.ewald_context_constants(omc.ef, kinds)


def _check_report(rep, ref, omc, tailcorrection, what):
    """a BaselineEnergyReport against the oracle's terms and the oracle's two constants"""
    _close_enough(rep.framework_vdw, ref["value"]["framework_vdw"], _tol(ref, "framework_vdw"), (what, "framework_vdw"))
    _close_enough(rep.framework_direct, ref["value"]["framework_direct"], _tol(ref, "framework_direct"), (what, "framework_direct"))
    _close_enough(rep.inter, ref["value"]["inter"], _tol(ref, "inter"), (what, "inter"))
    enc, static = _oracle_constants(omc)
    want = (2 * (ref["value"]["recip_framework"] + enc) + ref["value"]["recip_guests"] + static) if omc.has_ewald else 0.0
    tol = 2 * _tol(ref, "recip_framework") + _tol(ref, "recip_guests") + 1e-9 * abs(2 * enc + static)
    _close_enough(rep.reciprocal, want, tol, (what, "reciprocal"))
    assert rep.tailcorrection == tailcorrection, what


def _same_reports(a, b, ref, what):
    """two BaselineEnergyReports of one state from two routes, at the tolerance of the terms"""
    for name in ("framework_vdw", "framework_direct", "inter"):
        _close_enough(getattr(a, name), getattr(b, name), _tol(ref, name), (what, name))
    _close_enough(a.reciprocal, b.reciprocal, 2 * _tol(ref, "recip_framework") + _tol(ref, "recip_guests") + 1e-9 * abs(b.reciprocal), (what, "reciprocal"))


def _reference_of(mc, n_na, n_co2):
    key = ("ref", n_na, n_co2)
    if key not in _CACHE:
        mcd, pos = _population(mc, n_na, n_co2)
        omc = _oracle(mcd, pos)
        _CACHE[key] = (omc, _reference(omc))
    return _CACHE[key]


# ------------------------------------------------------------------ 1. small shapes
@pytest.mark.parametrize("n_na,n_co2,slots", [(1, 0, 1), (0, 1, 3), (0, 21, 63), (1, 21, 64), (2, 21, 65), (0, 43, 129), (2, 85, 257)])
def test_small_shapes(setup, n_na, n_co2, slots):
    """occupied atom slots 1, 3 (one CO2 alone: the pairs inside a molecule give inter = 0 exactly), 63, 64, 65, 129, 257: the device
    record against the oracle, the device route against the rows route and against the host mirror"""
    from ceg_hip.hostmirror import montecarlo as M
    mc, _owner = setup
    mcd, pos = _population(mc, n_na, n_co2)
    omc, ref = _reference_of(mc, n_na, n_co2)
    assert ref["natoms"] == slots
    dev = _device_chain(setup, mcd, pos)
    rec = dev.baseline_record()
    _check_record(rec, ref, slots)
    if ref["nmol"] == 1:
        assert float(rec["inter"]) == 0.0
    assert dev.baseline_record().tobytes() == rec.tobytes()                  # an unchanged state gives identical bytes
    device = dev.baseline_energy(route="device")
    _check_report(device, ref, omc, dev.mc.tailcorrection, (slots, "device"))
    _same_reports(device, dev.baseline_energy(), ref, (slots, "device against rows"))
    _same_reports(device, M.baseline_energy(_copy(mcd, pos)), ref, (slots, "device against the host mirror"))
    dev.close()


# ------------------------------------------------------------------ 2. holes and growth
def test_holes_and_growth(setup):
    """the 129-slot population, three molecules removed from the middle, then one Na (which fits no hole: fresh slots at the
    high-water mark) and one CO2 (which takes a hole) inserted: two holes stay, nmol and natoms are exact"""
    mc, _owner = setup
    mcd, pos = _population(mc, 0, 43)
    _m, full = _population(mc, 2, 85)
    dev = _device_chain(setup, mcd, pos)
    omc = _oracle(mcd, pos)
    for j in (20, 21, 7):
        dev.remove((1, j))
        omc.remove((1, j))
    for i, p in ((0, full[0][0]), (1, full[1][50])):
        dev.insert(i, p)
        omc.add(i, p)
    ref = _reference(omc)
    assert (ref["nmol"], ref["natoms"]) == (42, 124)
    rec = dev.baseline_record()
    _check_record(rec, ref, "holes")
    _check_record(dev.baseline_record(refresh=True), ref, "holes, refreshed")
    dev.close()


# ------------------------------------------------------------------ 3. blocked atoms
def test_blocked_atoms(setup):
    """the Na of the 65-slot population moved onto a point where the oracle's interpolation of its VdW grid gives 1e100, then (where
    the setup has such a point) onto one where the Coulomb grid gives exactly 1e100: the flagged term >= 1e90 on both sides, the
    others within tolerance"""
    from oracle import oracle as O
    mc, _owner = setup
    mcd, pos = _population(mc, 2, 21)
    dev = _device_chain(setup, mcd, pos)
    omc = _oracle(mcd, pos)
    rng = np.random.default_rng(5)
    points = rng.uniform(0.0, 1.0, (20000, 3)) @ np.asarray(mcd.mat, dtype=np.float64).T
    done = 0
    for term, grid in (("framework_vdw", omc.grids[mcd.ffidx[0][0] - 1]), ("framework_direct", omc.coulomb)):
        hit = np.nonzero(O.interpolate_points(grid, points, nthreads=1) == 1e100)[0]
        if len(hit) == 0:
            print(f"no point of the {term} grid interpolates to 1e100 among {len(points)}: nothing to flag")
            continue
        p = points[hit[0]][None, :]
        dev.accept((0, 1), p)
        omc.update((0, 1), p)
        ref = _reference(omc)
        assert ref["value"][term] >= 1e90
        rec = dev.baseline_record()
        assert float(rec[term]) >= 1e90
        _check_record(rec, ref, ("blocked", term))
        done += 1
    assert done >= 1                                                         # the VdW grid of Na has blocked nodes
    dev.close()


# ------------------------------------------------------------------ 4. and 5. the group
def _group_chains(setup, monkeypatch, cells):
    """[empty box, the Na + 4 CO2 setup, the 65-slot population, (cells:) a chain with neighbour cells, an exact chain] with oracles"""
    from ceg_hip.energy import DeviceMonteCarlo
    mc, owner = setup
    devs, omcs = [], []
    mcd, _p = _population(mc, 0, 0)
    devs.append(DeviceMonteCarlo(_copy(mcd, [[], []]), grids_from=owner))
    omcs.append(_oracle(mcd, [[], []]))
    d5, o5 = _chains(setup, 1, oracle=True)
    devs += d5
    omcs += o5
    _m, pos = _population(mc, 2, 21)
    devs.append(_device_chain(setup, mcd, pos))
    omcs.append(_oracle(mcd, pos))
    if cells:
        _m, pos = _population(mc, 1, 21)
        monkeypatch.setenv("CEG_HIP_MC_CELLS", "1")
        devs.append(_device_chain(setup, mcd, pos))
        monkeypatch.delenv("CEG_HIP_MC_CELLS")
        assert devs[-1].neighbour_cells() is not None
        omcs.append(_oracle(mcd, pos))
    _m, pos = _population(mc, 0, 21)
    devs.append(_device_chain(setup, mcd, pos, exact=True))
    omcs.append(_oracle(mcd, pos))
    return devs, omcs


def test_group(setup, monkeypatch):
    """five chains of five kinds in one group: every member against its own oracle, byte for byte what ceg_mc_baseline gave for the
    handle before it was grouped, and the same bytes from a second group call"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs, omcs = _group_chains(setup, monkeypatch, cells=True)
    alone = [d.baseline_record().tobytes() for d in devs]
    with DeviceMonteCarloGroup(devs) as group:
        recs = group.baseline_records()
        again = group.baseline_records()
        member = [d.baseline_record().tobytes() for d in devs]               # a grouped handle through its own entry point
        reports = group.baseline_energies()
    assert recs.tobytes() == again.tobytes()
    for c, (d, o) in enumerate(zip(devs, omcs)):
        ref = _reference(o)
        _check_record(recs[c], ref, ("group", c))
        assert recs[c].tobytes() == alone[c] == member[c], (c, recs[c])
        _check_report(reports[c], ref, o, d.mc.tailcorrection, ("group report", c))
    assert not np.asarray(recs[0].tolist()).any()                            # the empty box: zeros
    _close(devs)


def test_after_gcmc_sweeps(setup, monkeypatch):
    """the group without the cells chain after 60 steps of sweep_gcmc with swaps and positions=False: every member against the oracle
    state replayed from the log, the constants from the new counts, and the bookkeeping
    after - before = delta_moves + delta_swaps + sum over accepted swaps of (+-self_reciprocal - tc) + the change of
    2 energy_net_charges + static_contribution (the oracle's), within 1e-9 (|before| + |after|) + 1e-7 accepted: what
    compute_accept_move_swap calls diff is +-(E - self_reciprocal) + tc, while the state gains or loses E and the two constants."""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs, omcs = _group_chains(setup, monkeypatch, cells=False)
    K, S = len(devs), 60
    T = np.array([300.0, 500.0, 400.0, 600.0])
    sid = np.array([4, 9, 1, 6], dtype=np.uint32)
    caps = [len(_device_order(d)) + 6 for d in devs]
    moves = [mcrng.MoveTable(translation=1, random_translation=1, swap=1),
             mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1, random_reinsertion=1, swap=4)]
    assert moves[1].swap > 0
    with DeviceMonteCarloGroup(devs) as group:
        table = _tail(group.gcmc_species(moves, [1e9, 1e9]))
        reps = [Replay(d.mc, o, _device_order(d), table, T[c], 0.4, 0.8, caps[c]) for c, (d, o) in enumerate(zip(devs, omcs))]
        c_before = [_oracle_constants(o) for o in omcs]
        before = group.baseline_energies()
        stats, log = group.sweep_gcmc(S, SEED + 77, 0, temperature=T, dmax=0.4, thetamax=0.8, species=table, max_molecules=caps,
                                      stream_id=sid, log=True, positions=False)
        assert all(p is None for d in devs for kind in d.mc.positions for p in kind)
        recs = group.baseline_records()
        after = group.baseline_energies()
    checked = swaps = 0
    for c, rep in enumerate(reps):
        for s in range(S):
            rep.step(SEED + 77, s, int(sid[c]), log[s, c], (s, c))
        rep.check_stats(stats[c], c)
        assert [len(k) for k in devs[c]._slot] == [len(k) for k in rep.omc.positions]
        ref = _reference(rep.omc)
        _check_record(recs[c], ref, ("after the sweep", c))
        _check_report(after[c], ref, rep.omc, devs[c].mc.tailcorrection, ("after the sweep, report", c))
        accepted = int(stats[c]["accepted"].sum())
        swaps += int(stats[c]["accepted"][5:].sum())
        sw = log[:, c][(log["accepted"][:, c] != 0) & (log["kind"][:, c] >= 5)]
        extra = sum((1.0 if r["kind"] == 5 else -1.0) * float(table["self_reciprocal"][r["species"]]) - float(r["tc"]) for r in sw)
        enc0, st0 = c_before[c]
        enc1, st1 = _oracle_constants(rep.omc)
        b, a = float(before[c]), float(after[c])
        want = float(stats[c]["delta_moves"]) + float(stats[c]["delta_swaps"]) + extra + (2 * enc1 + st1) - (2 * enc0 + st0)
        print(f"chain {c}: baseline {b!r} -> {a!r}, bookkeeping {want!r}, accepted {accepted} ({len(sw)} swaps), counts {[len(k) for k in devs[c]._slot]}")
        if max(abs(b), abs(a), abs(want)) >= 1e90:                           # blocked atoms before or after: nothing a tolerance can test
            continue
        assert abs((a - b) - want) <= 1e-9 * (abs(b) + abs(a)) + 1e-7 * max(accepted, 1), (c, b, a, want)
        checked += 1
    assert checked >= 2 and swaps > 0, (checked, swaps)
    _close(devs)


# ------------------------------------------------------------------ 6. refresh
def test_refresh(setup):
    """200 accepted displacements through ceg_mc_accept, then CEG_MC_BASELINE_REFRESH: the structure factor of state() agrees with
    the oracle's to 1e-9 of its largest modulus, a later trial row agrees with the oracle, and a call without the flag leaves
    state() as it was, byte for byte"""
    mc, _owner = setup
    mcd, pos = _population(mc, 1, 21)
    dev = _device_chain(setup, mcd, pos)
    omc = _oracle(mcd, pos)
    rng = np.random.default_rng(11)
    for s in range(200):
        kind = 0 if s % 20 == 0 else 1
        j = int(rng.integers(len(omc.positions[kind])))
        new = _displace(rng, omc.positions[kind][j], 1)[0]
        dev.accept((kind, j), new)
        omc.update((kind, j), new)
    p0, s0 = dev.state()
    plain = dev.baseline_record()
    p1, s1 = dev.state()
    assert p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes()
    incremental = omc.total_structure_factor().copy()
    omc.compute_ewald()                                                      # what the refresh does: every column from the positions
    osf = omc.total_structure_factor()
    refreshed = dev.baseline_record(refresh=True)
    p2, s2 = dev.state()
    assert p2.tobytes() == p0.tobytes()
    top = np.abs(osf).max()
    print(f"structure factor: |device - oracle| before {np.abs(s0 - osf).max():.3e}, after the refresh {np.abs(s2 - osf).max():.3e}; "
          f"oracle incremental against recomputed {np.abs(incremental - osf).max():.3e}; largest modulus {top:.3e}")
    assert np.abs(s2 - osf).max() <= 1e-9 * top
    ref = _reference(omc)
    _check_record(plain, ref, "before the refresh")
    _check_record(refreshed, ref, "refreshed")
    assert dev.baseline_record().tobytes() == refreshed.tobytes()            # the sums of the refreshed state, without the flag
    _check(dev.trial((1, 3), np.empty((0, 3, 3)))[0], omc.movement_energy((1, 3)), "row after the refresh")
    new = _displace(rng, omc.positions[1][5], 1)
    _check(dev.trial((1, 5), new)[1], omc.movement_energy((1, 5), new[0]), "trial after the refresh")
    dev.close()


# ------------------------------------------------------------------ 7. no Ewald
def test_no_ewald(setup, hip_lib):
    """a handle created through the C ABI from the same tables with nk = 0 and no Coulomb grid: framework_direct and the two k-space
    sums are exactly 0, the rest within tolerance"""
    from ceg_hip.hostmirror.constants import COULOMBIC_CONVERSION_FACTOR
    lib = hip_lib
    mc, owner = setup
    mcd, pos = _population(mc, 2, 21)
    _omc, ref = _reference_of(mc, 2, 21)
    rules, offsets, handles, charge = owner._keep
    matT = np.ascontiguousarray(np.asarray(mcd.mat, dtype=np.float64).T.reshape(9))
    invT = np.ascontiguousarray(np.asarray(mcd.invmat, dtype=np.float64).T.reshape(9))
    h = C.c_void_p()
    _abi.check(lib, lib.ceg_mc_create(C.byref(h), 0, handles, None, _abi.dptr(charge), mcd.ff.nkinds, _abi.dptr(matT), _abi.dptr(invT),
                                      mcd.ff.cutoff ** 2, rules.ctypes.data, _abi.i32ptr(offsets), COULOMBIC_CONVERSION_FACTOR,
                                      None, None, None, None, 0, None, None))
    try:
        flat = np.ascontiguousarray(np.concatenate([p for kind in pos for p in kind]), dtype=np.float64)
        kinds = np.ascontiguousarray([ix - 1 for i, kind in enumerate(pos) for _p in kind for ix in mcd.ffidx[i]], dtype=np.int32)
        first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(p) for kind in pos for p in kind])]), dtype=np.int32)
        _abi.check(lib, lib.ceg_mc_set_guests(h, _abi.dptr(flat.reshape(-1)), _abi.i32ptr(kinds), _abi.i32ptr(first), len(first) - 1))
        for flags in (0, _abi.MC_BASELINE_REFRESH):
            rec = np.zeros(1, dtype=_abi.MC_BASELINE_DTYPE)
            _abi.check(lib, lib.ceg_mc_baseline(h, flags, rec.ctypes.data))
            r = rec[0]
            assert float(r["framework_direct"]) == 0.0 and float(r["recip_framework"]) == 0.0 and float(r["recip_guests"]) == 0.0, r
            assert (int(r["nmol"]), int(r["natoms"])) == (ref["nmol"], ref["natoms"])
            for name in ("framework_vdw", "inter"):
                _close_enough(float(r[name]), ref["value"][name], _tol(ref, name), ("no Ewald", flags, name))
    finally:
        lib.ceg_mc_destroy(h)


# ------------------------------------------------------------------ 8. refusals on the device
def test_poisoned_member_is_refused(setup, monkeypatch):
    """a member marked inconsistent by a failed ceg_mc_accept (the test hook of the library: no kernel is launched on bad data) makes
    ceg_mc_group_baseline fail with CEG_ERR_HIP and its index, ceg_mc_baseline on it likewise; the other members' states stay as
    they were, and after ceg_mc_set_guests on the member the group call works again"""
    from ceg_hip.energy import DeviceMonteCarloGroup
    devs, omcs = _chains(setup, 3, oracle=True)
    with DeviceMonteCarloGroup(devs) as group:
        good = group.baseline_records()
        states = [d.state() for d in devs]
        monkeypatch.setenv("CEG_HIP_MC_INJECT_FAILURE", "accept")
        with pytest.raises(_abi.CegError) as ei:
            devs[1].accept((0, 0), devs[1].mc.positions[0][0] + 0.1)
        assert ei.value.code == -3
        monkeypatch.delenv("CEG_HIP_MC_INJECT_FAILURE")
        for refresh in (False, True):
            with pytest.raises(_abi.CegError) as ei:
                group.baseline_records(refresh=refresh)
            assert ei.value.code == -3 and "chain 1" in str(ei.value)
            with pytest.raises(_abi.CegError) as ei:
                devs[1].baseline_record(refresh=refresh)
            assert ei.value.code == -3
        for c in (0, 2):
            p, s = devs[c].state()
            assert p.tobytes() == states[c][0].tobytes() and s.tobytes() == states[c][1].tobytes()
            assert devs[c].baseline_record().tobytes() == good[c].tobytes()
        devs[1].refresh()
        assert group.baseline_records().tobytes() == good.tobytes()
    _check_record(good[0], _reference(omcs[0]), "the setup's own state")
    _close(devs)
