"""The two tables of site hopping built on the device (ceg_site_tables / ceg_site_tables_device, csrc/ceg_site.hip): on the CIT-7
fixture against the ORACLE composing the reference's definition literally with one-molecule and two-molecule systems; at the tile
edges against the composed device route a caller had before (DeviceMonteCarlo trial rows plus the host constants); and end to end
through SiteHopping.from_setup and run_montecarlo against an mcrng replay on the device-built tables."""
import os
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
import interp_cases as IC
from ceg_hip import _abi, mcrng
from ceg_hip import sitehopping as SH

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "raspa"
FF = "BoulfelfelSholl2021"
NA = np.array([[3.019388765467742, 0.8997706038543032, 26.11901621898599]])
CO2 = np.array([[11.93940309885289, 8.48657378465003, 2.135736631609201], [11.10485516124311, 7.710040763525694, 1.991767166323031],
                [10.27030722363334, 6.933507742401357, 1.84779770103686]])


@pytest.fixture(scope="module")
def cit7(tmp_path_factory, hip_lib, oracle):
    """(M, the setup of Na alone, of CO2 alone): no molecule, blockfiles=[False], as the reference's constructor builds mc1 / mc2"""
    from ceg_hip.hostmirror import montecarlo as M
    raspa = tmp_path_factory.mktemp("site_tables") / "raspa"
    raspa.mkdir()
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(GOLDEN / sub, raspa / sub)
    ceg.setdir_RASPA(raspa)
    na = ceg.load_molecule_RASPA("Na", "TraPPE", FF).with_positions(NA)
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", FF).with_positions(CO2)
    out = (M, M.setup_montecarlo("CIT-7", FF, [(na, 0)], blockfiles=[False]), M.setup_montecarlo("CIT-7", FF, [(co2, 0)], blockfiles=[False]))
    yield out
    ceg.setdir_RASPA(GOLDEN)


def _min_image(mat, a, b):
    """the shortest distance between any atom of a and any atom of b over the 27 nearest images"""
    best = np.inf
    sh = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64) @ np.asarray(mat).T
    for p in np.atleast_2d(a):
        for q in np.atleast_2d(b):
            best = min(best, float(np.linalg.norm(p - q + sh, axis=1).min()))
    return best


def _oracle(mc):
    from oracle.montecarlo import OracleMonteCarlo
    return OracleMonteCarlo.from_setup(mc)


def _blocked_site(omc, shape, rng, mat):
    for _ in range(400):
        s = shape - shape[0] + mat @ rng.random(3)
        if omc.framework_interactions(0, s)[0] >= 1e90:
            return s
    raise AssertionError("no blocked site found")


def _open_site(omc, draw):
    """the first placement `draw()` offers that the framework does not block"""
    for _ in range(4000):
        s = draw()
        if omc.framework_interactions(0, s)[0] < 1e90:
            return s
    raise AssertionError("no open site found")


def _sites(mc, omc, shape, n):
    """open sites with a pair inside 2 A, pairs inside and beyond the cutoff, a pair across the cell boundary (the last two before the
    blocked one), and one site the framework blocks (the last)"""
    mat = np.asarray(mc.mat, dtype=np.float64)
    rng = np.random.default_rng(77)
    rel = shape - shape[0]

    def step(lo, hi):
        d = rng.normal(size=3)
        return d / np.linalg.norm(d) * rng.uniform(lo, hi)
    assert omc.framework_interactions(0, shape)[0] < 1e90
    sites = [shape, _open_site(omc, lambda: shape + step(1.0, 1.9)), _open_site(omc, lambda: shape + step(4.0, 8.0))]
    if n >= 8:
        sites += [_open_site(omc, lambda: shape + mat @ (np.array([0.5, 0.5, 0.5]) + 0.1 * (rng.random(3) - 0.5))),
                  _open_site(omc, lambda: rel + mat @ rng.random(3))]
    left = _open_site(omc, lambda: rel + mat @ np.array([0.97, rng.random(), rng.random()]))
    sites += [left, _open_site(omc, lambda: left + mat @ np.array([0.11 - 1.0, 0.0, 0.0]) + step(0.0, 1.0)), _blocked_site(omc, shape, rng, mat)]
    sites = np.array(sites)
    assert len(sites) == n
    cutoff = float(mc.ff.cutoff)
    near = np.array([[_min_image(mat, sites[i], sites[j]) if i != j else np.inf for j in range(n)] for i in range(n)])
    far = np.array([[min(_min_image(mat, p, q) for p in sites[i] for q in sites[j]) if i != j else 0.0 for j in range(n)] for i in range(n)])
    assert near[0, 1] < 2.0 and 2.0 < near[0, 2] < cutoff
    assert (far > cutoff).any(), "a pair with every atom pair beyond the cutoff"
    direct = min(np.linalg.norm(p - q) for p in sites[n - 3] for q in sites[n - 2])
    assert near[n - 3, n - 2] < cutoff < direct                             # close only across the cell boundary
    return sites


def _reference_tables(omc, sites):
    """sitehopping.jl:41-82 telescoped, with one-molecule and two-molecule systems of the oracle"""
    n = len(sites)
    fv, fd, rec = np.zeros(n), np.zeros(n), np.zeros(n)
    for i, s in enumerate(sites):
        omc.positions = [[np.array(s)]]
        rec[i] = omc.compute_ewald()                                # inter of one molecule is 0
        fv[i], fd[i] = omc.framework_interactions(0, s)
    inter, R = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            omc.positions = [[np.array(sites[i]), np.array(sites[j])]]
            R[i, j] = R[j, i] = omc.compute_ewald()
            inter[i, j] = inter[j, i] = omc.single_contribution_vdw(0, 0, sites[i])
    omc.positions = [[]]
    return fv, fd, rec, inter, R


def _compare_tables(got, ref, what):
    fw, rec, it = got
    fv, fd, r, inter, R = ref
    n = len(fw)
    for i in range(n):
        assert abs(rec[i] - r[i]) <= 1e-9 * abs(r[i]) + 1e-7, (what, "recip", i, rec[i], r[i])
        if fv[i] >= 1e90:
            assert fw[i] >= 1e90, (what, "blocked", i, fw[i])                  # blocked where the oracle is blocked
        else:
            want = fv[i] + fd[i] + r[i]
            assert abs(fw[i] - want) <= 1e-9 * (abs(fv[i]) + abs(fd[i]) + abs(r[i])) + 1e-7, (what, "framework", i, fw[i], want)
        assert it[i, i] == 1e100
        for j in range(n):
            if j == i:
                continue
            assert it[i, j].tobytes() == it[j, i].tobytes()
            want = inter[i, j] + R[i, j] - r[i] - r[j]
            if not np.isfinite(want) or abs(want) >= 1e90:
                assert not it[i, j] < 1e90, (what, i, j, it[i, j], want)
                continue
            tol = 1e-9 * (abs(inter[i, j]) + abs(R[i, j]) + abs(r[i]) + abs(r[j])) + 1e-7
            assert abs(it[i, j] - want) <= tol, (what, "interactions", i, j, it[i, j], want, tol)


@pytest.mark.parametrize("name,n", [("Na", 8), ("CO2", 6)])
def test_tables_against_the_oracle(cit7, name, n):
    from ceg_hip.energy import DeviceMonteCarlo
    M, mc_na, mc_co2 = cit7
    mc, shape = (mc_na, NA) if name == "Na" else (mc_co2, CO2)
    omc = _oracle(mc)
    sites = _sites(mc, omc, shape, n)
    ref = _reference_tables(omc, sites)
    assert (ref[0] >= 1e90).tolist() == [False] * (n - 1) + [True]                 # one site the framework blocks
    dev = DeviceMonteCarlo(mc, upload_guests=False)
    try:
        got = SH.build_site_tables(dev, sites)
        _compare_tables(got, ref, name)
        # with a guest the handle is refused, and nothing of it was written
        dev.insert(0, sites[0])
        with pytest.raises(_abi.CegError) as e:
            SH.build_site_tables(dev, sites)
        assert e.value.code == -5
        dev.remove((0, 0))
        again = SH.build_site_tables(dev, sites)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    finally:
        dev.close()


def _composed_route(dev, species, sites):
    """what a caller had before: n batch trials in the empty box plus, per site, an insertion and a batch trial against it"""
    mc = dev.mc
    n = len(sites)
    off1, off2 = SH.ewald_offsets(mc, species, sites[0])
    rows = dev.trial_insert(species, sites)
    rec = rows[:, 3] + off1
    inter, pair = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        dev.insert(species, sites[i])
        r = dev.trial_insert(species, sites)
        dev.remove((species, 0))
        inter[i], pair[i] = r[:, 2], r[:, 3] - rows[:, 3]
    return rows, rec, inter, pair, off2


@pytest.mark.parametrize("species", [0, 1, 5], ids=["1 atom", "3 atoms", "16 atoms"])
def test_tile_edges_on_synthetic_grids(hip_lib, species):
    from ceg_hip.energy import DeviceMonteCarlo
    import torch
    mc = IC.mc_setup("tric", blocking=True)
    dev = DeviceMonteCarlo(mc, upload_guests=False)
    rng = np.random.default_rng(40 + species)
    try:
        for n in (1, 2, 15, 16, 17, 33):
            sites = IC.mc_placements(mc, species, n, rng)
            fw, rec, it = SH.build_site_tables(dev, sites, species)
            rows, crec, inter, pair, off2 = _composed_route(dev, species, sites)
            assert it.shape == (n, n) and (np.diag(it) == 1e100).all()
            assert it.tobytes() == np.ascontiguousarray(it.T).tobytes()
            for i in range(n):
                assert abs(rec[i] - crec[i]) <= 1e-9 * abs(crec[i]) + 1e-7
                if rows[i, 0] >= 1e90 or rows[i, 1] >= 1e90:
                    assert fw[i] >= 1e90
                else:
                    assert abs(fw[i] - (rows[i, 0] + rows[i, 1] + crec[i])) <= 1e-9 * (abs(rows[i, 0]) + abs(rows[i, 1]) + abs(crec[i])) + 1e-7
                for j in range(n):
                    if i != j:
                        want = inter[i, j] + pair[i, j] + off2
                        assert abs(it[i, j] - want) <= 1e-9 * (abs(inter[i, j]) + abs(rows[i, 3]) + abs(rows[j, 3]) + abs(pair[i, j])) + 1e-7
            dfw, drec, dit = SH.build_site_tables(dev, sites, species, on_device=True)
            torch.cuda.synchronize()
            assert dfw.cpu().numpy().tobytes() == fw.tobytes() and drec.cpu().numpy().tobytes() == rec.tobytes()
            assert dit.cpu().numpy().tobytes() == it.tobytes()
    finally:
        dev.close()


@pytest.mark.parametrize("n", [17, 33])
def test_tile_edges_with_ewald_sums_and_pairs(cit7, n):
    """the same comparison where the reciprocal and the pair terms are not zero: Na in CIT-7 on random sites"""
    from ceg_hip.energy import DeviceMonteCarlo
    M, mc, _co2 = cit7
    mat = np.asarray(mc.mat, dtype=np.float64)
    rng = np.random.default_rng(n)
    sites = (mat @ rng.random((n, 3)).T).T.reshape(n, 1, 3)
    dev = DeviceMonteCarlo(mc, upload_guests=False)
    try:
        fw, rec, it = SH.build_site_tables(dev, sites)
        rows, crec, inter, pair, off2 = _composed_route(dev, 0, sites)
        assert it.tobytes() == np.ascontiguousarray(it.T).tobytes() and (np.diag(it) == 1e100).all()
        assert np.abs(pair).max() > 1.0 and np.abs(inter).max() > 1.0          # both terms are there
        for i in range(n):
            assert abs(rec[i] - crec[i]) <= 1e-9 * abs(crec[i]) + 1e-7
            for j in range(n):
                if i != j:
                    want = inter[i, j] + pair[i, j] + off2
                    if abs(want) >= 1e90:
                        assert it[i, j] >= 1e90
                        continue
                    assert abs(it[i, j] - want) <= 1e-9 * (abs(inter[i, j]) + abs(rows[i, 3]) + abs(rows[j, 3]) + abs(pair[i, j])) + 1e-7, (i, j)
    finally:
        dev.close()


def test_refusals(cit7, monkeypatch):
    from ceg_hip.energy import DeviceMonteCarlo
    M, mc, _co2 = cit7
    dev = DeviceMonteCarlo(mc, upload_guests=False)
    try:
        sites = np.tile(NA, (40, 1, 1)) + np.arange(40)[:, None, None] * 0.1
        monkeypatch.setenv("CEG_HIP_SITE_TABLE_LIMIT_MB", "1")
        with pytest.raises(_abi.CegError) as e:
            SH.build_site_tables(dev, np.tile(NA, (400, 1, 1)))             # 400 * 400 * 8 bytes > 1 MiB
        assert e.value.code == -5 and "CEG_HIP_SITE_TABLE_LIMIT_MB" in str(e.value)
        monkeypatch.delenv("CEG_HIP_SITE_TABLE_LIMIT_MB")
        bad = sites.copy(); bad[3, 0, 1] = np.nan
        with pytest.raises(_abi.CegError) as e:
            SH.build_site_tables(dev, bad)
        assert e.value.code == -1
    finally:
        dev.close()


def test_end_to_end_run_montecarlo(cit7):
    M, mc, _co2 = cit7
    mat = np.asarray(mc.mat, dtype=np.float64)
    omc = _oracle(mc)
    rng = np.random.default_rng(5)
    sites = []
    while len(sites) < 8:                                                   # open sites only
        s = NA - NA[0] + mat @ rng.random(3)
        if omc.framework_interactions(0, s)[0] < 1e90:
            sites.append(s)
    sh = SH.SiteHopping.from_setup(mc, np.array(sites), 3, seed=11)
    assert repr(sh) == "SiteHopping setup with 3 molecules among 8 sites" and len(set(sh.population.tolist())) == 3
    ninit, ncycles, m = 2, 6, 3
    T = np.array([2000.0] * ninit + [1500.0, 1200.0, 900.0, 600.0, 400.0, 300.0])
    with SH.DeviceSiteHoppingGroup.from_setups([sh]) as g:
        run = SH.run_montecarlo(g, T, ncycles, ninit, printevery=2, seed=99, track_min=True)          # the drift check passes
    assert run.cycles.tolist() == [0, 2, 4, 6] and run.energies.shape == (4, 1) and run.populations.shape == (4, 1, m)
    assert abs(run.initial_energy[0] - sh.baseline_energy()) <= 1e-9 * abs(sh.baseline_energy())
    first = mcrng.site_replay(sh.frameworkenergies, sh.interactions, sh.population, run.initial_energy[0], 99, 0, 0, T[:ninit], m)
    assert np.array_equal(run.populations[0, 0], first.population)
    second = mcrng.site_replay(sh.frameworkenergies, sh.interactions, first.population, run.energies[0, 0], 99, ninit * m, 0, T[ninit:], m)
    for f, idx in enumerate(run.cycles.tolist()[1:], start=1):
        assert np.array_equal(run.populations[f, 0], second.cycle_population[idx - 1])
        assert run.energies[f, 0].tobytes() == second.cycle_energy[idx - 1].tobytes()
    assert run.records["energy"][ninit:, 0].tobytes() == second.cycle_energy.tobytes()
    assert int(run.stats["attempted"][0]) == (ninit + ncycles) * m and int(run.stats["accepted"][0]) == first.accepted + second.accepted
    assert run.stats["accepted"][0] > 0
    mink, mine = mcrng.track_minimum(second.cycle_energy.reshape(-1, 1), run.energies[0], cycle0=1)
    assert run.minimum[0].tolist() == np.where(mink < 0, 0, mink).tolist() and run.minimum[1].tobytes() == mine.tobytes()
    # N quenches from random starts in one group
    q = SH.run_random_quenching(sh, 5, T[ninit:], ncycles, seed=3)
    assert q.start.shape == (5, m) and all(len(set(p.tolist())) == m for p in q.start)
    assert np.array_equal(q.start[2], mcrng.site_random_population(3, 2, 8, m)) and q.run.minimum[1].shape == (5,)
    assert (q.run.minimum[1] <= q.run.initial_energy).all()
