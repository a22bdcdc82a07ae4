"""The ORACLE's Monte-Carlo state (oracle/montecarlo.OracleMonteCarlo) with no guest at all: what the GPU tests of the empty box
(tests/test_gpu_mc_empty_box.py) lean on has to be right there itself.  CPU only: the framework grids come from the oracle's own
loop nests at a coarse 0.8 A step (the framework columns do not depend on the guests, and not on the step being the product's)."""
import math

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import grids as G
from ceg_hip.hostmirror import montecarlo as M
from ceg_hip.hostmirror.probes import ProbeSystem
from ceg_hip.hostmirror.utils import find_supercell

FFNAME = "BoulfelfelSholl2021"
NA = [[3.019388765467742, 0.8997706038543032, 26.11901621898599]]
CO2 = np.array([[11.93940309885289, 8.48657378465003, 2.135736631609201], [11.10485516124311, 7.710040763525694, 1.991767166323031],
                [10.27030722363334, 6.933507742401357, 1.84779770103686]])
SHIFTS = [[0, 0, 0], [-5.6, -0.4, 6.5], [3.0, 9.0, 11.0], [-8.0, 14.0, 4.0]]
RECIPROCAL_RTOL = 4 * 1.42e-12     # 4 x the measured worst case, see test_oracle_state_with_no_guests
SEED = 5150            # the placements of the GPU tests are drawn the same way (uniform fractional positions, random rotations)


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def placements(mat, base, kind, n, rng):
    """n insertion placements of species `kind` (0: Na, 1: CO2 with geometry `base` about its carbon): uniform fractional positions
    in the MC cell, every CO2 with a rotation of its own"""
    centres = (mat @ rng.uniform(0, 1, (n, 3)).T).T
    if kind == 0:
        return centres[:, None, :]
    return np.array([c + base @ rotation(rng).T for c in centres])


def draw_placements(omc, base, kind, n, rng, blocked_share=0.2):
    """n insertion placements of which int(blocked_share * n) are blocked and the others open ON THE ORACLE ALONE (its interpolation
    of the VdW grids gives the 1e100 blocking value, grids.jl:245-248), picked in drawing order from uniform candidates.  Uniform
    placements in CIT-7 are blocked three times out of four (measured below), so a kernel that blocked everything would pass most rows
    of an unfiltered draw."""
    from oracle import oracle as O
    want_blocked = int(blocked_share * n)
    out, nb = [], 0
    while len(out) < n:
        cand = placements(omc.mat, base, kind, 4 * n, rng)
        hit = np.zeros(len(cand), dtype=bool)
        for a, ix in enumerate(omc.ffidx[kind]):
            hit |= O.interpolate_points(omc.grids[ix - 1], cand[:, a, :]) >= 1e90
        for t, b in zip(cand, hit):
            if len(out) == n:
                break
            if b and nb < want_blocked:
                out.append(t); nb += 1
            elif not b and len(out) - nb < n - want_blocked:
                out.append(t)
    return np.array(out)


def _mol(name, positions):
    return ceg.load_molecule_RASPA(name, "TraPPE", FFNAME).with_positions(positions)


@pytest.fixture(scope="module")
def setups(oracle, forcefield):
    """(populated Na + 4 CO2 setup, setup of the same two species without molecules) in CIT-7 on oracle-built grids"""
    cache = {}

    def from_oracle(grid_path, syst_framework, ff, gridstep, atom_or_ef, mat, new, cutoff, ngpus=1):
        iscoulomb = isinstance(atom_or_ef, ceg.EwaldFramework)
        if not iscoulomb and not ff.needsvdwgrid(atom_or_ef):
            return G.EnergyGrid.trivial(True)
        key = ("coulomb" if iscoulomb else atom_or_ef, gridstep)
        if key not in cache:
            cset = ceg.GridCoordinatesSetup.from_cell(syst_framework.mat, gridstep)
            if iscoulomb:
                lam, thr = G.coulomb_scaling()
                g, _ = oracle.grid_coulomb(ProbeSystem.build(syst_framework, forcefield), atom_or_ef.alpha, cset, lam, thr)
            else:
                lam, thr = G.vdw_scaling()
                g, _ = oracle.grid_vdw(ProbeSystem.build(syst_framework, forcefield, atom_or_ef), cset, lam, thr)
            kelvin = (g.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32)                 # parse_grid, grids.jl:78
            cache[key] = G.EnergyGrid(cset, tuple(find_supercell(syst_framework.mat, 12.0)), 1e-6 if iscoulomb else math.inf, True, kelvin)
        return cache[key]

    mp = pytest.MonkeyPatch()
    mp.setattr(M, "retrieve_or_create_grid", from_oracle)
    try:
        full = M.setup_montecarlo("CIT-7", FFNAME, [_mol("Na", NA)] + [_mol("CO2", CO2 + np.array(s)) for s in SHIFTS], gridstep=0.8)
        empty = M.setup_montecarlo("CIT-7", FFNAME, [(_mol("Na", NA), 0), (_mol("CO2", CO2), 0)], gridstep=0.8)
    finally:
        mp.undo()
    return full, empty


def _longdouble_reciprocal(ef, pos, q):
    """2 sum kf Re(conj(S_fw) S) + sum kf |S|^2, S = sum_a q_a exp(i k.r_a), from the EwaldFramework's kvec_ijk, kfactors and cell matrix and plain
    cos / sin in numpy.longdouble (no power tables).  Also the largest partial-sum magnitude, to tell where a deviation comes from."""
    ld = np.longdouble
    inv = np.asarray(ef.invmat, dtype=ld)
    frac = np.asarray(pos, dtype=ld).reshape(-1, 3) @ inv.T                     # invmat * r
    ijk = np.asarray(ef.kvec_ijk, dtype=ld).reshape(-1, 3)
    twopi = ld(2) * np.arccos(ld(-1))
    ang = twopi * (ijk @ frac.T)                                               # [nk, natoms]
    qq = np.asarray(q, dtype=ld)
    sr, si = (np.cos(ang) * qq).sum(axis=1), (np.sin(ang) * qq).sum(axis=1)
    kf = np.asarray(ef.kfactors, dtype=ld)
    fw = np.asarray(ef.StoreRigidChargeFramework)
    fr, fi = np.asarray(fw.real, dtype=ld), np.asarray(fw.imag, dtype=ld)
    terms = np.concatenate([2 * kf * (fr * sr + fi * si), kf * (sr * sr + si * si)])
    return float(terms.sum()), float(np.abs(terms).sum())


def test_oracle_state_with_no_guests(setups):
    """B0.  For 24 placements of an inserted Na and 24 of an inserted CO2 (a sixth of them blocked), an OracleMonteCarlo with empty
    position lists (built directly, by from_setup of a setup without molecules, and by removing every molecule of the populated
    state) gives: inter == 0.0 exactly; the framework columns of the same placement in the populated Na + 4 CO2 state, to the bit;
    a reciprocal term equal to an 80-bit evaluation of 2 sum kf Re(conj(S_fw) S) + sum kf |S|^2 from plain cos / sin.
    The bound on that last comparison: 1e-12 relative was the plan (two FP64 sums of ~1.8 k terms each against an 80-bit sum).
    Measured: 1.68e-13 on the placements drawn here, but 1.41e-12 on a uniform draw of 48 that held a CO2 placement whose value is
    5.05e-3 of sum|terms| (2.1608464706648 vs 2.1608464706617): the deviation is 9.6e-15 of sum|terms| there and at most 1.8e-14
    of it anywhere, i.e. rounding of the summands, magnified by the cancellation between the framework term and the self term.  The
    bound is therefore 4 x that measured worst case, RECIPROCAL_RTOL = 5.7e-12.  (The drained state carries the residue of its five
    subtractions and is held to the MC tests' 1e-9 + 1e-7 K instead.)
    Blocked placements: uniform fractional positions in CIT-7 are blocked for Na 0.69 and for CO2 0.76 of the time on these grids
    (printed), far more than the quarter the GPU tests may contain, so they draw theirs with draw_placements."""
    from oracle.montecarlo import OracleMonteCarlo
    from oracle import hostlogic as H
    full, empty = setups
    assert [len(k) for k in empty.positions] == [0, 0]
    ofull = OracleMonteCarlo.from_setup(full)
    ofull.compute_ewald()
    direct = OracleMonteCarlo(full.mat, full.ff.cutoff, *full.ff.pair_table(), full.ff.nkinds, full.ffidx, full.charges, [[], []], full.grids,
                              full.coulomb, H.adapt_ewald_framework(full.ewald))
    drained = OracleMonteCarlo.from_setup(full)
    drained.compute_ewald()
    for kind in (1, 0):
        while drained.positions[kind]:
            drained.remove((kind, 0))
    from_empty = OracleMonteCarlo.from_setup(empty)
    states = {"direct": direct, "from_setup(empty)": from_empty, "drained": drained}
    for name in ("direct", "from_setup(empty)"):
        assert np.isfinite(states[name].compute_ewald())
        assert states[name].sums_re.shape == (direct.ef.num_kvecs, 1) and not states[name].sums_re.any() and not states[name].sums_im.any()
    assert drained.flat_positions().shape == (0, 3)
    rng = np.random.default_rng(SEED)
    base = CO2 - CO2[1]
    devs, blocked = [], {}
    uniform = {}
    for kind in (0, 1):
        u = placements(full.mat, base, kind, 400, rng)
        uniform[kind] = float(np.mean([ofull.framework_interactions(kind, t)[0] >= 1e90 for t in u]))
        trials = draw_placements(ofull, base, kind, 24, rng)
        q = direct._mol_charges(kind)
        nblocked = 0
        for t in trials:
            ref = ofull.insertion_energy(kind, t)
            exact, size = _longdouble_reciprocal(full.ewald, t, q)
            nblocked += bool(ref[0] >= 1e90)
            for name, omc in states.items():
                row = omc.insertion_energy(kind, t)
                assert row[2] == 0.0, (name, kind, row)
                assert row[0] == ref[0] and row[1] == ref[1], (name, kind, row, ref)
                if name != "drained":                                          # (the drained state keeps rounding residue of its removals)
                    dev = abs(row[3] - exact) / abs(exact)
                    devs.append((dev, abs(row[3] - exact) / size, abs(exact) / size, name, kind, float(row[3]), exact))
                else:
                    assert abs(row[3] - exact) <= 1e-9 * abs(exact) + 1e-7, (name, kind, row[3], exact)
        blocked[kind] = nblocked / len(trials)
    worst = max(devs)
    print(f"empty box oracle: worst reciprocal deviation from the longdouble sum {worst[0]:.2e} of the value ({worst[3]}, kind {worst[4]}: "
          f"{worst[5]!r} vs {worst[6]!r}, |value| / sum|terms| = {worst[2]:.2e}); worst deviation / sum|terms| {max(d[1] for d in devs):.2e}; "
          f"blocked share of uniform placements Na {uniform[0]:.2f}, CO2 {uniform[1]:.2f}, of the drawn ones Na {blocked[0]:.2f}, CO2 {blocked[1]:.2f}")
    assert worst[0] <= RECIPROCAL_RTOL, worst
    assert max(blocked.values()) <= 0.25, blocked


def test_oracle_add_three_remove_three(setups):
    """add x3, remove x3 on the empty state: positions are empty again and the total structure factor is within 1e-9 of the scale it
    had with the three molecules in."""
    from oracle.montecarlo import OracleMonteCarlo
    full, empty = setups
    omc = OracleMonteCarlo.from_setup(empty)
    omc.compute_ewald()
    rng = np.random.default_rng(SEED + 1)
    base = CO2 - CO2[1]
    for kind, index in ((1, 0), (0, 0), (1, 1)):
        assert omc.add(kind, placements(full.mat, base, kind, 1, rng)[0]) == index
    scale = np.abs(omc.total_structure_factor()).max()
    assert scale > 0.1
    assert omc.flat_positions().shape == (7, 3)
    assert omc.remove((1, 0)) == 1 and omc.remove((0, 0)) == 0 and omc.remove((1, 0)) == 0
    assert [len(k) for k in omc.positions] == [0, 0]
    assert omc.flat_positions().shape == (0, 3)
    assert omc.sums_re.shape[1] == 1
    assert np.abs(omc.total_structure_factor()).max() <= 1e-9 * scale
    row = omc.insertion_energy(0, placements(full.mat, base, 0, 1, rng)[0])
    assert row[2] == 0.0 and np.isfinite(row[3])
