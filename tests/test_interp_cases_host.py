"""CPU checks of ``tests/interp_cases.py``, so that ``tests/test_gpu_interp_synthetic.py`` cannot pass vacuously: the longdouble
reference against exact rational arithmetic (poly grids) and against mpmath on the reference's own formula (COEFF * X), the
float64 oracle and the host mirror within the derived bound of it, the cases against what they claim, and the block-mask references
against the oracle."""
import math
from fractions import Fraction

import numpy as np
import pytest

from ceg_hip import grids as G
from ceg_hip.hostmirror.coordinates import offsetpoint

import interp_cases as IC

LD = np.longdouble


def _fraction(x) -> Fraction:
    """a longdouble exactly"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


# ------------------------------------------------------------------------------------------------ the reference
def test_shifted_is_offsetpoint_bit_for_bit():
    for cell in IC.CELLS:
        for dims in IC.DIMS:
            cs = IC.cset(cell, dims)
            pts = IC.all_points(cs, seed=3)
            sh = IC.shifted(cs, pts)
            one = np.array([offsetpoint(p, cs) for p in pts])
            assert np.array_equal(sh.view(np.int64), one.view(np.int64)), (cell, dims)
            assert (sh >= 1).all() and (sh <= np.asarray(cs.npoints)).all()          # a wrapped point lands in [1, extent]: the clip is idle


def test_poly_data_are_exact_and_use_the_full_polynomial_where_it_fits():
    for dims in IC.DIMS:
        coeff = IC.poly_coefficients(dims, 300)
        data = IC.poly_data(IC.cset("ortho", dims), coeff)       # asserts integers below 2^24, unchanged by Float32
        assert np.count_nonzero(coeff) >= 12, (dims, coeff)
        assert coeff[1:, 1:, 1:].any(), dims                     # a monomial with every mixed derivative
        for ch in range(8):
            assert data[ch].any() or min(dims) == 0, (dims, ch)
    assert np.count_nonzero(IC.poly_coefficients((7, 5, 3), 300)) >= 45          # (a fifth of the draws in -2..2 are zeros)


def test_reference_is_the_polynomial_on_poly_grids():
    """the Hermite interpolant of a tricubic polynomial is the polynomial: exact rational evaluation at sh - 1, to 2^-60 T"""
    worst = 0.0
    for case in IC.catalogue():
        if case.family != "poly":
            continue
        value, T, _cell, _blocked, _skip = case.ref
        sh = IC.shifted(case.eg.csetup, case.pts)
        pick = np.unique(np.concatenate([np.arange(0, len(case.pts), 9), np.arange(len(case.pts) - 60, len(case.pts))]))   # tiny, far, beside among them
        for q in pick:
            exact = IC.poly_exact(case.info["coeff"], sh[q])
            err = abs(_fraction(value[q]) - exact)
            tol = _fraction(T[q]) / 2 ** 60
            assert err <= tol, (case.name, q, float(err), float(tol))
            if tol:
                worst = max(worst, float(err / tol))
    print(f"poly: worst |reference - polynomial| / (2^-60 T) = {worst:.3f}")


def test_reference_against_mpmath_on_the_formula_of_the_reference():
    """grids.jl:245-258 at 50 digits: a = COEFF X, sum a[i + 4j + 16k] rx^i ry^j rz^k, on a random grid"""
    import mpmath
    from ceg_hip.hostmirror.constants import tricubic_coeff
    mpmath.mp.dps = 50
    case = next(c for c in IC.catalogue() if c.name == "random-coulomb/tric/7x5x3")
    coeff = tricubic_coeff()
    assert np.array_equal(coeff, np.rint(coeff))
    rng = np.random.default_rng(5)
    pick = rng.choice(len(case.pts), 20, replace=False)
    value, T, _cell, _blocked, _skip = case.ref
    p0, p1, r = IC.stencil(case.eg.csetup, case.pts)
    for q in pick:
        X = G.gather_corners(case.eg.grid, p0[q], p1[q])
        a = [sum(int(coeff[row, col]) * mpmath.mpf(float(X[col])) for col in range(64) if coeff[row, col]) for row in range(64)]
        rs = [[mpmath.mpf(float(r[q, ax])) ** e for e in range(4)] for ax in range(3)]
        ref = sum(a[i + 4 * j + 16 * k] * rs[0][i] * rs[1][j] * rs[2][k] for k in range(4) for j in range(4) for i in range(4))
        hi = float(value[q])
        got = mpmath.mpf(hi) + mpmath.mpf(float(value[q] - LD(hi)))
        assert abs(got - ref) <= mpmath.mpf(float(T[q])) / 2 ** 60, (q, got, ref)


def test_oracle_within_the_bound_on_every_case(oracle):
    """the float64 oracle (COEFF * X) against the reference: blocked and NaN patterns equal, |oracle - reference| <= bound"""
    worst = {}
    for case in IC.catalogue():
        got = oracle.interpolate_points(case.eg, case.pts)
        w = IC.check_values(got, case.eg, case.pts, case.name, ref=case.ref)
        worst[case.family] = max(worst.get(case.family, 0.0), w)
    print("oracle, worst |got - reference| / (2^-53 T) per family: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) < IC.K


def test_host_mirror_within_the_bound_on_a_sample():
    rng = np.random.default_rng(8)
    cases = [c for c in IC.catalogue() if c.family in ("random", "poly-vdw")] + [c for c in IC.catalogue() if c.family == "blocking"][::17]
    for case in cases:
        pick = rng.choice(len(case.pts), 25, replace=False)
        got = np.array([G.interpolate_grid(case.eg, case.pts[q]) for q in pick])
        IC.check_values(got, case.eg, case.pts[pick], case.name, ref=tuple(x[pick] for x in case.ref))


def test_noderiv_reference_against_the_host_mirror_and_the_oracle(oracle):
    """the "no derivatives" branch: NaN exactly where the host mirror raises (an index beyond its axis), the value elsewhere; the
    oracle has the same NaN pattern and lies within the bound; (3,3,3) shows no NaN, (7,5,3) some"""
    for cell in IC.CELLS:
        for dims in ((3, 3, 3), (7, 5, 3)):
            cs = IC.cset(cell, dims)
            eg = IC.energy_grid(cs, IC.random_data(cs, 77), IC.VDW, higherorder=False)
            pts = IC.all_points(cs, seed=4)
            value, T = IC.reference_noderiv(eg, pts)
            assert np.isnan(value).any() == (dims == (7, 5, 3))
            got = oracle.interpolate_points(eg, pts)
            assert np.array_equal(np.isnan(got), np.isnan(value)), (cell, dims)
            m = ~np.isnan(value)
            assert (np.abs(got[m].astype(LD) - value[m]) <= IC.bound(T[m])).all()
            for q in np.random.default_rng(2).choice(len(pts), 60, replace=False):
                try:
                    one = G.interpolate_grid(eg, pts[q])
                except IndexError:
                    assert np.isnan(value[q]), (cell, dims, q)
                    continue
                assert abs(LD(one) - value[q]) <= IC.bound(T[q]), (cell, dims, q)


# ------------------------------------------------------------------------------------------------ the cases are what they claim
def test_tiny_negative_points_land_on_the_extent():
    for cell in IC.CELLS:
        for dims in IC.DIMS:
            cs = IC.cset(cell, dims)
            p0 = IC.stencil(cs, IC.tiny_negative())[0]
            on = p0 == np.asarray(cs.npoints)
            assert on.any(), (cell, dims)
            if cell == "ortho":
                assert on.any(axis=0).all(), (dims, on.any(axis=0))
                assert on[-2].all() and on[-1].all()             # (-1e-20,)*3 and (-1e-300,)*3: all three axes at once
    # and the wrap really rounds to 1.0
    assert (-1e-20 / 9.0) - math.floor(-1e-20 / 9.0) == 1.0


def test_blocking_grids_block_what_they_should():
    seen = set()
    for case in IC.catalogue():
        if case.family != "blocking":
            continue
        _value, _T, cell, blocked, skip = case.ref
        special, declared = case.info["special"], case.info["declared"]
        in_cell = (cell == np.asarray(case.info["p0"])).all(axis=1)
        assert in_cell.any(), case.name
        if declared == "vdw" and IC.BLOCKS[special]:
            assert blocked.any() and not blocked.all(), case.name
            assert blocked[in_cell].all(), case.name             # every point of the target cell sees the corner
            assert not skip.any()
        else:
            assert not blocked.any(), case.name
            assert skip.any() == (special == "inf"), case.name
        if special == "nan":
            assert np.isnan(case.ref[0][in_cell]).all()
        seen.add((case.info["where"], special, declared))
    assert len(seen) == 2 * 4 * 2
    for cell in IC.CELLS:                                        # eight distinct corners inside, four (or fewer) on the last layer
        n_in = {c.info["node"] for c in IC.catalogue() if c.family == "blocking" and c.info["where"] == "interior" and f"/{cell}/" in c.name}
        n_last = {c.info["node"] for c in IC.catalogue() if c.family == "blocking" and c.info["where"] == "last-layer" and f"/{cell}/" in c.name}
        assert len(n_in) == 8 and 1 <= len(n_last) <= 4
    assert IC.ABOVE > IC.THRESHOLD and float(IC.THRESHOLD) == 5e6 and not (IC.THRESHOLD > np.float32(5e6))


def test_every_one_hot_grid_is_seen():
    n = 0
    for case in IC.catalogue():
        if case.family == "one-hot":
            value = case.ref[0]
            assert (np.abs(value) > 1e-3).any(), case.name
            n += 1
    assert n == 128


def test_only_the_blocking_rule_gives_a_coulomb_value_of_1e100():
    """montecarlo.jl:500 passes a Coulomb value == 1e100 on without the charge.  The data of a Coulomb-declared Float32 grid cannot
    produce one; a VdW-declared grid in the Coulomb slot does, in a blocked cell (mc_setup(..., coulomb_vdw=True))"""
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e100))
    t = np.linspace(0.0, 1.0, 1001)
    _H, A = IC._hermite(t)
    assert float(max((A[0][0] + A[0][1] + A[1][0] + A[1][1]).max(), 1.0)) ** 3 * float(np.finfo(np.float32).max) < 1e100
    for case in IC.catalogue():
        if case.family == "huge":
            value, T, _c, blocked, skip = case.ref
            assert not blocked.any() and not skip.any() and (np.abs(value) > 3e38).all()
    for cell in IC.CELLS:
        mc = IC.mc_setup(cell, coulomb_vdw=True)
        assert mc.coulomb.ewald_precision == math.inf
        assert IC.reference(mc.coulomb, mc.coulomb_blocked_points)[3].all()
        assert all(G.interpolate_grid(mc.coulomb, p) == 1e100 for p in mc.coulomb_blocked_points)
        blocked = IC.reference(mc.coulomb, IC.all_points(mc.coulomb.csetup))[3]
        assert blocked.any() and not blocked.all()


# ------------------------------------------------------------------------------------------------ block masks
def test_block_from_grid_reference_against_the_oracle(oracle):
    for dims in IC.DIMS:
        cs = IC.cset("ortho", dims)
        cases = IC.block_single_entry_cases(dims) + [("random", IC.block_random_case(dims), None)]
        for name, value, count in cases:
            ref = IC.block_from_grid_reference(value)
            eg = G.EnergyGrid(cs, (1, 1, 1), math.inf, True, value[None])
            assert np.array_equal(oracle.block_from_grid(eg), ref), (dims, name)
            if count is not None:
                assert int(ref.sum()) == count, (dims, name, int(ref.sum()))
            else:
                assert ref.any()
        names = [n for n, _v, _c in cases]
        assert any(n.startswith("last-node-x/") for n in names) and len(names) == 9 * 5 + 1
    assert np.prod([d + 1 for d in IC.DIMS[-1]]) == 2688 and 2688 % 256          # several blocks and a partial last one


SPHERE_GRIDS = [(cell, dims) for cell in IC.CELLS for dims in ((7, 5, 3), (15, 13, 11))]


@pytest.mark.parametrize("cell,dims", SPHERE_GRIDS)
def test_sphere_cases(oracle, cell, dims):
    """the share of the mask set by 1, 257 and 2048 spheres lies between 20 % and 80 %; in the orthorhombic cell the oracle agrees with
    a round-based minimum image in longdouble away from the sphere surfaces"""
    cs = IC.cset(cell, dims)
    for n in (1, 257, 2048):
        centers, r2 = IC.sphere_case(cs, n, seed=n)
        mask = oracle.block_spheres(cs, centers, r2)
        share = float(mask.mean())
        print(f"spheres {cell} {dims} n = {n}: {share:.2f} of the lattice set")
        assert 0.2 <= share <= 0.8, (cell, dims, n, share)
        if cell == "ortho":
            ref, near = IC.sphere_minimage_longdouble(cs, centers, r2)
            assert near.mean() <= 0.01
            assert np.array_equal(mask[~near], ref[~near]), (dims, n)


@pytest.mark.parametrize("cell,dims", SPHERE_GRIDS)
def test_sphere_boundary_is_strict(oracle, cell, dims):
    centre, neighbour, r2 = IC.sphere_boundary_case(oracle, IC.cset(cell, dims))
    cs = IC.cset(cell, dims)
    c = IC.lattice_point(cs, centre)[None]
    open_ = oracle.block_spheres(cs, c, np.array([r2]))
    closed = oracle.block_spheres(cs, c, np.array([np.nextafter(r2, np.inf)]))
    assert open_[centre] and not open_[neighbour] and closed[centre] and closed[neighbour]


# ------------------------------------------------------------------------------------------------ Monte-Carlo columns
@pytest.mark.parametrize("cell", list(IC.CELLS))
def test_column_reference_against_the_host_mirror(cell):
    """framework_interactions (montecarlo.jl:490-504) of the host mirror on the synthetic setups: blocked where the reference is,
    within the summed bounds elsewhere; the placements hold what they claim (a tiny-negative atom, a node, a blocked atom)"""
    from ceg_hip.hostmirror import montecarlo as M
    for coulomb, blocking, coulomb_vdw in ((True, False, False), (False, False, False), (True, True, False), (True, False, True)):
        mc = IC.mc_setup(cell, coulomb, blocking, coulomb_vdw)
        assert mc.mat[0, 0] == 18.0 and [g.ewald_precision == math.inf for g in mc.grids[:4]] == [True, True, True, False]
        rng = np.random.default_rng(11)
        nblocked = ncoulomb = 0
        for s, ids in enumerate(mc.ffidx):
            pos = IC.mc_placements(mc, s, 5, rng)
            rows = np.array([M.framework_interactions(mc, ids, p) for p in pos])
            if not coulomb:
                assert not rows[:, 1].any()
            _w0, _w1, nb, nc = IC.check_rows(rows, mc, ids, pos, (cell, coulomb, blocking, coulomb_vdw, s))
            nblocked, ncoulomb = nblocked + nb, ncoulomb + nc
            if coulomb_vdw:                                      # a neutral atom and a charged one, in rows of their own
                assert nc >= 2 and (rows[3, 1] >= 1e90) and (rows[4, 1] >= 1e90)
                q = [mc.charges[ix] for ix in ids]
                assert (0.0 in q) == (len(ids) >= 3) and any(x not in (0.0, 1.0) for x in q)
            g = mc.grids[ids[-1] - 1]
            assert (IC.stencil(g.csetup, pos[0, -1][None])[0] == np.asarray(g.csetup.npoints)).any() or cell == "tric"
        assert (nblocked > 0) == blocking and (ncoulomb > 0) == coulomb_vdw
