"""The cases of ``tests/uniform_cases.py`` are what ``tests/test_gpu_uniform_class_cells.py`` runs on the device; this file asserts
on the CPU (host-only classification + the FP64 oracle, no GPU) that they exercise what they are meant to, so that the device test
cannot pass vacuously: every case classifies as expected, has points ON atoms (Inf / NaN), points without any pair in range (exact
zeros), and -- with an unshifted record -- a pair 1e-10 inside the cutoff whose loss would move the energy by more than 1e-3 K; the
fuzz reaches the ortho shortcut, the stale-vector range and neither, in both classes."""
import numpy as np
import pytest

from ceg_hip import _abi

import uniform_cases as UC

NAMED = UC.named_cases()
FUZZ = UC.fuzz_cases()
ALL = NAMED + FUZZ


def _classify(case):
    lib = _abi.load_library()
    pv, pc = case.probes()
    ff = pv.forcefield
    rules, offsets = ff.rule_table(pv.probe)
    kinds = np.ascontiguousarray(case.kinds, dtype=np.int64)
    q = np.ascontiguousarray(case.q, dtype=np.float64)
    consts = np.full(4, np.nan)
    rc = lib.ceg_uniform_class(_abi.i64ptr(kinds), _abi.dptr(q), len(kinds), rules.ctypes.data, _abi.i32ptr(offsets), ff.nkinds,
                               case.cutoff ** 2, _abi.dptr(consts))
    return rc, consts, ff


def test_default_force_field_is_unchanged():
    """uniform=None is the force field every other test uses; uniform= touches P's rules with A and D alone."""
    from util import tiny_forcefield
    a, b, u = tiny_forcefield(12.0), tiny_forcefield(12.0, uniform=None), tiny_forcefield(12.0, uniform=(50.0, 3.0, True))
    for i in range(7):
        for j in range(7):
            assert repr(a.interactions[i][j]) == repr(b.interactions[i][j])
            if {i, j} not in ({0, 4}, {3, 4}):
                assert repr(a.interactions[i][j]) == repr(u.interactions[i][j])
    ra, rd = u.interactions[0][4], u.interactions[3][4]
    assert ra.params == [50.0, 3.0] and ra.params == rd.params
    assert ra.shift == rd.shift == 4 * 50.0 * (3.0 / 12.0) ** 6 * ((3.0 / 12.0) ** 6 - 1) != 0.0
    assert tiny_forcefield(12.0, uniform=(50.0, 3.0, False)).interactions[0][4].shift == 0.0
    assert repr(u.interactions[1][4]) == repr(a.interactions[1][4])            # B keeps its Buckingham rule with P


def test_case_lists():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names) and len(FUZZ) == 24
    for c in ALL:
        nx, ny, nz = (d + 1 for d in c.dims)
        assert nx <= 22 and ny <= 20 and nz <= 24 and 40 <= len(c.pos) <= (900 if "cutoff21" in c.name else 200)
        assert set(np.unique(c.kinds)) == ({UC.A, UC.C} if c.multi else {UC.A, UC.C, UC.D})
        assert c.ortho + c.stale + c.plain == 1
        lo = np.asarray(c.cset().shift)
        hi = lo + np.asarray(c.cset().size)
        assert np.all(c.pts >= lo - 1e-9) and np.all(c.pts <= hi + 1e-9)        # what a culled points launch takes
        assert np.all(np.any((c.pts_out < lo) | (c.pts_out > hi), axis=1))
    byname = {c.name: c for c in NAMED}
    for cell, flag in (("orthorhombic", "ortho"), ("near-ortho", "ortho"), ("triclinic", "plain"), ("skewed-60", "stale"),
                       ("skewed-mixed", "stale"), ("skewed-60/unshifted", "stale"), ("skewed-mixed/cutoff9", "plain")):
        assert getattr(byname[cell + "/class1"], flag), (cell, flag)
    assert any(not c.shifted for c in NAMED) and any(c.uniform[0] < 0 for c in NAMED)


def test_the_three_plans_without_r2_tables():
    """alpha * cutoff > 5 takes the libm-grade Ewald term, CEG_HIP_NO_EW2 the erfcx table; the third plan has a cutoff whose
    r^2 tables would need more intervals than CEG_EW2_NI_MAX -- counted here with the key arithmetic of the table builder."""
    assert UC.ew2_intervals(12.0) == 165 and UC.ew2_intervals(13.5) <= UC.ew2_ni_max()
    seen = set()
    for c in NAMED:
        need = UC.ew2_intervals(c.cutoff)
        if c.ewk == 2:
            assert need <= UC.ew2_ni_max() and c.alpha * c.cutoff <= 5.0 and not c.env, c.name
        elif c.env:
            assert c.env == {"CEG_HIP_NO_EW2": "1"} and c.ewk == 1
            seen.add("env")
        elif c.alpha * c.cutoff > 5.0:
            assert c.ewk == 0
            seen.add("alpha")
        else:
            assert need > UC.ew2_ni_max() and c.ewk == 1 and c.alpha * c.cutoff <= 5.0, (c.name, need)
            seen.add("size")
    assert seen == {"env", "alpha", "size"}
    assert all(c.ewk == 2 and UC.ew2_intervals(c.cutoff) <= UC.ew2_ni_max() for c in FUZZ)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_classifies_as_expected(case):
    rc, consts, ff = _classify(case)
    assert rc == case.cls
    eps, sigma, shifted = case.uniform
    rule = ff.interactions[0][4]
    assert rule is ff.interactions[3][4] or rule == ff.interactions[3][4]
    assert consts[0] == 4.0 * eps and consts[1] == (sigma * sigma) * (sigma * sigma) * (sigma * sigma) and consts[2] == rule.shift
    assert (rule.shift != 0.0) == shifted
    act = case.active()
    if case.cls == 2:
        assert consts[3] == case.q[act][0] and np.all(case.q[act] == consts[3])
    else:
        assert len(np.unique(case.q[act])) > 1


def test_fuzz_reaches_every_branch_in_both_classes():
    for cls in (1, 2):
        for flag in ("ortho", "stale", "plain"):
            assert sum(1 for c in FUZZ if c.cls == cls and getattr(c, flag)) >= 2, (cls, flag)
    assert sum(1 for c in FUZZ if not c.shifted) >= 6
    assert sum(1 for c in FUZZ if np.any(np.abs(np.linalg.solve(c.mat, c.pos.T)) > 1.5)) == 12          # given unwrapped
    assert {c.cutoff for c in FUZZ} == {9.0, 10.5, 12.0}


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_is_not_vacuous(case, oracle):
    ref_v, ref_c = case.ref(oracle, "points_vdw"), case.ref(oracle, "points_coulomb")
    # a point ON a VdW-active atom: +Inf energy (-Inf for the inverted well of a negative epsilon) and NaN derivatives
    inf = np.inf if case.uniform[0] > 0 else -np.inf
    assert (ref_v[:, 0] == inf).any() and np.isnan(ref_v).any()
    assert np.isinf(ref_c).any()
    assert case.dense or int(np.all(ref_v == 0.0, axis=1).sum()) >= 10
    assert not case.dense or case.active().sum() >= len(case.pos) // 2
    assert np.all(ref_v[np.all(ref_v == 0.0, axis=1)] == 0.0)
    # grid points, 256 scattered points, 15 rays from atoms with 8 radii each -- and the two radii around sqrt(safemin2) when stale
    assert len(case.pts) == int(np.prod(np.asarray(case.dims) + 1)) + 256 + 15 * (10 if case.stale else 8)
    if not case.shifted:
        # the pair the shifted fixture cannot see: V(cutoff - 1e-10) is part of the sum, V(cutoff + 1e-10) is not
        assert len(case.cut_pairs) == 9
        jump = max(abs(ref_v[i, 0] - ref_v[j, 0]) for i, j in case.cut_pairs)
        assert jump > 1e-3, jump
