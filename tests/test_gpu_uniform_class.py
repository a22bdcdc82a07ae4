"""GPU tests of the uniform-class variants of the grid kernel (k_culled VDWK 4 / 5): one Lennard-Jones record -- and, class 2, one
charge -- for every VdW-active image, constants applied once per tile.  CHA fixture (Ar: LJ with Oz and Oa, same rule, shifted; Si
and Al carry no Ar rule) on a 22 x 20 x 18 grid and point lists of a few hundred points.  Every case is compared with the oracle
through the suite's compare functions at their present tolerances, and with the same library with the switch off
(``CEG_HIP_UNIFORM_CLASS=0`` at plan creation): raw FP64 sums through ``compare_raw`` at its default, stored grids through
``compare_grids`` with no floor on channel 0 -- a stored Float32 may round the other way when the FP64 sum moves in its last digits
(6e-8 relative), which ``compare_raw``'s 1e-9 is not meant for; the FP64 sums at the grid's own points go through ``compare_raw``.

The fixture's two oxygen kinds carry different charges (Oz -1.1427, Oa -0.9354): the plan as it comes is class 1.  Class 2 is
exercised with the Oa charges set to Oz's.

Other cells (wrap-boundary candidates, the stale-vector range, the ortho shortcut), other cutoffs, plans without the r^2-indexed
Ewald tables, unshifted records and records / charges of extreme size: ``tests/test_gpu_uniform_class_cells.py`` (cases from
``tests/uniform_cases.py``), which imports ``_switch`` / ``_build`` / ``_bits`` from here."""
import copy
import os
from contextlib import contextmanager

import numpy as np
import pytest

from ceg_hip import _abi, grids as G, workloads as W
from ceg_hip.hostmirror.interactions import FF, InteractionRule
from ceg_hip.hostmirror.probes import ProbeSystem
from ceg_hip.plan import GridPlan, MultiGridPlan
from oracle.compare import compare_grids

from util import compare_raw, grid_points, synthetic_probes

pytestmark = pytest.mark.gpu

CHA = "CHA_1.4_3b4eeb96"
DIMS = (21, 19, 17)               # 22 x 20 x 18 points: partial tiles along x and z
CULLED = _abi.ALGO_CULLED


@contextmanager
def _switch(value):
    old = os.environ.get("CEG_HIP_UNIFORM_CLASS")
    if value is None:
        os.environ.pop("CEG_HIP_UNIFORM_CLASS", None)
    else:
        os.environ["CEG_HIP_UNIFORM_CLASS"] = value
    try:
        yield
    finally:
        os.environ.pop("CEG_HIP_UNIFORM_CLASS", None) if old is None else os.environ.__setitem__("CEG_HIP_UNIFORM_CLASS", old)


def _plan(cset, pv, pc, alpha, switch=None):
    with _switch(switch):
        return GridPlan(cset, pv, pc, alpha)


def _with_charges(pc, q):
    return ProbeSystem(pc.positions, pc.mat, pc.invmat, pc.forcefield, pc.atomkinds, np.ascontiguousarray(q, dtype=np.float64), 0,
                       pc.num_supercell)


class _Ctx:
    def __init__(self, oracle):
        self.O = oracle
        self.w = W.fixture_workload(CHA, "Ar", 0.0, dims=DIMS)
        w = self.w
        ff = w.forcefield
        self.k_oz, self.k_oa = ff.sdict["Oz"], ff.sdict["Oa"]
        kinds = np.asarray(w.probe_vdw.atomkinds)
        self.is_o = (kinds == self.k_oz) | (kinds == self.k_oa)
        assert (kinds == self.k_oz).any() and (kinds == self.k_oa).any() and (~self.is_o).any()
        q = np.array(w.probe_coulomb.charges, dtype=np.float64)
        q_oz = q[kinds == self.k_oz][0]
        q1 = q.copy()
        q1[self.is_o] = q_oz
        self.pc_uniq = _with_charges(w.probe_coulomb, q1)          # one charge on every oxygen: class 2
        self.refs = {}

    def ref_grid(self, which, pc=None, pv=None):
        key = ("grid", which, id(pc), id(pv))
        if key not in self.refs:
            if which == "vdw":
                lam, thr = G.vdw_scaling()
                ref = self.O.grid_vdw(pv or self.w.probe_vdw, self.w.cset, lam, thr)[0]
            else:
                lam, thr = G.coulomb_scaling()
                ref = self.O.grid_coulomb(pc or self.w.probe_coulomb, self.w.alpha, self.w.cset, lam, thr)[0]
            self.refs[key] = (ref, pc, pv)          # (the probes are kept alive: their ids are the key)
        return self.refs[key][0]


@pytest.fixture(scope="module")
def ctx(hip_lib, oracle):
    return _Ctx(oracle)


def _build(plan, cset, mode, b=0, e=None):
    """-> (vdw, coulomb) float32 [8, e - b, ny, nz] of build_vdw / build_fused / build_coulomb on planes [b, e) stored from plane b"""
    import torch
    nx, ny, nz = cset.npoints
    e = nx if e is None else e
    m = e - b
    new = lambda: torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
    dv = new() if mode in ("vdw", "fused") else None
    dc = new() if mode in ("coulomb", "fused") else None
    if mode == "vdw":
        plan.build_vdw(dv.data_ptr(), m * ny * nz, b, e, b, CULLED)
    elif mode == "coulomb":
        plan.build_coulomb(dc.data_ptr(), m * ny * nz, b, e, b, CULLED)
    else:
        plan.build_fused(dv.data_ptr(), dc.data_ptr(), m * ny * nz, b, e, b, CULLED)
    torch.cuda.synchronize()
    return (dv.cpu().numpy() if dv is not None else None), (dc.cpu().numpy() if dc is not None else None)


def _bits(a):
    return a.view(np.uint32)


# ------------------------------------------------------------------ 1. qualifying plans
@pytest.mark.parametrize("cls", [1, 2])
def test_qualifying_plan_grids(ctx, cls):
    """Fused and VdW-only grid builds of the class-1 plan (the fixture as it is) and the class-2 plan (one oxygen charge), whole
    grid (partial tiles) and an x-range with a non-zero origin, against the oracle and against the switched-off plan."""
    w = ctx.w
    pc = w.probe_coulomb if cls == 1 else ctx.pc_uniq
    on, off = _plan(w.cset, w.probe_vdw, pc, w.alpha), _plan(w.cset, w.probe_vdw, pc, w.alpha, "0")
    assert on.uniform_class == cls and off.uniform_class == 0
    ref_v, ref_c = ctx.ref_grid("vdw"), ctx.ref_grid("coulomb", pc)
    nx = w.cset.npoints[0]
    for b, e in ((0, nx), (5, 16)):
        fv, fc = _build(on, w.cset, "fused", b, e)
        ov, oc = _build(off, w.cset, "fused", b, e)
        vv, _ = _build(on, w.cset, "vdw", b, e)
        xv, _ = _build(off, w.cset, "vdw", b, e)
        for got, ref, what in ((fv, ref_v, "fused/vdw"), (fc, ref_c, "fused/coulomb"), (vv, ref_v, "vdw")):
            worst = compare_grids(got, ref[:, b:e], f"class {cls} {what} [{b},{e}) vs oracle", floor0=0.0)
            print(f"class {cls} {what} [{b},{e}): worst relative error vs oracle {worst:.2e}")
        compare_grids(fv, ov, f"class {cls} fused/vdw on vs off", floor0=0.0)
        compare_grids(fc, oc, f"class {cls} fused/coulomb on vs off", floor0=0.0)
        compare_grids(vv, xv, f"class {cls} vdw on vs off", floor0=0.0)
        if cls == 1:      # the charges are per candidate in class 1: the Coulomb sums are those of the switched-off kernel
            assert np.array_equal(_bits(fc), _bits(oc))
        # the Coulomb-only build has no uniform variant
        assert np.array_equal(_bits(_build(on, w.cset, "coulomb", b, e)[1]), _bits(_build(off, w.cset, "coulomb", b, e)[1]))
    # the FP64 sums at the grid's points (points launches of the same variants)
    pts = grid_points(w.cset)
    for which, ref in (("vdw", ctx.O.points_vdw(w.probe_vdw, pts)), ("coulomb", ctx.O.points_coulomb(pc, w.alpha, pts))):
        got = on.eval_points(which, pts, CULLED)
        compare_raw(got, ref, f"class {cls} points/{which} vs oracle")
        compare_raw(got, off.eval_points(which, pts, CULLED), f"class {cls} points/{which} on vs off")
    on.close(); off.close()


# ------------------------------------------------------------------ 2. points on and near atoms
@pytest.mark.parametrize("cls", [1, 2])
def test_points_on_and_near_atoms(ctx, cls):
    """Points on atoms (r = 0: +Inf energy, NaN derivatives), inside the exact-path radius of 2 A, on both sides of it, and within
    1e-10 of the cutoff of an oxygen (VdW-active) and of a silicon (Coulomb only): the exact path adds into sums held in units of
    4 eps sigma^6 (and q) and is not counted for the shift -- NaN / Inf patterns and values must be the oracle's."""
    w = ctx.w
    pc = w.probe_coulomb if cls == 1 else ctx.pc_uniq
    pos = np.asarray(w.probe_vdw.positions)
    # the atoms nearest to the centre of the grid's bounding box (the culled evaluation takes points inside that box)
    lo, hi = np.asarray(w.cset.shift), np.asarray(w.cset.shift) + np.asarray(w.cset.size)
    order = np.argsort(np.linalg.norm(pos - 0.5 * (lo + hi), axis=1))
    o_atoms = [a for a in order if ctx.is_o[a]][:3]
    t_atoms = [a for a in order if not ctx.is_o[a]][:2]
    rng = np.random.default_rng(5)
    pts = []
    for a in o_atoms + t_atoms:
        for r in (0.0, 0.3, 0.99, 1.0, 1.5, 2.0 - 1e-9, 2.0, 2.0 + 1e-9, 2.5, 12.0 - 1e-10, 12.0, 12.0 + 1e-10):
            n = 0
            while n < 3:
                u = rng.normal(size=3)
                p = pos[a] + r * u / np.linalg.norm(u)
                if np.all(p > lo) and np.all(p < hi):
                    pts.append(p)
                    n += 1
    pts = np.array(pts)
    assert 100 <= len(pts) <= 400
    on, off = _plan(w.cset, w.probe_vdw, pc, w.alpha), _plan(w.cset, w.probe_vdw, pc, w.alpha, "0")
    assert on.uniform_class == cls
    ref_v, ref_c = ctx.O.points_vdw(w.probe_vdw, pts), ctx.O.points_coulomb(pc, w.alpha, pts)
    assert np.isinf(ref_v).any() and np.isnan(ref_v).any() and np.isinf(ref_c).any()
    for which, ref in (("vdw", ref_v), ("coulomb", ref_c)):
        got = on.eval_points(which, pts, CULLED)
        worst = compare_raw(got, ref, f"class {cls} near atoms/{which} vs oracle")
        print(f"class {cls} near atoms/{which}: worst relative error vs oracle {worst:.2e}")
        compare_raw(got, off.eval_points(which, pts, CULLED), f"class {cls} near atoms/{which} on vs off")
    on.close(); off.close()


def test_grid_points_on_atoms(hip_lib, oracle):
    """The positions of test_points_on_atoms_nan_inf_patterns with one VdW-active kind (A: shifted LJ) carrying one charge, plus two
    atoms of a kind without a rule (C) -- class 2 --, grid points ON atoms: fused grid build, NaN / Inf / 2e7 patterns of both grids.
    (Five VdW-active atoms, as there: with fewer, most grid points have no pair in range, the median of a channel -- the scale of
    compare_grids' floor -- is 0 and the 1e-19 the oracle's wrap arithmetic leaves of d3 at a point on an atom's axis, where the
    image list gives an exact 0, has no allowance.)"""
    L = 30.0
    mat = np.diag([L, L, L])
    cset = W.grid_setup_with_dims(mat, (15, 15, 15))                   # spacing 2.0 exactly, shift 0
    pos = np.array([[4.0, 6.0, 8.0], [10.0, 10.0, 10.0], [20.0, 2.0, 28.0], [11.3, 17.7, 5.1], [0.0, 0.0, 0.0],
                    [24.0, 22.0, 16.0], [16.0, 4.0, 20.0]])
    kinds = np.array([1, 1, 1, 1, 1, 3, 3])
    q = np.array([-0.7] * 5 + [1.0, 0.4])
    pv, pc = synthetic_probes(mat, pos, kinds, q)
    alpha = 0.265
    on, off = _plan(cset, pv, pc, alpha), _plan(cset, pv, pc, alpha, "0")
    assert on.uniform_class == 2 and off.uniform_class == 0
    lam, thr = G.vdw_scaling()
    ref_v = oracle.grid_vdw(pv, cset, lam, thr)[0]
    lam, thr = G.coulomb_scaling()
    ref_c = oracle.grid_coulomb(pc, alpha, cset, lam, thr)[0]
    assert (ref_v[0] == np.float32(2e7)).any() and np.isnan(ref_v[1:4]).any() and (ref_c[0] == np.float32(2e7)).any()
    fv, fc = _build(on, cset, "fused")
    compare_grids(fv, ref_v, "on-atoms fused/vdw")
    compare_grids(fc, ref_c, "on-atoms fused/coulomb")
    compare_grids(_build(on, cset, "vdw")[0], ref_v, "on-atoms vdw")
    ov, oc = _build(off, cset, "fused")
    compare_grids(fv, ov, "on-atoms fused/vdw on vs off")
    compare_grids(fc, oc, "on-atoms fused/coulomb on vs off")
    on.close(); off.close()


# ------------------------------------------------------------------ 3. the shift is applied per counted pair
def test_shift_with_one_and_with_no_pair_in_range(hip_lib, oracle):
    """Shifted LJ (kind A of the test force field, shift = -V(cutoff) != 0), ONE VdW-active atom: points with exactly one in-cutoff
    VdW pair (regular range, exact-path range, 1e-10 inside the cutoff) and with none (1e-10 outside, far away) -- a count-based shift
    that is off by one shows as +- shift = 0.14 K against sums of that size or an expected exact 0."""
    L = 40.0
    mat = np.diag([L, L, L])
    cset = W.grid_setup_with_dims(mat, (9, 9, 9))
    pos = np.array([[11.0, 12.0, 13.0], [30.0, 30.0, 30.0]])
    pv, pc = synthetic_probes(mat, pos, np.array([1, 3]), np.array([-0.8, 0.8]))
    rule = pv.forcefield.interactions[0][4]
    assert rule.shift != 0.0
    d = np.array([1.0, 2.0, 2.0]) / 3.0
    radii = [1.2, 1.9, 2.1, 3.0, 5.0, 9.0, 11.9, 12.0 - 1e-10, 12.0 + 1e-10, 12.5, 17.0]
    pts = np.array([pos[0] + r * d for r in radii] + [pos[0] - r * d for r in radii])
    on, off = _plan(cset, pv, pc, 0.265), _plan(cset, pv, pc, 0.265, "0")
    assert on.uniform_class == 2
    ref = oracle.points_vdw(pv, pts)
    inside = np.array([r < 12.0 for r in radii] * 2)
    assert np.all(ref[~inside] == 0.0) and np.all(ref[inside, 0] != 0.0)
    got = on.eval_points("vdw", pts, CULLED)
    assert np.all(got[~inside] == 0.0), "a point without a pair in range got a shift"
    # One pair: the sum is that pair's term, so the derivative columns need no floor.  The energy is V(r) - V(cutoff): near the
    # cutoff the two cancel (to 7e-12 K at 12 A - 1e-10 A) while each carries the rounding of its own evaluation -- 1/r^2 by
    # v_rcp_f64 + one Newton step is good to 2.2e-15, r^-6 to 6.6e-15, of a term of the size of the shift: 1e-14 |shift| absolute.
    # (A shift counted once too often or too seldom is 1 |shift|.)
    np.testing.assert_allclose(got[inside, 1:], ref[inside, 1:], rtol=1e-9, atol=0.0)
    np.testing.assert_allclose(got[inside, 0], ref[inside, 0], rtol=1e-9, atol=1e-14 * abs(rule.shift))
    compare_raw(got, off.eval_points("vdw", pts, CULLED), "one pair / no pair, on vs off")
    compare_raw(on.eval_points("coulomb", pts, CULLED), oracle.points_coulomb(pc, 0.265, pts), "one pair / no pair, coulomb")
    # the same through whole tiles of a grid: most points have no pair at all
    lam, thr = G.vdw_scaling()
    compare_grids(_build(on, cset, "fused")[0], oracle.grid_vdw(pv, cset, lam, thr)[0], "one atom fused/vdw")
    on.close(); off.close()


# ------------------------------------------------------------------ 4. plans that do not (fully) qualify
def test_two_oxygen_kinds_with_different_sigma_fall_back(ctx):
    """Oa's Ar rule given another sigma: class 0, the per-candidate records as before -- bit-identical with the switch on and off."""
    w = ctx.w
    ff = copy.deepcopy(w.forcefield)
    probe = w.probe_vdw.probe
    old = ff.interactions[ctx.k_oa - 1][probe - 1]
    new = InteractionRule(FF.LennardJones, [old.params[0], 3.2], old.shift, old.tailcorrection)
    ff.interactions[ctx.k_oa - 1][probe - 1] = ff.interactions[probe - 1][ctx.k_oa - 1] = new
    p0 = w.probe_vdw
    pv = ProbeSystem(p0.positions, p0.mat, p0.invmat, ff, p0.atomkinds, np.empty(0), probe, p0.num_supercell)
    on, off = _plan(w.cset, pv, ctx.pc_uniq, w.alpha), _plan(w.cset, pv, ctx.pc_uniq, w.alpha, "0")
    assert on.uniform_class == 0 and off.uniform_class == 0
    fv, fc = _build(on, w.cset, "fused")
    ov, oc = _build(off, w.cset, "fused")
    assert np.array_equal(_bits(fv), _bits(ov)) and np.array_equal(_bits(fc), _bits(oc))
    assert np.array_equal(_bits(_build(on, w.cset, "vdw")[0]), _bits(_build(off, w.cset, "vdw")[0]))
    lam, thr = G.vdw_scaling()
    compare_grids(fv, ctx.O.grid_vdw(pv, w.cset, lam, thr)[0], "two sigma / vdw vs oracle", floor0=0.0)
    compare_grids(fc, ctx.ref_grid("coulomb", ctx.pc_uniq), "two sigma / coulomb vs oracle", floor0=0.0)
    on.close(); off.close()


def test_one_differing_charge_takes_the_lj_only_deferral(ctx):
    """One oxygen charge of the class-2 system changed in its last bit: class 1 (the Lennard-Jones constants are deferred, the charges
    stay per candidate).  Capping the class at 1 by the switch changes nothing; the Coulomb sums are those of the switched-off plan
    bit for bit; both grids hold the oracle's values."""
    w = ctx.w
    q = np.array(ctx.pc_uniq.charges)
    a = np.flatnonzero(ctx.is_o)[11]
    q[a] = np.nextafter(q[a], 0.0)
    pc = _with_charges(w.probe_coulomb, q)
    on, cap, off = (_plan(w.cset, w.probe_vdw, pc, w.alpha, s) for s in (None, "1", "0"))
    assert (on.uniform_class, cap.uniform_class, off.uniform_class) == (1, 1, 0)
    fv, fc = _build(on, w.cset, "fused")
    cv, cc = _build(cap, w.cset, "fused")
    ov, oc = _build(off, w.cset, "fused")
    assert np.array_equal(_bits(fv), _bits(cv)) and np.array_equal(_bits(fc), _bits(cc))
    assert np.array_equal(_bits(fc), _bits(oc))
    compare_grids(fv, ov, "one charge / vdw on vs off", floor0=0.0)
    compare_grids(fv, ctx.ref_grid("vdw"), "one charge / vdw vs oracle", floor0=0.0)
    compare_grids(fc, ctx.ref_grid("coulomb", pc), "one charge / coulomb vs oracle", floor0=0.0)
    # the class-2 plan capped at 1 is this kernel as well
    c2 = _plan(w.cset, w.probe_vdw, ctx.pc_uniq, w.alpha, "1")
    assert c2.uniform_class == 1
    compare_grids(_build(c2, w.cset, "fused")[1], ctx.ref_grid("coulomb", ctx.pc_uniq), "class 2 capped / coulomb vs oracle", floor0=0.0)
    for p in (on, cap, off, c2):
        p.close()


# ------------------------------------------------------------------ 5. multi-probe plan whose probe 0 qualifies
def test_multi_probe_plan_with_a_qualifying_probe_0(ctx):
    """Ar + C_co2 in one multi-probe plan: the plain build_vdw / build_fused run probe 0 (Ar) with ITS uniform class and constants
    (the per-probe block, not the plan-level one), ceg_plan_build_multi keeps the per-candidate records: same values to rounding,
    the oracle's values, and the Coulomb grid of the multi call -- charges per candidate in class 1 -- bit for bit."""
    import torch
    w = ctx.w
    wc = W.fixture_workload(CHA, "C_co2", 0.0, dims=DIMS)
    plan = MultiGridPlan(w.cset, [w.probe_vdw, wc.probe_vdw], w.probe_coulomb, w.alpha)
    assert plan.uniform_class == 1
    nx, ny, nz = w.cset.npoints
    outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    oc = torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
    plan.build([o.data_ptr() for o in outs], oc.data_ptr(), nx * ny * nz, 0, nx)
    torch.cuda.synchronize()
    mv, mc = outs[0].cpu().numpy(), oc.cpu().numpy()
    compare_grids(mv, ctx.ref_grid("vdw"), "multi call / Ar vs oracle", floor0=0.0)
    gv, _ = _build(plan, w.cset, "vdw")
    fv, fc = _build(plan, w.cset, "fused")
    for got, what in ((gv, "build_vdw"), (fv, "build_fused")):
        compare_grids(got, ctx.ref_grid("vdw"), f"{what} of probe 0 vs oracle", floor0=0.0)
        compare_grids(got, mv, f"{what} of probe 0 vs the multi call", floor0=0.0)
    compare_grids(fc, ctx.ref_grid("coulomb"), "build_fused / coulomb vs oracle", floor0=0.0)
    assert np.array_equal(_bits(fc), _bits(mc))
    # the ordinary plan of the same probe runs the same launch on the same constants
    single = _plan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    sv, sc = _build(single, w.cset, "fused")
    assert np.array_equal(_bits(sv), _bits(fv)) and np.array_equal(_bits(sc), _bits(fc))
    # with the switch off the plain calls are the multi call's launches again
    with _switch("0"):
        plan0 = MultiGridPlan(w.cset, [w.probe_vdw, wc.probe_vdw], w.probe_coulomb, w.alpha)
    assert plan0.uniform_class == 0
    assert np.array_equal(_bits(_build(plan0, w.cset, "vdw")[0]), _bits(mv))
    for p in (plan, plan0, single):
        p.close()
