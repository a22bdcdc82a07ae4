"""GPU tests of the grid-kernel variants on the fine r^2-indexed Ewald table (k_culled EWK = 3: 64 intervals per octave of r^2, two
degree-5 polynomials): the fused builds of uniform class 1 / 2 (VDWK 4 / 5), the Coulomb-only build and the Coulomb point
evaluation.  Every plan is created twice, as it comes and with ``CEG_HIP_EW2_FINE=0`` (the ordinary table: 32 per octave, degree 6).

1. one pair: the bounds of ``test_fast_math_accuracy_single_pair`` (tests/test_gpu_parity.py), unchanged, with the fine table on;
   on and off within 3e-11 of the local column scale;
2. cases of ``tests/uniform_cases.py`` -- an orthogonal, a plain triclinic and a stale-vector cell, classes 1 and 2, cutoffs of 9,
   10.5 and 12 A -- on 18 x 16 x 14 points (4032: partial tiles along x and z): FP64 sums against the oracle at 1e-9, stored grids
   through ``compare_grids`` over the whole grid and over an x-range with a non-zero origin;
3. where the ordinary table stays -- per-candidate records, the Buckingham table, multi-probe records, a cutoff the fine table does
   not reach -- the switch changes no bit."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from ceg_hip import _abi, workloads as W
from ceg_hip.plan import GridPlan, MultiGridPlan
from oracle.compare import compare_grids

import uniform_cases as UC
from util import compare_raw, synthetic_probes

pytestmark = pytest.mark.gpu

CULLED = _abi.ALGO_CULLED
ALPHA = 0.26505830360350674
CHA = "CHA_1.4_3b4eeb96"
DIMS = (17, 15, 13)               # 18 x 16 x 14 points
CELLS = {"orthorhombic": "ortho", "triclinic": "plain", "skewed-60": "stale"}
CUTOFFS = (9.0, 10.5, 12.0)


@contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _plans(make, **env):
    """(on, off): the plan as it comes and with the fine table suppressed; `env` holds for both"""
    with _env(CEG_HIP_EW2_FINE=None, **env):
        on = make()
    with _env(CEG_HIP_EW2_FINE="0", **env):
        off = make()
    return on, off


def _build(plan, cset, mode, b=0, e=None):
    """-> (vdw, coulomb) float32 [8, e - b, ny, nz] of build_fused / build_coulomb on planes [b, e), stored from plane b"""
    import torch
    nx, ny, nz = cset.npoints
    e = nx if e is None else e
    m = e - b
    new = lambda: torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
    dv = new() if mode == "fused" else None
    dc = new()
    if mode == "fused":
        plan.build_fused(dv.data_ptr(), dc.data_ptr(), m * ny * nz, b, e, b, CULLED)
    else:
        plan.build_coulomb(dc.data_ptr(), m * ny * nz, b, e, b, CULLED)
    torch.cuda.synchronize()
    return (dv.cpu().numpy() if dv is not None else None), dc.cpu().numpy()


def _bits(a):
    return a.view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 1. one pair
def test_single_pair_sweep(hip_lib, oracle):
    """One Lennard-Jones atom with a charge in a 40 A cubic box (a uniform plan of class 2), 4096 points at r in [2.0001, 11.9999] A
    in random directions: no cancellation between atoms, so the FP64 outputs show the table's own error."""
    from scipy.ndimage import maximum_filter1d
    L = 40.0
    mat = np.diag([L, L, L])
    cset = W.grid_setup_with_dims(mat, (15, 15, 15))
    centre = np.array([20.0, 20.0, 20.0])
    rng = np.random.default_rng(77)
    r = np.linspace(2.0001, 11.9999, 4096)
    u = rng.normal(size=(len(r), 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pts = centre + r[:, None] * u
    pv, pc = synthetic_probes(mat, [centre], [1], [0.9094])
    on, off = _plans(lambda: GridPlan(cset, pv, pc, ALPHA))
    try:
        assert on.ew2_fine and not off.ew2_fine and on.uniform_class == 2 and off.uniform_class == 2
        for which, ref in (("vdw", oracle.points_vdw(pv, pts)), ("coulomb", oracle.points_coulomb(pc, ALPHA, pts))):
            got, got_off = on.eval_points(which, pts, CULLED), off.eval_points(which, pts, CULLED)
            assert np.all(np.isfinite(ref))
            env = maximum_filter1d(np.abs(ref), size=81, axis=0, mode="nearest")
            rel = np.abs(got - ref) / env
            rel_sum = np.abs(got - ref) / np.maximum(env, 1e-2 * np.abs(ref).max(axis=0))
            between = np.abs(got - got_off) / env
            print(f"fine table, max rel err {which}: local {rel.max():.2e} (r < 5.6 A: {rel[r < 5.6].max():.2e}), vs column scale "
                  f"{rel_sum.max():.2e}; on vs off {between.max():.2e}; ordinary table local {(np.abs(got_off - ref) / env).max():.2e}")
            tol_local = 1e-12 if which == "vdw" else 3e-11
            assert rel.max() < tol_local, (which, float(rel.max()), int(np.argmax(rel.max(axis=1))))
            assert rel[r < 5.6].max() < 1.5e-12 and rel_sum.max() < 5e-12, (which, float(rel_sum.max()))
            assert between.max() < 3e-11, (which, float(between.max()))
            if which == "vdw":                # the VdW launch reads no Ewald table
                assert np.array_equal(got, got_off)
        # the fused launch of the same plan (<5, 3>) on the 16^3 grid: both stored grids, on against off
        fv, fc = _build(on, cset, "fused")
        ov, oc = _build(off, cset, "fused")
        compare_grids(fv, ov, "one pair fused/vdw on vs off")
        compare_grids(fc, oc, "one pair fused/coulomb on vs off")
    finally:
        on.close(); off.close()


# ------------------------------------------------------------------ 2. cells, classes, cutoffs
def _cases():
    out = []
    for cell in CELLS:
        for cutoff in CUTOFFS:
            for cls in (1, 2):
                # (the atom on a grid point is a Coulomb-only one: with a VdW-active one the grid points in its planes carry VdW terms
                #  that are an exact 0 from the image list and a rounding residue in the oracle -- see uniform_cases.named_cases)
                out.append(UC._named(f"ew2-fine/{cell}/cutoff{cutoff:g}/class{cls}", cell, DIMS, cls, cutoff=cutoff,
                                     seed_tag=f"ew2-fine/{cell}/{cutoff:g}", on_grid_active=False))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_cells_classes_cutoffs(hip_lib, oracle, case):
    kind = CELLS[case.name.split("/")[1]]
    assert case.ortho == (kind == "ortho") and (case.plain or kind != "plain")
    if kind == "stale" and case.cutoff == 12.0:
        assert case.stale                         # (the stale-vector range of this cell begins between 10.5 and 12 A)
    cset = case.cset()
    assert tuple(cset.npoints) == (18, 16, 14)
    pv, pc = case.probes()
    on, off = _plans(lambda: GridPlan(cset, pv, pc, case.alpha))
    try:
        assert on.ew2_fine and not off.ew2_fine
        assert on.uniform_class == case.cls and off.uniform_class == case.cls and on.can_cull
        # FP64 sums at grid points, scattered points and points either side of 2 A and of the cutoff (POINTS launches)
        ref = case.ref(oracle, "points_coulomb")
        got = on.eval_points("coulomb", case.pts, CULLED)
        worst = compare_raw(got, ref, f"{case.name} points/coulomb vs oracle", rtol=1e-9)
        compare_raw(got, off.eval_points("coulomb", case.pts, CULLED), f"{case.name} points/coulomb on vs off", rtol=1e-9)
        compare_raw(on.eval_points("vdw", case.pts, CULLED), case.ref(oracle, "points_vdw"), f"{case.name} points/vdw vs oracle", rtol=1e-9)
        print(f"{case.name} points/coulomb: worst relative error vs oracle {worst:.2e}")
        # stored grids: whole grid and an x-range with a non-zero origin
        ref_v, ref_c = case.ref(oracle, "grid_vdw"), case.ref(oracle, "grid_coulomb")
        for b, e in ((0, 18), (6, 15)):
            tag = f"{case.name} [{b},{e})"
            fv, fc = _build(on, cset, "fused", b, e)
            ov, oc = _build(off, cset, "fused", b, e)
            compare_grids(fv, ref_v[:, b:e], f"{tag} fused/vdw vs oracle")
            compare_grids(fc, ref_c[:, b:e], f"{tag} fused/coulomb vs oracle")
            compare_grids(fv, ov, f"{tag} fused/vdw on vs off")
            compare_grids(fc, oc, f"{tag} fused/coulomb on vs off")
            _, cc = _build(on, cset, "coulomb", b, e)
            compare_grids(cc, ref_c[:, b:e], f"{tag} coulomb-only vs oracle")
            compare_grids(cc, _build(off, cset, "coulomb", b, e)[1], f"{tag} coulomb-only on vs off")
    finally:
        on.close(); off.close()


# ------------------------------------------------------------------ 3. where the ordinary table stays
def test_per_candidate_records_keep_the_ordinary_table(hip_lib):
    """CEG_HIP_UNIFORM_CLASS=0: the fused launch is <1, 2> whatever the plan holds"""
    case = UC._named("ew2-fine/triclinic/cutoff12/class1", "triclinic", DIMS, 1, seed_tag="ew2-fine/triclinic/12", on_grid_active=False)
    cset = case.cset()
    pv, pc = case.probes()
    on, off = _plans(lambda: GridPlan(cset, pv, pc, case.alpha), CEG_HIP_UNIFORM_CLASS="0")
    try:
        assert on.ew2_fine and not off.ew2_fine and on.uniform_class == 0 and off.uniform_class == 0
        fv, fc = _build(on, cset, "fused")
        ov, oc = _build(off, cset, "fused")
        assert _same_bits(fv, ov) and _same_bits(fc, oc)
    finally:
        on.close(); off.close()


def test_buckingham_probe_keeps_the_ordinary_table(hip_lib):
    """Na on CHA: the tabulated Buckingham class (VDWK 3) shares its interval key with the ordinary table"""
    w = W.fixture_workload(CHA, "Na", 0.0, dims=DIMS)
    on, off = _plans(lambda: GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha))
    try:
        assert on.ew2_fine and not off.ew2_fine and on.uniform_class == 0
        fv, fc = _build(on, w.cset, "fused")
        ov, oc = _build(off, w.cset, "fused")
        assert _same_bits(fv, ov) and _same_bits(fc, oc)
    finally:
        on.close(); off.close()


def test_two_probe_multi_build_keeps_the_ordinary_table(hip_lib):
    """ceg_plan_build_multi of Ar + C_co2 with the Coulomb grid: the multi-probe records leave no room for the fine table"""
    import torch
    w = W.fixture_workload(CHA, "Ar", 0.0, dims=DIMS)
    wc = W.fixture_workload(CHA, "C_co2", 0.0, dims=DIMS)
    on, off = _plans(lambda: MultiGridPlan(w.cset, [w.probe_vdw, wc.probe_vdw], w.probe_coulomb, w.alpha))
    try:
        assert on.ew2_fine and not off.ew2_fine
        nx, ny, nz = w.cset.npoints
        res = []
        for plan in (on, off):
            outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
            plan.build([o.data_ptr() for o in outs[:2]], outs[2].data_ptr(), nx * ny * nz, 0, nx)
            torch.cuda.synchronize()
            res.append([o.cpu().numpy() for o in outs])
        for a, b in zip(*res):
            assert _same_bits(a, b)
    finally:
        on.close(); off.close()


def test_cutoff_beyond_the_fine_table(hip_lib):
    """21 A: 432 fine intervals are more than the kernels hold (and 216 ordinary ones too: the erfcx variant runs)"""
    case = next(c for c in UC.named_cases() if c.name == "cutoff21/class1")
    cset = case.cset()
    pv, pc = case.probes()
    on, off = _plans(lambda: GridPlan(cset, pv, pc, case.alpha))
    try:
        assert not on.ew2_fine and not off.ew2_fine
        fv, fc = _build(on, cset, "fused")
        ov, oc = _build(off, cset, "fused")
        assert _same_bits(fv, ov) and _same_bits(fc, oc)
        assert _same_bits(_build(on, cset, "coulomb")[1], _build(off, cset, "coulomb")[1])
    finally:
        on.close(); off.close()
