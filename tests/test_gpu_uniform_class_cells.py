"""GPU tests of the uniform-class variants of the grid kernel (k_culled VDWK 4 / 5) away from the CHA fixture of
``tests/test_gpu_uniform_class.py``: the cells that exercise the min-image selection (wrap-boundary candidates, the stale-vector
range as upper end of the regular range, the ortho shortcut, a cell barely above 2 x cutoff), cutoffs of 9, 10.5, 14 and 21 A,
qualifying plans WITHOUT the r^2-indexed Ewald tables (FUSED then runs <1, 1> / <1, 0> while VDW still runs <4, 1>), unshifted
records, records and charges of extreme size and either sign, and a seeded fuzz of 24 configurations.  The cases come from
``tests/uniform_cases.py``; ``tests/test_uniform_class_cases_host.py`` asserts on the CPU that they reach what they are meant to.

Per case three plans: as it comes, with ``CEG_HIP_UNIFORM_CLASS=0`` (the per-candidate kernels) and, class 2, capped at 1.  The
reference is the CPU oracle; tolerances are the suite's: ``compare_raw`` at 1e-9 on the FP64 sums, ``compare_grids`` at its defaults
on the stored grids."""
import numpy as np
import pytest

from ceg_hip import _abi
from ceg_hip.plan import GridPlan, MultiGridPlan
from oracle.compare import compare_grids

import uniform_cases as UC
from test_gpu_uniform_class import _bits, _build, _switch
from util import compare_raw

pytestmark = pytest.mark.gpu

CULLED, AUTO = _abi.ALGO_CULLED, _abi.ALGO_AUTO
SENTINEL = 1.9e7


def _plan(case, switch, monkeypatch, cls=GridPlan, probes=None):
    pv, pc = case.probes(probes)
    with monkeypatch.context() as m:
        for k, v in case.env.items():
            m.setenv(k, v)
        with _switch(switch):
            return cls(case.cset(), pv, pc, case.alpha)


def _ordered(a):
    """Float32 bit patterns as integers that are monotonic in the value: their difference is the distance in ULPs"""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _worst_ulps(got, ref):
    """per stored channel: the largest Float32 ULP distance over the regular values (information, not an assertion)"""
    out = []
    for c in range(ref.shape[0]):
        m = np.isfinite(ref[c]) & (np.abs(ref[c]) < SENTINEL) & np.isfinite(got[c])
        out.append(int(np.abs(_ordered(got[c][m]) - _ordered(ref[c][m])).max()) if m.any() else 0)
    return out


def _ranges(nx):
    b = nx // 3
    return [(0, nx)] + ([(b, b + ((nx // 2) | 1))] if nx >= 6 else [])


def _check_points(case, oracle, on, off):
    ref_v, ref_c = case.ref(oracle, "points_vdw"), case.ref(oracle, "points_coulomb")
    zero = np.all(ref_v == 0.0, axis=1)
    assert case.dense or zero.sum() >= 10
    for which, ref in (("vdw", ref_v), ("coulomb", ref_c)):
        got = on.eval_points(which, case.pts, CULLED)
        worst = compare_raw(got, ref, f"{case.name} points/{which} vs oracle")
        print(f"{case.name} points/{which}: worst relative error vs oracle {worst:.2e}")
        compare_raw(got, off.eval_points(which, case.pts, CULLED), f"{case.name} points/{which} on vs off")
        if which == "vdw":
            assert np.all(got[zero] == 0.0), f"{case.name}: a point without a pair in range is not an exact 0 (a counted shift?)"
        # outside the grid box the library takes the literal kernel
        compare_raw(on.eval_points(which, case.pts_out, AUTO), case.ref(oracle, "out_" + which), f"{case.name} outside/{which}")


def _check_grids(case, oracle, on, off, cap):
    cset = case.cset()
    ref_v, ref_c = case.ref(oracle, "grid_vdw"), case.ref(oracle, "grid_coulomb")
    for b, e in _ranges(cset.npoints[0]):
        tag = f"{case.name} [{b},{e})"
        fv, fc = _build(on, cset, "fused", b, e)
        ov, oc = _build(off, cset, "fused", b, e)
        vv, _ = _build(on, cset, "vdw", b, e)
        xv, _ = _build(off, cset, "vdw", b, e)
        for got, ref, what in ((fv, ref_v, "fused/vdw"), (fc, ref_c, "fused/coulomb"), (vv, ref_v, "vdw")):
            worst = compare_grids(got, ref[:, b:e], f"{tag} {what} vs oracle")
            print(f"{tag} {what}: worst relative error vs oracle {worst:.2e}, worst ULP distance per channel {_worst_ulps(got, ref[:, b:e])}")
        compare_grids(fv, ov, f"{tag} fused/vdw on vs off")
        compare_grids(fc, oc, f"{tag} fused/coulomb on vs off")
        compare_grids(vv, xv, f"{tag} vdw on vs off")
        if case.cls == 1:         # the charges are per candidate in class 1: the Coulomb sums are those of the switched-off kernel
            assert np.array_equal(_bits(fc), _bits(oc)), f"{tag}: class 1 fused/coulomb differs from the switched-off build"
        if cap is not None:
            cv, cc = _build(cap, cset, "fused", b, e)
            assert np.array_equal(_bits(cc), _bits(oc)), f"{tag}: class 2 capped at 1, fused/coulomb differs from the switched-off build"
            compare_grids(cv, ref_v[:, b:e], f"{tag} capped fused/vdw vs oracle")
            compare_grids(cv, ov, f"{tag} capped fused/vdw vs off")
        if case.ewk != 2:         # without the r^2 tables the launch table sends FUSED to <1, e> whatever the class
            assert np.array_equal(_bits(fv), _bits(ov)) and np.array_equal(_bits(fc), _bits(oc)), f"{tag}: fused build without r^2 tables"
        # the Coulomb-only build has no uniform variant
        assert np.array_equal(_bits(_build(on, cset, "coulomb", b, e)[1]), _bits(_build(off, cset, "coulomb", b, e)[1]))


def _check_multi(case, oracle, monkeypatch):
    """P (uniform) and Q (Lennard-Jones with A, nothing with C) in one multi-probe plan: the plain builds run probe 0 with ITS class,
    ceg_plan_build_multi keeps the per-candidate records."""
    import torch
    from ceg_hip import grids as G
    cset = case.cset()
    plan = _plan(case, None, monkeypatch, MultiGridPlan, probes=(5, 6))
    assert plan.uniform_class == case.cls
    nx, ny, nz = cset.npoints
    outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    plan.build([o.data_ptr() for o in outs[:2]], outs[2].data_ptr(), nx * ny * nz, 0, nx)
    torch.cuda.synchronize()
    mv, mq, mc = (o.cpu().numpy() for o in outs)
    ref_v, ref_c = case.ref(oracle, "grid_vdw"), case.ref(oracle, "grid_coulomb")
    lam, thr = G.vdw_scaling()
    compare_grids(mv, ref_v, f"{case.name} multi call / P vs oracle")
    compare_grids(mq, oracle.grid_vdw(case.probes((5, 6))[0][1], cset, lam, thr)[0], f"{case.name} multi call / Q vs oracle")
    compare_grids(mc, ref_c, f"{case.name} multi call / coulomb vs oracle")
    gv, _ = _build(plan, cset, "vdw")
    fv, fc = _build(plan, cset, "fused")
    for got, what in ((gv, "build_vdw"), (fv, "build_fused")):
        compare_grids(got, ref_v, f"{case.name} {what} of probe 0 vs oracle")
        compare_grids(got, mv, f"{case.name} {what} of probe 0 vs the multi call")
    compare_grids(fc, ref_c, f"{case.name} build_fused / coulomb vs oracle")
    compare_grids(fc, mc, f"{case.name} build_fused / coulomb vs the multi call")
    if case.cls == 1:
        assert np.array_equal(_bits(fc), _bits(mc))
    plan.close()


def _check(case, oracle, monkeypatch):
    on, off = _plan(case, None, monkeypatch), _plan(case, "0", monkeypatch)
    cap = _plan(case, "1", monkeypatch) if case.cls == 2 else None
    try:
        assert on.uniform_class == case.cls and off.uniform_class == 0 and (cap is None or cap.uniform_class == 1)
        assert on.can_cull and off.can_cull
        _check_points(case, oracle, on, off)
        _check_grids(case, oracle, on, off, cap)
        if case.multi:
            _check_multi(case, oracle, monkeypatch)
    finally:
        for p in (on, off, cap):
            if p is not None:
                p.close()


@pytest.mark.parametrize("case", UC.named_cases(), ids=lambda c: c.name)
def test_named_cases(hip_lib, oracle, monkeypatch, case):
    _check(case, oracle, monkeypatch)


@pytest.mark.parametrize("case", UC.fuzz_cases(), ids=lambda c: c.name)
def test_fuzz_cases(hip_lib, oracle, monkeypatch, case):
    _check(case, oracle, monkeypatch)
