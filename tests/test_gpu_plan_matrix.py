"""The ordinary plan calls (ceg_plan_build_vdw / _coulomb / _fused, ceg_plan_eval_points) on every kind of plan.  include/ceg_hip.h:
"The ordinary ceg_plan_build_vdw / _coulomb / _fused calls work on a multi-probe plan too and use probe 0."  Every stored grid
against the CPU oracle's grid of probe 0 with the tolerance of the fixture-grid tests (compare_grids, no floor on channel 0), every
raw FP64 sum with compare_raw, and bit for bit against ceg_plan_build_multi of the same plan.  Run with `pytest -m gpu` on an MI355X."""
import os

import numpy as np
import pytest

from ceg_hip import _abi, grids as G
from ceg_hip.plan import GridPlan, MultiGridPlan
from oracle.compare import compare_grids

from test_gpu_parity import _probe_set
from util import compare_raw, grid_points

pytestmark = pytest.mark.gpu

BRUTE, CULLED = _abi.ALGO_BRUTEFORCE, _abi.ALGO_CULLED
CIT7, CHA = "CIT-7", "CHA_1.4_3b4eeb96"

# id -> (framework, spacing, probes of the plan (None: an ordinary GridPlan of Na), charges?, environment at creation)
PLANS = {
    "m1-na": (CHA, 0.7, ("Na",), True, {}),                               # vdwk == 3, one block
    "m2-na-first": (CIT7, 0.5, ("Na", "O_co2"), True, {}),                # probe 0 tabulated Buckingham; union image flags != probe 0's
    "m3-lj-first": (CIT7, 0.5, ("C_co2", "O_co2", "Na"), True, {}),       # probe 0 LJ, the plan's exact-path radius raised by Na's hard sphere
    "m2-nocharge": (CIT7, 0.5, ("Na", "C_co2"), False, {}),               # VdW only
    "m1-na-nobk2": (CHA, 0.7, ("Na",), True, {"CEG_HIP_NO_BK2": "1"}),    # probe 0 on the generic Buckingham path (vdwk == 2)
    "s-na": (CHA, 0.7, None, True, {}),                                   # the control: an ordinary plan
}
GRID_CALLS = ("build_vdw-culled", "build_vdw-brute", "build_vdw-slab", "build_coulomb-culled", "build_fused-culled")
POINT_CALLS = ("eval_vdw-culled", "eval_vdw-brute", "eval_coulomb-culled", "eval_coulomb-brute")
NEEDS_CHARGE = ("build_coulomb-culled", "build_fused-culled", "eval_coulomb-culled", "eval_coulomb-brute")


class _Ctx:
    """plans and oracle references, made once per module (the oracle's full grids are the expensive part)"""

    def __init__(self, oracle):
        self.oracle, self.plans, self.refs, self.sets = oracle, {}, {}, {}

    def probe_set(self, pid):
        fw, spacing, atoms, _q, _env = PLANS[pid]
        key = (fw, spacing, atoms or ("Na",))
        if key not in self.sets:
            self.sets[key] = _probe_set(fw, key[2], spacing)
        return self.sets[key]

    def plan(self, pid):
        if pid not in self.plans:
            _fw, _sp, atoms, charged, env = PLANS[pid]
            w, probes = self.probe_set(pid)
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                if atoms is None:
                    self.plans[pid] = GridPlan(w.cset, probes[0], w.probe_coulomb, w.alpha)
                else:
                    self.plans[pid] = MultiGridPlan(w.cset, probes, w.probe_coulomb if charged else None, w.alpha if charged else 0.0)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return self.plans[pid]

    def ref(self, pid, what):
        """what: 'vdw' / 'coulomb' (stored grids), ('pts',) the evaluation points, ('vdw', 'pts') / ('coulomb', 'pts') raw sums"""
        fw, spacing, atoms, _q, _env = PLANS[pid]
        key = (fw, spacing, (atoms or ("Na",))[0], what)
        if key not in self.refs:
            w, probes = self.probe_set(pid)
            O = self.oracle
            if what == "vdw":
                lam, thr = G.vdw_scaling()
                self.refs[key] = O.grid_vdw(probes[0], w.cset, lam, thr)[0]
            elif what == "coulomb":
                lam, thr = G.coulomb_scaling()
                self.refs[key] = O.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr)[0]
            elif what == ("pts",):
                rng = np.random.default_rng(20261)
                lattice = grid_points(w.cset)
                lattice = lattice[rng.choice(len(lattice), 1536, replace=False)]
                inside = np.asarray(w.cset.shift) + rng.uniform(0, 1, (512, 3)) * np.asarray(w.cset.size)
                self.refs[key] = np.concatenate([lattice, inside])
            elif what == ("vdw", "pts"):
                self.refs[key] = O.points_vdw(probes[0], self.ref(pid, ("pts",)))
            else:
                self.refs[key] = O.points_coulomb(w.probe_coulomb, w.alpha, self.ref(pid, ("pts",)))
        return self.refs[key]

    def close(self):
        for p in self.plans.values():
            p.close()


@pytest.fixture(scope="module")
def ctx(hip_lib, oracle):
    c = _Ctx(oracle)
    yield c
    c.close()


def _grids(plan, call, cset):
    """-> (vdw grid or None, coulomb grid or None, x range) of one ordinary build call, NaN where nothing was to be written"""
    import torch
    nx, ny, nz = cset.npoints
    name, how = call.split("-")
    b, e = (nx // 3, nx // 3 + ((nx // 2) | 1)) if how == "slab" else (0, nx)    # a compact slab: i_origin = i_begin > 0, odd plane count
    assert e <= nx
    m = e - b
    assert m >= 1 and (how != "slab" or (b > 0 and m % 2 == 1))
    algo = BRUTE if how == "brute" else CULLED
    new = lambda: torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
    dv = new() if name in ("build_vdw", "build_fused") else None
    dc = new() if name in ("build_coulomb", "build_fused") else None
    if name == "build_vdw":
        plan.build_vdw(dv.data_ptr(), m * ny * nz, b, e, b, algo)
    elif name == "build_coulomb":
        plan.build_coulomb(dc.data_ptr(), m * ny * nz, b, e, b, algo)
    else:
        plan.build_fused(dv.data_ptr(), dc.data_ptr(), m * ny * nz, b, e, b, algo)
    torch.cuda.synchronize()
    return (dv.cpu().numpy() if dv is not None else None), (dc.cpu().numpy() if dc is not None else None), (b, e)


@pytest.mark.parametrize("call", GRID_CALLS + POINT_CALLS)
@pytest.mark.parametrize("pid", sorted(PLANS))
def test_plain_call_on_plan(ctx, pid, call):
    """One ordinary call on one plan against the oracle's values for probe 0 (stored grids: compare_grids with floor0 = 0, the bound of
    every fixture grid of the suite; raw sums: compare_raw at its default).  On the plan without charges the calls that need them
    return CEG_ERR_INVALID and write nothing.  Where Na is probe 0 its hard sphere must clamp somewhere (2e7 stored): the grid has a
    live exact path."""
    plan = ctx.plan(pid)
    w, probes = ctx.probe_set(pid)
    charged = PLANS[pid][3]
    if call in NEEDS_CHARGE and not charged:
        if call in GRID_CALLS:
            with pytest.raises(_abi.CegError) as ei:
                _grids(plan, call, w.cset)
        else:
            with pytest.raises(_abi.CegError) as ei:
                plan.eval_points("coulomb", ctx.ref(pid, ("pts",))[:64], BRUTE if call.endswith("brute") else CULLED)
        assert ei.value.code == -1                                   # CEG_ERR_INVALID: refused before any launch
        return
    if call in POINT_CALLS:
        which = "vdw" if call.startswith("eval_vdw") else "coulomb"
        pts = ctx.ref(pid, ("pts",))
        got = plan.eval_points(which, pts, BRUTE if call.endswith("brute") else CULLED)
        worst = compare_raw(got, ctx.ref(pid, (which, "pts")), f"{pid}/{call}")
        print(f"{pid}/{call}: worst relative error {worst:.2e} over {len(pts)} points")
        return
    gv, gc, (b, e) = _grids(plan, call, w.cset)
    if gv is not None:
        worst = compare_grids(gv, ctx.ref(pid, "vdw")[:, b:e], f"{pid}/{call}/vdw", floor0=0.0)
        print(f"{pid}/{call}: vdw worst relative error {worst:.2e}")
        if (PLANS[pid][2] or ("Na",))[0] == "Na":
            assert (gv[0] == np.float32(2e7)).any(), "the hard sphere of Na clamps nowhere on this grid"
    if gc is not None:
        worst = compare_grids(gc, ctx.ref(pid, "coulomb")[:, b:e], f"{pid}/{call}/coulomb", floor0=0.0)
        print(f"{pid}/{call}: coulomb worst relative error {worst:.2e}")


@pytest.mark.parametrize("pid", [p for p in sorted(PLANS) if PLANS[p][2] is not None])
def test_plain_calls_equal_the_multi_call_bit_for_bit(ctx, pid):
    """The ordinary build_vdw / build_fused of a multi-probe plan give probe 0's grid and the Coulomb grid of ceg_plan_build_multi on
    the SAME plan, bit for bit: the header's promise that a grid does not depend on how a request is cut into launches, extended to
    "probe 0 through the ordinary call" (the single-probe kernel of probe 0's class on probe 0's constant block is what the multi
    call launches for that grid; the Lennard-Jones multi-probe variants keep each probe's sums in the same order).  Na's grid from
    the multi call holds a clamped value whichever probe it is."""
    import torch
    plan = ctx.plan(pid)
    w, probes = ctx.probe_set(pid)
    _fw, _sp, atoms, charged, _env = PLANS[pid]
    nx, ny, nz = w.cset.npoints
    outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda") for _ in atoms]
    oc = torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda") if charged else None
    plan.build([o.data_ptr() for o in outs], oc.data_ptr() if charged else 0, nx * ny * nz, 0, nx)
    torch.cuda.synchronize()
    multi_v = [o.cpu().numpy() for o in outs]
    assert (multi_v[atoms.index("Na")][0] == np.float32(2e7)).any()
    gv, _none, _r = _grids(plan, "build_vdw-culled", w.cset)
    assert np.array_equal(gv.view(np.uint32), multi_v[0].view(np.uint32)), "build_vdw vs probe 0 of build_multi"
    if charged:
        fv, fc, _r = _grids(plan, "build_fused-culled", w.cset)
        assert np.array_equal(fv.view(np.uint32), multi_v[0].view(np.uint32)), "build_fused (VdW) vs probe 0 of build_multi"
        assert np.array_equal(fc.view(np.uint32), oc.cpu().numpy().view(np.uint32)), "build_fused (Coulomb) vs build_multi"
        _n, gc, _r = _grids(plan, "build_coulomb-culled", w.cset)
        assert np.array_equal(gc.view(np.uint32), oc.cpu().numpy().view(np.uint32)), "build_coulomb vs build_multi"


def test_one_probe_multi_plan_equals_the_ordinary_plan(ctx):
    """m1-na against s-na: ceg_plan_build_fused of the one-probe multi plan and of the ordinary plan of the same probe are the same
    launch on the same tables -- bit-identical, as test_one_probe_of_any_rule_class_shares_the_pass_with_the_coulomb_grid asserts for
    the multi call."""
    w, _probes = ctx.probe_set("s-na")
    mv, mc, _r = _grids(ctx.plan("m1-na"), "build_fused-culled", w.cset)
    sv, sc, _r = _grids(ctx.plan("s-na"), "build_fused-culled", w.cset)
    assert np.array_equal(mv.view(np.uint32), sv.view(np.uint32))
    assert np.array_equal(mc.view(np.uint32), sc.view(np.uint32))
