"""GPU parity tests proper: the HIP kernels, called through the C ABI (libceg_hip.so), against
the CPU oracle / the committed golden samples.  Tolerance: 1e-6 relative on every stored
Float32 value (north_star), identical NaN / Inf / 2e7-sentinel patterns, bit-exact grid
geometry (indices and offsets are integers computed by the same formulas; positions are
checked bitwise through the raw FP64 path).  Run with `pytest -m gpu` on an MI355X."""
import math
import os
from pathlib import Path

import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi, grids as G, workloads as W
from ceg_hip.plan import GridPlan
from ceg_hip.hostmirror.utils import mat_from_parameters, perpendicular_lengths, prepare_periodic_distance_computations
from oracle.compare import compare_grids

from util import compare_raw, grid_points, random_atoms, synthetic_probes

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
CASES = {"cha_0.5": ("CHA_1.4_3b4eeb96", 0.5), "cha_0.1": ("CHA_1.4_3b4eeb96", 0.1), "cit7_0.15": ("CIT-7", 0.15)}
BRUTE, CULLED, AUTO = _abi.ALGO_BRUTEFORCE, _abi.ALGO_CULLED, _abi.ALGO_AUTO


# ------------------------------------------------------------------ golden samples
@pytest.mark.parametrize("case", sorted(CASES))
def test_golden_samples(hip_lib, case):
    """BASELINE configs 1 / 2 and the triclinic supercell case at the committed sample points:
    raw FP64 sums (both algorithms) and the Float32 values of full one-shot grid builds."""
    fwname, spacing = CASES[case]
    z = np.load(GOLDEN / f"samples_{case}.npz")
    i, j, k = z["idx"].T
    for atom in ("Ar", "Na"):
        w = W.fixture_workload(fwname, atom, spacing)
        np.testing.assert_array_equal(w.cset.dims, z["dims"])            # bit-exact geometry
        plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
        assert plan.can_cull
        for algo in (BRUTE, CULLED):
            compare_raw(plan.eval_points("vdw", z["points"], algo), z[f"raw_vdw_{atom}"], f"{case}/vdw/{atom}/algo{algo}")
            if atom == "Ar":
                compare_raw(plan.eval_points("coulomb", z["points"], algo), z["raw_coulomb"], f"{case}/coulomb/algo{algo}")
        plan.close()
        grid = G.build_vdw_array(w.probe_vdw, w.cset)
        compare_grids(grid[:, i, j, k], z[f"f32_vdw_{atom}"].T, f"{case}/grid/vdw/{atom}")
    grid = G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset)
    compare_grids(grid[:, i, j, k], z["f32_coulomb"].T, f"{case}/grid/coulomb")


# ------------------------------------------------------------------ full grids vs oracle
@pytest.mark.parametrize("fwname,spacing", [("CHA_1.4_3b4eeb96", 0.5), ("CIT-7", 0.3), ("CHA_1.4_3b4eeb96_Na_11812", 0.7)])
def test_full_grids_vs_oracle(hip_lib, oracle, fwname, spacing):
    for atom in ("Ar", "Na"):
        w = W.fixture_workload(fwname, atom, spacing)
        lam, thr = G.vdw_scaling()
        ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr)
        got = G.build_vdw_array(w.probe_vdw, w.cset)
        assert got.shape == ref.shape and got.dtype == np.float32
        # floor0 = 0: channel 0 (the energy) of the fixture grids -- Ar: LJ, Na: the tabulated Buckingham class -- within 1e-6
        # of the oracle's stored value with no absolute allowance
        compare_grids(got, ref, f"{fwname}/{atom}", floor0=0.0)
    lam, thr = G.coulomb_scaling()
    ref, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr)
    compare_grids(G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset), ref, f"{fwname}/coulomb", floor0=0.0)


def test_create_grid_files_roundtrip(hip_lib, oracle, tmp_path, forcefield):
    """create_grid_vdw / create_grid_coulomb -> file -> parse_grid -> interpolate_grid, vs the same
    through the oracle (the drop-in boundary as a caller sees it)."""
    fw = ceg.load_framework_RASPA("CIT-7", "BoulfelfelSholl2021")
    g = ceg.create_grid_vdw(tmp_path / "v.grid", fw, forcefield, 0.4, "Na")
    eg = ceg.parse_grid(tmp_path / "v.grid", False)
    assert eg.num_unitcell == (2, 3, 3)
    np.testing.assert_array_equal(eg.grid, (g.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32))
    w = W.fixture_workload("CIT-7", "Na", 0.4)
    lam, thr = G.vdw_scaling()
    ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr)
    compare_grids(g, ref, "create_grid_vdw")
    ew = ceg.initialize_ewald(fw)
    gc = ceg.create_grid_coulomb(tmp_path / "c.grid", fw, forcefield, 0.4, ew)
    ec = ceg.parse_grid(tmp_path / "c.grid", True)
    assert ec.ewald_precision == 1e-6
    lam, thr = G.coulomb_scaling()
    refc, _ = oracle.grid_coulomb(w.probe_coulomb, ew.alpha, w.cset, lam, thr)
    compare_grids(gc, refc, "create_grid_coulomb")
    ref_eg = G.EnergyGrid(eg.csetup, eg.num_unitcell, math.inf, True, (ref.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32))
    for p in ([3.1, 4.2, 5.3], [-2.0, 7.5, 1.0], [9.99, 0.01, 8.0]):
        a, b = ceg.interpolate_grid(eg, p), ceg.interpolate_grid(ref_eg, p)
        assert a == b or a == pytest.approx(b, rel=1e-5)


# ------------------------------------------------------------------ synthetic edge cases
def _check_all(plan, pv, pc, alpha, cset, oracle, what, algos=(BRUTE, CULLED)):
    pts = grid_points(cset)
    ref_v = oracle.points_vdw(pv, pts)
    ref_c = oracle.points_coulomb(pc, alpha, pts)
    for algo in algos:
        compare_raw(plan.eval_points("vdw", pts, algo), ref_v, f"{what}/vdw/algo{algo}")
        compare_raw(plan.eval_points("coulomb", pts, algo), ref_c, f"{what}/coulomb/algo{algo}")
    return ref_v, ref_c


@pytest.mark.parametrize("name,lengths,angles", [
    ("orthorhombic", (25.0, 27.0, 30.0), (90.0, 90.0, 90.0)),        # diagonal matrix: wrapped == nearest
    ("near-ortho", (26.0, 26.0, 26.0), (91.5, 88.6, 90.9)),          # ortho flag true, images dropped like the reference
    ("triclinic", (27.0, 29.0, 33.0), (94.07, 100.0, 85.0)),
    ("skewed-60", (31.0, 31.0, 31.0), (60.0, 60.0, 60.0)),            # safemin2 < cutoff2: stale-vector branch is live
    ("skewed-mixed", (30.0, 33.0, 36.0), (65.0, 110.0, 75.0)),
])
def test_cells_and_min_image_branches(hip_lib, oracle, name, lengths, angles):
    mat = mat_from_parameters(lengths, angles)
    assert perpendicular_lengths(mat).min() >= 24.0, perpendicular_lengths(mat)
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = 120
    pos = random_atoms(mat, n, rng)
    kinds = rng.integers(1, 5, n)
    q = rng.uniform(-1.2, 1.9, n)
    pv, pc = synthetic_probes(mat, pos, kinds, q)
    ortho, safemin2 = pv.periodic_setup()
    if name.startswith("skewed"):
        assert not ortho and safemin2 < 144.0
    if name == "near-ortho":
        assert ortho
    cset = W.grid_setup_with_dims(mat, (9, 7, 11))                     # 10 x 8 x 12 points: partial 4x4x4 tiles
    alpha = 0.26505830360350674
    plan = GridPlan(cset, pv, pc, alpha)
    assert plan.can_cull
    _check_all(plan, pv, pc, alpha, cset, oracle, name)
    plan.close()


def test_delta_argument_only_scales_the_derivative_channels(hip_lib, oracle):
    """`delta` at the C boundary is a scale factor of channels 1..7 (grids.jl:126-133) and nothing else: a caller that passes
    something other than size / dims (here 1e-3 of it) must still get the right images.  The cell is triclinic with
    perpendicular widths barely above 2 x cutoff, so that a tile CAN keep images other than the fractionally wrapped one; the
    plan-level shortcut that skips the per-candidate test used to be derived from `delta`."""
    import dataclasses
    mat = mat_from_parameters((24.9, 25.3, 25.8), (84.0, 97.0, 93.0))
    assert 24.0 <= perpendicular_lengths(mat).min() < 25.5, perpendicular_lengths(mat)
    rng = np.random.default_rng(2024)
    pos = random_atoms(mat, 150, rng)
    pv, pc = synthetic_probes(mat, pos, rng.integers(1, 5, 150), rng.uniform(-1, 1, 150))
    cset = W.grid_setup_with_dims(mat, (19, 17, 21))
    wrong = dataclasses.replace(cset, delta=cset.delta * 1e-3)
    alpha = 0.26505830360350674
    for cs, tag in ((cset, "true delta"), (wrong, "delta x 1e-3")):
        lam, thr = G.vdw_scaling()
        compare_grids(G.build_vdw_array(pv, cs), oracle.grid_vdw(pv, cs, lam, thr)[0], f"wrong-delta/vdw/{tag}")
        lam, thr = G.coulomb_scaling()
        compare_grids(G.build_coulomb_array(pc, alpha, cs), oracle.grid_coulomb(pc, alpha, cs, lam, thr)[0], f"wrong-delta/coulomb/{tag}")
    # and the value channel does not depend on delta at all
    np.testing.assert_array_equal(G.build_vdw_array(pv, cset)[0], G.build_vdw_array(pv, wrong)[0])


def test_random_cells_fuzz(hip_lib, oracle):
    """Seeded fuzz over what the named cases above fix by hand: 24 random cells (lengths 24.5-40 A, angles
    58-122 degrees, rejected until every perpendicular width is >= 24 A), 40-200 atoms of random kinds and
    charges, random cutoff (9-12 A), random odd grid dims; full-FP64 point sums of both kernels against the
    oracle at 1e-9.  Covers ortho / non-ortho, safemin below and above the cutoff, partial tiles."""
    rng = np.random.default_rng(20261004)
    seen = {"ortho": 0, "stale": 0, "plain": 0}
    done = 0
    while done < 24:
        lengths = rng.uniform(24.5, 40.0, 3)
        angles = rng.uniform(58.0, 122.0, 3) if done % 4 else rng.uniform(88.6, 91.4, 3)
        try:
            mat = mat_from_parameters(tuple(lengths), tuple(angles))
        except Exception:
            continue
        if not np.all(np.isfinite(mat)) or np.linalg.det(mat) <= 0 or perpendicular_lengths(mat).min() < 24.0:
            continue
        cutoff = float(rng.choice([9.0, 10.5, 12.0]))
        n = int(rng.integers(40, 200))
        pos = random_atoms(mat, n, rng, min_sep=1.2)
        if done % 2:                  # atoms given outside the unit cell (unwrapped input), as a CIF may list them
            pos = pos + (mat @ rng.integers(-2, 3, (3, n))).T
        pv, pc = synthetic_probes(mat, pos, rng.integers(1, 5, n), rng.uniform(-1.5, 1.5, n), cutoff=cutoff)
        ortho, safemin2 = pv.periodic_setup()
        seen["ortho" if ortho else ("stale" if safemin2 < cutoff ** 2 else "plain")] += 1
        dims = tuple(int(x) for x in 2 * rng.integers(0, 7, 3) + 1)             # 1 ... 13: down to 2 points per axis
        cset = W.grid_setup_with_dims(mat, dims)
        alpha = float(rng.uniform(0.2, 0.3))
        plan = GridPlan(cset, pv, pc, alpha)
        assert plan.can_cull
        _check_all(plan, pv, pc, alpha, cset, oracle, f"fuzz{done}: {np.round(lengths, 2)} {np.round(angles, 1)} cutoff {cutoff} dims {dims}")
        plan.close()
        done += 1
    assert min(seen.values()) >= 2, seen


@pytest.mark.parametrize("cutoff,edge", [(30.0, 64.0), (21.0, 47.0)])
def test_large_cutoff_many_bin_rows(hip_lib, oracle, cutoff, edge):
    """Cutoffs far beyond the reference's 12 A: the neighbourhood of a tile spans more than 64 bin rows, so the
    row enumeration of the culled kernel takes several passes and a tile sees thousands of candidates."""
    mat = mat_from_parameters((edge, edge + 3.0, edge + 5.0), (93.0, 97.0, 86.0))
    assert perpendicular_lengths(mat).min() >= 2 * cutoff
    rng = np.random.default_rng(int(cutoff))
    n = 900
    pos = random_atoms(mat, n, rng, min_sep=2.0)
    pv, pc = synthetic_probes(mat, pos, rng.integers(1, 5, n), rng.uniform(-1.0, 1.0, n), cutoff=cutoff)
    cset = W.grid_setup_with_dims(mat, (7, 9, 5))
    alpha = 4.5 / cutoff
    plan = GridPlan(cset, pv, pc, alpha)
    assert plan.can_cull and plan.num_images > 3 * n
    _check_all(plan, pv, pc, alpha, cset, oracle, f"cutoff {cutoff}")
    plan.close()


@pytest.mark.parametrize("variant", ["generic-vdw", "wide-hard-sphere", "libm-ewald"])
def test_kernel_variants_off_the_fast_path(hip_lib, oracle, variant):
    """Template variants the fixtures never select: generic rule runs in the hot loop (a LJ+Buckingham
    sum has no fast class), a hard sphere wider than the default exact-path radius (the radius must
    grow past it), and alpha*cutoff beyond the erfcx table's domain (libm-grade erfc/exp)."""
    mat = mat_from_parameters((27.0, 29.0, 33.0), (94.07, 100.0, 85.0))
    rng = np.random.default_rng(2024)
    n = 150
    pos = random_atoms(mat, n, rng)
    kinds = rng.integers(1, 5, n)
    q = rng.uniform(-1.2, 1.9, n)
    ffkw, alpha = {}, 0.26505830360350674
    if variant == "generic-vdw":
        ffkw = {"generic": True}
    elif variant == "wide-hard-sphere":
        ffkw = {"hs_radius": 2.7}
    else:
        alpha = 0.5                                        # alpha*12 = 6 > 5
    pv, pc = synthetic_probes(mat, pos, kinds, q, **ffkw)
    cset = W.grid_setup_with_dims(mat, (21, 19, 23))
    plan = GridPlan(cset, pv, pc, alpha)
    ref_v, ref_c = _check_all(plan, pv, pc, alpha, cset, oracle, variant)
    if variant == "wide-hard-sphere":
        assert np.isinf(ref_v[:, 0]).any()
    plan.close()
    lam, thr = G.vdw_scaling()
    compare_grids(G.build_vdw_array(pv, cset), oracle.grid_vdw(pv, cset, lam, thr)[0], variant + "/grid")
    lam, thr = G.coulomb_scaling()
    compare_grids(G.build_coulomb_array(pc, alpha, cset), oracle.grid_coulomb(pc, alpha, cset, lam, thr)[0], variant + "/cgrid")


def test_fast_math_accuracy_single_pair(hip_lib, oracle):
    """One atom, points at r in [2, 12) A in random directions: the culled kernel's hot-loop
    arithmetic (v_rsq/v_rcp Newton steps, table exp, r^2-indexed Ewald tables, csrc/ceg_math.h) against the
    oracle's libm, no cancellation between atoms -> 1e-12 relative on all 8 FP64 outputs of every VdW class (Coulomb beyond 5.6 A:
    see below)."""
    L = 40.0
    mat = np.diag([L, L, L])
    cset = W.grid_setup_with_dims(mat, (15, 15, 15))
    centre = np.array([20.0, 20.0, 20.0])
    rng = np.random.default_rng(77)
    r = np.linspace(2.0001, 11.9999, 4096)
    u = rng.normal(size=(len(r), 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pts = centre + r[:, None] * u
    from scipy.ndimage import maximum_filter1d
    for kind in (1, 4, 2):          # LJ, LJ, Buckingham + hard sphere (the single tabulated Buckingham class of the culled kernel)
        pv, pc = synthetic_probes(mat, [centre], [kind], [0.9094])
        plan = GridPlan(cset, pv, pc, 0.26505830360350674)
        for which, ref in (("vdw", oracle.points_vdw(pv, pts)), ("coulomb", oracle.points_coulomb(pc, 0.26505830360350674, pts))):
            got = plan.eval_points(which, pts, CULLED)
            assert np.all(np.isfinite(ref))
            # the LJ factors change sign (x6 = 1, 1/2, 2/7, 5/28): judge each value against the
            # local magnitude of its column (+-0.1 A window along r), not against a zero crossing
            env = maximum_filter1d(np.abs(ref), size=81, axis=0, mode="nearest")
            rel = np.abs(got - ref) / env
            # the same errors against a floor of 1 % of the column's largest magnitude: what a pair term can add to a sum
            rel_sum = np.abs(got - ref) / np.maximum(env, 1e-2 * np.abs(ref).max(axis=0))
            print(f"fast-math max rel err {which} kind {kind}: local {rel.max():.2e} (r < 8 A: {rel[r < 8.0].max():.2e}), "
                  f"vs column scale {rel_sum.max():.2e}")
            # VdW: 1e-12 everywhere.  Coulomb (r^2-indexed degree-6 tables, 32 intervals per octave of r^2): 1e-12 up to 8 A and
            # against the column scale; the interpolation error grows to 1e-11 of the term itself at the cutoff, where the
            # term is 1e-5 of its value at 2 A
            # (round 3: the tabulated Buckingham class -- A exp(-B r) from an r^2-indexed degree-7 table, third-order 1/sqrt step --
            #  meets the same 1e-12 as Lennard-Jones: measured 4e-14; round 2's degree-5 table needed 2e-10 here)
            tol_local = 1e-12 if which == "vdw" else 3e-11
            assert rel.max() < tol_local, (which, kind, float(rel.max()), int(np.argmax(rel.max(axis=1))))
            assert rel[r < 5.6].max() < 1.5e-12 and rel_sum.max() < 5e-12, (which, kind, float(rel_sum.max()))
        plan.close()


def test_points_on_atoms_nan_inf_patterns(hip_lib, oracle):
    """Grid points that coincide with atoms: LJ value +Inf and -Inf*0 = NaN derivatives, hard-sphere
    Inf, Coulomb Inf within 1 A -- must come out identically (then clamp to the 2e7 sentinel)."""
    L = 30.0
    mat = np.diag([L, L, L])
    cset = W.grid_setup_with_dims(mat, (15, 15, 15))                   # spacing 2.0 exactly, shift 0
    pos = np.array([[4.0, 6.0, 8.0], [10.0, 10.0, 10.0], [20.0, 2.0, 28.0], [11.3, 17.7, 5.1], [0.0, 0.0, 0.0]])
    kinds = np.array([1, 2, 4, 2, 1])
    q = np.array([1.0, -1.0, 0.5, 0.0, -0.7])
    pv, pc = synthetic_probes(mat, pos, kinds, q)
    alpha = 0.265
    plan = GridPlan(cset, pv, pc, alpha)
    ref_v, ref_c = _check_all(plan, pv, pc, alpha, cset, oracle, "on-atoms")
    assert np.isnan(ref_v).any() and np.isinf(ref_v).any() and np.isinf(ref_c).any() and np.isnan(ref_c).any()
    plan.close()
    for build, probe, sc, args in ((G.build_vdw_array, pv, G.vdw_scaling, ()), (G.build_coulomb_array, pc, G.coulomb_scaling, (alpha,))):
        got = build(probe, *args, cset)
        lam, thr = sc()
        ref = (oracle.grid_vdw(pv, cset, lam, thr) if not args else oracle.grid_coulomb(pc, alpha, cset, lam, thr))[0]
        compare_grids(got, ref, "on-atoms/grid")
        assert (ref[0] == np.float32(2e7)).any() and np.isnan(ref[1:4]).any()


def test_small_cell_forces_bruteforce(hip_lib, oracle):
    """A ProbeSystem that violates the 2*cutoff width rule (never produced by ProbeSystem itself,
    probes.jl:24, but legal at the C boundary): AUTO must fall back to the literal kernel, CULLED
    must refuse."""
    mat = mat_from_parameters((15.0, 16.0, 17.0), (80.0, 95.0, 100.0))
    rng = np.random.default_rng(3)
    pos = random_atoms(mat, 40, rng)
    pv, pc = synthetic_probes(mat, pos, rng.integers(1, 5, 40), rng.uniform(-1, 1, 40))
    cset = W.grid_setup_with_dims(mat, (7, 7, 7))
    plan = GridPlan(cset, pv, pc, 0.265)
    assert not plan.can_cull
    _check_all(plan, pv, pc, 0.265, cset, oracle, "small-cell", algos=(BRUTE, AUTO))
    with pytest.raises(_abi.CegError) as ei:
        plan.eval_points("vdw", grid_points(cset), CULLED)
    assert ei.value.code == -5
    plan.close()
    lam, thr = G.vdw_scaling()
    compare_grids(G.build_vdw_array(pv, cset), oracle.grid_vdw(pv, cset, lam, thr)[0], "small-cell/grid")


def test_empty_and_single_atom_frameworks(hip_lib, oracle):
    mat = np.diag([24.0, 25.0, 26.0])
    cset = W.grid_setup_with_dims(mat, (5, 5, 5))
    pv, pc = synthetic_probes(mat, [[1.0, 2.0, 3.0]], [1], [0.8])
    plan = GridPlan(cset, pv, pc, 0.265)
    _check_all(plan, pv, pc, 0.265, cset, oracle, "single")
    plan.close()
    pv0, pc0 = synthetic_probes(mat, np.empty((0, 3)), np.empty(0, dtype=np.int64), np.empty(0))
    got = G.build_vdw_array(pv0, cset)
    assert got.shape == (8, 6, 6, 6) and np.all(got == 0)
    assert np.all(G.build_coulomb_array(pc0, 0.265, cset) == 0)


def test_eval_points_outside_grid_box(hip_lib, oracle):
    w = W.fixture_workload("CIT-7", "Na", 1.0)
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    rng = np.random.default_rng(9)
    pts = rng.uniform(-60, 90, (300, 3))                                # far outside the unit-cell bounding box
    compare_raw(plan.eval_points("vdw", pts, AUTO), oracle.points_vdw(w.probe_vdw, pts), "outside/vdw")
    compare_raw(plan.eval_points("coulomb", pts, AUTO), oracle.points_coulomb(w.probe_coulomb, w.alpha, pts), "outside/coulomb")
    with pytest.raises(_abi.CegError):
        plan.eval_points("vdw", pts, CULLED)
    inside = w.cset.shift + rng.uniform(0, 1, (500, 3)) * w.cset.size   # unordered points: arbitrary 64-point "tiles"
    compare_raw(plan.eval_points("vdw", inside, CULLED), oracle.points_vdw(w.probe_vdw, inside), "scattered/vdw")
    compare_raw(plan.eval_points("coulomb", inside, CULLED), oracle.points_coulomb(w.probe_coulomb, w.alpha, inside), "scattered/coulomb")
    plan.close()


def test_library_rejects_invalid_rule_kinds(hip_lib):
    """A Monomial rule on a kind that occurs in the framework -> CEG_ERR_RULE (interactions.jl:462-465)."""
    w = W.fixture_workload("CIT-7", "Ar", 2.0)
    rules, off = w.forcefield.rule_table(w.probe_vdw.probe)
    k = w.forcefield.sdict["Oz"]
    rules[off[k - 1]]["kind"] = 5
    pos = np.ascontiguousarray(w.probe_vdw.positions)
    kinds = np.ascontiguousarray(w.probe_vdw.atomkinds)
    dims, size, shift, delta = G._grid_args(w.cset)
    grid = np.empty((8,) + w.cset.npoints, dtype=np.float32)
    lam, thr = G.vdw_scaling()
    mat, inv = G._matT(w.probe_vdw.mat), G._matT(w.probe_vdw.invmat)
    rc = hip_lib.ceg_grid_vdw(_abi.dptr(pos), _abi.i64ptr(kinds), len(kinds), _abi.dptr(mat), _abi.dptr(inv), 0, 144.2, 144.0,
                              rules.ctypes.data, _abi.i32ptr(off), w.forcefield.nkinds, _abi.i32ptr(dims), _abi.dptr(size),
                              _abi.dptr(shift), _abi.dptr(delta), lam, thr, _abi.fptr(grid), 1)
    assert rc == -4 and b"not valid in a VdW grid" in hip_lib.ceg_last_error()
    rc = hip_lib.ceg_grid_vdw(_abi.dptr(pos), _abi.i64ptr(kinds), len(kinds), _abi.dptr(mat), _abi.dptr(inv), 0, 144.2, 144.0,
                              rules.ctypes.data, _abi.i32ptr(off), w.forcefield.nkinds, _abi.i32ptr(dims), _abi.dptr(size),
                              _abi.dptr(shift), _abi.dptr(delta), lam, thr, _abi.fptr(grid), 99)
    assert rc == -2


# ------------------------------------------------------------------ plan API on device buffers
def test_slabs_fused_and_layouts(hip_lib, oracle):
    """x-slab builds into device memory (full buffer and compact slabs, odd split), fused ==
    separate, culled == brute force, all == oracle."""
    import torch
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Na", 0.9)
    nx, ny, nz = w.cset.npoints
    plane = ny * nz
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    dev = torch.device("cuda", 0)
    lam, thr = G.vdw_scaling()
    ref_v, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr)
    lam, thr = G.coulomb_scaling()
    ref_c, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr)
    full_v = torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device=dev)
    full_c = torch.full_like(full_v, float("nan"))
    s = torch.cuda.current_stream().cuda_stream
    cuts = [0, 5, 6, 19, nx]                                           # uneven slabs, one of a single plane
    for b, e in zip(cuts[:-1], cuts[1:]):
        plan.build_fused(full_v.data_ptr(), full_c.data_ptr(), nx * plane, b, e, 0, CULLED, s)
    torch.cuda.synchronize()
    compare_grids(full_v.cpu().numpy(), ref_v, "slabs/fused/vdw")
    compare_grids(full_c.cpu().numpy(), ref_c, "slabs/fused/coulomb")
    # compact slab buffers, separate kernels, brute force
    b, e = 7, 21
    loc_v = torch.empty((8, e - b, ny, nz), dtype=torch.float32, device=dev)
    loc_c = torch.empty_like(loc_v)
    plan.build_vdw(loc_v.data_ptr(), (e - b) * plane, b, e, b, BRUTE, s)
    plan.build_coulomb(loc_c.data_ptr(), (e - b) * plane, b, e, b, BRUTE, s)
    torch.cuda.synchronize()
    compare_grids(loc_v.cpu().numpy(), ref_v[:, b:e], "slab/brute/vdw")
    compare_grids(loc_c.cpu().numpy(), ref_c[:, b:e], "slab/brute/coulomb")
    # culled and brute force agree with each other far inside the tolerance
    compare_grids(loc_v.cpu().numpy(), full_v[:, b:e].cpu().numpy(), "slab/brute-vs-culled", rtol=2e-7)
    # argument validation
    for bad in ((-1, 3, 0), (3, 2, 0), (0, nx + 1, 0), (4, 6, 5)):
        with pytest.raises(_abi.CegError):
            plan.build_vdw(loc_v.data_ptr(), nx * plane, bad[0], bad[1], bad[2], AUTO, s)
    with pytest.raises(_abi.CegError):
        plan.build_vdw(loc_v.data_ptr(), 3, 0, 4, 0, AUTO, s)
    plan.close()


def test_block_cyclic_chunk_launches(hip_lib):
    """The launch pattern of bench.py at N > 1 (ceg_hip.distributed.CyclicPlan / PipelinedGather,
    "staged" placement): every rank's chunks are built into compact [8, m, ny, nz] blocks
    (channel stride m*ny*nz, i_origin = i_begin), stacked like all_gather_into_tensor stacks them
    and put in place with the same strided copy; the result equals the single-launch grid bit for
    bit (chunks start on tile boundaries)."""
    import torch
    from ceg_hip.distributed import cyclic_plan
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Ar", 0.5, dims=(63, 61, 57))        # nx = 64
    nx, ny, nz = w.cset.npoints
    plane = ny * nz
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    ref_v = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
    ref_c = torch.empty_like(ref_v)
    plan.build_fused(ref_v.data_ptr(), ref_c.data_ptr(), nx * plane, 0, nx, 0, CULLED, s)
    for world in (2, 4):
        full_v = torch.full_like(ref_v, float("nan"))
        full_c = torch.full_like(ref_c, float("nan"))
        cycs = [cyclic_plan(nx, world, rank, nchunks=4) for rank in range(world)]
        assert all(c is not None and c.m % 4 == 0 for c in cycs)
        m, K = cycs[0].m, cycs[0].nchunks
        locs_v = [torch.full((K, 8, m, ny, nz), float("nan"), dtype=torch.float32, device=dev) for _ in range(world)]
        locs_c = [torch.full_like(t, float("nan")) for t in locs_v]
        for rank, cyc in enumerate(cycs):
            for j in range(K):
                b, e = cyc.chunk(j)
                plan.build_fused(locs_v[rank][j].data_ptr(), locs_c[rank][j].data_ptr(), m * plane, b, e, b, CULLED, s)
        torch.cuda.synchronize()
        for j in range(K):
            lo, hi = cycs[0].block(j)
            for full, locs in ((full_v, locs_v), (full_c, locs_c)):
                stage = torch.stack([locs[r][j] for r in range(world)])          # what the all-gather produces
                full[:, lo:hi].unflatten(1, (world, m)).copy_(stage.permute(1, 0, 2, 3, 4))
        assert torch.equal(full_v, ref_v) and torch.equal(full_c, ref_c)
    plan.close()


def test_pipelined_gather_over_rccl_single_rank(hip_lib):
    """bench.py's N > 1 code path with the real backend: an RCCL ("nccl") process group of ONE rank
    (one GPU per box here; two ranks on one device are refused by RCCL), collectives forced on.
    Exercises all_gather_into_tensor on the side stream into the staging buffer / into slices of the
    final array, the event hand-off between the streams and the strided placement copy; the gloo
    tests cover the world > 1 index arithmetic."""
    import socket
    import torch
    import torch.distributed as dist
    from ceg_hip.distributed import PipelinedGather, allgather_grid, cyclic_plan
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Ar", 0.5, dims=(63, 61, 57))        # nx = 64
    nx, ny, nz = w.cset.npoints
    plane = ny * nz
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
        s = torch.cuda.current_stream().cuda_stream
        ref_v = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
        ref_c = torch.empty_like(ref_v)
        plan.build_fused(ref_v.data_ptr(), ref_c.data_ptr(), nx * plane, 0, nx, 0, CULLED, s)
        cyc = cyclic_plan(nx, 1, 0, nchunks=4)
        assert cyc.nchunks == 4 and cyc.m == 16
        for mode in ("staged", "inplace", "p2p"):
            fulls = [torch.full_like(ref_v, float("nan")), torch.full_like(ref_c, float("nan"))]
            locs = [torch.full((4, 8, cyc.m, ny, nz), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
            pipe = PipelinedGather(cyc, fulls, locs, mode=mode, force_collectives=True)

            def launch(j, ib, ie, blocks):
                plan.build_fused(blocks[0].data_ptr(), blocks[1].data_ptr(), cyc.m * plane, ib, ie, ib, CULLED,
                                 torch.cuda.current_stream().cuda_stream)
            for _ in range(2):                                        # twice: the staging buffers alternate and are reused
                pipe.run(launch)
            torch.cuda.synchronize()
            assert torch.equal(fulls[0], ref_v) and torch.equal(fulls[1], ref_c), mode
        # slab fallback (world 1 short-circuits to a copy)
        out = torch.empty_like(ref_v)
        allgather_grid(out, ref_v)
        assert torch.equal(out, ref_v)
        plan.close()
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ row f1: batched interpolation
def test_interpolation_batch_vs_oracle(hip_lib, oracle):
    """GPU interpolate_grid (ceg_interp_*) against the literal COEFF*X oracle: random points far
    outside the cell (wrap), points exactly on grid nodes and on the upper faces (p0 == extent
    guard), VdW blocking rule, Coulomb-style grid without it; then the device-resident path:
    grid built on the GPU, scaled in place like parse_grid, interpolated without leaving the GPU."""
    import torch
    from ceg_hip.interp import GridInterpolator
    for fwname, atom, sp in (("CIT-7", "Ar", 0.4), ("CHA_1.4_3b4eeb96", "Na", 0.8)):
        w = W.fixture_workload(fwname, atom, sp)
        nx, ny, nz = w.cset.npoints
        rng = np.random.default_rng(5)
        nodes = np.stack([rng.integers(0, nx, 200), rng.integers(0, ny, 200), rng.integers(0, nz, 200)], axis=1)
        nodes[:20] = [nx - 1, ny - 1, nz - 1]
        nodes[20:40, 0] = nx - 1
        on_nodes = nodes * w.cset.size / w.cset.dims + w.cset.shift
        pts = np.concatenate([rng.uniform(-70, 90, (4000, 3)), on_nodes, w.cset.shift + rng.uniform(0, 1, (2000, 3)) * w.cset.size])
        gv = G.build_vdw_array(w.probe_vdw, w.cset)
        gc = G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset)
        for grid, prec in ((gv, math.inf), (gc, 1e-6)):
            gk = (grid.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32)
            eg = G.EnergyGrid(w.cset, w.probe_vdw.num_supercell, prec, True, gk)
            ref = oracle.interpolate_points(eg, pts)
            it = GridInterpolator(eg)
            got = it(pts)
            it.close()
            assert np.array_equal(got == 1e100, ref == 1e100), "blocked pattern differs"
            m = ref != 1e100
            scale = np.median(np.abs(ref[m]))
            assert np.all(np.abs(got[m] - ref[m]) <= 1e-9 * np.abs(ref[m]) + 1e-10 * scale)
            assert (prec == math.inf) == bool((ref == 1e100).any())
        # device-resident: build -> scale in place -> interpolate, no host round trip of the grid
        plan = GridPlan(w.cset, w.probe_vdw, None, 0.0)
        dev = torch.device("cuda", 0)
        d_grid = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        plan.build_vdw(d_grid.data_ptr(), nx * ny * nz, 0, nx, 0, AUTO, s)
        _abi.check(hip_lib, hip_lib.ceg_scale_grid_device(d_grid.data_ptr(), d_grid.numel(), ceg.GRID_TO_KELVIN, 0, s))
        torch.cuda.synchronize()
        gk = (gv.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32)
        assert np.array_equal(d_grid.cpu().numpy(), gk, equal_nan=True)           # parse_grid's Float32 scaling, bitwise
        eg = G.EnergyGrid(w.cset, w.probe_vdw.num_supercell, math.inf, True, gk)
        it = GridInterpolator(eg, device_ptr=d_grid.data_ptr())
        d_pts = torch.from_numpy(pts).to(dev)
        d_out = torch.empty(len(pts), dtype=torch.float64, device=dev)
        it.on_device(d_pts.data_ptr(), len(pts), d_out.data_ptr(), s)
        torch.cuda.synchronize()
        host = GridInterpolator(eg)
        assert np.array_equal(d_out.cpu().numpy(), host(pts))
        host.close(); it.close(); plan.close()


# ------------------------------------------------------------------ BASELINE size, size-independent properties
def test_roofline_workload_properties(hip_lib, oracle):
    """256^3 x 11 664 atoms (BASELINE config 3).  The oracle would need ~15 CPU-hours for the full
    grid, so: (a) culled == brute force on a slab, (b) slab builds are independent of the split,
    (c) invariance under translating every atom by a lattice vector, (d) an oracle block."""
    import torch
    w = W.roofline_workload("Ar", 255)
    nx, ny, nz = w.cset.npoints
    plane = ny * nz
    dev = torch.device("cuda", 0)
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    assert plan.can_cull and plan.num_images > w.natoms
    s = torch.cuda.current_stream().cuda_stream
    full_v = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
    full_c = torch.empty_like(full_v)
    plan.build_fused(full_v.data_ptr(), full_c.data_ptr(), nx * plane, 0, nx, 0, CULLED, s)
    torch.cuda.synchronize()
    assert torch.isfinite(full_v).all() and torch.isfinite(full_c).all()
    assert (full_v[0] == 2e7).any() and (full_c[0] == 2e7).any()
    # (a) brute force on 8 x-planes
    b, e = 100, 108
    loc_v = torch.empty((8, e - b, ny, nz), dtype=torch.float32, device=dev)
    loc_c = torch.empty_like(loc_v)
    plan.build_fused(loc_v.data_ptr(), loc_c.data_ptr(), (e - b) * plane, b, e, b, BRUTE, s)
    torch.cuda.synchronize()
    compare_grids(full_v[:, b:e].cpu().numpy(), loc_v.cpu().numpy(), "R/culled-vs-brute/vdw")
    compare_grids(full_c[:, b:e].cpu().numpy(), loc_c.cpu().numpy(), "R/culled-vs-brute/coulomb")
    # (b) split independence (bitwise: same tiles, same candidate order only if tile origin is the same;
    #     slabs starting at multiples of 4 keep the tiling, so those are bit-identical)
    again = torch.empty_like(full_v)
    for sb, se in ((0, 64), (64, 200), (200, nx)):
        plan.build_vdw(again.data_ptr(), nx * plane, sb, se, 0, CULLED, s)
    torch.cuda.synchronize()
    assert torch.equal(again, full_v)
    odd = torch.empty((8, 7, ny, nz), dtype=torch.float32, device=dev)
    plan.build_vdw(odd.data_ptr(), 7 * plane, 33, 40, 33, CULLED, s)          # tiles shifted by one plane
    torch.cuda.synchronize()
    compare_grids(odd.cpu().numpy(), full_v[:, 33:40].cpu().numpy(), "R/shifted-tiles", rtol=2e-7)
    plan.close()
    # (c) lattice-translation invariance
    import copy
    pv2, pc2 = copy.copy(w.probe_vdw), copy.copy(w.probe_coulomb)
    t = w.probe_vdw.mat @ np.array([1.0, -1.0, 2.0])
    pv2.positions = w.probe_vdw.positions + t
    pc2.positions = pv2.positions
    plan2 = GridPlan(w.cset, pv2, pc2, w.alpha)
    v2 = torch.empty((8, 16, ny, nz), dtype=torch.float32, device=dev)
    c2 = torch.empty_like(v2)
    plan2.build_fused(v2.data_ptr(), c2.data_ptr(), 16 * plane, 120, 136, 120, CULLED, s)
    torch.cuda.synchronize()
    compare_grids(v2.cpu().numpy(), full_v[:, 120:136].cpu().numpy(), "R/translation/vdw")
    compare_grids(c2.cpu().numpy(), full_c[:, 120:136].cpu().numpy(), "R/translation/coulomb")
    plan2.close()
    # (d) oracle block: 16 planes x 2 rows
    i0, i1, j0, j1 = 120, 136, 128, 130
    lam, thr = G.vdw_scaling()
    ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr, i0, i1, j_begin=j0, j_end=j1)
    compare_grids(full_v[:, i0:i1, j0:j1].cpu().numpy(), ref[:, i0:i1, j0:j1], "R/oracle/vdw")
    lam, thr = G.coulomb_scaling()
    ref, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr, i0, i1, j_begin=j0, j_end=j1)
    compare_grids(full_c[:, i0:i1, j0:j1].cpu().numpy(), ref[:, i0:i1, j0:j1], "R/oracle/coulomb")


def test_fused_build_speed_canary(hip_lib):
    """Not a benchmark (bench.py is): the fused 256^3 x 11 664-atom build took 17.5 ms in round 1 and takes 12.9 - 14.1 ms box by box
    now; a build that needs more than 20 ms has lost its hot loop (spills, a table that no longer fits, a fallback path)."""
    import torch
    w = W.roofline_workload("Ar", 255)
    nx, ny, nz = w.cset.npoints
    dev = torch.device("cuda", 0)
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    v = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
    c = torch.empty_like(v)
    s = torch.cuda.current_stream().cuda_stream
    best = 1e9
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.build_fused(v.data_ptr(), c.data_ptr(), nx * ny * nz, 0, nx, 0, CULLED, s)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    plan.close()
    assert best < 20.0, f"fused build {best:.2f} ms"


def test_multi_device_oneshot(hip_lib, oracle, monkeypatch):
    """ngpus > 1 in the one-shot entry point (single process, one host thread + plan + slab per device).  On a
    one-GPU box the slabs are oversubscribed onto the one card (CEG_HIP_OVERSUBSCRIBE), which still runs the
    slab split, the per-device threads and their concurrent use of the caches; uneven splits included."""
    n = hip_lib.ceg_device_count()
    if n < 2:
        monkeypatch.setenv("CEG_HIP_OVERSUBSCRIBE", "1")
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Ar", 0.7)
    nx = w.cset.npoints[0]
    lam, thr = G.vdw_scaling()
    ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr)
    one = G.build_vdw_array(w.probe_vdw, w.cset, ngpus=1)
    for ng in (2, 3, 4) if n < 2 else (min(n, 4),):
        got = G.build_vdw_array(w.probe_vdw, w.cset, ngpus=ng)
        compare_grids(got, ref, f"multi-device x{ng}")
        assert np.array_equal(got, one, equal_nan=True) or np.allclose(got, one, rtol=1e-6, equal_nan=True)
    lamc, thrc = G.coulomb_scaling()
    refc, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lamc, thrc)
    compare_grids(G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset, ngpus=3 if n < 2 else min(n, 4)), refc, "multi-device coulomb")
    if n < 2:
        monkeypatch.delenv("CEG_HIP_OVERSUBSCRIBE")
        with pytest.raises(_abi.CegError) as ei:
            G.build_vdw_array(w.probe_vdw, w.cset, ngpus=2)
        assert ei.value.code == -2


def test_device_resident_oneshot(hip_lib, monkeypatch):
    """ceg_grid_vdw_device / ceg_grid_coulomb_device: the one-shot build with the assembled grid left in device memory (slab 0
    built in place, the other slabs gathered by hipMemcpyPeerAsync) is bit-identical to the host one-shot array, for 1 and
    (oversubscribed onto one card where there is only one) 2-4 slabs incl. uneven splits; and the grid goes on to the
    interpolation consumer without leaving the GPU (ceg_scale_grid_device + ceg_interp_create on the device pointer)."""
    import torch
    from ceg_hip.hostmirror.constants import GRID_TO_KELVIN
    from ceg_hip.interp import GridInterpolator
    n = hip_lib.ceg_device_count()
    w = W.fixture_workload("CIT-7", "Ar", 0.6)
    host_v = G.build_vdw_array(w.probe_vdw, w.cset)
    host_c = G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset)
    dev_v = G.build_vdw_device(w.probe_vdw, w.cset)
    assert dev_v.is_cuda and np.array_equal(dev_v.cpu().numpy(), host_v, equal_nan=True)
    if n < 2:
        monkeypatch.setenv("CEG_HIP_OVERSUBSCRIBE", "1")
    for ng in (2, 3, 4) if n < 2 else (min(n, 4),):
        assert np.array_equal(G.build_vdw_device(w.probe_vdw, w.cset, ngpus=ng).cpu().numpy(), host_v, equal_nan=True), ng
        assert np.array_equal(G.build_coulomb_device(w.probe_coulomb, w.alpha, w.cset, ngpus=ng).cpu().numpy(), host_c, equal_nan=True), ng
    # devices without peer access (forced: CEG_HIP_NO_PEER): the finished slabs travel through pinned host memory instead
    monkeypatch.setenv("CEG_HIP_NO_PEER", "1")
    ng = 3 if n < 2 else min(n, 4)
    assert np.array_equal(G.build_vdw_device(w.probe_vdw, w.cset, ngpus=ng).cpu().numpy(), host_v, equal_nan=True)
    assert np.array_equal(G.build_coulomb_device(w.probe_coulomb, w.alpha, w.cset, ngpus=ng).cpu().numpy(), host_c, equal_nan=True)
    monkeypatch.delenv("CEG_HIP_NO_PEER")
    if n < 2:
        monkeypatch.delenv("CEG_HIP_OVERSUBSCRIBE")
        with pytest.raises(_abi.CegError):
            G.build_vdw_device(w.probe_vdw, w.cset, ngpus=2)
    # build -> parse_grid's scaling -> interpolation handle, all on the device, against the host route
    _abi.check(hip_lib, hip_lib.ceg_scale_grid_device(dev_v.data_ptr(), dev_v.numel(), GRID_TO_KELVIN, 0, None))
    torch.cuda.synchronize()
    scaled = host_v.copy()
    np.multiply(scaled, GRID_TO_KELVIN, out=scaled, dtype=np.float64, casting="same_kind")       # as parse_grid does (grids.jl:78)
    g = G.EnergyGrid(w.cset, (1, 1, 1), float("inf"), True, scaled)
    pts = np.random.default_rng(3).uniform(-5, 40, (4096, 3))
    on_dev, on_host = GridInterpolator(g, 0, device_ptr=dev_v.data_ptr()), GridInterpolator(g, 0)
    a, b = on_dev(pts), on_host(pts)
    assert np.array_equal(a, b)
    on_dev.close(); on_host.close()


# ------------------------------------------------------------------ row f2: batched reciprocal Ewald + energy_grid
def test_reciprocal_batch_vs_oracle(hip_lib, oracle):
    """ceg_recip_* (sincospi tables in LDS, one wave per placement) against the literal oracle."""
    from ceg_hip.energy import ReciprocalEwald
    rng = np.random.default_rng(21)
    for fwname, sc in (("CHA_1.4_3b4eeb96", (1, 1, 1)), ("CIT-7", None), ("CHA_1.4_3b4eeb96_Na_11812", (1, 1, 1))):
        fw = ceg.load_framework_RASPA(fwname, "BoulfelfelSholl2021")
        ef = ceg.initialize_ewald(fw, sc)
        rec = ReciprocalEwald(ef)
        for molname in ("Na", "CO2"):
            mol = ceg.load_molecule_RASPA(molname, "TraPPE", "BoulfelfelSholl2021")
            base = np.asarray(mol.position, dtype=np.float64).reshape(-1, 3)
            pos = rng.uniform(-40, 60, (1003, 1, 3)) + base[None]          # not a multiple of the 4 waves per workgroup
            pos[0] = base                                                    # origin
            got = rec.energies(mol, pos)
            ref = oracle.reciprocal_energies(ef, mol, pos)
            assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-11 * np.abs(ref).max()), (fwname, molname)
        assert len(rec.energies(mol, np.empty((0, len(base), 3)))) == 0
        rec.close()


def test_reciprocal_rows_layout_edge_cases(hip_lib, oracle):
    """The row / segment layout of ceg_recip (round 3): a k-space too large for the LDS copy of its constants (precision 1e-12:
    the planes stay in global memory), the k-vectors handed over in a shuffled order (regrouped into rows by ceg_recip_create),
    a 16-atom rigid molecule, and a replaced structure factor -- each against the oracle / against the sorted order."""
    import ctypes as C
    from ceg_hip.energy import ReciprocalEwald
    from ceg_hip.hostmirror.ewald import ewald_context_constants
    rng = np.random.default_rng(77)
    fw = ceg.load_framework_RASPA("CIT-7", "BoulfelfelSholl2021")
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", "BoulfelfelSholl2021")
    base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
    pos = rng.uniform(-30, 50, (257, 1, 3)) + base[None]
    for precision in (1e-6, 1e-12):
        ef = ceg.initialize_ewald(fw, None, precision)
        nk = len(ef.kfactors)
        assert (nk > 4000) == (precision < 1e-9)          # 1e-12: > 64 KB of constants
        rec = ReciprocalEwald(ef)
        got = rec.energies(co2, pos)
        ref = oracle.reciprocal_energies(ef, co2, pos)
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-11 * np.abs(ref).max()), precision
        rec.close()
        # shuffled order through the C ABI
        perm = rng.permutation(nk)
        ijk = np.ascontiguousarray(np.asarray(ef.kvec_ijk, dtype=np.int32)[perm])
        kf = np.ascontiguousarray(np.asarray(ef.kfactors, dtype=np.float64)[perm])
        sf = np.asarray(ef.StoreRigidChargeFramework)[perm]
        re_, im_ = np.ascontiguousarray(sf.real), np.ascontiguousarray(sf.imag)
        ks = np.asarray(ef.kspace.ks, dtype=np.int32)
        inv = np.ascontiguousarray(np.asarray(ef.invmat, dtype=np.float64).T.reshape(-1))      # column-major
        h = C.c_void_p()
        _abi.check(hip_lib, hip_lib.ceg_recip_create(C.byref(h), 0, _abi.i32ptr(ijk.reshape(-1)), _abi.dptr(kf), _abi.dptr(re_),
                                                     _abi.dptr(im_), nk, _abi.i32ptr(ks), _abi.dptr(inv)))
        q = np.ascontiguousarray(co2.atomic_charge, dtype=np.float64)
        enc, static = ewald_context_constants(ef, ((co2,),))
        out = np.empty(len(pos))
        _abi.check(hip_lib, hip_lib.ceg_recip_energy(h, _abi.dptr(pos.reshape(-1)), _abi.dptr(q), len(q), len(pos), enc, static, _abi.dptr(out)))
        assert np.all(np.abs(out - got) <= 1e-12 * np.abs(got).max())
        # a replaced structure factor (single_contribution_ewald's "rest") and both constants zero
        sf2 = sf * np.exp(1j * rng.uniform(0, 6.28, nk))
        _abi.check(hip_lib, hip_lib.ceg_recip_set_structure_factor(h, _abi.dptr(np.ascontiguousarray(sf2.real)), _abi.dptr(np.ascontiguousarray(sf2.imag))))
        out2 = np.empty(len(pos))
        _abi.check(hip_lib, hip_lib.ceg_recip_energy(h, _abi.dptr(pos.reshape(-1)), _abi.dptr(q), len(q), len(pos), 0.0, 0.0, _abi.dptr(out2)))
        frac = np.einsum("ij,naj->nai", np.asarray(ef.invmat), pos.reshape(len(pos), -1, 3))
        S = (q[None, :, None] * np.exp(2j * np.pi * np.einsum("nai,ki->nak", frac, ijk.astype(np.float64)))).sum(axis=1)     # [n, nk]
        want = 2.0 * (kf * (np.conj(sf2)[None] * S).real).sum(axis=1) + (kf * np.abs(S) ** 2).sum(axis=1)
        assert np.all(np.abs(out2 - want) <= 1e-9 * np.abs(want).max())
        # 16 atoms (the most the kernel holds)
        big = rng.uniform(-5, 5, (33, 16, 3))
        q16 = np.ascontiguousarray(rng.uniform(-1, 1, 16))
        out3 = np.empty(len(big))
        _abi.check(hip_lib, hip_lib.ceg_recip_energy(h, _abi.dptr(big.reshape(-1)), _abi.dptr(q16), 16, len(big), 0.0, 0.0, _abi.dptr(out3)))
        frac = np.einsum("ij,naj->nai", np.asarray(ef.invmat), big)
        S = (q16[None, :, None] * np.exp(2j * np.pi * np.einsum("nai,ki->nak", frac, ijk.astype(np.float64)))).sum(axis=1)
        want = 2.0 * (kf * (np.conj(sf2)[None] * S).real).sum(axis=1) + (kf * np.abs(S) ** 2).sum(axis=1)
        assert np.all(np.abs(out3 - want) <= 1e-9 * np.abs(want).max())
        hip_lib.ceg_recip_destroy(h)


def _local_minima(grid, tolerance=1e-2, faces_only=False):
    """CEG.local_minima (basins.jl:40-98): strict minimum over the 26 periodic neighbours (or the 6
    face neighbours), kept when within ``tolerance`` of the global one; sorted like Julia's
    CartesianIndex (last axis first), 1-based."""
    ok = np.ones(grid.shape, dtype=bool)
    for d in np.ndindex(3, 3, 3):
        if d != (1, 1, 1) and (not faces_only or sum(x != 1 for x in d) == 1):
            ok &= grid < np.roll(grid, (d[0] - 1, d[1] - 1, d[2] - 1), axis=(0, 1, 2))
    idx = np.argwhere(ok)
    emin = grid[ok].min()
    if tolerance >= 0:
        idx = idx[grid[tuple(idx.T)] <= emin + abs(emin * tolerance)]
    return sorted((tuple(int(x) + 1 for x in i) for i in idx), key=lambda t: t[::-1])


def test_reference_energy_grid_flow(hip_lib, tmp_path):
    """The reference's own end-to-end test (test/runtests.jl:24-50), run through this repo's path:
    setup_RASPA -> .grid files built by the HIP kernels at 0.15 A -> energy_grid at 0.3 A (batched
    GPU interpolation + GPU reciprocal Ewald) -> local minima.  Pins: minima INDICES (exact) and
    energies (runtests.jl literals, rtol 1e-3 there; what we reach is asserted tighter)."""
    from ceg_hip.energy import GpuEnergySetup
    raspa = tmp_path / "raspa"
    raspa.mkdir()
    for sub in ("forcefield", "molecules", "structures"):
        os.symlink(GOLDEN / "raspa" / sub, raspa / sub)
    ceg.setdir_RASPA(raspa)
    try:
        # --- Ar in CHA + Na (VdW only, blocking spheres from CHA.block)
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96_Na_11812", "BoulfelfelSholl2021", "Ar", "TraPPE", blockfile=None)
        gs = GpuEnergySetup(setup)
        egrid = gs.energy_grid(0.3)
        vdw, coul = ceg.energy_point(setup, [[0.0, 0.0, 0.0]])
        assert coul == 0.0 and vdw != 0.0
        assert egrid[0, 0, 0] == pytest.approx(vdw, rel=1e-9)                               # runtests.jl:30
        # runtests.jl:36 lists (56,88,49), (52,50,91), (51,51,91).  The last two are diagonal neighbours
        # (E = -1841.02 and -1832.66 K), so the 26-neighbour rule of basins.jl:40-98 at this commit can
        # only keep the lower one; the literal list is what the face-neighbour rule gives.  Both are pinned.
        assert _local_minima(egrid, faces_only=True) == [(56, 88, 49), (52, 50, 91), (51, 51, 91)]
        assert _local_minima(egrid) == [(56, 88, 49), (52, 50, 91)]
        assert egrid[51, 49, 90] == egrid.min()
        assert egrid[51, 49, 90] == pytest.approx(-1841.0165092850448, rel=1e-7)            # runtests.jl:38 (rtol 1e-3 there)
        assert (egrid == 1e100).any()                                                       # blocked pockets
        gs.close()
        # --- Na+ in CHA (Buckingham + hard-sphere VdW grid, Coulomb grid, reciprocal Ewald)
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021", "Na", "TraPPE")
        gs = GpuEnergySetup(setup)
        e0 = gs.energy_points(np.zeros((1, 1, 3)))[0]
        assert e0[0] == pytest.approx(-11083.13758653269, rel=1e-7)                          # runtests.jl:44
        assert e0[1] == pytest.approx(-1.8509402225092095e6, rel=1e-8)                       # runtests.jl:45
        host = ceg.energy_point(setup, [[0.0, 0.0, 0.0]])
        assert e0[0] == pytest.approx(host[0], rel=1e-10) and e0[1] == pytest.approx(host[1], rel=1e-10)
        egrid = gs.energy_grid(0.3)
        assert egrid[0, 0, 0] == pytest.approx(e0[0] + e0[1], rel=1e-12)                     # runtests.jl:46
        assert _local_minima(egrid, 0.0) == [(29, 60, 60)]                                  # runtests.jl:49
        # runtests.jl:50 (rtol 1e-3 there).  The literal is reproduced to 4.0e-5 only, although the
        # origin literals above are met to 1e-8: the CPU oracle (interpolate_with_oracle + compute_ewald
        # mirror, scripts in test_reference_pins) gives -1927971.7327074807 at this node, digit for digit
        # what the GPU path returns, so the last digits of the literal predate the reference's current code.
        assert egrid[28, 59, 59] == pytest.approx(-1.9278944364761321e6, rel=1e-4)
        assert egrid[28, 59, 59] == pytest.approx(-1927971.7327074807, rel=1e-9)
        gs.close()
        # --- blocking sphere straddling a periodic boundary (runtests.jl:269-272); the sphere scan of
        #     parse_blockfile runs on the GPU inside setup_RASPA
        setup = ceg.setup_RASPA("CIT7block", "BoulfelfelSholl2021", "Ar", "TraPPE")
        assert not setup.block.empty
        assert ceg.energy_point(setup, [[12.5, 0.8, 0.3]]) == (1e100, 0.0)
        assert ceg.energy_point(setup, [[20.175808361078516, 10.58027451750961, 9.185277912816744]]) == (1e100, 0.0)
        gs = GpuEnergySetup(setup)
        pts = np.concatenate([[[12.5, 0.8, 0.3]], np.random.default_rng(4).uniform(0.0, 12.0, (200, 3))])[:, None, :]
        e = gs.energy_points(pts)
        assert tuple(e[0]) == (1e100, 0.0) and np.all(e[:, 1] == 0.0)
        host = np.array([ceg.energy_point(setup, p)[0] for p in pts])
        assert np.array_equal(e[:, 0] == 1e100, host == 1e100) and (host != 1e100).any()
        ok = host != 1e100
        assert np.allclose(e[ok, 0], host[ok], rtol=1e-9, atol=1e-9)
        gs.close()
    finally:
        ceg.setdir_RASPA(GOLDEN / "raspa")


# ------------------------------------------------------------------ SURVEY 8d variants of the roofline run
def test_truncated_and_synthetic_workloads(hip_lib, oracle):
    """The two other inputs SURVEY §8d names for BASELINE config 3: the exact-10 000-atom truncation of
    the tiled CHA framework (a framework with a hole: tiles with few/no candidates) and the fully
    synthetic 40 A cube (orthorhombic fast branch, random positions, alternating charges)."""
    for w, planes in ((W.roofline_workload("Ar", 63, truncate=10000), (0, 31, 63)), (W.synthetic_workload(3000, 47), (0, 17, 47))):
        nx, ny, nz = w.cset.npoints
        gv = G.build_vdw_array(w.probe_vdw, w.cset)
        gc = G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset)
        for i in planes:
            lam, thr = G.vdw_scaling()
            ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr, i, i + 1)
            compare_grids(gv[:, i:i + 1], ref[:, i:i + 1], f"{w.name}/vdw/plane{i}")
            lam, thr = G.coulomb_scaling()
            ref, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr, i, i + 1)
            compare_grids(gc[:, i:i + 1], ref[:, i:i + 1], f"{w.name}/coulomb/plane{i}")


# ------------------------------------------------------------------ row f4: blocking masks
def test_block_masks_vs_oracle(hip_lib, oracle, tmp_path):
    """ceg_block_spheres (parse_blockfile scan, literal min-image routine in the UNIT cell -- small cells,
    image search live) and ceg_block_from_grid (BlockFile(::EnergyGrid)) against the oracle, bit for bit."""
    root = GOLDEN / "raspa" / "structures" / "block"
    synth = tmp_path / "five.block"
    synth.write_text("5\n0.05 0.5 0.95 2.5\n0.5 0.5 0.5 4.0\n0.99 0.01 0.5 1.2\n0.3 0.7 0.1 0.9\n0.0 0.0 0.0 3.3\n")
    for fwname, blk, sp in (("CIT7block", root / "CIT7block.block", 0.15), ("CHA_1.4_3b4eeb96", synth, 0.3), ("CIT-7", synth, 0.2)):
        fw = ceg.load_framework_RASPA(fwname, "BoulfelfelSholl2021")
        cset = ceg.GridCoordinatesSetup.from_cell(fw.mat, sp)
        centers, r2 = G.read_block_spheres(blk, cset)
        ref = oracle.block_spheres(cset, centers, r2)
        got = G.parse_blockfile_gpu(blk, cset)
        assert ref.any() and np.array_equal(got.block, ref), fwname
    assert G.parse_blockfile_gpu(root / "CHA.block", cset).empty            # "0" file
    # BlockFile(g) on a grid built by the HIP kernels (Na in CHA: hard-sphere walls above 5e6 K)
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Na", 0.4)
    gv = G.build_vdw_array(w.probe_vdw, w.cset)
    gk = (gv.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32)
    eg = G.EnergyGrid(w.cset, (1, 1, 1), math.inf, True, gk)
    ref = oracle.block_from_grid(eg)
    got = G.blockfile_from_grid_gpu(eg)
    assert ref.any() and not ref.all() and np.array_equal(got.block, ref)


def test_consumer_edge_cases(hip_lib, oracle):
    """Empty and degenerate inputs of the f2/f3 entry points: no guest atoms, no placements, a molecule
    larger than the kernels hold, a trial atom exactly on a guest atom (r = 0), the excluded molecule
    being the only one."""
    import ctypes as C
    from ceg_hip.hostmirror import montecarlo as M
    from ceg_hip.energy import PairEnergies, ReciprocalEwald
    ff = ceg.parse_forcefield_RASPA("BoulfelfelSholl2021")
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", "BoulfelfelSholl2021")
    base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
    ids = [ff.sdict[a] for a in co2.atomic_symbol]
    mat = np.array([[30.0, 0, 0], [2.0, 31.0, 0], [-3.0, 1.0, 29.0]]).T
    charges = np.full(len(ff.sdict) + 1, np.nan)
    for k, ix in enumerate(ids):
        charges[ix] = co2.atomic_charge[k]
    guests = [base + np.array([5.0, 5.0, 5.0]), base + np.array([9.0, 6.0, 5.5])]
    mc = M.MonteCarloSetup(ff, mat, np.linalg.inv(mat), [ids], charges, [guests], ceg.EwaldFramework.empty(mat),
                           G.EnergyGrid.trivial(True), [], 0.0)
    pe = PairEnergies(ff, mc.mat, mc.invmat)
    trial = np.stack([base + np.array([7.0, 5.0, 5.0]), guests[1], base + np.array([35.0 + 7.0, 5.0 - 31.0, 5.0])])   # free, on top of guest 1, wrapped
    # no guest atoms uploaded yet
    assert np.array_equal(pe.energies(trial, ids), np.zeros(3))
    pe.set_atoms(np.concatenate(guests), ids * 2, [0, 0, 0, 1, 1, 1])
    assert len(pe.energies(np.empty((0, 3, 3)), ids)) == 0
    got = pe.energies(trial, ids, exclude_molecule=0)
    ref = oracle.single_contribution_vdw(mc, (0, 0), trial)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    fin = np.isfinite(ref)
    assert np.allclose(got[fin], ref[fin], rtol=1e-10, atol=1e-9)
    assert not np.isfinite(ref[1])                                   # r = 0 pairs: the reference's Inf/NaN, reproduced
    # batches of growing and shrinking size through ONE handle (it keeps its device buffers between calls and only ever grows them)
    rng = np.random.default_rng(9)
    for n in (5, 3000, 7, 40000, 1):
        tr = (rng.uniform(0, 1, (n, 3)) @ mc.mat.T)[:, None, :] + base[None]
        got_n = pe.energies(tr, ids, exclude_molecule=1)
        ref_n = oracle.single_contribution_vdw(mc, (0, 1), tr)
        fin = np.isfinite(ref_n)
        assert np.array_equal(np.isfinite(got_n), fin) and np.allclose(got_n[fin], ref_n[fin], rtol=1e-9, atol=1e-9), n
    # every guest excluded
    pe.set_atoms(guests[0], ids, [0, 0, 0])
    assert np.array_equal(pe.energies(trial, ids, exclude_molecule=0), np.zeros(3))
    # 17-atom molecule: refused, not truncated
    big = np.zeros((1, 17, 3))
    rc = hip_lib.ceg_pairs_energy(pe._h, _abi.dptr(big.reshape(-1)), _abi.i32ptr(np.zeros(17, dtype=np.int32)), 17, 1, -1,
                                  _abi.dptr(np.zeros(1)))
    assert rc == -5
    pe.close()
    fw = ceg.load_framework_RASPA("CIT-7", "BoulfelfelSholl2021")
    rec = ReciprocalEwald(ceg.initialize_ewald(fw))
    rc = hip_lib.ceg_recip_energy(rec._h, _abi.dptr(big.reshape(-1)), _abi.dptr(np.zeros(17)), 17, 1, 0.0, 0.0, _abi.dptr(np.zeros(1)))
    assert rc == -5 and b"16" in hip_lib.ceg_last_error()
    rec.close()


def _plan_images(hip_lib, plan_handle):
    import ctypes as C
    n = int(hip_lib.ceg_plan_num_images(plan_handle))
    nb = np.zeros(3, dtype=np.int32)
    _abi.check(hip_lib, hip_lib.ceg_plan_copy_images(plan_handle, None, None, None, None, _abi.i32ptr(nb)))
    xyzq = np.empty((n, 4)); kind = np.full(n, -7, dtype=np.int32); atom = np.empty(n, dtype=np.int32)
    start = np.empty(int(nb.prod()) + 1, dtype=np.int32)
    _abi.check(hip_lib, hip_lib.ceg_plan_copy_images(plan_handle, _abi.dptr(xyzq.reshape(-1)), _abi.i32ptr(kind), _abi.i32ptr(atom), _abi.i32ptr(start), _abi.i32ptr(nb)))
    return xyzq, kind, atom, start, tuple(int(x) for x in nb)


@pytest.mark.parametrize("case", ["roofline-fused", "cit7-vdw-only", "cha-coulomb-only", "skewed-synthetic"])
def test_image_list_built_on_the_device(hip_lib, monkeypatch, case):
    """The lattice-image list of a plan is built ON THE DEVICE since round 4 (csrc/ceg_images.hip: count / scan / emit / stable sort
    by bin -- per-bin counting sort, or hipcub's radix sort with CEG_HIP_IMAGES_SORT=radix -- / gather) instead of by the host loop of build_images (csrc/ceg_api.hip) -- the host-side analogue of the ProbeSystem
    tiling, probes.jl:37-53.  The two builds must agree BYTE for byte: positions, charges, kind + rule flags, atom indices, bin
    starts -- for a fused plan (every atom listed), a VdW-only plan (atoms without a rule left out), a Coulomb-only plan (no kinds)
    and a skewed synthetic cell; and a build through each list gives bit-identical grids."""
    from ceg_hip.plan import GridPlan
    import torch
    monkeypatch.setenv("CEG_HIP_IMAGE_CACHE", "0")                  # every plan builds its own list
    if case == "roofline-fused":
        w = W.roofline_workload("Ar", 63)
        args = (w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    elif case == "cit7-vdw-only":
        w = W.fixture_workload("CIT-7", "Ar", 0.5)
        args = (w.cset, w.probe_vdw, None, 0.0)
    elif case == "cha-coulomb-only":
        w = W.fixture_workload("CHA_1.4_3b4eeb96", "Na", 0.6)
        args = (w.cset, None, w.probe_coulomb, w.alpha)
    else:
        mat = mat_from_parameters((30.0, 33.0, 36.0), (65.0, 110.0, 75.0))
        rng = np.random.default_rng(12)
        pos = random_atoms(mat, 200, rng)
        pv, pc = synthetic_probes(mat, pos, rng.integers(1, 5, 200), rng.uniform(-1, 1, 200))
        cset = W.grid_setup_with_dims(mat, (23, 19, 17))
        w = None
        args = (cset, pv, pc, 0.265)
    lists, grids = {}, {}
    for where in ("device", "device-radix", "host"):                # device: the lean form (per-bin counting sort), device-radix: the first form
        monkeypatch.delenv("CEG_HIP_IMAGES_ON_HOST", raising=False)
        monkeypatch.delenv("CEG_HIP_IMAGES_SORT", raising=False)
        if where == "host":
            monkeypatch.setenv("CEG_HIP_IMAGES_ON_HOST", "1")
        elif where == "device-radix":
            monkeypatch.setenv("CEG_HIP_IMAGES_SORT", "radix")
        plan = GridPlan(*args)
        lists[where] = _plan_images(hip_lib, plan._h)
        cset = args[0]
        nx, ny, nz = cset.npoints
        out = torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
        if args[1] is not None:
            plan.build_vdw(out.data_ptr(), nx * ny * nz, 0, nx)
        else:
            plan.build_coulomb(out.data_ptr(), nx * ny * nz, 0, nx)
        torch.cuda.synchronize()
        grids[where] = out.cpu().numpy()
        plan.close()
    for other in ("device-radix",):
        for q in range(4):
            assert np.array_equal(lists["device"][q].view(np.uint8), lists[other][q].view(np.uint8)), (other, q)
        assert np.array_equal(grids["device"].view(np.int32), grids[other].view(np.int32))
    d, h = lists["device"], lists["host"]
    assert d[4] == h[4] and len(d[0]) == len(h[0]) > 0
    assert np.array_equal(d[0].view(np.int64), h[0].view(np.int64)), "positions / charges differ"
    assert np.array_equal(d[1], h[1]) and np.array_equal(d[2], h[2]) and np.array_equal(d[3], h[3])
    assert d[3][0] == 0 and d[3][-1] == len(d[0]) and (np.diff(d[3]) >= 0).all()
    if case == "cit7-vdw-only":                                     # Si / Al carry no Ar rule: a third of the framework is not listed
        assert (d[1] >> 25 & 1).all() and len(np.unique(d[2])) < 1080
    if case == "cha-coulomb-only":
        assert (d[1] == -1).all()                                   # a Coulomb-only plan carries no kinds
    assert np.array_equal(grids["device"].view(np.int32), grids["host"].view(np.int32))


def test_bench_line_and_exchange_rehearsal(hip_lib):
    """bench.py --full: exactly ONE line on stdout, valid JSON with the contract's keys, the
    roofline / cpu_baseline objects, and -- with --force-exchange -- the N > 1 code path (RCCL group, chunked
    build, collectives on the side stream) ending in a grid that passes the oracle spot check."""
    import json
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    for extra in ([], ["--force-exchange"]):
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--full", "--n", "63", "--steps", "2", "--warmup", "1", "--cpu-rows", "1"] + extra,
                           capture_output=True, text=True, timeout=600, env={**os.environ, "MASTER_PORT": str(port)})
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                    "dtype", "data", "config", "roofline"):
            assert key in d, key
        assert d["steps"] == 2 and d["n_gpus"] == 1 and d["value"] > 0 and d["dtype"] == "f64"
        assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
        rf = d["roofline"]
        assert rf["bound"] == "valu_fp64" and d["roofline_hbm"]["bound"] == "hbm" and 0 < rf["frac_nominal"] < 1.5
        # frac = executed FP64 flops (PMC instruction counts of this library on this workload) / time / peak: only where
        # profiles/pmc_summary.json holds a record of this configuration taken on these kernel sources (the default 256^3 run)
        if rf["pmc"] is not None:       # (a record taken on other kernel sources still gives a figure, flagged: frac_stale)
            assert 0 < rf["frac"] < 1 and rf["frac"] == rf["frac_executed"] and 0 < rf["frac_issue"] < 1
            assert rf["pmc"]["source"] == "profiles/pmc_summary.json" and rf["frac_stale"] == rf["pmc"]["stale"]
        else:
            assert rf["frac"] is None and rf["achieved"] is None
        assert d["selfcheck"]["max_rel_err"] <= 1e-6
        if extra:
            assert d["exchange"]["mode"] == "staged" and "block-cyclic" in d["config"]["parallelism"] and "oneshot" not in d
        else:
            assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
            # the API path the Julia shim binds, timed in the same run (host arrays in and out: PCIe-bound, never `value`)
            one = d["oneshot"]
            for fn in ("ceg_grid_vdw", "ceg_grid_coulomb", "ceg_grids_multi"):
                for route in ("pageable", "page_locked"):
                    assert one[fn][route]["best_ms"] > 0 and len(one[fn][route]["ms"]) == one["reps"], (fn, route)


def test_bench_plain_run_and_dumped_outputs(hip_lib, oracle, tmp_path):
    """A plain bench.py run (no --full): ONE line with the contract's keys and none of what --full adds, `steps` timed steps;
    --dump-outputs writes the grids of the last timed step -- at 64^3 every point -- which match the oracle, and a second run
    with the same arguments writes the same values bit for bit."""
    import json
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--n", "63", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
            assert key in d, key
        assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True
        assert d["value"] == pytest.approx(64 ** 3 / (d["ms_per_step"] * 1e-3))
        assert not {"roofline", "roofline_hbm", "selfcheck", "oneshot", "cpu_baseline"} & set(d), sorted(d)
        assert sorted(p.name for p in out.iterdir()) == ["coulomb.npy", "points.npy", "vdw.npy"]
        dumps.append({n: np.load(out / f"{n}.npy") for n in ("vdw", "coulomb", "points")})
    a, b = dumps
    assert a["points"].dtype == np.float64 and np.array_equal(a["points"], np.arange(64 ** 3))
    for name in ("vdw", "coulomb"):
        assert a[name].dtype == np.float32 and a[name].shape == (8, 64 ** 3)
        assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), name
    w = W.roofline_workload("Ar", 63)
    scratch = np.empty((8, 64, 64, 64), dtype=np.float32)
    for i0, i1 in ((0, 2), (31, 33), (62, 64)):
        lam, thr = G.vdw_scaling()
        ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr, i0, i1, out=scratch)
        compare_grids(a["vdw"].reshape(8, 64, 64, 64)[:, i0:i1], ref[:, i0:i1], f"dumped vdw planes {i0}:{i1}")
        lam, thr = G.coulomb_scaling()
        ref, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr, i0, i1, out=scratch)
        compare_grids(a["coulomb"].reshape(8, 64, 64, 64)[:, i0:i1], ref[:, i0:i1], f"dumped coulomb planes {i0}:{i1}")


def test_bench_full_size_exchange_rehearsal(hip_lib):
    """The N > 1 code path of the benchmark AT THE BENCHMARK'S SIZE on one card: 256^3 x 11 664 atoms, the
    default 8 block-cyclic chunks of 32 planes, an RCCL group of one rank with the collectives forced on (side-stream
    all_gather_into_tensor per chunk, staged placement) -- the chunked launch set the driver's N-GPU run issues per rank at N = 1.
    The assembled grids must pass the oracle spot check (one plane out of the first and of the last chunk) exactly like the
    single-launch run does."""
    import json
    import socket
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--cpu-rows", "0", "--force-exchange"],
                       capture_output=True, text=True, timeout=900, env={**os.environ, "MASTER_PORT": str(port)})
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][0])
    assert d["config"]["grid_points"] == 256 ** 3 and d["config"]["framework_atoms"] == 11664
    assert d["exchange"]["mode"] == "staged" and "8 chunks of 32 planes" in d["config"]["parallelism"], d["config"]["parallelism"]
    assert d["roofline"]["launches_per_step"] == 8
    assert d["selfcheck"]["ok"] and d["selfcheck"]["max_rel_err"] <= 1e-6 and len(d["selfcheck"]["x_planes"]) >= 2
    assert 5.0 < d["ms_per_step"] < 60.0, d["ms_per_step"]


def test_grid_beyond_32bit_indexing(hip_lib, oracle):
    """Maximum size: a 1024^3 grid (1.07e9 points, 8.6e9 floats = 34 GB per grid, channel stride beyond 2^30
    floats, flat offsets beyond 2^32) built into device memory through the plan API; sampled points of every
    channel -- first and last planes, corners, random interior -- against the oracle.  Few atoms so that the
    build itself stays around a second."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip("needs 34 GB of device memory")
    mat = np.diag([60.0, 60.0, 60.0])
    rng = np.random.default_rng(77)
    pos = random_atoms(mat, 40, rng, min_sep=3.0)
    pv, _ = synthetic_probes(mat, pos, rng.integers(1, 5, 40), np.zeros(40))
    n = 1023
    cset = W.grid_setup_with_dims(mat, (n, n, n))
    nx = ny = nz = n + 1
    plan = GridPlan(cset, pv, None, 0.0)
    dev = torch.device("cuda", 0)
    grid = torch.empty((8, nx, ny, nz), dtype=torch.float32, device=dev)
    grid.fill_(float("nan"))
    s = torch.cuda.current_stream().cuda_stream
    plan.build_vdw(grid.data_ptr(), nx * ny * nz, 0, nx, 0, AUTO, s)
    torch.cuda.synchronize()
    idx = np.concatenate([rng.integers(0, nx, (3000, 3)),
                          np.array([[0, 0, 0], [n, n, n], [n, 0, n], [0, n, 0], [n, n, 0], [1023, 1023, 1022], [512, 1023, 1023]]),
                          np.stack([np.full(500, n), rng.integers(0, ny, 500), rng.integers(0, nz, 500)], axis=1)])
    pts = np.stack([idx[:, a] * cset.size[a] / cset.dims[a] + cset.shift[a] for a in range(3)], axis=1)
    lam, thr = G.vdw_scaling()
    ref = oracle.set_gridpoints(oracle.points_vdw(pv, pts), cset.delta, lam, thr)            # float32[n, 8]
    ti = torch.from_numpy(idx).to(dev)
    got = grid[:, ti[:, 0], ti[:, 1], ti[:, 2]].T.cpu().numpy()
    assert not np.isnan(got).any()
    compare_grids(got.T[:, :, None, None], ref.T[:, :, None, None], "1024^3 samples")
    assert not torch.isnan(grid[7, -1, -1, -8:]).any() and not torch.isnan(grid[0, 0, 0, :8]).any()
    del grid
    plan.close()
    torch.cuda.empty_cache()


def test_oneshot_reentrant_from_several_threads(hip_lib):
    """the one-shot entry points must be re-entrant across different output buffers.  Four host
    threads build different grids at the same time (ctypes releases the GIL during the call), repeatedly,
    sharing the library's pinned / device / stream / block caches; every result equals the sequential one."""
    import threading
    ws = [W.fixture_workload("CIT-7", "Na", 0.25), W.fixture_workload("CHA_1.4_3b4eeb96", "Ar", 0.4)]
    jobs = [(lambda w=w: G.build_vdw_array(w.probe_vdw, w.cset)) for w in ws] + \
           [(lambda w=w: G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset)) for w in ws]
    ref = [j() for j in jobs]
    for rnd in range(3):
        out = [None] * len(jobs)
        err = []

        def run(t):
            try:
                out[t] = jobs[t]()
            except Exception as e:          # noqa: BLE001
                err.append((t, repr(e)))
        th = [threading.Thread(target=run, args=(t,)) for t in range(len(jobs))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not err, err
        for t in range(len(jobs)):
            assert np.array_equal(out[t], ref[t], equal_nan=True), (rnd, t)
    assert hip_lib.ceg_release_cached_buffers() == 0
    again = jobs[0]()                        # caches are rebuilt on demand
    assert np.array_equal(again, ref[0], equal_nan=True)


def test_bench_two_and_three_ranks_on_one_gpu(hip_lib):
    """bench.py's N > 1 path with real kernels and more than one rank: 2 and 3 ranks share the GPU over the
    gloo backend (RCCL refuses two ranks on one device) -- block-cyclic chunks gathered with the placement the
    built-in autotune picks, and the padded slab gather when nx is not divisible -- and rank 0's assembled grid must pass
    the oracle spot check exactly."""
    import json
    import socket
    import subprocess
    import sys
    import time
    root = Path(__file__).resolve().parent.parent
    for nranks, dims, mode in ((2, 63, "staged"), (3, 63, "slab"), (2, 63, "fallback")):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), str(root / "bench.py"), "--full", "--gpus", str(nranks), "--backend", "gloo", "--dims", str(dims),
               "--steps", "2", "--warmup", "1", "--cpu-rows", "0"] + (["--gather", "auto"] if mode == "staged" else [])
        # (--gather auto is opt-in since round 3; one of its candidates is made to raise: it must be skipped, not fatal.  "fallback": the
        #  pipelined exchange itself raises in its guarded first step -> contiguous slabs + one all-gather per channel, still a valid line)
        env = {**os.environ, "CEG_BENCH_FAIL_CANDIDATE": "4 chunks, inplace"}
        if mode == "fallback":
            env["CEG_BENCH_FAIL_PIPELINE"] = "1"
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == nranks and d["scaling"] == "strong"
        if mode == "staged":            # --gather auto: chunk counts x {staged, inplace} were each timed, the fastest ran
            tried = d["exchange"]["autotune_ms"]        # e.g. {"8 chunks, staged": ms, "8 chunks, inplace": ms, "4 chunks, staged": ...}
            assert tried["4 chunks, inplace"] is None                       # the injected failure: skipped on every rank
            done = {k: v for k, v in tried.items() if v is not None}
            assert d["exchange"]["mode"] in ("staged", "inplace") and len(done) >= 3 and all(v > 0 for v in done.values())
            assert {k.split(", ")[1] for k in tried} == {"staged", "inplace"} and "8 chunks, staged" in done
        elif mode == "fallback":
            assert d["exchange"]["mode"] == "slab (fallback)" and "injected" in d["exchange"]["fallback_reason"]
            assert "x-slab sharding" in d["config"]["parallelism"]
        else:
            assert d["exchange"]["mode"] == mode
        assert d["selfcheck"]["max_rel_err"] <= 1e-6 and d["selfcheck"]["points"] > 0 and d["selfcheck"]["ok"]
        assert d["exchange"]["bytes_gathered_per_rank"] > 0
    # ONE rank failing is not repaired in-process: the ranks agree through the rendezvous store -- no collective on the
    # failure path -- and every one of them exits non-zero with the reason, promptly, instead of pairing an all_reduce with the peers'
    # all_gather or hanging.  "rank1": before its first collective (the peer is already inside its exchange); "late1": after.
    for inject in ("rank1", "late1"):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), str(root / "bench.py"), "--gpus", "2", "--backend", "gloo", "--dims", "63",
               "--steps", "2", "--warmup", "1", "--cpu-rows", "0"]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                           env={**os.environ, "CEG_BENCH_FAIL_PIPELINE": inject, "CEG_BENCH_FIRST_STEP_TIMEOUT": "60"})
        assert r.returncode != 0, (inject, r.stdout[-500:])
        assert "cannot be agreed on" in r.stderr and "injected" in r.stderr, r.stderr[-3000:]
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]           # no result line from a broken run
        assert time.perf_counter() - t0 < 300, "the failing run must end promptly"


def test_grid_file_streamed_by_the_library(hip_lib, tmp_path, forcefield):
    """ceg_grid_vdw_file / ceg_grid_coulomb_file (row f4, device -> file): the .grid file written chunk by
    chunk during the build is byte-identical to the one the host writer produces from the returned array;
    file-only mode (no host array) gives the same bytes; an unwritable path is an error, not a silent skip."""
    import ctypes as C
    fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021")
    for spacing in (0.45, 0.2):                         # one chunk / several chunks of the pipeline
        g = ceg.create_grid_vdw(tmp_path / "v.grid", fw, forcefield, spacing, "Na")
        cset, nuc = G._setup_grid_common(fw, spacing, forcefield.cutoff)
        G.write_grid_file(tmp_path / "v_host.grid", cset, nuc, g)
        assert (tmp_path / "v.grid").read_bytes() == (tmp_path / "v_host.grid").read_bytes()
        ew = ceg.initialize_ewald(fw)
        gc = ceg.create_grid_coulomb(tmp_path / "c.grid", fw, forcefield, spacing, ew)
        G.write_grid_file(tmp_path / "c_host.grid", cset, nuc, gc, ew.precision)
        assert (tmp_path / "c.grid").read_bytes() == (tmp_path / "c_host.grid").read_bytes()
        eg = ceg.parse_grid(tmp_path / "c.grid", True)
        assert eg.ewald_precision == 1e-6 and tuple(eg.csetup.dims) == tuple(cset.dims)
    # file only: grid pointer NULL
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Na", 0.2)
    header, trailer = G._file_frame(w.cset, (1, 1, 1), None)
    ff = w.probe_vdw.forcefield
    rules, offsets = ff.rule_table(w.probe_vdw.probe)
    ortho, safemin2 = w.probe_vdw.periodic_setup()
    lam, thr = G.vdw_scaling()
    dims, size, shift, delta = G._grid_args(w.cset)
    pos = np.ascontiguousarray(w.probe_vdw.positions, dtype=np.float64)
    kinds = np.ascontiguousarray(w.probe_vdw.atomkinds, dtype=np.int64)
    mat, invmat = G._matT(w.probe_vdw.mat), G._matT(w.probe_vdw.invmat)
    args = (_abi.dptr(pos), _abi.i64ptr(kinds), len(kinds), _abi.dptr(mat), _abi.dptr(invmat), int(ortho), safemin2,
            w.probe_vdw.cutoff2, rules.ctypes.data, _abi.i32ptr(offsets), ff.nkinds, _abi.i32ptr(dims), _abi.dptr(size),
            _abi.dptr(shift), _abi.dptr(delta), lam, thr, None, 1)
    path = tmp_path / "only.grid"
    _abi.check(hip_lib, hip_lib.ceg_grid_vdw_file(*args, os.fsencode(str(path)), header, len(header), trailer, len(trailer)))
    assert path.read_bytes() == (tmp_path / "v.grid").read_bytes()
    rc = hip_lib.ceg_grid_vdw_file(*args, os.fsencode(str(tmp_path / "no_such_dir" / "x.grid")), header, len(header), trailer, len(trailer))
    assert rc == -1 and b"cannot open" in hip_lib.ceg_last_error()


def test_grid_file_never_visible_when_the_build_fails(hip_lib, tmp_path):
    """The cache of the reference only checks isfile(path) (raspa.jl:426) and the reference opens the file after the
    grid is complete (grids.jl:151,178): a streamed build that fails after its file was opened must leave nothing at
    `path` -- neither a new full-size file with a zero payload nor a truncated older one -- and no temporary behind."""
    w = W.fixture_workload("CIT-7", "Ar", 0.5)
    header, trailer = G._file_frame(w.cset, (1, 1, 1), None)
    ff = w.probe_vdw.forcefield
    rules, offsets = ff.rule_table(w.probe_vdw.probe)
    rules = rules.copy()
    lam, thr = G.vdw_scaling()
    dims, size, shift, delta = G._grid_args(w.cset)
    pos = np.ascontiguousarray(w.probe_vdw.positions, dtype=np.float64)
    kinds = np.ascontiguousarray(w.probe_vdw.atomkinds, dtype=np.int64)
    mat, invmat = G._matT(w.probe_vdw.mat), G._matT(w.probe_vdw.invmat)
    ortho, safemin2 = w.probe_vdw.periodic_setup()

    def call(rt, path):
        return hip_lib.ceg_grid_vdw_file(_abi.dptr(pos), _abi.i64ptr(kinds), len(kinds), _abi.dptr(mat), _abi.dptr(invmat), int(ortho),
                                         safemin2, w.probe_vdw.cutoff2, rt.ctypes.data, _abi.i32ptr(offsets), ff.nkinds, _abi.i32ptr(dims),
                                         _abi.dptr(size), _abi.dptr(shift), _abi.dptr(delta), lam, thr, None, 1, os.fsencode(str(path)),
                                         header, len(header), trailer, len(trailer))
    good = tmp_path / "good.grid"
    assert call(rules, good) == 0 and good.stat().st_size > len(header) + len(trailer)
    reference_bytes = good.read_bytes()
    # a rule the kernels refuse (Monomial has no VdW grid form, interactions.jl:462-465) on a kind that is present:
    # detected by the plan, i.e. after oneshot() has created its output file
    present = int(kinds[0]) - 1
    bad = rules.copy()
    assert offsets[present + 1] > offsets[present]
    bad[offsets[present]]["kind"] = 5
    fresh = tmp_path / "fresh.grid"
    assert call(bad, fresh) != 0
    assert not fresh.exists()
    # an older complete file at the same path survives a failed rebuild untouched
    assert call(bad, good) != 0
    assert good.read_bytes() == reference_bytes
    assert sorted(p.name for p in tmp_path.iterdir()) == ["good.grid"]


# ------------------------------------------------------------------ multi-probe plans (all grids of a setup in one pass)
def _probe_set(fwname, atoms, spacing=None, dims=None, tile=None):
    ws = [W.fixture_workload(fwname, a, spacing or 0.0, dims=dims, tile=tile) for a in atoms]
    return ws[0], [w.probe_vdw for w in ws]


@pytest.mark.parametrize("fwname,atoms,spacing", [
    ("CHA_1.4_3b4eeb96", ("C_co2", "O_co2"), 0.45),                       # CO2 in CHA: the reference's own test molecule (2 VdW + Coulomb)
    ("CHA_1.4_3b4eeb96_Na_11812", ("Ar", "C_co2", "O_co2", "N_n2"), 0.7),  # four probes; Na cations in the framework: a second LJ kind
    ("CIT-7", ("O_co2", "Ar", "C_co2"), 0.4),                             # triclinic 2x3x3 supercell, three probes
    ("CIT-7", ("Na", "C_co2", "O_co2"), 0.4),                             # MIXED classes (round 4): the Na + CO2 setup of runtests.jl:240-258 --
                                                                          # a tabulated Buckingham cation beside two Lennard-Jones probes
    ("CHA_1.4_3b4eeb96", ("C_co2", "O_co2", "Ar"), 0.45),                 # CO2 + Ar in CHA: three Lennard-Jones probes + Coulomb in one call
    ("CHA_1.4_3b4eeb96", ("Ar", "Na", "O_co2", "Na"), 0.7),               # the Buckingham probe neither first nor alone (and listed twice)
])
def test_multi_probe_build(hip_lib, oracle, fwname, atoms, spacing):
    """ceg_plan_create_multi / ceg_plan_build_multi: the K VdW grids + the Coulomb grid of one framework from one image list in one
    call (raspa.jl:497-520 asks for them one by one).  (1) every grid within the suite's tolerance of the oracle; (2) every grid
    BIT-identical to the one the same plan produces when asked for that grid alone, and to any other grouping of the request into
    launches (fused pair + VdW rest, VdW only, one by one); (3) slabs with i_origin, skipped outputs.  Probes of several rule
    classes share the plan (round 4): the Lennard-Jones-only ones share accumulating loops, a Buckingham cation is launched with
    the kernel of its class, alone or fused with the Coulomb grid."""
    import torch
    from ceg_hip.plan import MultiGridPlan
    w, probes = _probe_set(fwname, atoms, spacing)
    cset = w.cset
    nx, ny, nz = cset.npoints
    dev = torch.device("cuda", 0)
    K = len(probes)
    plan = MultiGridPlan(cset, probes, w.probe_coulomb, w.alpha)
    cs = nx * ny * nz

    def build(which, coulomb, env=None):
        outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device=dev) if q in which else None for q in range(K)]
        oc = torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device=dev) if coulomb else None
        if env is not None:
            os.environ["CEG_HIP_MULTI_FUSED_NP"] = env
        try:
            plan.build([o.data_ptr() if o is not None else 0 for o in outs], oc.data_ptr() if oc is not None else 0, cs, 0, nx)
        finally:
            os.environ.pop("CEG_HIP_MULTI_FUSED_NP", None)
        torch.cuda.synchronize()
        return [o.cpu().numpy() if o is not None else None for o in outs], (oc.cpu().numpy() if oc is not None else None)

    allv, allc = build(range(K), True)
    lam, thr = G.vdw_scaling()
    for q, pr in enumerate(probes):
        compare_grids(allv[q], oracle.grid_vdw(pr, cset, lam, thr)[0], f"multi/{fwname}/{atoms[q]}", floor0=0.0)
    lam, thr = G.coulomb_scaling()
    compare_grids(allc, oracle.grid_coulomb(w.probe_coulomb, w.alpha, cset, lam, thr)[0], f"multi/{fwname}/coulomb", floor0=0.0)
    # one grid at a time, and other groupings of the same request: bit-identical
    for q in range(K):
        one, _ = build([q], False)
        assert np.array_equal(one[q].view(np.int32), allv[q].view(np.int32)), (atoms[q], "alone")
    _, conly = build([], True)
    assert np.array_equal(conly.view(np.int32), allc.view(np.int32))
    for env in ("0", "1"):
        v2, c2 = build(range(K), True, env)
        assert np.array_equal(c2.view(np.int32), allc.view(np.int32)), env
        for q in range(K):
            assert np.array_equal(v2[q].view(np.int32), allv[q].view(np.int32)), (atoms[q], env)
    vonly, _ = build(range(K), False)
    for q in range(K):
        assert np.array_equal(vonly[q].view(np.int32), allv[q].view(np.int32)), (atoms[q], "vdw only")
    # a slab with an origin, the last probe skipped
    b, e = nx // 3, nx - 2
    m = e - b
    outs = [torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device=dev) for _ in range(K - 1)]
    oc = torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device=dev)
    plan.build([o.data_ptr() for o in outs], oc.data_ptr(), m * ny * nz, b, e, b)
    torch.cuda.synchronize()
    for q in range(K - 1):
        assert np.array_equal(outs[q].cpu().numpy().view(np.int32), allv[q][:, b:e].view(np.int32))
    assert np.array_equal(oc.cpu().numpy().view(np.int32), allc[:, b:e].view(np.int32))
    # against the ordinary single-probe plans: same values up to the order of the FP64 sums
    for q, pr in enumerate(probes[:2]):
        compare_grids(G.build_vdw_array(pr, cset), allv[q], f"multi vs single plan/{atoms[q]}", floor0=0.0)
    plan.close()


def test_mixed_class_probes_through_the_one_shot_call(hip_lib, oracle):
    """ceg_grids_multi (the one-shot C entry point the Julia shim binds) with probes of several rule classes -- refused until round 3
    (CEG_ERR_UNSUPPORTED), one call now: Na (Buckingham + hard sphere) + C_co2 + O_co2 + Coulomb in CIT-7, the reference's own
    Na + CO2 setup (runtests.jl:240-258, raspa.jl:497-520); every grid against the oracle with no floor on channel 0, and
    bit-identical on 1 and 3 (oversubscribed) slabs."""
    atoms = ("Na", "C_co2", "O_co2")
    w, probes = _probe_set("CIT-7", atoms, 0.5)
    vg, cg = G.build_multi_arrays(probes, w.probe_coulomb, w.alpha, w.cset)
    lam, thr = G.vdw_scaling()
    for a, pr, g in zip(atoms, probes, vg):
        compare_grids(g, oracle.grid_vdw(pr, w.cset, lam, thr)[0], f"one-shot mixed / {a}", floor0=0.0)
    lam, thr = G.coulomb_scaling()
    compare_grids(cg, oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lam, thr)[0], "one-shot mixed / coulomb", floor0=0.0)
    assert (vg[0][0] == np.float32(2e7)).any()                       # the hard sphere of Na clamps
    os.environ["CEG_HIP_OVERSUBSCRIBE"] = "1"
    try:
        v3, c3 = G.build_multi_arrays(probes, w.probe_coulomb, w.alpha, w.cset, ngpus=3)
    finally:
        os.environ.pop("CEG_HIP_OVERSUBSCRIBE", None)
    for a, b in zip(vg + [cg], v3 + [c3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # probes that do not share a framework are refused on the host side
    other = W.fixture_workload("CHA_1.4_3b4eeb96", "Ar", 0.7)
    with pytest.raises(ValueError):
        G.build_multi_arrays([probes[0], other.probe_vdw], None, 0.0, w.cset)


def test_one_probe_of_any_rule_class_shares_the_pass_with_the_coulomb_grid(hip_lib, oracle):
    """A multi-probe call with ONE probe takes any rule class (Na: Buckingham + hard sphere): its VdW grid and the Coulomb grid
    come out of the fused single-probe kernel -- bit-identical to ceg_plan_build_fused of an ordinary plan, and the oracle's values."""
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "Na", 0.7)
    (gv,), gc = G.build_multi_arrays([w.probe_vdw], w.probe_coulomb, w.alpha, w.cset)
    lv, tv = G.vdw_scaling()
    lc, tc = G.coulomb_scaling()
    rv, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lv, tv)
    rc, _ = oracle.grid_coulomb(w.probe_coulomb, w.alpha, w.cset, lc, tc)
    compare_grids(gv, rv, "one-probe multi call / Na VdW vs oracle", floor0=0.0)
    compare_grids(gc, rc, "one-probe multi call / Coulomb vs oracle", floor0=0.0)
    import torch
    nx, ny, nz = w.cset.npoints
    plan = GridPlan(w.cset, w.probe_vdw, w.probe_coulomb, w.alpha)
    dv = torch.empty((8, nx, ny, nz), dtype=torch.float32, device="cuda")
    dc = torch.empty_like(dv)
    plan.build_fused(dv.data_ptr(), dc.data_ptr(), nx * ny * nz, 0, nx)
    torch.cuda.synchronize()
    plan.close()
    assert np.array_equal(dv.cpu().numpy().view(np.uint32), gv.view(np.uint32))
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), gc.view(np.uint32))
    # a VdW-only one-probe call as well
    (gv2,), none = G.build_multi_arrays([w.probe_vdw], None, 0.0, w.cset)
    assert none is None
    compare_grids(gv2, rv, "one-probe multi call, VdW only / Na vs oracle", floor0=0.0)


def test_setup_raspa_builds_missing_grids_in_one_pass(hip_lib, oracle, tmp_path):
    """setup_RASPA for CO2 in CIT-7 (raspa.jl:472-531): the three grids it needs -- C_co2, O_co2, Coulomb -- are created by ONE
    multi-probe call (grids.create_grids_multi) instead of three builds; the files have the reference's format (parse_grid reads
    them), hold the oracle's values, and the resulting CrystalEnergySetup gives the same energy_point as the one-by-one path.
    Na (Buckingham + hard sphere) shares ONE pass with the Coulomb grid (one-probe call)."""
    import shutil
    golden = Path(__file__).parent / "golden" / "raspa"
    try:
        setups = {}
        for multi in (True, False):
            raspa = tmp_path / f"raspa_{int(multi)}"
            raspa.mkdir()
            for sub in ("forcefield", "molecules", "structures"):
                os.symlink(golden / sub, raspa / sub)
            ceg.setdir_RASPA(raspa)
            setups[multi] = ceg.setup_RASPA("CIT-7", "BoulfelfelSholl2021", "CO2", "TraPPE", gridstep=0.4, multi=multi)
            files = sorted(p.name for p in (raspa / "grids").rglob("*.grid"))
            assert len(files) == 3 and any("C_co2" in f for f in files) and any("O_co2" in f for f in files) and any("Ewald" in f for f in files), files
        a, b = setups[True], setups[False]
        for ga, gb in zip(a.grids + [a.coulomb], b.grids + [b.coulomb]):
            assert ga.grid.shape == gb.grid.shape and ga.num_unitcell == gb.num_unitcell == (2, 3, 3)
            compare_grids(np.ascontiguousarray(ga.grid), np.ascontiguousarray(gb.grid), "setup_RASPA multi vs one-by-one", sentinel=1.9e7 * ceg.GRID_TO_KELVIN, floor0=0.0)
        # against the oracle
        w = W.fixture_workload("CIT-7", "C_co2", 0.4)
        lam, thr = G.vdw_scaling()
        ref, _ = oracle.grid_vdw(w.probe_vdw, w.cset, lam, thr)
        idx = a.atomsidx[1] if a.molecule.atomic_symbol[1].startswith("C") else a.atomsidx[0]
        got = a.grids[idx].grid
        compare_grids(np.ascontiguousarray(got), (ref.astype(np.float64) * ceg.GRID_TO_KELVIN).astype(np.float32), "setup_RASPA multi / C_co2 vs oracle",
                      sentinel=1.9e7 * ceg.GRID_TO_KELVIN)
        pos = np.array([[3.1, 4.2, 5.3], [3.1, 4.2, 6.46], [3.1, 4.2, 4.14]])
        ea, eb = ceg.energy_point(a, pos), ceg.energy_point(b, pos)
        assert ea[0] == pytest.approx(eb[0], rel=1e-6) and ea[1] == pytest.approx(eb[1], rel=1e-6)
        # a cation: not Lennard-Jones-only -> its VdW grid and the Coulomb grid still share ONE pass (fused single-probe kernel);
        # the same values as the one-by-one path
        calls = []
        real = G.create_grids_multi
        import ceg_hip.hostmirror.setup_raspa as SR
        SR.create_grids_multi = lambda *a, **k: (calls.append(a[5]), real(*a, **k))[1]
        try:
            na = ceg.setup_RASPA("CIT-7", "BoulfelfelSholl2021", "Na", gridstep=0.6, new=True)
        finally:
            SR.create_grids_multi = real
        assert len(calls) == 1 and len(calls[0]) == 1, calls
        # the multi path never leaves a truncated file at a cache path: the second of the two files fails half way ->
        # neither target is touched, no temporary stays behind, and the next call builds both
        from ceg_hip.hostmirror.raspa import getdir_RASPA
        raspa = Path(getdir_RASPA())
        before = {p: p.read_bytes() for p in (raspa / "grids").rglob("*") if p.is_file()}
        assert len(before) >= 2
        os.environ["CEG_HIP_INJECT_WRITE_FAILURE"] = "1"
        try:
            with pytest.raises(OSError):
                ceg.setup_RASPA("CIT-7", "BoulfelfelSholl2021", "Na", gridstep=0.6, new=True)
        finally:
            os.environ.pop("CEG_HIP_INJECT_WRITE_FAILURE", None)
        after = {p: p.read_bytes() for p in (raspa / "grids").rglob("*") if p.is_file()}
        assert after == before, sorted(str(x) for x in set(after) ^ set(before))
        na1 = ceg.setup_RASPA("CIT-7", "BoulfelfelSholl2021", "Na", gridstep=0.6, new=True, multi=False)
        assert na.grids[0].grid.shape[0] == 8 and np.isfinite(ceg.energy_point(na, np.array([[3.1, 4.2, 5.3]]))[0])
        compare_grids(np.ascontiguousarray(na.grids[0].grid), np.ascontiguousarray(na1.grids[0].grid), "Na VdW: shared pass vs one by one", sentinel=1.9e7 * ceg.GRID_TO_KELVIN, floor0=0.0)
        compare_grids(np.ascontiguousarray(na.coulomb.grid), np.ascontiguousarray(na1.coulomb.grid), "Na Coulomb: shared pass vs one by one", sentinel=1.9e7 * ceg.GRID_TO_KELVIN, floor0=0.0)
    finally:
        ceg.setdir_RASPA(golden)


def test_plain_c_caller(hip_lib, tmp_path):
    """examples/grid_vdw.c (gcc -std=c99, linked against libceg_hip.so) builds a VdW grid through ceg_grid_vdw: the file it writes
    holds, in channel 0, the minimum-image Lennard-Jones sum of its 32 atoms (numpy, float64) wherever the value is not clamped."""
    import shutil, subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    root = Path(__file__).resolve().parent.parent
    libdir = root / "crystalenergygrids.jl_amd" / "csrc"
    exe, out = tmp_path / "grid_vdw", tmp_path / "out.f32"
    subprocess.run([gcc, "-std=c99", "-I", str(root / "include"), str(root / "examples" / "grid_vdw.c"), "-o", str(exe),
                    "-L", str(libdir), "-lceg_hip", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    N, a = 23, 26.0
    grid = np.fromfile(out, dtype=np.float32).reshape(8, N + 1, N + 1, N + 1)
    basis = np.array([[0.05, 0.05, 0.05], [0.55, 0.55, 0.05], [0.55, 0.05, 0.55], [0.05, 0.55, 0.55]])
    pos, eps, sig = [], [], []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                for b in range(4):
                    pos.append((np.array([i, j, k]) + basis[b]) * a / 2)
                    eps.append(120.0 if b % 2 == 0 else 80.0)
                    sig.append(3.4 if b % 2 == 0 else 3.0)
    pos, eps, sig = np.array(pos), np.array(eps), np.array(sig)
    ax = np.arange(N + 1) * a / N
    P = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    d = P[:, None, :] - pos[None, :, :]
    d -= a * np.round(d / a)
    r2 = (d * d).sum(-1)
    x6 = (sig[None] ** 2 / r2) ** 3
    e = np.where(r2 < 144.0, 4.0 * eps[None] * x6 * (x6 - 1.0), 0.0).sum(1)
    lam = 1.0 / (0.01 * 120.27221933)
    want = (e * lam).reshape(N + 1, N + 1, N + 1)
    ok = np.abs(want) < 1e5
    assert ok.sum() > 4000
    assert np.allclose(grid[0][ok], want[ok], rtol=1e-6, atol=1e-6 * np.abs(want[ok]).max())


def test_image_cache_is_shared_and_changes_nothing(hip_lib, monkeypatch):
    """The lattice-image list of a plan is cached on the device and shared between plans that need the same one (the K + 1
    one-shot calls of a setup_RASPA; ceg_image_cache_stats): same framework + same per-atom flags -> a hit, another probe whose
    active kinds differ or a Coulomb plan -> its own list; results bit-identical with the cache switched off."""
    import ctypes as C

    def stats():
        h, m, e = C.c_int64(), C.c_int64(), C.c_int64()
        hip_lib.ceg_image_cache_stats(C.byref(h), C.byref(m), C.byref(e))
        return h.value, m.value, e.value

    hip_lib.ceg_release_cached_buffers()
    ws = {a: W.fixture_workload("CHA_1.4_3b4eeb96", a, 0.7) for a in ("C_co2", "O_co2", "Ar")}
    h0, m0, _ = stats()
    g1 = G.build_vdw_array(ws["C_co2"].probe_vdw, ws["C_co2"].cset)
    g2 = G.build_vdw_array(ws["O_co2"].probe_vdw, ws["O_co2"].cset)      # same active kinds (every framework atom): shared list
    g3 = G.build_vdw_array(ws["Ar"].probe_vdw, ws["Ar"].cset)            # Si / Al carry no Ar rule: another list
    g4 = G.build_vdw_array(ws["C_co2"].probe_vdw, ws["C_co2"].cset)
    gc = G.build_coulomb_array(ws["Ar"].probe_coulomb, ws["Ar"].alpha, ws["Ar"].cset)
    gc2 = G.build_coulomb_array(ws["Ar"].probe_coulomb, ws["Ar"].alpha, ws["Ar"].cset)
    h1, m1, e1 = stats()
    assert (h1 - h0, m1 - m0) == (3, 3) and e1 == 3, (h1 - h0, m1 - m0, e1)
    assert np.array_equal(g1.view(np.int32), g4.view(np.int32)) and np.array_equal(gc.view(np.int32), gc2.view(np.int32))
    monkeypatch.setenv("CEG_HIP_IMAGE_CACHE", "0")
    for a, g in (("C_co2", g1), ("O_co2", g2), ("Ar", g3)):
        assert np.array_equal(G.build_vdw_array(ws[a].probe_vdw, ws[a].cset).view(np.int32), g.view(np.int32)), a
    assert np.array_equal(G.build_coulomb_array(ws["Ar"].probe_coulomb, ws["Ar"].alpha, ws["Ar"].cset).view(np.int32), gc.view(np.int32))
    assert stats()[0] == h1                                               # switched off: no look-ups
    monkeypatch.delenv("CEG_HIP_IMAGE_CACHE")
    hip_lib.ceg_release_cached_buffers()
    assert stats()[2] == 0


def test_cached_grid_file_straight_to_the_device(hip_lib, oracle, tmp_path, forcefield):
    """ceg_interp_create_from_file: the reference's "Retrieved ... grid" path (raspa.jl:426-438 -> parse_grid, grids.jl:61-94)
    without the host array.  The handle made from the file interpolates bit-identically to parse_grid + GridInterpolator(g),
    the header it reports is parse_grid's, a Coulomb file (136-byte header) and a VdW file, with and without the `mat` argument;
    truncated / missing files are errors."""
    from ceg_hip.interp import GridInterpolator
    fw = ceg.load_framework_RASPA("CIT-7", "BoulfelfelSholl2021")
    ceg.create_grid_vdw(tmp_path / "v.grid", fw, forcefield, 0.35, "Ar")
    ceg.create_grid_coulomb(tmp_path / "c.grid", fw, forcefield, 0.35, ceg.initialize_ewald(fw))
    rng = np.random.default_rng(9)
    pts = rng.uniform(-40, 60, (5000, 3))
    for name, isc in (("v.grid", False), ("c.grid", True)):
        eg = ceg.parse_grid(tmp_path / name, isc)
        host = GridInterpolator(eg)
        ref = host(pts)
        for mat in (None, fw.mat):
            it, hdr = GridInterpolator.from_file(tmp_path / name, isc, mat=mat, with_header=True)
            got = it(pts)
            if mat is not None:            # the caller's matrices, as parse_grid(file, iscoulomb, mat): same bits in, same bits out
                assert np.array_equal(got, ref), name
            else:                          # the file's own matrix, inverted in the library: the wrap differs in the last bit
                m = ref != 1e100
                assert np.array_equal(got == 1e100, ~m) and np.allclose(got[m], ref[m], rtol=1e-9, atol=1e-9 * np.median(np.abs(ref[m])))
            assert tuple(hdr.dims) == tuple(int(x) for x in eg.csetup.dims) and tuple(hdr.num_unitcell) == eg.num_unitcell == (2, 3, 3)
            assert np.array_equal(np.array(hdr.size), eg.csetup.size) and np.array_equal(np.array(hdr.shift), eg.csetup.shift)
            assert hdr.has_mat == 1 and hdr.spacing == eg.csetup.spacing
            assert (hdr.ewald_precision == 1e-6) if isc else math.isinf(hdr.ewald_precision)
            it.close()
        host.close()
        assert (ref == 1e100).any() == (not isc)                       # the VdW blocking rule came along
        lit = oracle.interpolate_points(eg, pts[:500])
        m = lit != 1e100
        assert np.all(np.abs(ref[:500][m] - lit[m]) <= 1e-9 * np.abs(lit[m]) + 1e-10 * np.median(np.abs(lit[m])))
    data = (tmp_path / "v.grid").read_bytes()
    (tmp_path / "short.grid").write_bytes(data[: len(data) // 2])
    for bad in ("short.grid", "missing.grid"):
        with pytest.raises(_abi.CegError) as ei:
            GridInterpolator.from_file(tmp_path / bad, False)
        assert ei.value.code == -1
    # a crafted header whose point count wraps around 64 bits (dims 2^20 - 1 on every axis: nodes = 2^60, nodes * 32 = 2^65 = 0 mod 2^64,
    # so that "header + payload == file size" would hold for a header-only file): refused before anything is allocated or read
    import struct
    crafted = bytearray(data[:128])
    crafted[8:20] = struct.pack("<3i", 2 ** 20 - 1, 2 ** 20 - 1, 2 ** 20 - 1)
    (tmp_path / "crafted.grid").write_bytes(bytes(crafted))
    with pytest.raises(_abi.CegError) as ei:
        GridInterpolator.from_file(tmp_path / "crafted.grid", False)
    assert ei.value.code == -1 and "shorter" in str(ei.value)
    for wrong, isc in (("v.grid", True), ("c.grid", False)):           # a VdW file opened as a Coulomb grid and the reverse
        with pytest.raises(_abi.CegError) as ei:
            GridInterpolator.from_file(tmp_path / wrong, isc)
        assert ei.value.code == -1 and "iscoulomb" in str(ei.value)
    (tmp_path / "nomat.grid").write_bytes(data[:-72])                  # a RASPA-made file has no trailing matrix (grids.jl:80-90)
    with pytest.raises(_abi.CegError):
        GridInterpolator.from_file(tmp_path / "nomat.grid", False)
    it = GridInterpolator.from_file(tmp_path / "nomat.grid", False, mat=fw.mat)
    assert np.array_equal(it(pts[:100]), GridInterpolator(ceg.parse_grid(tmp_path / "v.grid", False, fw.mat))(pts[:100]))
    it.close()


def test_interpolation_without_derivatives(hip_lib, oracle):
    """EnergyGrid.higherorder == false: the trilinear branch of interpolate_grid (grids.jl:259-269), which addresses the
    [z, y, x, channel] array as [x, y, z, 1].  GPU (ceg_interp_set_higherorder), host mirror and oracle agree; on a cubic grid
    every point is in bounds, on a non-cubic one the out-of-bounds pattern (Julia: BoundsError; here NaN / IndexError) matches."""
    from ceg_hip.interp import GridInterpolator
    rng = np.random.default_rng(21)
    for dims in ((21, 21, 21), (25, 17, 21)):
        mat = np.diag([20.0, 20.0, 20.0]) + np.array([[0, 1.5, -0.7], [0, 0, 2.1], [0, 0, 0]])
        cset = W.grid_setup_with_dims(mat, dims)
        nx, ny, nz = cset.npoints
        grid = rng.normal(size=(8, nx, ny, nz)).astype(np.float32)
        eg = G.EnergyGrid(cset, (1, 1, 1), math.inf, False, grid)
        pts = rng.uniform(-30, 50, (3000, 3))
        ref = oracle.interpolate_points(eg, pts)
        it = GridInterpolator(eg)
        got = it(pts)
        it.close()
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.array_equal(got[ok], ref[ok])                       # same operation order, no contraction: bitwise
        assert ok.all() == (len(set(dims)) == 1) and ok.any()
        for q in range(40):
            if ok[q]:
                # (the mirror's numpy mat-vec rounds the wrapped position differently in the last bit: 1e-14 in r)
                assert G.interpolate_grid(eg, pts[q]) == pytest.approx(ref[q], rel=1e-10, abs=1e-12)
            else:
                with pytest.raises(IndexError):
                    G.interpolate_grid(eg, pts[q])
        # and the tricubic branch of the same data is something else entirely
        eg3 = G.EnergyGrid(cset, (1, 1, 1), 1e-6, True, grid)
        assert not np.allclose(oracle.interpolate_points(eg3, pts[ok][:50]), ref[ok][:50])


@pytest.mark.parametrize("name,lengths,angles", [
    ("skewed-60", (31.0, 31.0, 31.0), (60.0, 60.0, 60.0)),             # safemin2 < cutoff2: the stale-vector branch is live
    ("skewed-mixed", (30.0, 33.0, 36.0), (65.0, 110.0, 75.0)),
    ("near-ortho", (26.0, 26.0, 26.0), (91.5, 88.6, 90.9)),            # ortho flag: images dropped like the reference does
    ("orthorhombic", (25.0, 27.0, 30.0), (90.0, 90.0, 90.0)),
])
def test_multi_probe_cells_and_min_image_branches(hip_lib, oracle, name, lengths, angles, monkeypatch):
    """The multi-probe kernels in the cells that exercise the min-image selection rule (wrap-boundary images, the stale image
    vector of utils.jl:234-245, the ortho shortcut): three synthetic Lennard-Jones probes (one with a shifted rule, one with a
    kind it does not interact with, one whose rule is a LJ + CoulombEwaldDirect sum) + Coulomb, points that fall on atoms; every
    grid against the oracle, and against the same request through ceg_grids_multi on 1 and 3 (oversubscribed) slabs."""
    import torch
    import zlib
    from ceg_hip.plan import MultiGridPlan
    mat = mat_from_parameters(lengths, angles)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 7)
    n = 160
    pos = random_atoms(mat, n, rng)
    kinds = rng.integers(1, 5, n)
    kinds[kinds == 2] = 4                                       # no Buckingham kind: P (5) would not be Lennard-Jones-only
    q = rng.uniform(-1.2, 1.9, n)
    probes, pc = synthetic_probes(mat, pos, kinds, q, probes=(6, 5, 7))
    cset = W.grid_setup_with_dims(mat, (21, 17, 19))
    pos[0] = cset.shift + cset.size / cset.dims * np.array([3, 4, 5])      # an atom exactly on a grid point
    probes, pc = synthetic_probes(mat, pos, kinds, q, probes=(6, 5, 7))
    alpha = 0.26505830360350674
    nx, ny, nz = cset.npoints
    dev = torch.device("cuda", 0)
    plan = MultiGridPlan(cset, probes, pc, alpha)
    outs = [torch.full((8, nx, ny, nz), float("nan"), dtype=torch.float32, device=dev) for _ in range(4)]
    plan.build([o.data_ptr() for o in outs[:3]], outs[3].data_ptr(), nx * ny * nz, 0, nx)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    plan.close()
    lam, thr = G.vdw_scaling()
    for k, pr in enumerate(probes):
        compare_grids(got[k], oracle.grid_vdw(pr, cset, lam, thr)[0], f"multi/{name}/probe{k}")
    lam, thr = G.coulomb_scaling()
    refc = oracle.grid_coulomb(pc, alpha, cset, lam, thr)[0]
    compare_grids(got[3], refc, f"multi/{name}/coulomb")
    assert np.isnan(refc).any() or np.isinf(oracle.points_coulomb(pc, alpha, pos[:1])).any()
    for ng in (1, 3):
        if ng > hip_lib.ceg_device_count():
            monkeypatch.setenv("CEG_HIP_OVERSUBSCRIBE", "1")
        vg, cg = G.build_multi_arrays(probes, pc, alpha, cset, ngpus=ng)
        for k in range(3):
            assert np.array_equal(vg[k].view(np.int32), got[k].view(np.int32)), (name, ng, k)
        assert np.array_equal(cg.view(np.int32), got[3].view(np.int32)), (name, ng)
    vg, cg = G.build_multi_arrays(probes[:2], None, 0.0, cset)      # VdW grids only, no charges in the plan
    for k in range(2):
        compare_grids(vg[k], got[k], f"multi/{name}/vdw-only plan/probe{k}")
    assert cg is None


def test_page_locked_result_arrays(hip_lib, monkeypatch):
    """ceg_host_grid_alloc: a result array in page-locked memory of the library makes the one-shot pipelines copy every chunk D2H straight
    to its place (no ring, no host threads).  Bit-identical to the ordinary route for ceg_grid_vdw / ceg_grid_coulomb / ceg_grids_multi,
    one and three (oversubscribed) slabs, several chunks; the memory returns to the cache and is reused; foreign pointers are refused."""
    import ctypes as C
    import gc
    w = W.fixture_workload("CHA_1.4_3b4eeb96", "C_co2", 0.3)              # 109 x 102 x 95 points x 8 channels = 34 MB: several chunks
    w2 = W.fixture_workload("CHA_1.4_3b4eeb96", "O_co2", 0.3)
    for ng in (1, 3):
        if ng > hip_lib.ceg_device_count():
            monkeypatch.setenv("CEG_HIP_OVERSUBSCRIBE", "1")
        # (the reference is the ordinary route with the SAME slab split: a slab that does not start on a multiple of 4 planes shifts
        #  the tiles, which reorders the FP64 sums -- a one-ULP difference in a value or two against the one-slab build)
        ref_v = G.build_vdw_array(w.probe_vdw, w.cset, ngpus=ng)
        ref_c = G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset, ngpus=ng)
        out = G.alloc_host_grid(w.cset)
        out[:] = np.nan
        got = G.build_vdw_array(w.probe_vdw, w.cset, ngpus=ng, out=out)
        assert got is out and np.array_equal(out.view(np.int32), ref_v.view(np.int32)), ng
        out[:] = np.nan
        G.build_coulomb_array(w.probe_coulomb, w.alpha, w.cset, ngpus=ng, out=out)
        assert np.array_equal(out.view(np.int32), ref_c.view(np.int32)), ng
        addr = out.ctypes.data
        del out, got
        gc.collect()
        again = G.alloc_host_grid(w.cset)                              # the array went back to the cache: same memory again
        assert again.ctypes.data == addr
        del again
        gc.collect()
    vg, cg = G.build_multi_arrays([w.probe_vdw, w2.probe_vdw], w.probe_coulomb, w.alpha, w.cset, pinned=True)
    vr, cr = G.build_multi_arrays([w.probe_vdw, w2.probe_vdw], w.probe_coulomb, w.alpha, w.cset)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(vg + [cg], vr + [cr]))
    with pytest.raises(ValueError):
        G.build_vdw_array(w.probe_vdw, w.cset, out=np.empty((8, 3, 3, 3), dtype=np.float32))
    foreign = np.zeros(16, dtype=np.float32)
    assert hip_lib.ceg_host_grid_free(foreign.ctypes.data_as(_abi.c_float_p)) == -1 and hip_lib.ceg_host_grid_free(None) == 0
    bad = np.array([0, 3, 3], dtype=np.int32)
    assert not hip_lib.ceg_host_grid_alloc(_abi.i32ptr(bad))
    # the page-locked memory in callers' hands is bounded (CEG_HIP_PINNED_LIMIT_MB): what makes it a safe default for a garbage-collected
    # caller (julia/CEGHip.jl result_array falls back to an ordinary Array when the library refuses)
    del vg, cg
    gc.collect()
    monkeypatch.setenv("CEG_HIP_PINNED_LIMIT_MB", "48")                  # one 34 MB array fits, two do not
    first = G.alloc_host_grid(w.cset)
    with pytest.raises(_abi.CegError) as ei:
        G.alloc_host_grid(w.cset)
    assert "CEG_HIP_PINNED_LIMIT_MB" in str(ei.value)
    del first
    gc.collect()
    second = G.alloc_host_grid(w.cset)                                   # freed arrays do not count
    del second
