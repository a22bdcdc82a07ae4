"""Case generator (pure CPU) for the tests of the uniform-class grid kernels (k_culled VDWK 4 / 5) away from the CHA fixture:
other cells, cutoffs, Ewald variants, unshifted records, records and charges of extreme size.  ``named_cases()`` and
``fuzz_cases(seed)`` return ``Case`` records; ``tests/test_uniform_class_cases_host.py`` asserts on the CPU that the cases are not
vacuous, ``tests/test_gpu_uniform_class_cells.py`` runs them on the device.

Every case draws its kinds from {A, D, C} of ``tiny_forcefield(uniform=(eps, sigma, shifted))``: A and D share one Lennard-Jones
record with probe P, C has no rule with P, and B -- in the table with a Buckingham rule -- is absent.  Class 1: random charges;
class 2: one charge on every A / D atom.

Few atoms are VdW-active (A / D), most are C: a point with NO pair in range must come out as an exact 0 (a shift counted once too
often would show there), and with a cutoff of 12 A in a cell 25 A wide such points only exist when the active atoms are sparse.
Their number is ACTIVE_PER_SPHERE x cell volume / cutoff-sphere volume, so that about exp(-2.5) = 8 % of the points see none."""
from __future__ import annotations

import re
import zlib
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ceg_hip import workloads as W
from ceg_hip.hostmirror.utils import mat_from_parameters, perpendicular_lengths

from util import grid_points, random_atoms, synthetic_probes

A, B, C, D = 1, 2, 3, 4
ALPHA = 0.26505830360350674
AR_O = (107.69, 3.15)                  # the Lennard-Jones numbers of kind A in tiny_forcefield (Ar - O)
ACTIVE_PER_SPHERE = 2.5
ACTIVE_PER_SPHERE_FUZZ = 2.0           # the fuzz has grids down to 2 x 2 x 2 points: fewer points, more of them without a pair
FUZZ_SEED = 20261126                   # chosen so that every condition of test_uniform_class_cases_host.py holds
R_EXACT2 = 4.0                         # CEG_R_EXACT2 (no hard sphere in these force fields: the exact-path radius stays 2 A)

CELLS = {
    "orthorhombic": ((25.0, 27.0, 30.0), (90.0, 90.0, 90.0)),        # diagonal matrix: wrapped == nearest
    "near-ortho": ((26.0, 26.0, 26.0), (91.5, 88.6, 90.9)),          # ortho flag true, images dropped like the reference
    "triclinic": ((27.0, 29.0, 33.0), (94.07, 100.0, 85.0)),
    "skewed-60": ((31.0, 31.0, 31.0), (60.0, 60.0, 60.0)),           # safemin2 < cutoff2: stale-vector branch is live
    "skewed-mixed": ((30.0, 33.0, 36.0), (65.0, 110.0, 75.0)),
    "barely-2cutoff": ((24.9, 25.3, 25.8), (84.0, 97.0, 93.0)),      # a tile CAN keep images other than the wrapped one
}


@dataclass
class Case:
    name: str
    mat: np.ndarray
    pos: np.ndarray
    kinds: np.ndarray
    q: np.ndarray
    cutoff: float
    alpha: float
    dims: tuple
    uniform: tuple                     # (eps, sigma, shifted)
    cls: int                           # expected uniform class of the plan as it comes
    env: dict                          # environment at plan creation
    ortho: bool
    stale: bool
    plain: bool
    pts: np.ndarray                    # points inside the grid box (culled POINTS launches): grid points, scattered, near atoms
    pts_out: np.ndarray                # points up to +-3 cells outside the box (the library takes the literal kernel for them)
    cut_pairs: list                    # (i, j): pts[i] is 1e-10 inside the cutoff of an A / D atom, pts[j] 1e-10 outside, same ray
    ewk: int = 2                       # Ewald arithmetic the plan must come out with: 2 r^2 tables, 1 erfcx table, 0 libm-grade
    multi: bool = False                # also run as MultiGridPlan([P, Q])
    dense: bool = False                # two atoms in three are VdW-active: every point has pairs in range, no exact-zero rows
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def shifted(self) -> bool:
        return bool(self.uniform[2])

    def cset(self):
        return W.grid_setup_with_dims(self.mat, self.dims)

    def probes(self, probes=None):
        return synthetic_probes(self.mat, self.pos, self.kinds, self.q, cutoff=self.cutoff, probes=probes, uniform=self.uniform)

    def active(self) -> np.ndarray:
        return (self.kinds == A) | (self.kinds == D)

    def ref(self, oracle, what: str):
        """The oracle's FP64 sums / stored grids of this case, computed once: 'points_vdw', 'points_coulomb', 'out_vdw',
        'out_coulomb', 'grid_vdw', 'grid_coulomb'."""
        if what not in self._cache:
            from ceg_hip import grids as G
            pv, pc = self.probes()
            if what == "points_vdw":
                r = oracle.points_vdw(pv, self.pts)
            elif what == "points_coulomb":
                r = oracle.points_coulomb(pc, self.alpha, self.pts)
            elif what == "out_vdw":
                r = oracle.points_vdw(pv, self.pts_out)
            elif what == "out_coulomb":
                r = oracle.points_coulomb(pc, self.alpha, self.pts_out)
            elif what == "grid_vdw":
                lam, thr = G.vdw_scaling()
                r = oracle.grid_vdw(pv, self.cset(), lam, thr)[0]
            elif what == "grid_coulomb":
                lam, thr = G.coulomb_scaling()
                r = oracle.grid_coulomb(pc, self.alpha, self.cset(), lam, thr)[0]
            else:
                raise KeyError(what)
            r.setflags(write=False)
            self._cache[what] = r
        return self._cache[what]


# ------------------------------------------------------------------ r^2-table size (key arithmetic of build_ew2_table_uncached)
def _ew2_constants():
    text = (Path(__file__).resolve().parent.parent / "crystalenergygrids.jl_amd" / "csrc" / "ceg_internal.h").read_text()
    logm = re.search(r"constexpr\s+int\s+CEG_EW2_LOGM\s*=\s*(\d+)\s*;", text)
    ni_max = re.search(r"constexpr\s+int\s+CEG_EW2_NI_MAX\s*=\s*(\d+)\s*;", text)
    assert logm and ni_max, "CEG_EW2_LOGM / CEG_EW2_NI_MAX are no longer plain integer constants of csrc/ceg_internal.h: update this reader"
    return 20 - int(logm.group(1)), int(ni_max.group(1))


def ew2_intervals(cutoff: float, r_exact2: float = R_EXACT2) -> int:
    """Intervals the r^2-indexed Ewald tables need from r_exact2 to the cutoff: key(s) = high word of s >> CEG_EW2_SHIFT."""
    shift, _ = _ew2_constants()
    key = lambda s: int(np.array([s], dtype=np.float64).view(np.uint64)[0] >> np.uint64(32)) >> shift
    c2 = cutoff * cutoff
    return key(c2 * (1.0 + 4e-9) + 4e-9) - key(r_exact2) + 1


def ew2_ni_max() -> int:
    return _ew2_constants()[1]


# ------------------------------------------------------------------ building blocks
def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def _pick_kinds(n, mat, cutoff, rng, first_active=True, per_sphere=ACTIVE_PER_SPHERE):
    """Sparse A / D atoms among C atoms (see the module docstring); both A and D occur, at least 3 active and 2 C atoms."""
    vol = abs(np.linalg.det(mat))
    sphere = 4.0 / 3.0 * np.pi * cutoff ** 3
    nact = int(round(per_sphere * vol / sphere))
    nact = max(3, min(nact, n - 2, int(0.7 * n)))
    idx = rng.permutation(n)[:nact]
    if first_active and 0 not in idx:
        idx[0] = 0
    kinds = np.full(n, C, dtype=np.int64)
    kinds[idx] = np.where(rng.random(nact) < 0.5, A, D)
    kinds[idx[0]], kinds[idx[1]] = A, D
    return kinds


def _anchors(pos, kinds, lo, hi):
    """The three A / D atoms and the two C atoms nearest to the centre of the grid's box, among the atoms inside it."""
    inside = np.all(pos > lo, axis=1) & np.all(pos < hi, axis=1)
    order = [a for a in np.argsort(np.linalg.norm(pos - 0.5 * (lo + hi), axis=1)) if inside[a]]
    act = [a for a in order if kinds[a] in (A, D)][:3]
    non = [a for a in order if kinds[a] == C][:2]
    assert len(act) == 3 and len(non) == 2, "too few atoms inside the grid box"
    return act, non


def _points(mat, pos, kinds, cutoff, dims, stale, safemin2, rng, anchors):
    """(pts, pts_out, cut_pairs): see Case."""
    cset = W.grid_setup_with_dims(mat, dims)
    lo, hi = np.asarray(cset.shift, dtype=np.float64), np.asarray(cset.shift) + np.asarray(cset.size)
    pts = [grid_points(cset), lo + rng.uniform(0, 1, (256, 3)) * (hi - lo)]
    # outside: every coordinate up to 3 box sizes beyond the box, at least one of them beyond it
    out = lo + rng.uniform(-3, 4, (256, 3)) * (hi - lo)
    for p in out:
        if np.all(p >= lo) and np.all(p <= hi):
            ax = int(rng.integers(0, 3))
            p[ax] = hi[ax] + rng.uniform(0.1, 3.0) * (hi - lo)[ax]
    radii = [0.0, 0.3, 1.5, 2.0 - 1e-9, 2.0 + 1e-9, cutoff - 1e-10, cutoff, cutoff + 1e-10]
    if stale:
        radii += [np.sqrt(safemin2) * (1.0 - 1e-10), np.sqrt(safemin2) * (1.0 + 1e-10)]
    rmax = max(radii)
    act, non = anchors
    near, cut_pairs = [], []
    base = sum(len(p) for p in pts)
    for a in act + non:
        for _ in range(3):
            for _try in range(10000):
                u = _unit(rng)
                far = pos[a] + rmax * u
                if np.all(far > lo) and np.all(far < hi):          # the box is convex: every shorter radius is inside too
                    break
            else:
                raise AssertionError("no direction keeps the cutoff shell of an anchor atom inside the grid box")
            if a in act:
                cut_pairs.append((base + len(near) + 5, base + len(near) + 7))
            near += [pos[a] + r * u for r in radii]
    pts.append(np.array(near))
    return np.concatenate(pts), out, cut_pairs


def _charges(kinds, cls, rng, q_uniform, lo=-1.2, hi=1.9):
    q = rng.uniform(lo, hi, len(kinds))
    if cls == 2:
        q[(kinds == A) | (kinds == D)] = q_uniform
    return q


def _flags(mat, cutoff):
    from ceg_hip.hostmirror.utils import prepare_periodic_distance_computations
    ortho, safemin = prepare_periodic_distance_computations(mat)
    safemin2 = safemin * safemin
    stale = (not ortho) and safemin2 < cutoff * cutoff
    return bool(ortho), bool(stale), bool(not ortho and not stale), safemin2


def _named(name, cell, dims, cls, *, cutoff=12.0, alpha=ALPHA, uniform=(*AR_O, True), q_uniform=-0.7, env=None, ewk=2, n=120,
           min_sep=1.6, scale_to=None, mat=None, seed_tag=None, multi=False, on_grid_active=True,
           dense=False):
    if mat is None:
        mat = mat_from_parameters(*CELLS[cell])
    if scale_to is not None:                           # every perpendicular width >= scale_to
        mat = mat * max(1.0, scale_to / perpendicular_lengths(mat).min() * (1.0 + 1e-12))
    assert perpendicular_lengths(mat).min() >= 2.0 * cutoff, (name, perpendicular_lengths(mat))
    # positions, kinds and points depend on the geometry alone (cell, cutoff, dims): the two classes of a case share them
    key = (seed_tag or f"{cell}/{cutoff}", tuple(dims), n, multi, on_grid_active, dense)
    if key not in _GEOMETRY:
        rng = np.random.default_rng(zlib.crc32(key[0].encode()))
        pos = random_atoms(mat, n, rng, min_sep=min_sep)
        cset = W.grid_setup_with_dims(mat, dims)
        lo, hi = np.asarray(cset.shift, dtype=np.float64), np.asarray(cset.shift) + np.asarray(cset.size)
        on = np.minimum(np.array([3, 4, 5]), np.asarray(dims))
        pos[0] = lo + (hi - lo) / np.asarray(dims) * on    # an atom exactly on a grid point (kind A / D: see _pick_kinds)
        kinds = _pick_kinds(n, mat, cutoff, rng, first_active=on_grid_active)
        if dense:
            kinds = rng.choice(np.array([A, D, C]), n)
            kinds[:3] = (A if on_grid_active else C), D, C
        if not on_grid_active and kinds[0] != C:           # the atom on the grid point is a Coulomb-only one
            other = int(np.flatnonzero(kinds == C)[0])
            kinds[0], kinds[other] = kinds[other], kinds[0]
        if multi:
            kinds[kinds == D] = A                          # Q's rule with D is a Lennard-Jones + CoulombEwaldDirect sum
        flags = _flags(mat, cutoff)
        _GEOMETRY[key] = (pos, kinds, flags, _points(mat, pos, kinds, cutoff, dims, flags[1], flags[3], rng, _anchors(pos, kinds, lo, hi)))
    pos, kinds, (ortho, stale, plain, safemin2), (pts, out, cut_pairs) = _GEOMETRY[key]
    q = _charges(kinds, cls, np.random.default_rng(zlib.crc32(name.encode())), q_uniform)
    return Case(name, mat, pos, kinds, q, cutoff, alpha, tuple(dims), tuple(uniform), cls, dict(env or {}), ortho, stale, plain,
                pts, out, cut_pairs, ewk, multi, dense)


_NAMED = None
_GEOMETRY = {}
_FUZZ = {}


def named_cases():
    global _NAMED
    if _NAMED is not None:
        return _NAMED
    cases = []

    def both(tag, cell, dims, **kw):
        for cls in (1, 2):
            cases.append(_named(f"{tag}/class{cls}", cell, dims, cls, **kw))

    # the five cells of test_cells_and_min_image_branches; the barely-2-cutoff cell of the delta test
    for cell in ("orthorhombic", "near-ortho", "triclinic", "skewed-60", "skewed-mixed"):
        both(cell, cell, (9, 7, 11))
    # The atom on the grid point is a Coulomb-only one (C) here.  With a VdW-active one, grid point (3, 3, 6) lies in its x-plane at
    # r = 2.036 A, just outside the exact path: its d3 term (x y z G3(r), x = 0) is an exact 0 from the image list, while the oracle's
    # wrap arithmetic leaves a residue of 1.7e-15 A in x and with it -1.84e-9 of a raw d3 sum of -7.504e-4 (sum of |pair terms|
    # 8.2e-4) -- a residue of the oracle's arithmetic at a term that is exactly 0, not summation-order noise: 2.5e-6 of
    # the stored value, against compare_grids' 1e-6 -- with sparse active atoms the channel's median, the scale of its floor, is 4e-3
    # (measured on the device: got -0.00191381318, oracle -0.00191381795; 8 such points, channel 7 only; the FP64 sums at the same
    # points pass compare_raw).  The switched-off plan (per-candidate kernels) is off the oracle at exactly the same points, in
    # build_fused and build_vdw alike: the difference lies between image list and oracle, not in the uniform variants.
    # The coarser grids of the other cases have no grid point that close in a plane of the atom; in this cell the 2e7 / NaN patterns
    # of a stored VdW grid at a point ON a VdW-active atom are therefore not checked (they are in every other cell).
    both("barely-2cutoff", "barely-2cutoff", (19, 17, 21), n=150, on_grid_active=False)
    # an unshifted record: a pair kept or dropped wrongly at the cutoff moves channel 0 by V(cutoff) = 0.14 K
    both("skewed-60/unshifted", "skewed-60", (9, 7, 11), uniform=(*AR_O, False))
    # other cutoffs: other ew2_base / ew2_ni, other hi_lo / hi_span
    both("skewed-mixed/cutoff9", "skewed-mixed", (9, 7, 11), cutoff=9.0)
    both("triclinic/cutoff10.5", "triclinic", (9, 7, 11), cutoff=10.5)
    # qualifying plans without the r^2 tables: FUSED runs <1, 1> / <1, 0>, VDW still <4, 1>
    both("triclinic/no-ew2", "triclinic", (9, 7, 11), env={"CEG_HIP_NO_EW2": "1"}, ewk=1)
    both("triclinic/alpha0.5", "triclinic", (9, 7, 11), alpha=0.5, ewk=0)
    both("triclinic/cutoff14", "triclinic", (9, 7, 11), cutoff=BIG_CUTOFF, scale_to=2.0 * BIG_CUTOFF, ewk=1)
    # the 21 A case of test_large_cutoff_many_bin_rows: several row passes (441 A^2 would need 216 intervals: no r^2 tables either)
    edge = 47.0
    both("cutoff21", None, (7, 9, 5), cutoff=21.0, alpha=4.5 / 21.0, n=900, min_sep=2.0, seed_tag="cutoff21", ewk=1,
         mat=mat_from_parameters((edge, edge + 3.0, edge + 5.0), (93.0, 97.0, 86.0)))
    # records away from the Ar - O numbers (units 1/U on the exact path, U at the end of a tile) and class-2 charges of other sizes
    # and signs.  check_vdw_grid admits a negative epsilon (an inverted well: -Inf at r = 0), and so does the detector (|4 eps|)
    extremes = [((0.02, 2.2, True), 2.5), ((900.0, 2.2, True), -0.05), ((5.0, 5.5, True), 1e-5), ((-60.0, 3.0, True), -0.7)]
    for cell in ("orthorhombic", "skewed-60"):
        for uni, qu in extremes:
            both(f"{cell}/eps{uni[0]:g}-sigma{uni[1]:g}", cell, (9, 7, 11), uniform=uni, q_uniform=qu)
    # probe Q beside P in one multi-probe plan
    both("skewed-mixed/multi", "skewed-mixed", (9, 7, 11), multi=True)
    # Beyond the sparse cases: two atoms in three VdW-active, so that a point sums some 50 Lennard-Jones pairs through the variants
    # (wrap-boundary candidates and the stale range among them).  A periodic cell 25 to 36 A wide has no point farther than the cutoff
    # from every one of 80 atoms: these cases have no exact-zero rows, the sparse ones above keep that check.
    for cell in ("near-ortho", "skewed-60", "skewed-mixed"):
        both(f"{cell}/dense", cell, (9, 7, 11), dense=True)
    both("barely-2cutoff/dense", "barely-2cutoff", (19, 17, 21), n=150, on_grid_active=False, dense=True)
    _NAMED = cases
    return cases


# A cutoff whose r^2 tables would need more than CEG_EW2_NI_MAX intervals: 32 intervals per octave of r^2 from 4 A^2 give 160 up to
# 128 A^2, and 196 A^2 = 1.53125 x 128 lies in the 18th interval of the next octave: 178 > 176.  (13.5 A: 182.25 = 1.4238 x 128,
# 14th interval, 174 -- that cutoff still gets the tables.)
BIG_CUTOFF = 14.0


def fuzz_cases(seed: int = FUZZ_SEED):
    """24 configurations in the manner of test_random_cells_fuzz (same cell sampler), uniform palette.  Configuration i: class
    1 + i % 2; record unshifted when i % 3 == 2; near-ortho cell when i % 4 == (i // 4) % 2 -- one in every block of four, on both
    classes (with i % 4 == 0 every near-ortho cell would be class 1); atoms given unwrapped when i is odd."""
    if seed in _FUZZ:
        return _FUZZ[seed]
    rng = np.random.default_rng(seed)
    cases = _FUZZ.setdefault(seed, [])
    i = 0
    while i < 24:
        lengths = rng.uniform(24.5, 40.0, 3)
        near_ortho = i % 4 == (i // 4) % 2
        angles = rng.uniform(88.6, 91.4, 3) if near_ortho else rng.uniform(58.0, 122.0, 3)
        try:
            mat = mat_from_parameters(tuple(lengths), tuple(angles))
        except Exception:
            continue
        if not np.all(np.isfinite(mat)) or np.linalg.det(mat) <= 0 or perpendicular_lengths(mat).min() < 24.0:
            continue
        cutoff = float(rng.choice([9.0, 10.5, 12.0]))
        n = int(rng.integers(40, 201))
        pos = random_atoms(mat, n, rng, min_sep=1.2)
        cls = 1 + i % 2
        eps = float(np.exp(rng.uniform(np.log(5.0), np.log(500.0))))
        sigma = float(rng.uniform(2.2, 4.2))
        uniform = (eps, sigma, i % 3 != 2)
        kinds = _pick_kinds(n, mat, cutoff, rng, first_active=False, per_sphere=ACTIVE_PER_SPHERE_FUZZ)
        dims = tuple(int(x) for x in 2 * rng.integers(0, 7, 3) + 1)             # 1 ... 13: down to 2 points per axis
        cset = W.grid_setup_with_dims(mat, dims)
        lo, hi = np.asarray(cset.shift, dtype=np.float64), np.asarray(cset.shift) + np.asarray(cset.size)
        anchors = _anchors(pos, kinds, lo, hi)
        if i % 2:                     # atoms given outside the unit cell, as a CIF may list them -- all but the five anchor atoms,
            move = rng.integers(-2, 3, (3, n))         # whose shells of points must lie inside the grid box
            move[:, anchors[0] + anchors[1]] = 0
            pos = pos + (mat @ move).T
        ortho, stale, plain, safemin2 = _flags(mat, cutoff)
        pts, out, cut_pairs = _points(mat, pos, kinds, cutoff, dims, stale, safemin2, rng, anchors)
        qu = float(rng.uniform(0.2, 1.5) * rng.choice([-1.0, 1.0]))
        q = _charges(kinds, cls, rng, qu, -1.5, 1.5)
        alpha = float(rng.uniform(0.2, 0.3))
        name = f"fuzz{i:02d}-seed{seed}"
        cases.append(Case(name, mat, pos, kinds, q, cutoff, alpha, dims, uniform, cls, {}, ortho, stale, plain, pts, out, cut_pairs))
        i += 1
    return cases
