"""Synthetic grids, points, a high-precision reference and a derived error bound for the two device implementations of
``interpolate_grid`` (csrc/ceg_consumers.h: ``interp_point``, all 64 terms on one thread -- k_interpolate, k_egrid_terms -- and
``interp_corner``, one corner per lane and three shuffles -- mc_trial_row, k_mcw_frame, the baseline kernel), and the cases of the
block-mask kernels (csrc/ceg_block.hip).  No tests here: ``tests/test_interp_cases_host.py`` checks this file on the CPU (the
reference against exact rational arithmetic, mpmath, the oracle and the host mirror; the cases against what they claim),
``tests/test_gpu_interp_synthetic.py`` runs the cases on the device.

Grids.  Cells ``diag(9, 11, 13)`` and ``mat_from_parameters((9, 11, 13), (65, 110, 75))``; dims (1,1,1), (1,3,5), (5,3,1), (7,5,3),
(3,3,3), (15,13,11) (``grid_setup_with_dims``: dims = nodes - 1 per axis, odd).  Data float32[8, nx, ny, nz]:
  poly      a tricubic polynomial in index coordinates with integer coefficients in -2..2, the seven derivative channels its
            analytic derivatives.  Every datum must be an integer below 2^24 to be exact in Float32: monomials are taken in the
            order of their largest value on the grid for as long as that holds in all eight channels (all 64 up to (7,5,3); at
            (15,13,11), where x^3 y^3 z^3 reaches 1e10, the low-order ones).  The interpolant is then the polynomial itself.
            Declared Coulomb; where every axis has four nodes or more also declared VdW, with an integer constant added that puts
            the median node value at 5e6 (poly-vdw: a blocking pattern with structure, values next to the threshold).
  one-hot   dims (1,1,1): a single 1.0 at one (node, channel), 64 grids -- every one of the 64 weights alone.
  random    normal data, per-channel scales (1e3, 3e2, 3e2, 3e2, 1e2, 1e2, 1e2, 30), mixed signs.
  blocking  a random grid with ONE value-channel entry replaced by 5e6f (not blocked: the rule is a strict >), the next float
            above it (blocked), +inf (blocked) or NaN (not blocked: NaN > 5e6 is false), the entry sitting in turn at every corner
            of an interior cell and of a cell of the last layer (p0 == extent, p1 = p0 on that axis: reached by the tiny-negative
            points only).  The same arrays are declared VdW and Coulomb (ewald_precision 1e-6: no rule, the finite values added up).
  huge      a Coulomb grid constant at the largest Float32 in channel 0, zero derivatives, used at node points only.
A Coulomb value of exactly 1e100, which montecarlo.jl:500 adds without the charge, cannot come from the data of a Coulomb-DECLARED
grid: Float32(1e100) is Inf, and 27 x 3.4e38 bounds every finite interpolant (asserted in the host module).  It comes from the
blocking rule: a grid in the Coulomb slot of a setup that is declared VdW (ewald_precision = Inf) returns 1e100 in a blocked
cell, and the three copies of the rule (mc_trial_row, k_mcw_frame, the baseline kernel) must add it as it is, not times the charge.
``mc_setup(..., coulomb_vdw=True)`` builds that setup; its placements put atoms of charge 0.0 and of charge -0.35 (0.7 for the
one-atom species) into the blocked cell.
Non-finite data in a cell that is not blocked are out of scope where they are infinite (``reference`` marks such points): the
Hermite form and COEFF * X differ in Inf / NaN class there.  A NaN datum gives NaN in every form, and that is compared.

Points of a grid (``points``): 200 uniform in +-40 A; every node; 50 on faces (r = 0 on one axis); lattice translations mat @ k;
+-0.0; the tiny-negative set -- (-1e-20, y, z) and its permutations, (-1e-20,)*3, (-1e-300,)*3: abc - floor(abc) rounds to exactly
1.0, and the point lands on p0 == extent -- ; 20 uniform in +-1e5 A; for three nodes the doubles next below and above the node
coordinate on each axis.

Reference.  ``sh`` = offsetpoint (hostmirror.coordinates, float64, the reference's operation order: ``shifted`` below is its
vectorised form, held to it bit for bit by the host module), p0 = clip(floor(sh), 1, ext), p1 = p0 + (p0 != ext), r = sh - floor(sh);
value = the tensor-product Hermite sum over the 64 (corner, channel) data in np.longdouble, from the Float32 data and the float64 r;
T = the same sum with every datum replaced by its absolute value and every Hermite polynomial by the sum of the absolute values of
its monomials (2t^3 + 3t^2 + 1 for 2t^3 - 3t^2 + 1, ...).  blocked = VdW and any of the 8 corner values > 5e6.

Bound = K 2^-53 T with K = 128.  Roundings on the longest path of the device code, each at most 2^-53 of a quantity that T bounds:
  a Hermite weight from t: t^2, t^3, 3 t^2 (2 t^3 is exact), two additions                         5, times three weights   15
  the products (x y) (z0 v0 + z1 v1): x y, z0 v0, the inner sum, the outer product (the Float32 datum widens exactly)         4
  63 additions of the 64 terms (one thread: in sequence; one corner per lane: 7 in the lane, 3 shuffles: fewer)               63
  Monte-Carlo columns only: the sum over at most 16 atoms (15 additions, against the summed T) and the charge product         16
                                                                                                                      total   98
plus second-order terms of (1 + 2^-53)^98; contraction into fused multiply-adds only removes roundings.  98 < K = 128.  The
no-derivatives branch (8 terms, 3 products each, 7 additions, a 1 - r per axis) needs 14.  For scale: the float64 oracle
(COEFF * X and 64 monomials) stays within K = 6.3 on these cases (printed by the host module)."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import numpy as np

from ceg_hip import grids as G, workloads as W
from ceg_hip.hostmirror.utils import mat_from_parameters

LD = np.longdouble
K = 128
U = LD(2.0) ** -53
F32 = np.float32
THRESHOLD = F32(5e6)
ABOVE = np.nextafter(THRESHOLD, F32(np.inf))
SCALES = np.array([1e3, 3e2, 3e2, 3e2, 1e2, 1e2, 1e2, 30.0])
# channel -> derivative order along (x, y, z): value, dx, dy, dz, dxy, dxz, dyz, dxyz
CHANNELS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
CELLS = {"ortho": np.diag([9.0, 11.0, 13.0]), "tric": mat_from_parameters((9.0, 11.0, 13.0), (65.0, 110.0, 75.0))}
DIMS = ((1, 1, 1), (1, 3, 5), (5, 3, 1), (7, 5, 3), (3, 3, 3), (15, 13, 11))
VDW, COULOMB = math.inf, 1e-6

_csets = {}


def cset(cell: str, dims):
    key = (cell, tuple(int(d) for d in dims))
    if key not in _csets:
        _csets[key] = W.grid_setup_with_dims(CELLS[cell], key[1])
    return _csets[key]


def energy_grid(cs, data, precision=VDW, higherorder=True) -> G.EnergyGrid:
    data = np.ascontiguousarray(data, dtype=F32)
    assert data.shape == (8,) + tuple(cs.npoints)
    return G.EnergyGrid(cs, (1, 1, 1), precision, higherorder, data)


# ---------------------------------------------------------------------------------------------- data families
def random_data(cs, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(8,) + tuple(cs.npoints)) * SCALES[:, None, None, None]).astype(F32)


def poly_coefficients(dims, seed) -> np.ndarray:
    """int64[4, 4, 4] coefficients c[i, j, k] of x^i y^j z^k in -2..2; monomials enter in the order of their largest value on the grid
    while the bound sum |c| max|d monomial| stays below 2^24 in every channel (then every datum is an integer exact in Float32)"""
    rng = np.random.default_rng(seed)
    n = [int(d) for d in dims]                                   # the largest index coordinate per axis
    draw = rng.integers(-2, 3, (4, 4, 4))
    order = sorted(itertools.product(range(4), repeat=3), key=lambda e: (n[0] ** e[0] * n[1] ** e[1] * n[2] ** e[2], e))
    coeff = np.zeros((4, 4, 4), dtype=np.int64)
    total = [0] * 8
    for e in order:
        c = int(draw[e])
        add = []
        for o in CHANNELS:
            f = 1
            for a in range(3):
                f *= _dfactor(e[a], o[a]) * n[a] ** max(e[a] - o[a], 0)
            add.append(abs(c) * f)
        if all(t + a < 2 ** 24 for t, a in zip(total, add)):
            coeff[e] = c
            total = [t + a for t, a in zip(total, add)]
    return coeff


def _dfactor(e, o):
    """d^o/dx^o x^e = _dfactor x^(e - o), o in (0, 1)"""
    return 1 if o == 0 else e


def poly_data(cs, coeff) -> np.ndarray:
    nx, ny, nz = cs.npoints
    x = [np.arange(n, dtype=np.int64) for n in (nx, ny, nz)]
    out = np.zeros((8, nx, ny, nz), dtype=np.int64)
    for ch, o in enumerate(CHANNELS):
        for e in itertools.product(range(4), repeat=3):
            if coeff[e] == 0 or any(o[a] > e[a] for a in range(3)):
                continue
            f = [_dfactor(e[a], o[a]) * x[a] ** (e[a] - o[a]) for a in range(3)]
            out[ch] += coeff[e] * f[0][:, None, None] * f[1][None, :, None] * f[2][None, None, :]
    assert np.abs(out).max() < 2 ** 24
    data = out.astype(F32)
    assert np.array_equal(data.astype(np.int64), out)
    return data


def poly_exact(coeff, sh) -> Fraction:
    """the polynomial at index coordinates sh - 1 (sh: three float64), exactly"""
    x = [Fraction(float(s)) - 1 for s in sh]
    return sum(int(coeff[e]) * x[0] ** e[0] * x[1] ** e[1] * x[2] ** e[2] for e in itertools.product(range(4), repeat=3) if coeff[e])


def one_hot_grids(cell: str):
    """[(node (i, j, k), channel, EnergyGrid)] on dims (1, 1, 1): Coulomb-declared, so that no rule interferes"""
    cs = cset(cell, (1, 1, 1))
    out = []
    for node in itertools.product(range(2), repeat=3):
        for ch in range(8):
            d = np.zeros((8, 2, 2, 2), dtype=F32)
            d[(ch,) + node] = 1.0
            out.append((node, ch, energy_grid(cs, d, COULOMB)))
    return out


SPECIAL = {"5e6f": THRESHOLD, "above": ABOVE, "inf": F32(np.inf), "nan": F32(np.nan)}
BLOCKS = {"5e6f": False, "above": True, "inf": True, "nan": False}


def corner_nodes(cs, p0):
    """the distinct 0-based nodes of the cell with 1-based lower corner p0 (four or fewer where p0 == extent on an axis)"""
    ext = np.asarray(cs.npoints)
    p0 = np.asarray(p0)
    p1 = p0 + (p0 != ext)
    return sorted({tuple(int((p1 if s[a] else p0)[a]) - 1 for a in range(3)) for s in itertools.product(range(2), repeat=3)})


def interior_cell(cs, seed=0):
    """(p0, points[16, 3]): a cell away from the last layer that 16 points drawn inside it really land in (in a triclinic cell the
    nodes of the bounding box lie partly outside the unit cell and are wrapped elsewhere)"""
    rng = np.random.default_rng(seed)
    dims = np.asarray(cs.dims)
    cells = [c for c in itertools.product(*(range(1, int(d) + 1) for d in dims))]
    for q in rng.permutation(len(cells)):
        p0 = np.array(cells[q])
        pts = ((p0 - 1) + rng.uniform(0.05, 0.95, (16, 3))) * cs.size / cs.dims + cs.shift
        if np.array_equal(stencil(cs, pts)[0], np.tile(p0, (16, 1))):
            return p0, pts
    raise AssertionError("no cell holds its own points")


def last_layer_cell(cs, pts):
    """(p0, index into pts): the cell of the first point with p0 == extent on some axis"""
    p0 = stencil(cs, pts)[0]
    hit = np.nonzero((p0 == np.asarray(cs.npoints)).any(axis=1))[0]
    assert len(hit), "no point on the last layer"
    return p0[hit[0]], int(hit[0])


def blocking_grids(cs, base, p0):
    """[(name, node, data)]: `base` with channel 0 at one corner node of cell p0 replaced by each special value"""
    out = []
    for node in corner_nodes(cs, p0):
        for name, v in SPECIAL.items():
            d = base.copy()
            d[(0,) + node] = v
            out.append((name, node, d))
    return out


def huge_coulomb(cs) -> G.EnergyGrid:
    d = np.zeros((8,) + tuple(cs.npoints), dtype=F32)
    d[0] = np.finfo(F32).max
    return energy_grid(cs, d, COULOMB)


# ---------------------------------------------------------------------------------------------- points
def node_points(cs) -> np.ndarray:
    nx, ny, nz = cs.npoints
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    idx = np.stack([ii, jj, kk], axis=-1).reshape(-1, 3)
    return idx * cs.size / cs.dims + cs.shift


def tiny_negative(seed=0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    out = []
    for a in range(3):
        for _ in range(3):
            p = rng.uniform(-40.0, 40.0, 3)
            p[a] = -1e-20
            out.append(p)
    for a in range(3):                                           # two axes tiny, one free
        p = np.full(3, -1e-20)
        p[a] = rng.uniform(-40.0, 40.0)
        out.append(p)
    out += [np.full(3, -1e-20), np.full(3, -1e-300)]
    return np.array(out)


def points(cs, seed=0) -> dict:
    """name -> float64[n, 3]; ``all_points`` concatenates them in this order"""
    rng = np.random.default_rng(seed)
    mat = cs.cell.mat
    nodes = node_points(cs)
    out = {"uniform": rng.uniform(-40.0, 40.0, (200, 3)), "nodes": nodes}
    faces = rng.uniform(-40.0, 40.0, (50, 3))
    for q in range(50):
        a = q % 3
        faces[q, a] = int(rng.integers(0, cs.npoints[a])) * cs.size[a] / cs.dims[a] + cs.shift[a]
    out["faces"] = faces
    ks = [k for k in itertools.product((-1, 0, 1), repeat=3)] + [(1000, -777, 3), (-2, 5, -40), (7, 0, 0)]
    out["lattice"] = np.array([(mat[:, 0] * k[0] + mat[:, 1] * k[1]) + mat[:, 2] * k[2] for k in ks])
    out["zeros"] = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0]])
    out["tiny"] = tiny_negative(seed)
    out["far"] = rng.uniform(-1e5, 1e5, (20, 3))
    beside = []
    for n in nodes[rng.choice(len(nodes), 3, replace=False)]:
        for a in range(3):
            for to in (-np.inf, np.inf):
                p = n.copy()
                p[a] = np.nextafter(p[a], to)
                beside.append(p)
    out["beside"] = np.array(beside)
    return out


def all_points(cs, seed=0) -> np.ndarray:
    return np.concatenate(list(points(cs, seed).values()))


# ---------------------------------------------------------------------------------------------- reference and bound
def shifted(cs, pts) -> np.ndarray:
    """hostmirror.coordinates.offsetpoint for every row of pts: the same float64 operations in the same order (wrap_atom sums the
    separately rounded products left to right); offsetpoint wraps by itself"""
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    I, M = cs.cell.invmat, cs.cell.mat
    abc = (I[:, 0] * p[:, 0, None] + I[:, 1] * p[:, 1, None]) + I[:, 2] * p[:, 2, None]
    abc = abc - np.floor(abc)
    new = (M[:, 0] * abc[:, 0, None] + M[:, 1] * abc[:, 1, None]) + M[:, 2] * abc[:, 2, None]
    return (new - cs.shift) * cs.dims / cs.size + 1


def stencil(cs, pts):
    """(p0 int64[n, 3], p1, r float64[n, 3]), 1-based"""
    sh = shifted(cs, pts)
    f = np.floor(sh)
    ext = np.asarray(cs.npoints, dtype=np.int64)
    p0 = np.clip(f.astype(np.int64), 1, ext)
    p1 = p0 + (p0 != ext)
    return p0, p1, sh - f


def _hermite(t):
    """[order][end] for t float64[n]: the basis in longdouble and the sums of the absolute values of its monomials (t >= 0)"""
    t = t.astype(LD)
    t2 = t * t
    t3 = t2 * t
    return ([[2 * t3 - 3 * t2 + 1, -2 * t3 + 3 * t2], [t3 - 2 * t2 + t, t3 - t2]],
            [[2 * t3 + 3 * t2 + 1, 2 * t3 + 3 * t2], [t3 + 2 * t2 + t, t3 + t2]])


def reference(eg, pts):
    """-> (value longdouble[n], T longdouble[n], cell int64[n, 3], blocked bool[n], out_of_scope bool[n]).  `value` is the raw sum
    also where `blocked`; out_of_scope: not blocked and an infinite datum among the 64."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 here"
    cs, g = eg.csetup, np.asarray(eg.grid)
    assert g.dtype == F32
    p0, p1, r = stencil(cs, pts)
    n = len(p0)
    H, A = zip(*(_hermite(r[:, a]) for a in range(3)))
    value, T = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    blocked, infinite = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in itertools.product(range(2), repeat=3):
            ix = [(p1 if s[a] else p0)[:, a] - 1 for a in range(3)]
            d = g[:, ix[0], ix[1], ix[2]]                        # float32[8, n]
            blocked |= d[0] > THRESHOLD
            infinite |= np.isinf(d).any(axis=0)
            for ch, o in enumerate(CHANNELS):
                value += d[ch].astype(LD) * (H[0][o[0]][s[0]] * H[1][o[1]][s[1]] * H[2][o[2]][s[2]])
                T += np.abs(d[ch]).astype(LD) * (A[0][o[0]][s[0]] * A[1][o[1]][s[1]] * A[2][o[2]][s[2]])
    blocked &= eg.ewald_precision == math.inf
    return value, T, p0, blocked, infinite & ~blocked


def reference_noderiv(eg, pts):
    """The "no derivatives" branch as written in grids.jl:259-269 -> (value, T): channel 1 at the eight corners with trilinear
    weights, indexed g.grid[x, y, z, 1] although the array is [z, y, x, channel] -- the first array index, which runs along z,
    receives the x cell index and the third, along x, the z cell index; NaN beyond an axis (Julia: BoundsError); no blocking rule."""
    cs, g = eg.csetup, np.asarray(eg.grid)
    nx, ny, nz = cs.npoints
    p0, p1, r = stencil(cs, pts)
    rl = r.astype(LD)
    w = [[1 - rl[:, a], rl[:, a]] for a in range(3)]
    value, T = np.zeros(len(p0), dtype=LD), np.zeros(len(p0), dtype=LD)
    for s in itertools.product(range(2), repeat=3):
        a, b, c = [(p1 if s[q] else p0)[:, q] for q in range(3)]            # g.grid[a, b, c, 1], 1-based: a along z, b y, c x
        inside = (a >= 1) & (a <= nz) & (b >= 1) & (b <= ny) & (c >= 1) & (c <= nx)
        d = np.where(inside, g[0, np.clip(c, 1, nx) - 1, np.clip(b, 1, ny) - 1, np.clip(a, 1, nz) - 1].astype(LD), LD(np.nan))
        ws = w[0][s[0]] * w[1][s[1]] * w[2][s[2]]
        value += d * ws
        T += np.abs(d) * ws
    return value, T


def bound(T):
    return K * U * T


def ratio(got, value, T) -> float:
    """worst |got - value| / (2^-53 T) over the finite entries (0 where T == 0 and the values are equal)"""
    err = np.abs(np.asarray(got).astype(LD) - value)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(T > 0, err / (U * T), np.where(err == 0, LD(0), LD(np.inf)))
    return float(q.max()) if len(q) else 0.0


def check_values(got, eg, pts, what, ref=None):
    """The one form of every check: 1e100 where the reference is blocked, NaN where it is NaN, |got - value| <= bound elsewhere
    (points out of scope excepted).  -> worst |got - value| / (2^-53 T)"""
    value, T, _cell, blocked, skip = ref if ref is not None else reference(eg, pts)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == value.shape, (what, got.shape, value.shape)
    assert np.array_equal((got == 1e100)[~skip], blocked[~skip]), (what, "blocked pattern", np.nonzero(((got == 1e100) != blocked) & ~skip)[0][:8])
    nan = np.isnan(value) & ~blocked & ~skip
    assert np.array_equal(np.isnan(got) & ~blocked & ~skip, nan), (what, "NaN pattern", np.nonzero((np.isnan(got) & ~blocked & ~skip) != nan)[0][:8])
    m = ~blocked & ~skip & ~nan
    assert np.isfinite(got[m]).all(), what
    worst = ratio(got[m], value[m], T[m])
    bad = np.abs(got[m].astype(LD) - value[m]) > bound(T[m])
    assert not bad.any(), (what, worst, np.nonzero(m)[0][bad][:8])
    return worst


# ---------------------------------------------------------------------------------------------- the catalogue
class Case:
    """a grid, its points and (computed once, on first use) its reference"""

    def __init__(self, name, eg, pts, family, **info):
        self.name, self.eg, self.pts, self.family, self.info = name, eg, np.ascontiguousarray(pts, dtype=np.float64), family, info
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = reference(self.eg, self.pts)
        return self._ref

    def __repr__(self):
        return f"Case({self.name})"


BLOCKING_DIMS = (7, 5, 3)
_catalogue = None


def catalogue():
    """Every (grid, points) case, built once: random (VdW and Coulomb) and poly on every cell and dims, the 64 one-hot grids per cell,
    the blocking family on BLOCKING_DIMS per cell, the huge Coulomb grid at its nodes."""
    global _catalogue
    if _catalogue is not None:
        return _catalogue
    out = []
    for ci, cell in enumerate(CELLS):
        for di, dims in enumerate(DIMS):
            cs = cset(cell, dims)
            pts = all_points(cs, seed=10 * ci + di)
            tag = f"{cell}/{'x'.join(map(str, dims))}"
            base = random_data(cs, 100 + 10 * ci + di)
            out.append(Case(f"random-vdw/{tag}", energy_grid(cs, base, VDW), pts, "random"))
            out.append(Case(f"random-coulomb/{tag}", energy_grid(cs, random_data(cs, 200 + 10 * ci + di), COULOMB), pts, "random"))
            coeff = poly_coefficients(dims, 300 + di)
            # Coulomb-declared: the interpolant is compared everywhere
            data = poly_data(cs, coeff)
            out.append(Case(f"poly-coulomb/{tag}", energy_grid(cs, data, COULOMB), pts, "poly", coeff=coeff))
            if min(dims) >= 3:
                # VdW-declared, with an integer constant that puts the median node value at 5e6: a blocking pattern with structure
                shift = 5_000_000 - int(np.median(data[0]))
                lifted = data.copy()
                lifted[0] = (data[0].astype(np.int64) + shift).astype(F32)
                assert np.abs(data[0].astype(np.int64) + shift).max() < 2 ** 24 and 0.2 < (lifted[0] > THRESHOLD).mean() < 0.8
                out.append(Case(f"poly-vdw/{tag}", energy_grid(cs, lifted, VDW), pts, "poly-vdw"))
        pts1 = all_points(cset(cell, (1, 1, 1)), seed=50 + ci)
        for node, ch, eg in one_hot_grids(cell):
            out.append(Case(f"one-hot/{cell}/node{node[0]}{node[1]}{node[2]}/ch{ch}", eg, pts1, "one-hot", node=node, channel=ch))
        cs = cset(cell, BLOCKING_DIMS)
        base = random_data(cs, 400 + ci)
        pts = all_points(cs, seed=60 + ci)
        inner, inside = interior_cell(cs, seed=ci)
        pts = np.concatenate([pts, inside])
        last, _q = last_layer_cell(cs, pts)
        for where, p0 in (("interior", inner), ("last-layer", last)):
            for vname, node, data in blocking_grids(cs, base, p0):
                for decl, prec in (("vdw", VDW), ("coulomb", COULOMB)):
                    out.append(Case(f"blocking-{decl}/{cell}/{where}/node{node[0]}.{node[1]}.{node[2]}/{vname}", energy_grid(cs, data, prec), pts,
                                    "blocking", special=vname, declared=decl, node=node, p0=tuple(int(x) for x in p0), where=where))
        csh = cset(cell, (5, 3, 1))
        out.append(Case(f"huge-coulomb/{cell}", huge_coulomb(csh), node_points(csh), "huge"))
    _catalogue = out
    return out


# ---------------------------------------------------------------------------------------------- block masks
BLOCK_VALUES = {"5e6f": (THRESHOLD, False), "above": (ABOVE, True), "+inf": (F32(np.inf), True), "nan": (F32(np.nan), False),
                "-inf": (F32(-np.inf), False)}


def block_from_grid_reference(value, threshold=THRESHOLD) -> np.ndarray:
    """BlockFile(g::EnergyGrid) (grids.jl:190-201): every CELL -- origins 0 .. n - 2 per axis -- whose origin value exceeds the
    threshold blocks its eight corners; the last node of an axis is no cell origin.  value float32[nx, ny, nz] -> bool."""
    nx, ny, nz = value.shape
    with np.errstate(invalid="ignore"):
        hot = value[:-1, :-1, :-1] > threshold
    out = np.zeros(value.shape, dtype=bool)
    for di, dj, dk in itertools.product(range(2), repeat=3):
        out[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk] |= hot
    return out


def block_entries(dims):
    """name -> 0-based node of the single entry: first cell, an interior cell, the last cell origin (n - 2) and the last node (n - 1)
    on each axis (the other two axes at the first cell; at n = 2 the last cell origin is the first cell)"""
    n = [int(d) + 1 for d in dims]
    out = {"first": (0, 0, 0), "interior": tuple((x - 1) // 2 for x in n)}
    for a in range(3):
        for name, i in (("origin", n[a] - 2), ("node", n[a] - 1)):
            e = [0, 0, 0]
            e[a] = i
            out[f"last-{name}-{'xyz'[a]}"] = tuple(e)
    out["last-node-xyz"] = tuple(x - 1 for x in n)
    return out


def block_single_entry_cases(dims):
    """[(name, value float32[nx, ny, nz], expected number of set points or None)]"""
    n = tuple(int(d) + 1 for d in dims)
    out = []
    for ename, e in block_entries(dims).items():
        for vname, (v, hot) in BLOCK_VALUES.items():
            value = np.zeros(n, dtype=F32)
            value[e] = v
            is_origin = all(e[a] <= n[a] - 2 for a in range(3))
            out.append((f"{ename}/{vname}", value, 8 if (hot and is_origin) else 0))
    return out


def block_random_case(dims, seed=0):
    rng = np.random.default_rng(seed)
    n = tuple(int(d) + 1 for d in dims)
    value = rng.normal(0.0, 1e3, n).astype(F32)
    value[rng.random(n) < 0.1] = F32(1e7)
    value[0, 0, 0] = F32(1e7)                                    # (a lattice of eight nodes has one cell: never empty)
    return value


def sphere_abi_args(cs):
    """(dims, delta, shift, mat, invmat, ortho, safemin2) as ceg_block_spheres takes them (matrices column-major)"""
    from ceg_hip.hostmirror.utils import prepare_periodic_distance_computations
    ortho, safemin = prepare_periodic_distance_computations(cs.cell.mat)
    return (np.ascontiguousarray(cs.dims, dtype=np.int32), np.ascontiguousarray(cs.delta, dtype=np.float64),
            np.ascontiguousarray(cs.shift, dtype=np.float64), G._matT(cs.cell.mat), G._matT(cs.cell.invmat), int(ortho), float(safemin) ** 2)


def sphere_case(cs, nspheres, seed=0):
    """(centers[n, 3], radius2[n]): centres uniform in the cell, radii within 20 % of the one at which n spheres of a Poisson process
    cover half the cell: 1 - exp(-n (4/3) pi r^3 / V) = 1/2"""
    rng = np.random.default_rng(seed)
    n = int(nspheres)
    if n == 0:
        return np.empty((0, 3)), np.empty(0)
    vol = abs(np.linalg.det(cs.cell.mat))
    r = (math.log(2.0) * vol * 3.0 / (4.0 * math.pi * n)) ** (1.0 / 3.0)
    centers = rng.uniform(0.0, 1.0, (n, 3)) @ cs.cell.mat.T
    if n == 1:                                                   # one sphere of half the cell volume (wider than the cell: it meets its images)
        return np.ascontiguousarray(centers), np.array([(0.5 * vol * 3.0 / (4.0 * math.pi)) ** (2.0 / 3.0)])
    return np.ascontiguousarray(centers), (r * rng.uniform(0.8, 1.2, n)) ** 2


def lattice_point(cs, node) -> np.ndarray:
    """inverse_offsetpoint of a 0-based node as the kernel forms it: i * delta + shift"""
    return np.asarray(node, dtype=np.float64) * cs.delta + cs.shift


def sphere_boundary_case(oracle, cs):
    """(centre node, its x-neighbour, radius2): radius2 is exactly the squared distance the scan computes from the centre to the
    neighbour (the literal minimum-image routine on centre .- point)"""
    from ceg_hip.hostmirror.utils import prepare_periodic_distance_computations
    centre = tuple(int(n) // 2 for n in cs.npoints)
    neighbour = (centre[0] + 1, centre[1], centre[2])
    ortho, safemin = prepare_periodic_distance_computations(cs.cell.mat)
    d = lattice_point(cs, centre) - lattice_point(cs, neighbour)
    r2 = float(oracle.periodic_distance2(d, cs.cell.mat, cs.cell.invmat, ortho, safemin ** 2)[0])
    assert 0.0 < r2 < 4.0 * float(cs.delta[0]) ** 2
    return centre, neighbour, r2


def sphere_minimage_longdouble(cs, centers, radius2):
    """Orthorhombic cells only: (mask bool[nx, ny, nz], near bool[nx, ny, nz]) from a round-based minimum image in longdouble; `near`:
    |d^2 - r^2| <= 1e-9 r^2 for some sphere"""
    L = np.diag(cs.cell.mat).astype(LD)
    assert np.array_equal(np.diag(np.diag(cs.cell.mat)), cs.cell.mat)
    nx, ny, nz = cs.npoints
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    p = (np.stack([ii, jj, kk], axis=-1).reshape(-1, 3) * cs.delta + cs.shift).astype(LD)
    mask, near = np.zeros(len(p), dtype=bool), np.zeros(len(p), dtype=bool)
    for c, r2 in zip(np.asarray(centers, dtype=np.float64), np.asarray(radius2, dtype=np.float64)):
        d = c.astype(LD) - p
        d = d - L * np.rint(d / L)
        d2 = (d * d).sum(axis=1)
        mask |= d2 < LD(r2)
        near |= np.abs(d2 - LD(r2)) <= LD(1e-9) * LD(r2)
    return mask.reshape(nx, ny, nz), near.reshape(nx, ny, nz)


# ---------------------------------------------------------------------------------------------- Monte-Carlo setups on synthetic grids
MC_VDW_DIMS = ((7, 5, 3), (1, 3, 5), (15, 13, 11))              # the VdW grids of kinds 1, 2, 3 (1-based ff index); kind 4 has none
MC_COULOMB_DIMS = (5, 3, 1)
MC_CHARGES = (0.7, -0.35, 0.0, 1.3)
MC_SIZES = (1, 3, 4, 5, 8, 16)
MC_SPECIES = [[1 + a % 3 for a in range(m)] for m in MC_SIZES] + [[4, 1]]          # kinds cycle with period 3; the last species holds the kind without a grid


def mc_setup(cell: str, coulomb=True, blocking=False, coulomb_vdw=False):
    """An empty-box MonteCarloSetup on synthetic grids: no Ewald sums (EwaldFramework.empty), the MC cell the 2 x 1 x 1 supercell of the
    grid cell, a force field whose guest kinds do not interact (util.tiny_forcefield: kinds 1 to 4 meet only the probes), so that
    columns 2 and 3 of every row are exactly 0.  `blocking`: the grid of kind 1 carries the next float above 5e6 at one corner of an
    interior cell; ``setup.blocked_points`` lie in that cell.  `coulomb_vdw`: the grid in the Coulomb slot is declared VdW and carries the
    same value at one corner of an interior cell; ``setup.coulomb_blocked_points`` lie there (every point of it interpolates to 1e100)."""
    from ceg_hip.hostmirror import montecarlo as M
    from ceg_hip.hostmirror.ewald import EwaldFramework
    from util import tiny_forcefield
    ci = list(CELLS).index(cell)
    mat = CELLS[cell] * np.array([2.0, 1.0, 1.0])[None, :]
    ff = tiny_forcefield()
    grids = [G.EnergyGrid.trivial(True) for _ in range(ff.nkinds)]              # a zero grid: no framework term for that kind
    for k, dims in enumerate(MC_VDW_DIMS):
        cs = cset(cell, dims)
        grids[k] = energy_grid(cs, random_data(cs, 500 + 10 * ci + k), VDW)
    blocked_points = None
    if blocking:
        cs = grids[0].csetup
        p0, blocked_points = interior_cell(cs, seed=7 + ci)
        data = grids[0].grid.copy()
        data[(0,) + corner_nodes(cs, p0)[5]] = ABOVE
        grids[0] = energy_grid(cs, data, VDW)
    cs = cset(cell, MC_COULOMB_DIMS)
    coul = energy_grid(cs, random_data(cs, 600 + ci), COULOMB) if coulomb else G.EnergyGrid.trivial(True)
    coulomb_blocked_points = None
    if coulomb_vdw:
        assert coulomb
        p0, coulomb_blocked_points = interior_cell(cs, seed=17 + ci)
        data = coul.grid.copy()
        data[(0,) + corner_nodes(cs, p0)[2]] = ABOVE
        coul = energy_grid(cs, data, VDW)
    charges = np.full(ff.nkinds + 1, np.nan)
    charges[1:5] = MC_CHARGES
    mc = M.MonteCarloSetup(ff, mat, np.linalg.inv(mat), [list(s) for s in MC_SPECIES], charges, [[] for _ in MC_SPECIES],
                           EwaldFramework.empty(mat), coul, grids, 0.0)
    mc.blocked_points = blocked_points
    mc.coulomb_blocked_points = coulomb_blocked_points
    return mc


def mc_placements(mc, species: int, n: int, rng) -> np.ndarray:
    """float64[n, m, 3]: every atom drawn from the point families of the grids -- uniform in +-40 A for most; one row with an atom on a
    tiny-negative point (row 0, last atom), one with an atom on a node of one of the grids (row 1 % n, atom m // 2), one with an
    atom of kind 1 in the blocked cell (row 2 % n, atom 0; blocking setups only); where the Coulomb slot holds a blocking grid, row 3 % n
    has its last atom of charge 0.0 (else atom 0) in the blocked cell of that grid and row 4 % n atom 1 (atom 0 of a one-atom species)"""
    m = len(mc.ffidx[species])
    pos = rng.uniform(-40.0, 40.0, (n, m, 3))
    tiny = tiny_negative()
    pos[0, m - 1] = tiny[int(rng.integers(len(tiny)))]
    g = mc.grids[int(rng.integers(3))]
    nodes = node_points(g.csetup)
    pos[1 % n, m // 2] = nodes[int(rng.integers(len(nodes)))]
    if mc.blocked_points is not None and mc.ffidx[species][0] == 1:
        pos[2 % n, 0] = mc.blocked_points[int(rng.integers(len(mc.blocked_points)))]
    cb = getattr(mc, "coulomb_blocked_points", None)
    if cb is not None:
        neutral = [a for a, ix in enumerate(mc.ffidx[species]) if mc.charges[ix] == 0.0]
        pos[3 % n, neutral[-1] if neutral else 0] = cb[int(rng.integers(len(cb)))]
        pos[4 % n, min(1, m - 1)] = cb[int(rng.integers(len(cb)))]
    return pos


def column_reference(mc, ids, pos):
    """Columns 0 and 1 of the rows of a molecule with the 1-based kinds `ids` at pos[n, m, 3] (montecarlo.jl:490-504):
    -> (v0, t0, blocked0, v1, t1, nb1): v0 = sum_a value(VdW grid of kind a, x_a); v1 = sum_a q_a c(x_a) over the atoms whose Coulomb
    value is not 1e100, nb1 the number of atoms whose value is (a VdW-declared grid in the Coulomb slot, blocked cell): each of those adds
    1e100 WITHOUT its charge; t0, t1 the summed T (|q_a| T for column 1): the bounds add up"""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, len(ids), 3)
    n = len(pos)
    v0, t0, v1, t1 = (np.zeros(n, dtype=LD) for _ in range(4))
    blocked = np.zeros(n, dtype=bool)
    nb1 = np.zeros(n, dtype=np.int64)
    hascoulomb = mc.coulomb.ewald_precision != -math.inf
    for a, ix in enumerate(ids):
        g = mc.grids[ix - 1]
        if g.ewald_precision != -math.inf:
            value, T, _cell, blk, skip = reference(g, pos[:, a])
            assert not skip.any()
            v0 += value
            t0 += T
            blocked |= blk
        if hascoulomb:
            value, T, _cell, blk, skip = reference(mc.coulomb, pos[:, a])
            assert not skip.any()
            q = LD(float(mc.charges[ix]))
            v1 += np.where(blk, LD(0), q * value)
            t1 += np.where(blk, LD(0), abs(q) * T)
            nb1 += blk
    return v0, t0, blocked, v1, t1, nb1


def check_rows(rows, mc, ids, pos, what):
    """rows[n, >= 2] against column_reference: column 0 >= 1e90 where an atom is blocked, within the summed bound elsewhere; column 1
    within its bound, and nb1 1e100 (the other atoms vanish in its rounding: 2^-50 relative) where nb1 atoms sit in a blocked cell of
    the Coulomb slot -- not q 1e100 and not 0.  -> (worst ratio of column 0, of column 1, blocked rows, rows with nb1 > 0)"""
    v0, t0, blocked, v1, t1, nb1 = column_reference(mc, ids, pos)
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.shape[0] == len(v0), (what, rows.shape, len(v0))
    assert np.array_equal(rows[:, 0] >= 1e90, blocked), (what, "blocked rows", rows[:, 0], blocked)
    assert np.isfinite(rows[:, :2]).all(), what
    m, c = ~blocked, nb1 == 0
    for got, v, t, col in ((rows[m, 0], v0[m], t0[m], 0), (rows[c, 1], v1[c], t1[c], 1)):
        bad = np.abs(got.astype(LD) - v) > bound(t)
        assert not bad.any(), (what, col, ratio(got, v, t), np.nonzero(bad)[0][:8])
    want = nb1[~c] * 1e100
    assert (np.abs(rows[~c, 1] - want) <= 2.0 ** -50 * want).all(), (what, "1e100 without the charge", rows[~c, 1], nb1[~c])
    return ratio(rows[m, 0], v0[m], t0[m]), ratio(rows[c, 1], v1[c], t1[c]), int(blocked.sum()), int((~c).sum())
