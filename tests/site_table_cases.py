"""Synthetic cases, a high-precision reference and a derived error bound for the two tables of site hopping, ``ceg_site_tables`` /
``ceg_site_tables_device`` (second half of csrc/ceg_site.hip: k_site_points, k_site_recip_pairs, k_site_real_pairs).  No tests here:
``tests/test_site_table_cases_host.py`` checks this file on the CPU (the placement claims, the reference against the oracle and
against ``recip_cases.reference`` of two-molecule systems, the bounds against a float64 NumPy evaluation, the tile arithmetic),
``tests/test_gpu_site_table_shapes.py`` runs the cases on the device.

Everything goes through the C ABI with synthetic inputs -- ``ceg_interp_create`` handles behind ``ceg_mc_create``, then
``ceg_site_tables[_device]`` with the explicit offsets OFFSET_ONE / OFFSET_PAIR -- so that n, m, the kinds, nk and ks are free choices.

Setup.  The cell of ``recip_cases.general_cell`` (all nine entries of the matrix and of its inverse non-zero) for ``mat`` and for
``ewald_invmat``; one case on the upper-triangular 40 A cell of ``pair_rule_cases.cell``.  Four kinds with the charges 0.7, -0.35, 0.0,
1.3; a molecule of m atoms has the kinds (0, 1, 0, 2, 3)[a % 5].  VdW grids (``interp_cases`` random data on the triclinic 9 x 11 x 13 A
cell, dims as MC_VDW_DIMS) for the kinds 0, 1, 2 and none for kind 3, a Coulomb grid; the grid of kind 0 carries the next float above
5e6 at one corner of an interior cell.  The rule table is symmetric and every pair of kinds has an entry of its own (ENTRY_OF_PAIR: ten
different entries of ``pair_rule_cases.entries``, among them LJ, LJ+CED, Buckingham, CED alone and, for (0, 0), HS+Buckingham+CED with
the summed radius 1.5 A), so a repeated kind index reaches another entry.

Sites (``sites``).  Placements of one rigid model (``recip_cases.molecule`` geometry, +-3 A) under random rotations.  By index:
0 a uniform point of the cell; 1 the same orientation 3 A away; 2 the same 5 A away plus the lattice vector mat (3, -2, 1) -- about
100 A outside the cell, close to site 0 only across cell faces; 3 the same 0.4 A away plus mat (-1, 2, 0): its first atom (kind 0)
overlaps the hard sphere of site 0's; 4 a placement whose first atom lies in the blocked cell of the grid of kind 0; the others uniform
in the cell, every second one moved by a lattice vector with coefficients in -2..2.  A drawn site any of whose kind-0 atoms the grid
blocks is drawn again, so site 4 is the only blocked one.  The host module asserts on every case, with ``literal_r2``: atoms tens of A
outside the cell, site pairs wholly beyond the cutoff, pairs close only across a face, the share of hard-sphere overlaps (at least one
pair from n = 4; at most 5 % of the pairs from n = 15, where 5 % is more than five pairs), and that no atom pair lies within relative
1e-9 of cutoff^2 or of the hard-sphere radius^2 -- except in the case ``thresholds``, which places one-atom sites at +-1e-12, +-2e-16 and 0
relative to both and asserts only that the device decides as ``literal_r2`` does (the kernel forms r^2 with contraction off in the order
``literal_r2`` restates; its table gives exactly -1.75 K inside the cutoff, +inf inside the sphere, 0 outside).

Reference, per element, in np.longdouble.
  recip[i]          ``recip_cases.reference`` with 2 ENC + STATIC = OFFSET_ONE
  framework[i]      (v0 + v1 of ``interp_cases.column_reference``) + recip[i]; >= 1e90 where an atom is blocked
  interactions[i,j] P_ij + 2 sum_k kf_k Re(S_i conj S_j) + OFFSET_PAIR; P_ij the sum over the m x m atom pairs of ``entry_energy_ld`` at
                    ``literal_r2`` (pos_i - pos_j, the kernel's order), S_i as in ``recip_cases.reference`` (f reduced by rint, the phase
                    reduced again, one cos / sin per (atom, k-vector): ``structure_factors``); +inf where a hard sphere is overlapped.

Tolerance, per element, from the operations of the kernels; u = 2^-53; nothing in it is fitted to what the device returns.
  S_i (fill_tables + molecule_sf), error of the complex number in units of u A, A = sum |q|:
    phase        f = I0 x + I3 y + I6 z rounds three times at most at F_ax = sum_c |invmat[ax, c] r_c| (contraction only removes
                 roundings), f - rint(f) is exact, mm * ff rounds once at |mm| / 2: 2 pi sum_ax k_ax (3 F_ax + 0.5), as ``recip_cases.bound``
    amplitude    three table entries by sincos_2pi, 1.9e-16 = 1.72 u per component, 2.43 u per complex entry              7.3
                 the y.z product: two products and a sum per component, on numbers below 1                               2.83
                 the charge: one product per component                                                                    1.42
                 the x product: two products per component (none where they fuse into the sum)                            2.83
                 m fused sums: two additions per atom and component, each at the running sum of |q| -- 1.42 * 2 sum_a A_a / A,
                 A_a = |q_0| + .. + |q_a|: at most 2.83 m                                                                  acc
                 C_S = 14.4 + acc (``sf_count``): 59.7 at most (m = 16, all of the charge on the first atom), 17.2 (m = 1) to 37.6 (m = 16) here
  recip[i]       E = sum kf (2 Re(conj F S) + |S|^2): an error dS moves a term by 2 kf (|F| + |S|) |dS| <= 2 kf (|F| A + A^2) |dS| / A,
                 which is at most TWICE the term's share of T = ``recip_cases.magnitude`` (T holds A^2 once) -- recip_cases.bound's
                 phase part was derived for k_recip and counts it once.  Then kf (F.x S.x + F.y S.y): two products, a sum, kf (4, times
                 sqrt 2: 6); the same for |S|^2 (within the 6); ceil(nk / 256) additions per thread (the q += MC_THREADS walk); six
                 shuffle levels and four wave sums; 2 tot + tot, + off1 (2).  Hence
                     recip_bound = u (2 (phase + C_S) + 18 + ceil(nk / 256)) T
                 against recip_cases.bound's u (phase + 32) T: both constants are larger because the count demands it.
  pair term      R_ij = 2 sum kf Re(S_i conj S_j); the errors of S_i and of S_j enter once each, every term is at most 2 kf A^2; the MFMA
                 adds 2 nk4 products to the accumulator one after the other (nk4 = nk rounded up to 4), each addition rounding at most
                 at the running sum; w = 2 kf is exact, w * a rounds once per operand and component (2).  Hence
                     pair_recip_bound = u (2 * 2 pi sum_ax k_ax (3 F_ax + 0.5) + 2 nk4 + c) T_pair,   T_pair = sum_k 2 kf_k A^2,
                 F_ax over both sites, c = 2 C_S + 2 (36.5 to 77.2 here; 121.4 at most).
  P_ij           1e-9 of the summed sizes of ``entry_energy_ld`` (``test_gpu_pair_rules._assert_energies``' rtol): rule_energy calls
                 the library's exp / erfc / pow, whose error the source does not give.
  grid terms     ``interp_cases.bound`` of the summed T, as ``check_rows`` uses it.
  joins          (fv + fd) + rec and (P + R) + off2: 4 u of the summed magnitudes.

Measured on the CPU (the host module prints them, per case): a float64 NumPy evaluation of the same formulas (``structure_factors`` and
the sums in float64; not the code under test) stays within 0.022 of recip_bound and within 0.028 of pair_recip_bound over all cases (the
largest at nk = 3; 0.002 to 0.013 at nk = 114 and above); the oracle's float64 pair sums stay within 1.3e-6 of the P_ij tolerance.
Measured on an MI355X, worst error / tolerance (recip, framework, interactions): edges 0.0058, 0.0007, 0.0045; tiles17 0.0054, 0.0006,
0.0039; molecule 0.0052, 0.0022, 0.0104 (m = 1); kloop 0.0210, 0.0084, 0.0264 (all at nk = 3 to 9; 0.0080, 0.0020, 0.0055 from nk = 255);
terms 0.0035, 0.0032, 0.0047; lds 0.0023, 0.0001, 0.0046; triangular 0.0040, 0.0005, 0.0056.  The launch with exactly 64 KiB of tables
(plus the 704 bytes of static LDS of k_site_points) is accepted.

Cases (the smallest shapes at which each mechanism can still fail; a tile is 16 x 16 sites):
  edges      n in 1, 2, 15, 16, 17, 31, 32, 33, 48, 49 with m = 3 and the 114 k-vectors of ``recip_cases.kset((5, 4, 3))``
  tiles17    n = 257, m = 3: 17 x 17 tiles; compared: rows and columns 0-16, 15 either side of every multiple of 16 along row 40 and
             column 200, the last 17 rows and columns, 256 random pairs; symmetry and the diagonal in full
  molecule   m in 1, 2, 5, 8, 16 at n = 33
  kloop      nk in 0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 316 at n = 17, m = 3, picked from ``half_space((7, 6, 5))``; k-vector 0 has
             kf = 20, so a lane beyond nk that is not weighted zero shows
  terms      n = 33: all charges zero; a rule table of empty entries; no grids at all; (recip = NULL runs on ``edges-n33``)
  lds        m = 16 with ks = (101, 38, 38), stride 256: exactly 64 KiB of tables; five k-vectors on the last entries of every axis; and
             ks = (102, 38, 38), stride 257: refused
  triangular ``edges-n33`` once more in the upper-triangular cell
  thresholds see above"""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from ceg_hip import _abi, grids as G
from ceg_hip.hostmirror.constants import COULOMBIC_CONVERSION_FACTOR as COULOMBIC
from ceg_hip.hostmirror.interactions import FF

import interp_cases as IC
import pair_rule_cases as PR
import recip_cases as RC

LD = np.longdouble
U = 2.0 ** -53
TILE = 16
MC_THREADS = 256                                  # restated from csrc/ceg_mc_state.h
CHARGES = (0.7, -0.35, 0.0, 1.3)
KIND_PATTERN = (0, 1, 0, 2, 3)
ENC, STATIC = -7.5, 123.25
OFFSET_ONE = 2.0 * ENC + STATIC                   # 108.25, exact
OFFSET_PAIR = -41.625
CUTOFF = PR.CUTOFF
SPHERE = PR.SPHERE
BASE_KS = (5, 4, 3)
PICK_KS = (7, 6, 5)
LDS_KS = {256: (101, 38, 38), 257: (102, 38, 38)}
# entry of pair_rule_cases.entries() per unordered pair of kinds: all different
ENTRY_OF_PAIR = {(0, 0): "HS+Buckingham+CED", (0, 1): "LJ+CED", (0, 2): "Buckingham", (0, 3): "CED", (1, 1): "LJ", (1, 2): "LJ+LJ",
                 (1, 3): "Monomial", (2, 2): "Exponential", (2, 3): "LJ+NoInteraction+CED", (3, 3): "Coulomb"}
CELLS = {"general": np.linalg.inv(RC.general_cell()), "triangular": PR.cell("triangular")}


def kinds_of(m: int) -> np.ndarray:
    return np.array([KIND_PATTERN[a % len(KIND_PATTERN)] for a in range(m)], dtype=np.int32)


# ---------------------------------------------------------------------------------------------- the rule tables
class PairTable(PR.Table):
    """a ``pair_rule_cases.Table`` whose entry is chosen by the PAIR of kinds: entry_of[a][b] (symmetric), None = no rule"""

    def __init__(self, name, cutoff, ents, entry_of):
        self.name, self.cutoff, self.entries = name, float(cutoff), ents
        self.entry_of = entry_of
        self.nkinds = nk = len(entry_of)
        rules, offsets = [], [0]
        for a in range(nk):
            for b in range(nk):
                e = entry_of[a][b]
                if e is not None:
                    rules += ents[e][1]
                offsets.append(len(rules))
        self.rules = np.zeros(max(len(rules), 1), dtype=_abi.RULE_DTYPE)
        for q, (kind, p, shift) in enumerate(rules):
            self.rules[q]["kind"] = kind
            self.rules[q]["p"] = p
            self.rules[q]["shift"] = shift
        self.nrules = len(rules)
        self.offsets = np.asarray(offsets, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def table(which: str) -> PairTable:
    nk = len(CHARGES)
    if which == "full":
        ents = PR.entries()
        names = [e[0] for e in ents]
        of = [[names.index(ENTRY_OF_PAIR[(min(a, b), max(a, b))]) for b in range(nk)] for a in range(nk)]
    elif which == "empty":
        ents = [("empty", [])]
        of = [[0] * nk for _ in range(nk)]
    elif which == "thresholds":
        ents = [("HS+NoInteraction", [(int(FF.HardSphere), (0.9, 0.6, 0.0), 0.0), (int(FF.NoInteraction), (0.0, 0.0, 0.0), 1.75)])]
        of = [[0] * nk for _ in range(nk)]
    else:
        raise KeyError(which)
    return PairTable(which, CUTOFF, ents, of)


# ---------------------------------------------------------------------------------------------- grids
@functools.lru_cache(maxsize=None)
def grid_set():
    """(VdW EnergyGrid or None per kind, Coulomb EnergyGrid, points[16, 3] inside the blocked cell of the grid of kind 0)"""
    vdw = [None] * len(CHARGES)
    for k, dims in enumerate(IC.MC_VDW_DIMS):
        cs = IC.cset("tric", dims)
        vdw[k] = IC.energy_grid(cs, IC.random_data(cs, 700 + k), IC.VDW)
    cs = vdw[0].csetup
    p0, inside = IC.interior_cell(cs, seed=11)
    data = np.array(vdw[0].grid, dtype=IC.F32, copy=True)
    data[(0,) + IC.corner_nodes(cs, p0)[5]] = IC.ABOVE
    vdw[0] = IC.energy_grid(cs, data, IC.VDW)
    cs = IC.cset("tric", IC.MC_COULOMB_DIMS)
    return vdw, IC.energy_grid(cs, IC.random_data(cs, 710), IC.COULOMB), inside


def _grid_view(with_grids: bool, kind_charge):
    """what ``interp_cases.column_reference`` reads of a MonteCarloSetup: grids by 1-based kind, the Coulomb grid, the charges"""
    vdw, coul, _inside = grid_set()
    none = G.EnergyGrid.trivial(True)
    charges = np.concatenate([[np.nan], kind_charge])
    if not with_grids:
        return SimpleNamespace(grids=[none] * len(CHARGES), coulomb=none, charges=charges)
    return SimpleNamespace(grids=[g if g is not None else none for g in vdw], coulomb=coul, charges=charges)


def _blocked(pos, kinds) -> np.ndarray:
    """bool[n]: a kind-0 atom of the site lies in a cell the grid of kind 0 blocks"""
    g0 = grid_set()[0][0]
    out = np.zeros(len(pos), dtype=bool)
    for a in np.nonzero(kinds == 0)[0]:
        out |= IC.reference(g0, pos[:, a])[3]
    return out


# ---------------------------------------------------------------------------------------------- k-spaces
@functools.lru_cache(maxsize=None)
def kset_of(spec) -> RC.KSet:
    if spec[0] == "none":
        return RC.with_constants((3, 3, 3), np.empty((0, 3)), 1)
    if spec[0] == "base":
        return RC.kset(BASE_KS, seed=51)
    if spec[0] == "pick":                           # nk of the half space, as egrid_shape_cases.kset_of picks them; kf[0] large
        n = spec[1]
        full = RC.half_space(PICK_KS)
        pick = np.sort(np.random.default_rng(42 + n).choice(len(full), n, replace=False))
        k = RC.with_constants(PICK_KS, full[pick], 43 + n)
        k.kf[0] = 20.0
        return k
    if spec[0] == "lds":                            # the last entry of every axis: i = kx, j = +-ky, k = +-kz
        kx, ky, kz = LDS_KS[spec[1]]
        return RC.with_constants((kx, ky, kz), [[kx, ky, kz], [kx, -ky, -kz], [0, ky, -kz], [1, 0, 0], [kx // 2, -ky, kz]], 61)
    raise KeyError(spec)


# ---------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    family: str
    n: int
    m: int
    cell: str = "general"
    kspec: tuple = ("base",)
    charges: str = "mixed"          # "zero": every kind has charge 0
    table: str = "full"
    grids: bool = True
    seed: int = 0
    refused: bool = False

    @property
    def kinds(self) -> np.ndarray:
        return kinds_of(self.m)

    @property
    def kind_charge(self) -> np.ndarray:
        return np.zeros(len(CHARGES)) if self.charges == "zero" else np.array(CHARGES)

    @property
    def q(self) -> np.ndarray:
        return self.kind_charge[self.kinds]

    @property
    def mat(self) -> np.ndarray:
        return CELLS[self.cell]

    @property
    def inv(self) -> np.ndarray:
        return np.linalg.inv(CELLS[self.cell])

    @property
    def k(self) -> RC.KSet:
        return kset_of(self.kspec)


EDGE_N = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
MOLECULE_M = (1, 2, 5, 8, 16)
KLOOP_NK = (0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 316)
CASES = [Case(f"edges-n{n}", "edges", n, 3, seed=100 + n) for n in EDGE_N]
CASES += [Case("tiles17", "tiles17", 257, 3, seed=257)]
CASES += [Case(f"molecule-m{m}", "molecule", 33, m, seed=200 + m) for m in MOLECULE_M]
CASES += [Case(f"kloop-nk{nk}", "kloop", 17, 3, kspec=("pick", nk) if nk else ("none",), seed=300 + nk) for nk in KLOOP_NK]
CASES += [Case("terms-zero-charges", "terms", 33, 3, charges="zero", seed=401), Case("terms-empty-rules", "terms", 33, 3, table="empty", seed=402),
          Case("terms-no-grids", "terms", 33, 3, grids=False, seed=403)]
CASES += [Case("lds-stride256", "lds", 17, 16, kspec=("lds", 256), seed=501), Case("lds-stride257", "lds", 17, 16, kspec=("lds", 257), seed=501, refused=True)]
CASES += [Case("triangular-n33", "triangular", 33, 3, cell="triangular", seed=133)]
CASES += [Case("thresholds", "thresholds", 21, 1, kspec=("none",), table="thresholds", grids=False, seed=601)]
BY_NAME = {c.name: c for c in CASES}
COMPARED = [c.name for c in CASES if not c.refused and c.family != "thresholds"]
THRESHOLD_DELTAS = (1e-12, -1e-12, 2e-16, -2e-16, 0.0)


def _rotation(rng) -> np.ndarray:
    a, b, c, d = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _unit(rng) -> np.ndarray:
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


@functools.lru_cache(maxsize=None)
def sites(name: str) -> np.ndarray:
    """float64[n, m, 3] of a case: see the module docstring"""
    c = BY_NAME[name]
    if c.family == "thresholds":
        return _threshold_sites(c)
    rng = np.random.default_rng(c.seed)
    mat, kinds = c.mat, c.kinds
    _q, model = RC.molecule(c.m, 31 + c.m)
    inside = grid_set()[2]
    while True:
        shape = model @ _rotation(rng).T
        s0 = mat @ rng.random(3) + shape
        head = np.array([s0, s0 + 3.0 * _unit(rng), s0 + 5.0 * _unit(rng) + mat @ np.array([3.0, -2.0, 1.0]),
                         s0 + 0.4 * _unit(rng) + mat @ np.array([-1.0, 2.0, 0.0])])
        if not _blocked(head, kinds).any():
            break
    shape = model @ _rotation(rng).T
    s4 = inside[int(rng.integers(len(inside)))] - shape[0] + shape
    out = list(head) + [s4]
    while len(out) < c.n:
        cand = []
        for _ in range(c.n):
            f = rng.random(3)
            if (len(out) + len(cand)) % 2:
                f = f + rng.integers(-2, 3, 3)
            cand.append(mat @ f + model @ _rotation(rng).T)
        cand = np.array(cand)
        out += list(cand[~_blocked(cand, kinds)])
    return np.ascontiguousarray(np.array(out[:c.n]))


def _threshold_sites(c: Case) -> np.ndarray:
    """site 0 and, per threshold (cutoff^2, sphere^2) and delta, two sites at r^2 = threshold (1 + delta) from it, the second one moved
    by a lattice vector"""
    rng = np.random.default_rng(c.seed)
    mat = c.mat
    s0 = mat @ np.array([0.31, 0.52, 0.47])
    out = [s0]
    for t in (CUTOFF ** 2, SPHERE ** 2):
        for d in THRESHOLD_DELTAS:
            r = math.sqrt(t * (1.0 + d))
            out.append(s0 + r * _unit(rng))
            out.append(s0 + r * _unit(rng) + mat @ rng.integers(-2, 3, 3))
    assert len(out) == c.n
    return np.ascontiguousarray(np.array(out).reshape(c.n, 1, 3))


# ---------------------------------------------------------------------------------------------- the tile arithmetic
def launch_shape(n: int):
    """(n_pad, tiles, [(ti, tj) that write]) of ceg_site_tables_device, restated"""
    n_pad = (n + TILE - 1) // TILE * TILE
    tiles = n_pad // TILE
    return n_pad, tiles, [(ti, tj) for ti in range(tiles) for tj in range(tiles) if ti <= tj]


def compared_pairs(c: Case):
    """(I, J), I < J: every pair, or for n = 257 the subset of the module docstring"""
    n = c.n
    if n <= 64:
        I, J = np.triu_indices(n, 1)
        return I, J
    sel = set()
    edge = set(range(17)) | set(range(n - 17, n))
    for a in edge:
        sel |= {(min(a, b), max(a, b)) for b in range(n) if b != a}
    near = sorted({b for t in range(TILE, n, TILE) for b in range(t - 15, t + 16) if 0 <= b < n})
    for fixed in (40, 200):
        sel |= {(min(fixed, b), max(fixed, b)) for b in near if b != fixed}
    rng = np.random.default_rng(9)
    while len(sel) < len(edge) * n + 256:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            sel.add((min(a, b), max(a, b)))
    pairs = np.array(sorted(sel))
    return pairs[:, 0], pairs[:, 1]


# ---------------------------------------------------------------------------------------------- reference
def pair_r2(c: Case, pos, I, J) -> np.ndarray:
    """float64[npairs, m (atom of i), m (atom of j)]: ``literal_r2`` of pos_i - pos_j, the r^2 the rules are given"""
    m = c.m
    out = np.empty((len(I), m, m))
    for ai in range(m):
        for aj in range(m):
            out[:, ai, aj] = PR.literal_r2(c.mat, c.inv, pos[J, aj], pos[I, ai])
    return out


def pair_energies(c: Case, r2):
    """(P longdouble[npairs] (+inf where a sphere is overlapped), size longdouble[npairs]) from r2[npairs, m, m]"""
    t = table(c.table)
    kinds = c.kinds
    P, size = np.zeros(len(r2), dtype=LD), np.zeros(len(r2), dtype=LD)
    for ai in range(c.m):
        for aj in range(c.m):
            e = t.entry_of[int(kinds[aj])][int(kinds[ai])]
            if e is None:
                continue
            v, s = PR.entry_energy_ld(t, e, r2[:, ai, aj])
            P, size = P + v, size + s
    return P, size


def structure_factors(inv, k: RC.KSet, q, pos, dtype=LD):
    """(Re S, Im S)[n, nk] as ``recip_cases.reference`` forms them, in ``dtype``"""
    two_pi = RC.TWO_PI if dtype is LD else dtype(2.0 * np.pi)
    inv = np.asarray(inv, dtype=np.float64).reshape(3, 3).astype(dtype)
    q = np.asarray(q, dtype=np.float64).astype(dtype)
    p = np.asarray(pos, dtype=np.float64).reshape(-1, len(q), 3).astype(dtype)
    mm = np.asarray(k.ijk, dtype=np.int64).reshape(-1, 3).astype(dtype)
    f = p[..., 0, None] * inv[:, 0] + p[..., 1, None] * inv[:, 1] + p[..., 2, None] * inv[:, 2]
    f = f - np.rint(f)
    ph = f[..., None, 0] * mm[:, 0] + f[..., None, 1] * mm[:, 1] + f[..., None, 2] * mm[:, 2]
    ph = ph - np.rint(ph)
    ang = two_pi * ph
    return (np.cos(ang) * q[None, :, None]).sum(axis=1), (np.sin(ang) * q[None, :, None]).sum(axis=1)


def recip_from_sf(k: RC.KSet, sre, sim, dtype=LD):
    kf = k.kf.astype(dtype)
    fre, fim = k.sf.real.astype(dtype), k.sf.imag.astype(dtype)
    cross = (kf * (fre * sre + fim * sim)).sum(axis=-1)
    own = (kf * (sre * sre + sim * sim)).sum(axis=-1)
    return dtype(2) * (cross + dtype(ENC)) + (own + dtype(STATIC))


def pair_recip_from_sf(k: RC.KSet, sre, sim, I, J, dtype=LD, chunk=4096):
    kf = k.kf.astype(dtype)
    out = np.zeros(len(I), dtype=dtype)
    for b in range(0, len(I), chunk):
        i, j = I[b:b + chunk], J[b:b + chunk]
        out[b:b + chunk] = dtype(2) * (kf * (sre[i] * sre[j] + sim[i] * sim[j])).sum(axis=-1)
    return out


def sf_count(q) -> float:
    """C_S of the module docstring"""
    a = np.abs(np.asarray(q, dtype=np.float64))
    if a.sum() == 0.0:
        return 0.0
    return 14.4 + 1.42 * 2.0 * float(np.cumsum(a).sum() / a.sum())


def _phase(c: Case, pos) -> np.ndarray:
    """float64[n]: 2 pi sum_ax k_ax (3 F_ax + 0.5)"""
    F = np.einsum("xc,nac->nax", np.abs(c.inv), np.abs(pos)).max(axis=1)
    return 2.0 * np.pi * ((3.0 * F + 0.5) * np.asarray(c.k.ks, dtype=np.float64)).sum(axis=1)


def recip_bound(c: Case, pos) -> np.ndarray:
    k = c.k
    T = RC.magnitude(k.kf, k.sf, c.q, ENC, STATIC)
    if k.nk == 0:
        return np.full(len(pos), U * 2.0 * T)
    return U * (2.0 * (_phase(c, pos) + sf_count(c.q)) + 18.0 + math.ceil(k.nk / MC_THREADS)) * T


def pair_magnitude(c: Case) -> float:
    a = float(np.abs(c.q).sum())
    return float((2.0 * c.k.kf * a * a).sum())


def pair_recip_bound(c: Case, pos, I, J) -> np.ndarray:
    k = c.k
    if k.nk == 0:
        return np.zeros(len(I))
    F = np.einsum("xc,nac->nax", np.abs(c.inv), np.abs(pos)).max(axis=1)
    Fij = np.maximum(F[I], F[J])
    phase = 2.0 * np.pi * ((3.0 * Fij + 0.5) * np.asarray(k.ks, dtype=np.float64)).sum(axis=1)
    nk4 = (k.nk + 3) // 4 * 4
    return U * (2.0 * phase + 2.0 * nk4 + 2.0 * sf_count(c.q) + 2.0) * pair_magnitude(c)


@dataclass
class Expected:
    case: Case
    pos: np.ndarray
    recip: np.ndarray           # longdouble[n]
    recip_tol: np.ndarray
    grid: np.ndarray            # longdouble[n]: v0 + v1
    grid_T: np.ndarray
    blocked: np.ndarray         # bool[n]
    I: np.ndarray
    J: np.ndarray
    r2: np.ndarray              # float64[npairs, m, m]
    P: np.ndarray               # longdouble[npairs], +inf where hard
    P_size: np.ndarray
    R: np.ndarray               # longdouble[npairs]
    R_tol: np.ndarray
    sre: np.ndarray
    sim: np.ndarray

    @property
    def hard(self):
        return ~np.isfinite(self.P)

    @property
    def framework(self):
        return self.grid + self.recip

    @property
    def framework_tol(self):
        T = RC.magnitude(self.case.k.kf, self.case.k.sf, self.case.q, ENC, STATIC)
        return IC.bound(self.grid_T) + self.recip_tol + 4.0 * U * (self.grid_T + LD(T))

    @property
    def interactions(self):
        return (self.P + self.R) + LD(OFFSET_PAIR)

    @property
    def interactions_tol(self):
        return LD(1e-9) * self.P_size + self.R_tol + 4.0 * U * (self.P_size + LD(pair_magnitude(self.case)) + abs(OFFSET_PAIR))


@functools.lru_cache(maxsize=None)
def expected(name: str) -> Expected:
    c = BY_NAME[name]
    pos = sites(name)
    k = c.k
    recip = RC.reference(c.inv, k.ijk, k.kf, k.sf, c.q, pos, ENC, STATIC)
    v0, t0, blocked, v1, t1, nb1 = IC.column_reference(_grid_view(c.grids, c.kind_charge), [int(x) + 1 for x in c.kinds], pos)
    assert not nb1.any()
    I, J = compared_pairs(c)
    r2 = pair_r2(c, pos, I, J)
    P, size = pair_energies(c, r2)
    sre, sim = structure_factors(c.inv, k, c.q, pos)
    R = pair_recip_from_sf(k, sre, sim, I, J)
    return Expected(c, pos, recip, recip_bound(c, pos), v0 + v1, t0 + t1, blocked, I, J, r2, P, size, R, pair_recip_bound(c, pos, I, J), sre, sim)


def float64_evaluation(e: Expected):
    """(recip float64[n], R float64[npairs]): the same formulas evaluated by NumPy in float64"""
    c = e.case
    sre, sim = structure_factors(c.inv, c.k, c.q, e.pos, dtype=np.float64)
    return recip_from_sf(c.k, sre, sim, dtype=np.float64), pair_recip_from_sf(c.k, sre, sim, e.I, e.J, dtype=np.float64)


def _ratio(err, tol) -> float:
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(tol > 0, err / tol, np.where(err == 0, LD(0), LD(np.inf)))
    return float(q.max()) if len(q) else 0.0


def _worst(what, err, tol, got, ref, index):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(tol > 0, err / tol, np.where(err == 0, LD(0), LD(np.inf)))
    w = int(np.argmax(q))
    return f"{what}: worst element {index(w)}: got {float(got[w])!r}, reference {float(ref[w])!r}, error / bound = {float(q[w]):.4g}"


def compare(e: Expected, fw, rec, it) -> dict:
    """The one form of the check: every compared element within its tolerance, blocked and hard-sphere elements not below 1e90, the
    diagonal 1e100, [i][j] and [j][i] the same bytes.  -> {term: worst error / bound}; raises AssertionError naming the worst element"""
    c = e.case
    n = c.n
    fw, rec, it = np.asarray(fw, dtype=np.float64), np.asarray(rec, dtype=np.float64), np.asarray(it, dtype=np.float64).reshape(n, n)
    assert fw.shape == (n,) and rec.shape == (n,)
    assert (np.diag(it) == 1e100).all(), (c.name, "diagonal", np.nonzero(np.diag(it) != 1e100)[0][:8])
    assert it.tobytes() == np.ascontiguousarray(it.T).tobytes(), (c.name, "not symmetric bit for bit")
    out = {}
    err = np.abs(rec.astype(LD) - e.recip)
    out["recip"] = _ratio(err, e.recip_tol)
    assert (err <= e.recip_tol).all(), (c.name, _worst("recip", err, e.recip_tol, rec, e.recip, lambda w: w))
    assert np.array_equal(fw >= 1e90, e.blocked), (c.name, "blocked sites", np.nonzero((fw >= 1e90) != e.blocked)[0][:8])
    free = ~e.blocked
    err = np.abs(fw[free].astype(LD) - e.framework[free])
    out["framework"] = _ratio(err, e.framework_tol[free])
    assert (err <= e.framework_tol[free]).all(), (c.name, _worst("framework", err, e.framework_tol[free], fw[free], e.framework[free],
                                                                 lambda w: int(np.nonzero(free)[0][w])))
    got = it[e.I, e.J]
    hard = e.hard
    assert not (got[hard] < 1e90).any(), (c.name, "hard-sphere overlaps below 1e90", e.I[hard][got[hard] < 1e90][:8], e.J[hard][got[hard] < 1e90][:8])
    soft = ~hard
    assert np.isfinite(got[soft]).all(), (c.name, "not finite", e.I[soft][~np.isfinite(got[soft])][:8], e.J[soft][~np.isfinite(got[soft])][:8])
    err = np.abs(got[soft].astype(LD) - e.interactions[soft])
    tol = e.interactions_tol[soft]
    out["interactions"] = _ratio(err, tol)
    assert (err <= tol).all(), (c.name, _worst("interactions", err, tol, got[soft], e.interactions[soft],
                                               lambda w: (int(e.I[soft][w]), int(e.J[soft][w]))))
    # the pair term alone where the rule sum is small against it: the ratio to pair_recip_bound + the joins (reported, and asserted
    # above as part of the whole tolerance)
    small = soft & (np.asarray(e.P_size, dtype=np.float64) * 1e-9 < 0.01 * np.asarray(e.R_tol, dtype=np.float64))
    if small.any() and c.k.nk:
        errs = np.abs(it[e.I[small], e.J[small]].astype(LD) - e.interactions[small])
        out["pair-recip"] = _ratio(errs, e.interactions_tol[small])
    large = soft & (np.asarray(e.P_size, dtype=np.float64) * 1e-9 > 100.0 * np.asarray(e.R_tol, dtype=np.float64))
    if large.any():                                               # and the rule sums alone where they dominate
        errs = np.abs(it[e.I[large], e.J[large]].astype(LD) - e.interactions[large])
        out["pair-sum"] = _ratio(errs, e.interactions_tol[large])
    return out


def threshold_expected(c: Case) -> np.ndarray:
    """float64[n, n] of the case ``thresholds``, exactly: (P + 0) + OFFSET_PAIR with P in {+inf, -1.75, 0} by ``literal_r2``"""
    pos = sites(c.name)
    n = c.n
    s = 0.9 + 0.6
    out = np.full((n, n), 1e100)
    I, J = np.triu_indices(n, 1)
    r2 = pair_r2(c, pos, I, J)[:, 0, 0]
    P = np.where(r2 < CUTOFF ** 2, np.where(r2 < s * s, np.inf, 0.0) - 1.75, 0.0)
    out[I, J] = out[J, I] = P + OFFSET_PAIR
    return out


# ---------------------------------------------------------------------------------------------- the C ABI
class Device:
    """ceg_interp_create handles, ceg_mc_create and ceg_site_tables[_device] for a case"""

    def __init__(self, c: Case, lib=None):
        from ceg_hip.interp import GridInterpolator
        self.lib = lib or _abi.load_library()
        self.case = c
        nk = len(CHARGES)
        vdw, coul, _inside = grid_set()
        self.interp = [GridInterpolator(g) if (c.grids and g is not None) else None for g in vdw]
        self.coulomb = GridInterpolator(coul) if c.grids else None
        handles = (C.c_void_p * nk)(*[it._h if it is not None else None for it in self.interp])
        t = table(c.table)
        k = c.k
        charge = np.ascontiguousarray(c.kind_charge, dtype=np.float64)
        matT, invT = RC.colmajor(c.mat), RC.colmajor(c.inv)
        if k.nk:
            ijk = np.ascontiguousarray(k.ijk.reshape(-1), dtype=np.int32)
            re_, im_ = np.ascontiguousarray(k.sf.real), np.ascontiguousarray(k.sf.imag)
            kargs = (_abi.i32ptr(ijk), _abi.dptr(k.kf), _abi.dptr(re_), _abi.dptr(im_), k.nk, _abi.i32ptr(k.ks), _abi.dptr(invT))
        else:
            kargs = (None, None, None, None, 0, None, None)
        self._keep = (handles, charge, matT, invT, kargs, t)
        h = C.c_void_p()
        _abi.check(self.lib, self.lib.ceg_mc_create(C.byref(h), 0, handles, self.coulomb._h if self.coulomb is not None else None, _abi.dptr(charge), nk,
                                                    _abi.dptr(matT), _abi.dptr(invT), t.cutoff ** 2, t.rules.ctypes.data, _abi.i32ptr(t.offsets), COULOMBIC,
                                                    *kargs))
        self.h = h

    def tables(self, pos, with_recip=True, fill=np.nan):
        """ceg_site_tables -> (framework, recip or None, interactions, return code); the outputs hold ``fill`` beforehand"""
        c = self.case
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, c.m, 3)
        n = len(pos)
        fw, rec, it = np.full(n, fill), np.full(n, fill), np.full((n, n), fill)
        rc = self.lib.ceg_site_tables(self.h, _abi.i32ptr(c.kinds), c.m, _abi.dptr(pos.reshape(-1)), n, OFFSET_ONE, OFFSET_PAIR, _abi.dptr(fw),
                                      _abi.dptr(rec) if with_recip else None, _abi.dptr(it.reshape(-1)))
        return fw, (rec if with_recip else None), it, rc

    def tables_device(self, pos, fill=np.nan):
        """ceg_site_tables_device into torch tensors -> (framework, recip, interactions, return code) as NumPy arrays"""
        import torch
        c = self.case
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, c.m, 3)
        n = len(pos)
        fw, rec = (torch.full((n,), fill, dtype=torch.float64, device="cuda") for _ in range(2))
        it = torch.full((n, n), fill, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = self.lib.ceg_site_tables_device(self.h, _abi.i32ptr(c.kinds), c.m, _abi.dptr(pos.reshape(-1)), n, OFFSET_ONE, OFFSET_PAIR,
                                             C.c_void_p(fw.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(it.data_ptr()))
        torch.cuda.synchronize()
        return fw.cpu().numpy(), rec.cpu().numpy(), it.cpu().numpy(), rc

    def close(self) -> None:
        if self.h:
            self.lib.ceg_mc_destroy(self.h)
            self.h = None
        for it in self.interp + [self.coulomb]:
            if it is not None:
                it.close()
