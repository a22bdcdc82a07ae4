"""Synthetic cases, a high-precision reference and a derived error bound for ``ceg_energy_grid`` / ``ceg_energy_grid_reduced``
(csrc/ceg_egrid.hip) at the orientation counts and row lengths its callers use.  No tests here: ``tests/test_egrid_shape_cases_host.py``
checks this file on the CPU (the launch lists against the arithmetic of ``egrid_run``, the reference against the oracle, the bound
against a float64 evaluation of the factorised formula and against the tolerance of ``test_gpu_energy_grid._assert_matches``, the
claims of the reduction cases), ``tests/test_gpu_energy_grid_shapes.py`` runs the cases on the device.

Everything goes through the C ABI with synthetic inputs, so that every shape is a free choice: the cell of
``recip_cases.general_cell``, k-spaces of ``recip_cases.kset`` / ``with_constants``, grids of ``interp_cases`` behind
``GridInterpolator`` handles, molecules of ``recip_cases.molecule``, steps[a] = mat[:, a] / num[a], and orientations of
``hostmirror.lebedev.rotation_matrices`` on seeded random unit vectors: 43 = 1 x 43 (``islinear=True``: what the reference produces
for a linear symmetric guest at num_rotate = 40, the 86-point Lebedev grid halved), 70 = 5 x 14 (``islinear=False``: a non-linear
guest), 129 = the first 129 of 5 x 26, every other count a prefix of the 43-list (up to 43) or of the 70-list.

Reference of an element, in np.longdouble:  vdw + (direct + reciprocal).  The atom positions are formed in float64 in the operation
order of grids.jl:389 / :396 / :409 (``test_gpu_energy_grid._positions``); ``interp_cases.reference`` gives the grid terms at them,
``recip_cases.reference`` the reciprocal term.

Tolerance of an element:  ``interp_cases.bound`` of the summed T of the grid terms (|q_a| T for the Coulomb grid)  +  ``recip_bound``.
``recip_cases.bound`` was derived for k_recip, which takes the float64 positions and forms f = invmat r from them.  The kernels here
never form a position for the reciprocal term: the phase of (k-vector, atom, lattice point, rotation) is
    sum_axis frac(i_axis (k . g_axis))  +  sum_c frac(k_c frac(invmat R p)_c),          g_axis = invmat step_axis,
every product i d and k_c f_c formed exactly (``frac_of_product``).  Against the reference this differs, in units of 2^-53, by
  * the roundings of the reference's own float64 position, which the factorised form does not have: five in the offset
    (iA sA + iB sB) + iC sC and one in offset + R p (R p itself is the same float64 number in both):          6 X_c per coordinate
  * g_axis (three roundings of sum_j |invmat[c, j] step_j|) and d = k . g_axis (three more), times i_axis:     6 O_c
  * f = invmat (R p) (three roundings):                                                                         3 P_c
  * one rounding of at most 2^-54 in each of the six reduced products:                                          3
with O_c = |iA sA_c| + |iB sB_c| + |iC sC_c|, P_c = max over the atoms of sum_j |R_cj p_j|, X_c = O_c + P_c.  With F_c = sum_j
|invmat[c, j]| X_j (formed from the PARTS of the position: the offset and R p may cancel in the position itself) the phase is off
by at most 2^-53 (12 sum_c k_c F_c + 3) turns, 2 pi times that in the angle, and every term of E moves by that times its size (the
self term k_f |T_R|^2 by twice the error of T_R, whose phases lack the lattice part: 2 (1 + 3) <= 12).  Amplitudes: six sincos_2pi
(2 each), k_f conj(S_f) (1), five complex products (3 each), the charge sum of T_R (at most 16 fused multiply-adds), the three
operations that join the terms: 47; the self term carries the error of T_R twice and a block reduction: below 75.  The contraction
adds 2 nkp products to an accumulator one after the other inside the matrix instructions: at most 2 nkp roundings of the running
sum.  Hence
    recip_bound = 2^-53 (2 pi (12 sum_c k_c F_c + 3) + 2 nkp + 80) T,            T = recip_cases.magnitude, nkp = nk rounded up to 16,
a larger constant than recip_cases.bound's (3 F_c + 0.5 per axis, 32), derived from the operations of k_egrid_tables / k_egrid_T /
k_egrid_cross and from nothing the device returns.  Measured on the CPU (the host module prints them, per case): the float64
NumPy evaluation of the same factorised formula (``factorised_float64``: exact products through longdouble, numpy's cos / sin and
sums; not the code under test) stays within 0.018 of recip_bound (nk = 1; 0.009 to 0.010 at nk = 15 to 17; 0.0009 to 0.0056 with
114 and 316 k-vectors), and the whole tolerance is between 0.016 and 0.23 of ``_assert_matches``' 1e-9 (|vdw| + |direct| + |recip|) +
1e-11 max|recip| (0.23: 16 atoms; 0.03 to 0.09 on the nrot and numA tables); recip_bound is 2.3 to 9.2 times recip_cases.bound at
the same positions.

Compared elements (``subset``): cases of more than 8000 elements compare the first and last 16 points of
the row and 16 either side of every workgroup boundary (iA a multiple of 128) for every (iB, iC), at the first and last rotation
of every tile of 16, plus 64 random elements.  The reduction checks always use every point.

The exact case of the reduction.  The issue that asked for these tests proposed VdW grids holding one constant integer c, "every
free element 3c exactly".  That does not hold for c != 0: the Hermite weights 2t^3 - 3t^2 + 1 and -2t^3 + 3t^2 add up to 1 only to
rounding, and neither do the four products wx wy: evaluated in float64 as interp_point orders it, a grid of 7.0 misses 7.0 by one
to four units in the last place at a third of all points, a grid of 4.0 at a tenth (asserted in the host module; the reference's
COEFF X form is exact there, the Hermite form of the device is only within its bound), so the elements would differ in their last bits and neither ties nor "the mean of equal elements" would be exercised.  Two variants that
ARE exact take its place: ``zero`` -- three real VdW grid handles of zeros, no Coulomb grid, no k-space: every term is an exact zero,
3c = 0; ``constant`` -- no VdW grids, a Coulomb grid of zeros and a k-space without k-vectors: every free element is
2 energy_net_charges + static_contribution = 108.25 exactly, a non-zero constant (a mean formed without its ``min +`` would show).
Both carry a block mask of spheres (``interp_cases.sphere_case``, radii scaled) on the cell tric 15 x 13 x 11; the blocked set per
rotation comes from ``blocked_host`` (the operation order of blocked_at, coordinates.jl:83-101) and no atom lies within 1e-6 of a
rounding boundary of the mask index or of the wrap.  The molecule's first atom sits 0.25 A from the lattice point, so a lattice
point next to a blocked node is blocked at every rotation."""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ceg_hip import _abi, grids as G
from ceg_hip.hostmirror.lebedev import rotation_matrices

import interp_cases as IC
import recip_cases as RC
from test_gpu_energy_grid import _positions

LD = np.longdouble
KC, MAX_TILES, MAX_WAVES, RED_LANES = 16, 4, 8, 16          # restated from csrc/ceg_egrid.hip
CELL_INV = RC.general_cell()
CELL_MAT = np.linalg.inv(CELL_INV)
ENC, STATIC = -7.5, 123.25
BASE_KS = (5, 4, 3)
FULL_BELOW = 8000                                            # cases of at most this many elements are compared in full


# ---------------------------------------------------------------------------------------------- the launch arithmetic of egrid_run
def launches(nrot: int):
    """[(r0, NT)] of k_egrid_cross<NT> for one slab"""
    return [(r0, min(MAX_TILES, (nrot - r0 + 15) // 16)) for r0 in range(0, nrot, 16 * MAX_TILES)]


def row_shape(numA: int):
    """(waves per workgroup, grid.y)"""
    tiles = (numA + 15) // 16
    return min(MAX_WAVES, tiles), (tiles + MAX_WAVES - 1) // MAX_WAVES


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _rotation_lists():
    rng = np.random.default_rng(4370)
    u = rng.normal(size=(43 + 14 + 26, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return rotation_matrices(u[:43], True), rotation_matrices(u[43:57], False), rotation_matrices(u[57:], False)


def rotations(nrot: int) -> np.ndarray:
    lin, non, long_ = _rotation_lists()
    assert len(lin) == 43 and len(non) == 70 and len(long_) == 130
    src = lin if nrot <= 43 else (non if nrot <= 70 else long_)
    return np.ascontiguousarray(src[:nrot])


@dataclass(frozen=True)
class Case:
    name: str
    nrot: int
    num: Tuple[int, int, int]
    natoms: int = 3
    kset: tuple = ("half", BASE_KS, 1.0)          # ("half", ks, rho) | ("pick", ks, n): n k-vectors drawn from the half space | ("none",)
    coulomb: str = "zeros"                        # "zeros" | "random"
    vdw: tuple = ()                               # per atom: None or (cell, dims, seed); () = no VdW grid at all
    enc: float = 0.0
    static: float = 0.0
    launches: tuple = ()                          # what egrid_run must launch: ((r0, NT), ...)
    waves: int = 0
    grid_y: int = 0


def _case(name, nrot, num, expect_launches, expect_row, **kw) -> Case:
    return Case(name, nrot, tuple(num), launches=tuple(expect_launches), waves=expect_row[0], grid_y=expect_row[1], **kw)


# nrot -> the launch list, restated from egrid_run by hand
NROT_LAUNCHES = {15: [(0, 1)], 16: [(0, 1)], 17: [(0, 2)], 32: [(0, 2)], 33: [(0, 3)], 43: [(0, 3)], 48: [(0, 3)], 49: [(0, 4)],
                 64: [(0, 4)], 65: [(0, 4), (64, 1)], 70: [(0, 4), (64, 1)], 129: [(0, 4), (64, 4), (128, 1)]}
# numA -> (waves, grid.y)
NUMA_ROWS = {1: (1, 1), 16: (1, 1), 17: (2, 1), 128: (8, 1), 129: (8, 2), 145: (8, 2)}
NK_SETS = {0: ("none",), 1: ("pick", (3, 3, 3), 1), 15: ("pick", BASE_KS, 15), 16: ("pick", BASE_KS, 16), 17: ("pick", BASE_KS, 17),
           316: ("half", (7, 5, 4), 1.03)}

NROT_CASES = [_case(f"nrot{n}", n, (17, 3, 2), l, (2, 1)) for n, l in NROT_LAUNCHES.items()]
NUMA_CASES = [_case(f"numA{a}-nrot{n}", n, (a, 3, 2), NROT_LAUNCHES[n], NUMA_ROWS[a]) for n in (17, 65) for a in NUMA_ROWS]
NK_CASES = [_case(f"nk{nk}", 33, (17, 3, 2), [(0, 3)], (2, 1), kset=ks, enc=ENC if nk == 0 else 0.0, static=STATIC if nk == 0 else 0.0,
                  coulomb="random" if nk == 0 else "zeros") for nk, ks in NK_SETS.items()]
NATOMS_CASES = [_case(f"natoms{n}", 43, (17, 3, 2), [(0, 3)], (2, 1), natoms=n, enc=ENC, static=STATIC) for n in (1, 16)]
_COMPOSITE_VDW = (("ortho", (7, 5, 3), 71), None, ("tric", (15, 13, 11), 72))
COMPOSITE_CASES = [_case(f"composite-nrot{n}", n, (17, 3, 3), NROT_LAUNCHES[n], (2, 1), coulomb="random", vdw=_COMPOSITE_VDW, enc=ENC, static=STATIC)
                   for n in (43, 70)]
ELEMENT_CASES = NROT_CASES + NUMA_CASES + NK_CASES + NATOMS_CASES + COMPOSITE_CASES
BY_NAME = {c.name: c for c in ELEMENT_CASES}
assert len(BY_NAME) == len(ELEMENT_CASES)
COULOMB_DIMS = ("tric", (7, 5, 3))


@functools.lru_cache(maxsize=None)
def kset_of(spec) -> RC.KSet:
    if spec[0] == "none":
        return RC.with_constants((3, 3, 3), np.empty((0, 3)), 1)
    if spec[0] == "half":
        return RC.kset(spec[1], spec[2], seed=41)
    _kind, ks, n = spec
    full = RC.half_space(ks)
    pick = np.sort(np.random.default_rng(42 + n).choice(len(full), n, replace=False))
    return RC.with_constants(ks, full[pick], 43 + n)


@dataclass
class Inputs:
    case: Case
    k: RC.KSet
    q: np.ndarray
    base: np.ndarray
    rots: np.ndarray
    steps: list
    vdw: list                                     # EnergyGrid or None per atom
    coulomb: Optional[G.EnergyGrid]


def _steps(num):
    return [CELL_MAT[:, a] / num[a] for a in range(3)]


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> Inputs:
    c = BY_NAME[name]
    q, base = RC.molecule(c.natoms, 7 + c.natoms)
    vdw = [None] * c.natoms
    for a, spec in enumerate(c.vdw):
        if spec is not None:
            cs = IC.cset(spec[0], spec[1])
            vdw[a] = IC.energy_grid(cs, IC.random_data(cs, spec[2]), IC.VDW)
    cs = IC.cset(*COULOMB_DIMS)
    data = IC.random_data(cs, 73) if c.coulomb == "random" else np.zeros((8,) + tuple(cs.npoints), dtype=IC.F32)
    return Inputs(c, kset_of(c.kset), q, np.ascontiguousarray(base), rotations(c.nrot), _steps(c.num), vdw, IC.energy_grid(cs, data, IC.COULOMB))


# ---------------------------------------------------------------------------------------------- the compared elements
def subset(c: Case):
    """-> (r, iA, iB, iC) index arrays of the compared elements"""
    numA, numB, numC = c.num
    if c.nrot * numA * numB * numC <= FULL_BELOW:
        r, iA, iB, iC = np.meshgrid(np.arange(c.nrot), np.arange(numA), np.arange(numB), np.arange(numC), indexing="ij")
        return r.ravel(), iA.ravel(), iB.ravel(), iC.ravel()
    a_sel = set(range(min(16, numA))) | set(range(max(0, numA - 16), numA))
    for edge in range(16 * MAX_WAVES, numA, 16 * MAX_WAVES):
        a_sel |= set(range(edge - 16, min(edge + 16, numA)))
    r_sel = {0, c.nrot - 1}
    for t in range(0, c.nrot, 16):
        r_sel |= {t, min(t + 15, c.nrot - 1)}
    r, iA, iB, iC = np.meshgrid(sorted(r_sel), sorted(a_sel), np.arange(numB), np.arange(numC), indexing="ij")
    rng = np.random.default_rng(5)
    extra = [rng.integers(0, n, 64) for n in (c.nrot, numA, numB, numC)]
    flat = np.unique(np.concatenate([np.ravel_multi_index((r.ravel(), iA.ravel(), iB.ravel(), iC.ravel()), (c.nrot,) + c.num),
                                     np.ravel_multi_index(tuple(extra), (c.nrot,) + c.num)]))
    return np.unravel_index(flat, (c.nrot,) + c.num)


# ---------------------------------------------------------------------------------------------- reference and bound
def recip_bound(inp: Inputs, idx) -> np.ndarray:
    """see the module docstring"""
    r, iA, iB, iC = idx
    k = inp.k
    absI = np.abs(CELL_INV)
    O = sum(np.abs(i[:, None] * s[None, :]) for i, s in zip((iA, iB, iC), inp.steps))                        # [n, 3]
    P = np.einsum("rcj,aj->rac", np.abs(inp.rots), np.abs(inp.base)).max(axis=1)                             # [nrot, 3]
    F = (O + P[r]) @ absI.T                                                                                  # [n, c]
    nkp = (k.nk + KC - 1) // KC * KC
    kk = np.asarray(k.ks, dtype=np.float64)
    return 2.0 ** -53 * (2.0 * np.pi * (12.0 * (F * kk).sum(axis=1) + 3.0) + 2.0 * nkp + 80.0) * RC.magnitude(k.kf, k.sf, inp.q, inp.case.enc, inp.case.static)


@dataclass
class Expected:
    idx: tuple
    ref: np.ndarray               # longdouble[n]
    tol: np.ndarray               # float64[n]
    vdw: np.ndarray               # the three terms of the reference, longdouble[n]
    direct: np.ndarray
    recip: np.ndarray
    tol_recip: np.ndarray         # the part of tol that belongs to the reciprocal term
    pos: np.ndarray               # [n, natoms, 3]


def element_positions(inp: Inputs, idx) -> np.ndarray:
    pos = _positions(inp.base, inp.rots, inp.case.num, inp.steps)
    return np.ascontiguousarray(pos[idx])


def reference_terms(pos, vdw_grids, coulomb, q, invmat, k: RC.KSet, enc, static):
    """-> (vdw, direct, reciprocal, T of the grid terms), longdouble[n] each, of molecules at pos[n, natoms, 3]; ``coulomb`` None: a
    Coulomb grid of zeros (direct = 0 exactly)"""
    n = len(pos)
    vdw, direct, T = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for a in range(pos.shape[1]):
        if vdw_grids[a] is not None:
            value, t, _cell, blocked, skip = IC.reference(vdw_grids[a], pos[:, a])
            assert not blocked.any() and not skip.any()
            vdw += value
            T += t
        if coulomb is not None:
            value, t, _cell, blocked, skip = IC.reference(coulomb, pos[:, a])
            assert not blocked.any() and not skip.any()
            direct += LD(float(q[a])) * value
            T += abs(float(q[a])) * t
    return vdw, direct, RC.reference(invmat, k.ijk, k.kf, k.sf, q, pos, enc, static, chunk=64), T


@functools.lru_cache(maxsize=None)
def expected(name: str) -> Expected:
    """the reference and the tolerance of the compared elements of a case, computed once"""
    inp = inputs(name)
    c = inp.case
    idx = subset(c)
    pos = element_positions(inp, idx)
    vdw, direct, recip, T = reference_terms(pos, inp.vdw, inp.coulomb if c.coulomb != "zeros" else None, inp.q, CELL_INV, inp.k, c.enc, c.static)
    tol_recip = recip_bound(inp, idx)
    return Expected(idx, vdw + (direct + recip), IC.bound(T).astype(np.float64) + tol_recip, vdw, direct, recip, tol_recip, pos)


def _frac_exact(i, d):
    """frac_of_product of the kernels: i * d mod 1 with the product formed exactly (i holds at most 11 bits: exact in longdouble)"""
    p = np.asarray(i, dtype=LD) * np.asarray(d, dtype=LD)
    hi = p.astype(np.float64)
    lo = (p - hi.astype(LD)).astype(np.float64)
    return (hi - np.rint(hi)) + lo


def _expi(fr):
    ang = 2.0 * np.pi * fr
    return np.cos(ang) + 1j * np.sin(ang)


def factorised_float64(inp: Inputs) -> np.ndarray:
    """The reciprocal term of every element, float64[nrot, numA, numB, numC], by the factorised formula of csrc/ceg_egrid.hip in
    float64 NumPy: the yardstick of ``recip_bound``, not the code under test."""
    c, k = inp.case, inp.k
    m = k.ijk.astype(np.float64).reshape(-1, 3)
    tabs = []
    for ax in range(3):
        g = CELL_INV @ inp.steps[ax]
        d = m @ g
        tabs.append(_expi(_frac_exact(np.arange(c.num[ax], dtype=np.float64)[:, None], d[None, :])))
    tabs[2] = tabs[2] * (k.kf * np.conj(k.sf))[None, :]
    R, b = inp.rots, inp.base
    rp = (R[:, None, :, 0] * b[None, :, None, 0] + R[:, None, :, 1] * b[None, :, None, 1]) + R[:, None, :, 2] * b[None, :, None, 2]      # [nrot, a, 3]
    f = rp @ CELL_INV.T
    f = f - np.rint(f)
    e = np.ones(f.shape[:2] + (k.nk,), dtype=np.complex128)
    for ax in range(3):
        e = e * _expi(_frac_exact(m[None, None, :, ax], f[:, :, None, ax]))
    T = (inp.q[None, :, None] * e).sum(axis=1)                                                               # [nrot, nk]
    own = (k.kf[None, :] * (T.real ** 2 + T.imag ** 2)).sum(axis=1)
    W = tabs[0][:, None, None, :] * (tabs[1][None, :, None, :] * tabs[2][None, None, :, :])                  # [iA, iB, iC, nk]
    W = W.reshape(int(np.prod(c.num)), k.nk)
    cross = (W.real @ T.real.T - W.imag @ T.imag.T).T.reshape((c.nrot,) + c.num)
    return 2.0 * (cross + c.enc) + (own[:, None, None, None] + c.static)


def assert_matches_tolerance(e: Expected) -> np.ndarray:
    """the tolerance of test_gpu_energy_grid._assert_matches at the compared elements (its max|recip| over these elements only)"""
    vdw, direct, recip = (x.astype(np.float64) for x in (e.vdw, e.direct, e.recip))
    return 1e-9 * (np.abs(vdw) + np.abs(direct) + np.abs(recip)) + 1e-11 * np.abs(recip).max()


# ---------------------------------------------------------------------------------------------- the reduction cases
EXACT_NROT = (16, 17, 33, 70, 129)
EXACT_NUM = {16: (33, 5, 4), 17: (33, 5, 4), 33: (33, 5, 4), 70: (33, 3, 2), 129: (33, 3, 2)}          # fewer points at 70 and 129: see exact_blocked
EXACT_VALUE = {"zero": 0.0, "constant": 2.0 * ENC + STATIC}
BLOCK_CELL = ("tric", (15, 13, 11))
BLOCK_SPHERES, BLOCK_SEED, BLOCK_RADIUS_SCALE = 40, 3, 1.15
ATOM0 = np.array([0.11, -0.07, 0.05]) + 0.09          # the molecule's first atom, 0.25 A from the lattice point
EXACT_MOLECULE_SEED = 48                                  # seeds and offset chosen on the CPU for the claims the host module asserts


def exact_molecule():
    q, base = RC.molecule(3, EXACT_MOLECULE_SEED)
    return q, np.ascontiguousarray(base - base[0] + ATOM0)


@functools.lru_cache(maxsize=None)
def block_mask():
    """(csetup, mask uint8[nx, ny, nz]): nodes inside one of the spheres (minimum image over the 27 neighbouring cells, float64)"""
    cs = IC.cset(*BLOCK_CELL)
    centers, radius2 = IC.sphere_case(cs, BLOCK_SPHERES, BLOCK_SEED)
    radius2 = radius2 * BLOCK_RADIUS_SCALE ** 2
    nodes = IC.node_points(cs)
    mat = cs.cell.mat
    shifts = np.array([mat @ np.array(v, dtype=np.float64) for v in np.ndindex(3, 3, 3)]) - mat @ np.ones(3)
    mask = np.zeros(len(nodes), dtype=bool)
    for ctr, r2 in zip(centers, radius2):
        d = nodes[:, None, :] - ctr[None, None, :] + shifts[None, :, :]
        mask |= ((d * d).sum(axis=2) < r2).any(axis=1)
    return cs, np.ascontiguousarray(mask.reshape(tuple(cs.npoints)).astype(np.uint8))


def blocked_host(cs, mask, pts):
    """BlockFile getindex (coordinates.jl:83-101) for every row of pts, in the operation order of blocked_at -> (blocked bool[n],
    margin float64[n]: the distance of the point from the nearest rounding boundary -- of round(shifted) and of the floor in the
    wrap -- in the units of the rounded quantity)"""
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    I = cs.cell.invmat
    abc = (I[:, 0] * p[:, 0, None] + I[:, 1] * p[:, 1, None]) + I[:, 2] * p[:, 2, None]
    sh = IC.shifted(cs, p)
    i = np.clip(np.rint(sh).astype(np.int64) - 1, 0, np.asarray(cs.dims))
    margin = np.minimum(np.abs(np.abs(sh - np.rint(sh)) - 0.5).min(axis=1), np.abs(abc - np.rint(abc)).min(axis=1))
    return mask[i[:, 0], i[:, 1], i[:, 2]] != 0, margin


@functools.lru_cache(maxsize=None)
def exact_blocked(nrot: int):
    """-> (blocked bool[nrot, numA, numB, numC], smallest margin): an element is blocked when any of its atoms is"""
    cs, mask = block_mask()
    _q, base = exact_molecule()
    num = EXACT_NUM[nrot]
    pos = _positions(base, rotations(nrot), num, _steps(num))
    b, margin = blocked_host(cs, mask, pos.reshape(-1, 3))
    return b.reshape(pos.shape[:5]).any(axis=4), float(margin.min())


def first_free(blocked) -> np.ndarray:
    """int[numA, numB, numC]: the first rotation that is not blocked, nrot where none is"""
    free = ~blocked
    return np.where(free.any(axis=0), free.argmax(axis=0), blocked.shape[0])


def weights(nrot: int) -> np.ndarray:
    """positive, non-uniform, spanning a factor of 40 (as test_gpu_energy_grid_reduced._weights)"""
    return np.random.default_rng(590).uniform(0.05, 2.0, nrot)


def mean_bound(full, T, w):
    """-> (mirror mean, 1e-12 sum(f |x|)/sum(f)) over the first axis of ``full``: test_gpu_energy_grid_reduced._mean_bound restated for
    up to 129 orientations.  A term that is not flushed to zero has |(m - x)/T| <= 745, so the rounding of the argument moves f by at
    most 745 * 2^-53 = 8.3e-14 relative; the device's exp a few 2^-53 more; two sums of 129 non-negative terms, taken in another
    order on the device than in the mirror, at most 129 * 2^-53 = 1.4e-14 each on either side, 5.7e-14 in all (it was below 2e-14
    for the 64 the bound was first written for); the quotient and the products a few 2^-53.  Together below 1.5e-13: 1e-12 keeps a
    factor of six in hand where it had ten."""
    from ceg_hip.hostmirror.utils import mean_boltzmann
    shape = (slice(None),) + (None,) * (full.ndim - 1)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        m = full.min(axis=0) - 30.0 * T
        f = np.exp((m[None] - full) / T)
        if w is not None:
            f = f * np.asarray(w)[shape]
        return mean_boltzmann(full, T, w), 1e-12 * (f * np.abs(full)).sum(axis=0) / f.sum(axis=0)


def nan_case():
    """(vdw grids per atom with ONE NaN datum in the value channel of the first, charges, geometry, rotations, num): 17 rotations on
    17 x 3 x 2 points"""
    cs = IC.cset("ortho", (7, 5, 3))
    data = IC.random_data(cs, 81)
    data[0, 3, 2, 1] = np.nan
    q, base = RC.molecule(3, 10)
    return [IC.energy_grid(cs, data, IC.VDW), None, IC.energy_grid(cs, IC.random_data(cs, 82), IC.VDW)], q, np.ascontiguousarray(base), rotations(17), (17, 3, 2)


# ---------------------------------------------------------------------------------------------- the C ABI
class Device:
    """the handles of one call's grids and k-space, and the two entry points"""

    def __init__(self, lib, vdw, coulomb, k: Optional[RC.KSet], q, base, rots, num, enc=0.0, static=0.0, block=None):
        from ceg_hip.interp import GridInterpolator
        self.lib = lib
        self._open = []
        cache = {}

        def handle(eg):
            if eg is None:
                return None
            if id(eg) not in cache:
                cache[id(eg)] = GridInterpolator(eg)
                self._open.append(cache[id(eg)])
            return cache[id(eg)]._h
        self.natoms, self.nrot, self.num = len(base), len(rots), tuple(int(n) for n in num)
        self.handles = (C.c_void_p * self.natoms)(*[handle(g) for g in vdw])
        self.coulomb = handle(coulomb)
        self.recip = None
        if coulomb is not None:
            self.recip = RC.Handle(k, CELL_INV, lib)
            self._open.append(self.recip)
        self.q = np.ascontiguousarray(q, dtype=np.float64)
        self.base = np.ascontiguousarray(base, dtype=np.float64).reshape(-1)
        self.rot_cm = np.ascontiguousarray(np.asarray(rots, dtype=np.float64).transpose(0, 2, 1).reshape(-1))
        self.steps = np.ascontiguousarray(np.stack(_steps(self.num)).reshape(-1))
        self.numv = np.array(self.num, dtype=np.int32)
        self.enc, self.static = float(enc), float(static)
        self.block = None
        if block is not None:
            cs, mask = block
            self.block = (np.ascontiguousarray(mask, dtype=np.uint8), np.ascontiguousarray(cs.dims, dtype=np.int32),
                          np.ascontiguousarray(cs.size, dtype=np.float64), np.ascontiguousarray(cs.shift, dtype=np.float64),
                          G._matT(cs.cell.mat), G._matT(cs.cell.invmat))

    @classmethod
    def of_case(cls, lib, inp: Inputs):
        return cls(lib, inp.vdw, inp.coulomb, inp.k, inp.q, inp.base, inp.rots, inp.case.num, inp.case.enc, inp.case.static)

    @property
    def points(self) -> int:
        return int(np.prod(self.num))

    def _args(self):
        b = self.block
        bargs = (None,) * 6 if b is None else (b[0].ctypes.data, _abi.i32ptr(b[1]), _abi.dptr(b[2]), _abi.dptr(b[3]), _abi.dptr(b[4]), _abi.dptr(b[5]))
        return (self.handles, self.coulomb, self.recip.h if self.recip is not None else None, _abi.dptr(self.base), _abi.dptr(self.q), self.natoms,
                _abi.dptr(self.rot_cm), self.nrot, _abi.dptr(self.steps), _abi.i32ptr(self.numv), *bargs, self.enc, self.static)

    def lattice(self, flat, lead=()):
        """a flat output of the C ABI (iA fastest of the points, the leading axes slowest) -> [*lead, numA, numB, numC]"""
        numA, numB, numC = self.num
        n = len(lead)
        return flat.reshape(lead + (numC, numB, numA)).transpose(*range(n), n + 2, n + 1, n)

    def elements_array(self, flat):
        numA, numB, numC = self.num
        return flat.reshape(numC, numB, numA, self.nrot).transpose(3, 2, 1, 0)

    def elements(self, out_ptr: Optional[int] = None, stream: int = 0):
        """ceg_energy_grid -> float64[nrot, numA, numB, numC]; with ``out_ptr`` (device memory) asynchronous on ``stream``, nothing returned"""
        if out_ptr is not None:
            _abi.check(self.lib, self.lib.ceg_energy_grid(*self._args(), C.c_void_p(int(out_ptr)), 1, C.c_void_p(stream) if stream else None))
            return None
        out = np.full(self.nrot * self.points, np.nan)
        _abi.check(self.lib, self.lib.ceg_energy_grid(*self._args(), out.ctypes.data, 0, None))
        return self.elements_array(out)

    def reduced(self, temps=(), w=None, want_min=True, want_argmin=True, out_ptrs=None, stream: int = 0):
        """ceg_energy_grid_reduced -> (mean [ntemps, numA, numB, numC] or None, min or None, argmin or None); with ``out_ptrs`` =
        (mean, min, argmin) device addresses asynchronous on ``stream``, nothing returned"""
        t = np.ascontiguousarray(temps, dtype=np.float64).reshape(-1)
        nt = len(t)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        assert w is None or len(w) == self.nrot
        head = (*self._args(), _abi.dptr(t) if nt else None, nt, _abi.dptr(w) if w is not None else None)
        if out_ptrs is not None:
            pm, pn, pa = (C.c_void_p(int(p)) if p else None for p in out_ptrs)
            _abi.check(self.lib, self.lib.ceg_energy_grid_reduced(*head, pm, pn, pa, 1, C.c_void_p(stream) if stream else None))
            return None
        mean = np.full(nt * self.points, np.nan) if nt else None
        mn = np.full(self.points, np.nan) if want_min else None
        amin = np.full(self.points, -1, dtype=np.int32) if want_argmin else None
        _abi.check(self.lib, self.lib.ceg_energy_grid_reduced(*head, mean.ctypes.data if nt else None, mn.ctypes.data if want_min else None,
                                                              amin.ctypes.data if want_argmin else None, 0, None))
        return (self.lattice(mean, (nt,)) if nt else None, self.lattice(mn) if want_min else None, self.lattice(amin) if want_argmin else None)

    def close(self) -> None:
        for h in self._open:
            h.close()
        self._open = []
