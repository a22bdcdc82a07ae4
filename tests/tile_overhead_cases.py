"""Cases (pure CPU) for the bookkeeping of the grid kernel outside its pair loops -- tile box, row scan, flat index -> row, chunk
staging: ``cases()`` returns ``TCase`` records, ``run_case`` launches one on the device and returns every stored array by name.
``tests/perf/record_tile_overhead_golden.py`` records those arrays from a library (``CEG_HIP_LIB``) into
``tests/golden/tile_overhead/``; ``tests/test_gpu_tile_overhead.py`` compares the library under test with them bit for bit and
with the oracle; ``tests/test_tile_overhead_cases_host.py`` asserts on the CPU, through ``tile_walk`` -- a numpy mirror of
build_images (csrc/ceg_api.hip) and of the row pass of k_culled --, that the cases contain what they are meant to contain.

The grids are tiny on purpose: what can go wrong here depends on the shape of the grid and on the bin rows of a tile, not on size."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ceg_hip.hostmirror.coordinates import CellMatrix, GridCoordinatesSetup
from ceg_hip.hostmirror.utils import mat_from_parameters

from util import random_atoms, synthetic_probes
import uniform_cases as UC

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "tile_overhead"
A, B, C, D = 1, 2, 3, 4
ALPHA = UC.ALPHA
BIN_TARGET = (4.5, 4.5, 1.5)           # build_images: bin edges aimed at, A


def cset_with_points(mat, npoints) -> GridCoordinatesSetup:
    """workloads.grid_setup_with_dims without its odd-dims rule: any number of points per axis (the C ABI takes dims >= 1)"""
    cell = CellMatrix.from_mat(np.asarray(mat, dtype=np.float64))
    a, b, c = cell.mat[:, 0], cell.mat[:, 1], cell.mat[:, 2]
    size = np.abs(a) + np.abs(b) + np.abs(c)
    shift = np.minimum(a, 0.0) + np.minimum(b, 0.0) + np.minimum(c, 0.0)
    d = np.asarray(npoints, dtype=np.int32) - 1
    assert np.all(d >= 1)
    delta = size / d
    return GridCoordinatesSetup(cell, float(np.max(delta)), d, size, shift, np.array([np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)]), delta)


@dataclass
class TCase:
    name: str
    mat: np.ndarray
    pos: np.ndarray
    kinds: np.ndarray
    q: np.ndarray
    cutoff: float
    alpha: float
    npoints: tuple
    uniform: tuple | None              # tiny_forcefield(uniform=...); None: the force field with the Buckingham kind B
    launches: list                     # (mode, i_begin, i_end): mode fused / vdw / coulomb / multi; ("points", 0, 0): eval_points of both sums
    uniform_class: int = 0             # what the plan must report
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def slug(self) -> str:
        return self.name.replace("/", "_").replace(" ", "_")

    def cset(self):
        return cset_with_points(self.mat, self.npoints)

    def probes(self, probes=None):
        return synthetic_probes(self.mat, self.pos, self.kinds, self.q, cutoff=self.cutoff, probes=probes, uniform=self.uniform)

    def points(self) -> np.ndarray:
        """131 points inside the grid box: two full tiles of 64 and a partial one"""
        cs = self.cset()
        rng = np.random.default_rng(zlib.crc32(("pts/" + self.name).encode()))
        return np.asarray(cs.shift) + rng.uniform(0.02, 0.98, (131, 3)) * np.asarray(cs.size)

    def ref(self, oracle, what: str):
        if what not in self._cache:
            from ceg_hip import grids as G
            pv, pc = self.probes()
            if what == "vdw":
                r = oracle.grid_vdw(pv, self.cset(), *G.vdw_scaling())[0]
            elif what == "vdw_q":
                r = oracle.grid_vdw(self.probes((5, 6))[0][1], self.cset(), *G.vdw_scaling())[0]
            elif what == "coulomb":
                r = oracle.grid_coulomb(pc, self.alpha, self.cset(), *G.coulomb_scaling())[0]
            elif what == "points_vdw":
                r = oracle.points_vdw(pv, self.points())
            else:
                r = oracle.points_coulomb(pc, self.alpha, self.points())
            r.setflags(write=False)
            self._cache[what] = r
        return self._cache[what]


def _make(name, cell, npoints, launches, *, cls=1, cutoff=12.0, n=120, uniform=(*UC.AR_O, True), kinds_from=(A, D, C), mat=None, min_sep=1.6):
    if mat is None:
        mat = mat_from_parameters(*UC.CELLS[cell])
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pos = random_atoms(mat, n, rng, min_sep=min_sep)
    kinds = rng.choice(np.array(kinds_from), n)
    kinds[:len(kinds_from)] = kinds_from
    q = rng.uniform(-1.2, 1.9, n)
    if cls == 2:
        q[(kinds == A) | (kinds == D)] = -0.7
    return TCase(name, mat, pos, kinds.astype(np.int64), q, cutoff, ALPHA, tuple(npoints), uniform, list(launches),
                 cls if uniform is not None else 0)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    full = lambda npts: [("fused", 0, npts[0])]
    # 4n + 1, 4n + 2, 4n + 3 points on one axis at a time (the others full tiles), then on all three: partial tiles, clamped corner lanes
    for ax in range(3):
        for rem in (1, 2, 3):
            npts = [8, 8, 8]
            npts[ax] = 8 + rem
            out.append(_make(f"shape/{'xyz'[ax]}{8 + rem}", "orthorhombic", npts, full(npts)))
    out.append(_make("shape/9x10x11", "triclinic", (9, 10, 11), full((9, 10, 11)), cls=2))
    out.append(_make("shape/7x5x6", "triclinic", (7, 5, 6), full((7, 5, 6))))
    # fewer than 4 points on one axis
    out.append(_make("thin/3x8x9", "orthorhombic", (3, 8, 9), full((3, 8, 9))))
    out.append(_make("thin/8x2x9", "orthorhombic", (8, 2, 9), full((8, 2, 9)), cls=2))
    out.append(_make("thin/9x8x3", "orthorhombic", (9, 8, 3), full((9, 8, 3))))
    # x ranges: i_begin not a multiple of 4 with the output stored from plane i_begin, a one-plane slab; every code shape of a
    # uniform plan on them (13 x 9 x 10 points: 1 x 3 x 3 to 3 x 3 x 3 tiles -- the last workgroup of 4 or 8 waves is never full)
    ranges = [(3, 13), (5, 6), (2, 9)]
    for cls in (1, 2):
        out.append(_make(f"ranges/class{cls}", "skewed-mixed", (13, 9, 10),
                         [(m, b, e) for m in ("fused", "vdw", "coulomb") for b, e in ranges] + [("points", 0, 0)], cls=cls))
    # a handful of atoms in a large cell: most bin rows of a tile are empty, between non-empty ones
    big = mat_from_parameters((58.0, 61.0, 64.0), (90.0, 90.0, 90.0))
    out.append(_make("sparse/30-atoms", None, (11, 10, 9), [("fused", 0, 11), ("vdw", 0, 11), ("coulomb", 1, 10), ("points", 0, 0)],
                     n=30, mat=big, min_sep=6.0))
    # cutoffs on one cell: chunk boundaries fall at other places inside the rows
    for cutoff in (9.0, 10.5, 12.0):
        out.append(_make(f"cutoff/{cutoff:g}", "triclinic", (9, 6, 7), [("fused", 0, 9), ("coulomb", 0, 9)], cutoff=cutoff, cls=2, n=150))
    # the Buckingham kind B beside the Lennard-Jones kinds: the tabulated / per-candidate classes
    out.append(_make("buckingham", "triclinic", (9, 6, 7), [("fused", 0, 9), ("vdw", 2, 9), ("points", 0, 0)], uniform=None,
                     kinds_from=(A, B, C, D)))
    # P and Q in one multi-probe plan (Q: Lennard-Jones with A, nothing with C)
    out.append(_make("multi", "skewed-mixed", (9, 6, 7), [("multi", 0, 9), ("multi", 3, 8)], kinds_from=(A, C)))
    _CASES = out
    return out


def dense21():
    """The 21 A case of tests/uniform_cases.py (900 atoms, 8 x 10 x 6 points): more than 64 bin rows per tile, many chunks"""
    c = next(c for c in UC.named_cases() if c.name == "cutoff21/class1")
    t = TCase("dense21", c.mat, c.pos, c.kinds, c.q, c.cutoff, c.alpha, tuple(d + 1 for d in c.dims), c.uniform,
              [("fused", 0, 8), ("vdw", 1, 6), ("coulomb", 0, 8)], 1)
    return t


def all_cases():
    return cases() + [dense21()]


# ------------------------------------------------------------------ device side (used by the recorder and by the GPU test)
def run_case(case, monkeypatch_env=None) -> dict:
    """Every launch of `case` on the library that is loaded: name -> float32 [8, e - b, ny, nz] grids / float64 [n, 8] raw sums"""
    import torch
    from ceg_hip import _abi
    from ceg_hip.plan import GridPlan, MultiGridPlan
    CULLED = _abi.ALGO_CULLED
    cs = case.cset()
    nx, ny, nz = cs.npoints
    out = {}
    multi = any(m == "multi" for m, _, _ in case.launches)
    if multi:
        pvs, pc = case.probes((5, 6))
        plan = MultiGridPlan(cs, pvs, pc, case.alpha)
    else:
        pv, pc = case.probes()
        plan = GridPlan(cs, pv, pc, case.alpha)
    try:
        assert plan.can_cull if hasattr(plan, "can_cull") else True
        assert plan.uniform_class == case.uniform_class, (case.name, plan.uniform_class)
        for mode, b, e in case.launches:
            if mode == "points":
                pts = case.points()
                out["points/vdw"] = plan.eval_points("vdw", pts, CULLED)
                out["points/coulomb"] = plan.eval_points("coulomb", pts, CULLED)
                continue
            m = e - b
            new = lambda: torch.full((8, m, ny, nz), float("nan"), dtype=torch.float32, device="cuda")
            tag = f"{mode}[{b},{e})"
            if mode == "fused":
                v, c = new(), new()
                plan.build_fused(v.data_ptr(), c.data_ptr(), m * ny * nz, b, e, b, CULLED)
                res = {"vdw": v, "coulomb": c}
            elif mode == "vdw":
                v = new()
                plan.build_vdw(v.data_ptr(), m * ny * nz, b, e, b, CULLED)
                res = {"vdw": v}
            elif mode == "coulomb":
                c = new()
                plan.build_coulomb(c.data_ptr(), m * ny * nz, b, e, b, CULLED)
                res = {"coulomb": c}
            else:
                v, w, c = new(), new(), new()
                plan.build([v.data_ptr(), w.data_ptr()], c.data_ptr(), m * ny * nz, b, e, b)
                res = {"vdw": v, "vdw_q": w, "coulomb": c}
            torch.cuda.synchronize()
            for k, t in res.items():
                out[f"{tag}/{k}"] = t.cpu().numpy()
    finally:
        plan.close()
    return out


# ------------------------------------------------------------------ host mirror of the image bins and of the row pass
def image_bins(case):
    """build_images (csrc/ceg_api.hip) in numpy: (lo, bin, nb, bin_start) of the lattice images in the grid box grown by the cutoff"""
    cs = case.cset()
    margin = case.cutoff * (1.0 + 1e-6) + 1e-6
    lo = np.asarray(cs.shift) - margin
    hi = np.asarray(cs.shift) + np.asarray(cs.size) + margin
    nb = np.maximum(1, np.floor((hi - lo) / np.array(BIN_TARGET)).astype(int))
    binw = (hi - lo) / nb
    sh = np.array([(a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)], dtype=np.float64)
    P = (case.pos[None, :, :] + (sh @ np.asarray(case.mat).T)[:, None, :]).reshape(-1, 3)
    P = P[np.all((P >= lo) & (P <= hi), axis=1)]
    b = np.clip(np.floor((P - lo) / binw).astype(int), 0, nb - 1)
    key = (b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]
    return lo, binw, nb, np.searchsorted(np.sort(key), np.arange(nb.prod() + 1))


def tile_walk(case, b, e):
    """Per tile of the launch on planes [b, e): the image counts of its bin rows, in the order the kernel's lanes own them
    (one list per row pass of 64 rows).  -> list of lists of int arrays"""
    cs = case.cset()
    lo, binw, nb, start = image_bins(case)
    npts = np.array(cs.npoints)
    rc2 = case.cutoff ** 2 * (1.0 + 1e-9) + 1e-9
    rc = np.sqrt(rc2)
    binof = lambda x, ax: int(min(nb[ax] - 1, max(0, np.floor((x - lo[ax]) / binw[ax]))))
    coord = lambda idx: np.asarray(idx) * np.asarray(cs.size) / np.asarray(cs.dims) + np.asarray(cs.shift)
    tiles = []
    for i0 in range(b, e, 4):
        for j0 in range(0, npts[1], 4):
            for k0 in range(0, npts[2], 4):
                last = np.array([e - 1, npts[1] - 1, npts[2] - 1])
                blo, bhi = coord([i0, j0, k0]), coord(np.minimum(np.array([i0, j0, k0]) + 3, last))
                bx0, bx1 = binof(blo[0] - rc, 0), binof(bhi[0] + rc, 0)
                by0, by1 = binof(blo[1] - rc, 1), binof(bhi[1] + rc, 1)
                counts = []
                for bx in range(bx0, bx1 + 1):
                    for by in range(by0, by1 + 1):
                        x0, y0 = lo[0] + bx * binw[0], lo[1] + by * binw[1]
                        gx = max(0.0, blo[0] - (x0 + binw[0]), x0 - bhi[0])
                        gy = max(0.0, blo[1] - (y0 + binw[1]), y0 - bhi[1])
                        d2 = gx * gx + gy * gy
                        cnt = 0
                        if d2 < rc2:
                            zr = np.sqrt(rc2 - d2)
                            rb = (bx * nb[1] + by) * nb[2]
                            cnt = int(start[rb + binof(bhi[2] + zr, 2) + 1] - start[rb + binof(blo[2] - zr, 2)])
                        counts.append(cnt)
                counts = np.array(counts)
                tiles.append([counts[r:r + 64] for r in range(0, len(counts), 64)])
    return tiles


def walk_stats(case):
    """What the launches of `case` contain, over all tiles: most rows in a tile, and whether some row pass has an empty row between
    non-empty ones / a non-empty row right after an empty one at a chunk start / a row straddling a chunk boundary; chunks per tile"""
    if "walk" in case._cache:
        return case._cache["walk"]
    st = case._cache["walk"] = dict(max_rows=0, empty_between=False, straddle=False, start_on_boundary=False, max_chunks=0, tiles=[])
    for mode, b, e in case.launches:
        if mode == "points":
            continue
        tiles = tile_walk(case, b, e)
        st["tiles"].append(len(tiles))
        for passes in tiles:
            st["max_rows"] = max(st["max_rows"], sum(len(p) for p in passes))
            chunks = 0
            for cnt in passes:
                nz = np.flatnonzero(cnt)
                if len(nz) >= 2 and np.any(cnt[nz[0]:nz[-1]] == 0):
                    st["empty_between"] = True
                incl = np.cumsum(cnt)
                excl = incl - cnt
                total = int(incl[-1]) if len(incl) else 0
                chunks += (total + 63) // 64
                for cb in range(64, total, 64):
                    if np.any((excl < cb) & (incl > cb)):
                        st["straddle"] = True
                    if np.any((excl == cb) & (cnt > 0)):
                        st["start_on_boundary"] = True
            st["max_chunks"] = max(st["max_chunks"], chunks)
    return st
