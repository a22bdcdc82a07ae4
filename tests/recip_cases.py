"""Synthetic k-spaces, a high-precision reference and a derived error bound for the reciprocal Ewald kernel (k_recip,
csrc/ceg_recip.hip).  No tests here: ``tests/test_recip_cases_host.py`` checks this file on the CPU (the reference against mpmath
and the oracle, the case table against ``ceg_recip_launch_shape``), ``tests/test_gpu_recip_shapes.py`` runs the cases on the device.

The k-spaces are built from integers and handed to the C ABI directly, which decouples what the fixtures tie together: the table
stride (kx + 1) + (2 ky + 1) + (2 kz + 1), the number of k-vectors and the number of atoms -- the three inputs of the choice among
the eight k_recip<C_IN_LDS, WAVES> instantiations and the placements a wave walks (``per_wave``).

Matrices: ``invmat`` is the 3 x 3 matrix M of f = M r (row = fractional axis); the C ABI takes it column-major (``colmajor``)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ceg_hip import _abi

LD = np.longdouble
TWO_PI = LD("6.283185307179586476925286766559005768394")
LDS_STATIC = 8 * 48 * 8 + 16 * 8          # s_pos[8][48] + s_q[16] of k_recip: 3200 bytes beside the dynamic LDS


@dataclass
class KSet:
    ks: np.ndarray          # int32[3]
    ijk: np.ndarray         # int32[nk, 3]
    kf: np.ndarray          # float64[nk], > 0
    sf: np.ndarray          # complex128[nk]

    @property
    def nk(self) -> int:
        return len(self.kf)

    @property
    def stride(self) -> int:
        return int(self.ks[0] + 1 + 2 * self.ks[1] + 1 + 2 * self.ks[2] + 1)

    def take(self, idx) -> "KSet":
        idx = np.asarray(idx)
        return KSet(self.ks, np.ascontiguousarray(self.ijk[idx]), np.ascontiguousarray(self.kf[idx]), np.ascontiguousarray(self.sf[idx]))


def constants(nk: int, rng):
    """kf > 0 over three decades; sf complex normal(0, 30) with a tenth of the entries exactly zero."""
    kf = 10.0 ** rng.uniform(-3.0, 0.0, nk)
    sf = rng.normal(0.0, 30.0, nk) + 1j * rng.normal(0.0, 30.0, nk)
    sf[rng.random(nk) < 0.1] = 0.0
    return kf, sf


def with_constants(ks, ijk, seed) -> KSet:
    ijk = np.ascontiguousarray(np.asarray(ijk, dtype=np.int32).reshape(-1, 3))
    kf, sf = constants(len(ijk), np.random.default_rng(seed))
    return KSet(np.asarray(ks, dtype=np.int32), ijk, kf, sf)


def half_space(ks, rho=1.0) -> np.ndarray:
    """The integer half-space ellipsoid (i/kx)^2 + (j/ky)^2 + (k/kz)^2 <= rho^2 with i > 0 or (i == 0 and (j > 0 or (j == 0 and
    k > 0))), inside the box; an axis with ks = 0 contributes index 0 only.  Sorted by row: (j, k) then i."""
    kx, ky, kz = (int(x) for x in ks)
    i, j, k = np.meshgrid(np.arange(0, kx + 1), np.arange(-ky, ky + 1), np.arange(-kz, kz + 1), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    r2 = np.zeros(len(i))
    for v, m in ((i, kx), (j, ky), (k, kz)):
        if m > 0:
            r2 += (v / m) ** 2
    keep = (r2 <= rho * rho * (1 + 1e-12)) & ((i > 0) | ((i == 0) & ((j > 0) | ((j == 0) & (k > 0)))))
    ijk = np.stack([i[keep], j[keep], k[keep]], axis=1)
    order = np.lexsort((ijk[:, 0], ijk[:, 2], ijk[:, 1]))
    return ijk[order].astype(np.int32)


def kset(ks, rho=1.0, holes=0, dups=0, shuffle=False, seed=0) -> KSet:
    """``half_space(ks, rho)`` with ``holes`` interior entries of rows deleted (an entry whose two neighbours along i stay), ``dups``
    entries repeated (each copy with constants of its own) and, with ``shuffle``, the list in random order."""
    rng = np.random.default_rng(seed)
    ijk = half_space(ks, rho)
    if holes:
        have = {tuple(v) for v in ijk}
        interior = [q for q, (i, j, k) in enumerate(ijk) if (i - 1, j, k) in have and (i + 1, j, k) in have]
        gone, blocked = [], set()
        for q in rng.permutation(interior):
            t = tuple(ijk[q])
            if t in blocked:
                continue
            gone.append(q)
            blocked |= {(t[0] - 1, t[1], t[2]), (t[0] + 1, t[1], t[2])}          # the neighbours of a hole stay
            if len(gone) == holes:
                break
        assert len(gone) == holes, "not enough interior entries for the holes"
        ijk = np.delete(ijk, gone, axis=0)
    if dups:
        ijk = np.concatenate([ijk, ijk[rng.choice(len(ijk), dups, replace=True)]])
    if shuffle:
        ijk = ijk[rng.permutation(len(ijk))]
    kf, sf = constants(len(ijk), rng)
    return KSet(np.asarray(ks, dtype=np.int32), np.ascontiguousarray(ijk, dtype=np.int32), kf, sf)


# ---------------------------------------------------------------------------------------------- reference and bound
def reference(invmat, ijk, kf, sf, q, pos, enc, static, chunk=16) -> np.ndarray:
    """E = 2 (sum_k kf Re(conj(sf) S) + enc) + (sum_k kf |S|^2 + static), S(k) = sum_a q_a exp(2 pi i k.f_a), f = invmat r, in
    np.longdouble (64-bit mantissa): f reduced by rint, the phase k.f reduced by rint again, one cos / sin per (atom, k-vector).
    pos [n, natoms, 3] -> longdouble[n]."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 here"
    inv = np.asarray(invmat, dtype=np.float64).reshape(3, 3).astype(LD)
    q = np.asarray(q, dtype=np.float64).astype(LD)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, len(q), 3)
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    kfl = np.asarray(kf, dtype=np.float64).astype(LD)
    sre, sim = np.asarray(sf).real.astype(LD), np.asarray(sf).imag.astype(LD)
    enc, static = LD(enc), LD(static)
    out = np.empty(len(pos), dtype=LD)
    m = ijk.astype(LD)
    for b in range(0, len(pos), chunk):
        p = pos[b:b + chunk].astype(LD)
        f = p[..., 0, None] * inv[:, 0] + p[..., 1, None] * inv[:, 1] + p[..., 2, None] * inv[:, 2]          # [n, a, ax]
        f = f - np.rint(f)
        ph = f[..., None, 0] * m[:, 0] + f[..., None, 1] * m[:, 1] + f[..., None, 2] * m[:, 2]                # [n, a, nk]
        ph = ph - np.rint(ph)
        ang = TWO_PI * ph
        s_re = (np.cos(ang) * q[None, :, None]).sum(axis=1)
        s_im = (np.sin(ang) * q[None, :, None]).sum(axis=1)
        cross = (kfl * (sre * s_re + sim * s_im)).sum(axis=-1)
        own = (kfl * (s_re * s_re + s_im * s_im)).sum(axis=-1)
        out[b:b + chunk] = LD(2) * (cross + enc) + (own + static)
    return out


def magnitude(kf, sf, q, enc, static) -> float:
    """T = sum_k kf (2 |sf_k| A + A^2) + |2 enc| + |static| with A = sum |q|: the sum of the absolute values of the terms of E."""
    a = float(np.abs(q).sum())
    return float((np.asarray(kf) * (2.0 * np.abs(sf) * a + a * a)).sum()) + abs(2.0 * enc) + abs(static)


def bound(invmat, ks, kf, sf, q, pos, enc, static) -> np.ndarray:
    """The tolerance of a float64 evaluation, per placement: 2^-53 (2 pi sum_ax k_ax (3 F_ax + 0.5) + 32) T.
    F_ax = max over the atoms of sum_c |invmat[ax, c] r_c| -- the three products and sums that form f each round at that size, and
    an error of f is multiplied by up to 2 pi k_ax in the angle; 0.5 for the rounding of m ff; 32 for sincos, the two complex
    products, at most 9 recurrence steps and the reductions.  Nothing in it is fitted to what the kernel returns."""
    inv = np.abs(np.asarray(invmat, dtype=np.float64).reshape(3, 3))
    pos = np.abs(np.asarray(pos, dtype=np.float64).reshape(-1, len(q), 3))
    F = np.einsum("xc,nac->nax", inv, pos).max(axis=1)                                        # [n, ax]
    k = np.asarray(ks, dtype=np.float64)
    return 2.0 ** -53 * (2.0 * np.pi * ((3.0 * F + 0.5) * k).sum(axis=1) + 32.0) * magnitude(kf, sf, q, enc, static)


# ---------------------------------------------------------------------------------------------- the C ABI
def colmajor(invmat) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(invmat, dtype=np.float64).reshape(3, 3).T.reshape(-1))


def _ijkptr(k: KSet):
    return _abi.i32ptr(np.ascontiguousarray(k.ijk.reshape(-1))) if k.nk else None


def launch_shape(k: KSet, natoms: int, n: int, lib=None):
    """ceg_recip_launch_shape -> (waves, c_in_lds, per_wave, dynamic LDS bytes); raises _abi.CegError on a refusal."""
    lib = lib or _abi.load_library()
    out = np.zeros(4, dtype=np.int32)
    _abi.check(lib, lib.ceg_recip_launch_shape(_ijkptr(k), k.nk, _abi.i32ptr(k.ks), natoms, n, _abi.i32ptr(out)))
    return int(out[0]), bool(out[1]), int(out[2]), int(out[3])


def layout(k: KSet, lib=None):
    """ceg_recip_layout -> (nrounds, nslots, number of segments = (round, lane) pairs that hold a k-vector)."""
    lib = lib or _abi.load_library()
    nr, ns = C.c_int32(), C.c_int32()
    slot = np.zeros(max(k.nk, 1), dtype=np.int64)
    _abi.check(lib, lib.ceg_recip_layout(_ijkptr(k), k.nk, _abi.i32ptr(k.ks), C.byref(nr), C.byref(ns), None, None))
    desc = np.zeros(max(nr.value * 64, 1), dtype=np.int32)
    _abi.check(lib, lib.ceg_recip_layout(_ijkptr(k), k.nk, _abi.i32ptr(k.ks), C.byref(nr), C.byref(ns), slot.ctypes.data, desc.ctypes.data))
    if k.nk == 0:
        return 0, 0, 0
    L = (desc[:nr.value * 64] >> 27).reshape(nr.value, 64)[:, 0]
    first = np.concatenate([[0], np.cumsum(L)])
    rnd = np.searchsorted(first, slot // 64, side="right") - 1
    return nr.value, ns.value, len(np.unique(rnd * 64 + slot % 64))


SEGMENT_KS = (2, 7, 7)          # rows of at most three k-vectors: see trimmed_to_segments


def trimmed_to_segments(k: KSet, nseg: int) -> KSet:
    """The shortest prefix of ``k`` (row order) that ceg_recip_layout cuts into exactly ``nseg`` segments.  With rows longer than
    three k-vectors there may be none: the layout chooses its segment length by cost and steps around a last round that holds a
    single segment; rows of at most three k-vectors are one segment each whatever it chooses."""
    for m in range(nseg, k.nk + 1):
        t = k.take(np.arange(m))
        if layout(t)[2] == nseg:
            return t
    raise AssertionError(f"no prefix with {nseg} segments")


class Handle:
    """ceg_recip_create / _energy / _destroy for a KSet and a cell."""

    def __init__(self, k: KSet, invmat, lib=None):
        self.lib = lib or _abi.load_library()
        self.k, self.invmat = k, np.asarray(invmat, dtype=np.float64).reshape(3, 3)
        re_, im_ = np.ascontiguousarray(k.sf.real), np.ascontiguousarray(k.sf.imag)
        h = C.c_void_p()
        _abi.check(self.lib, self.lib.ceg_recip_create(C.byref(h), 0, _ijkptr(k), _abi.dptr(k.kf) if k.nk else None, _abi.dptr(re_) if k.nk else None,
                                                       _abi.dptr(im_) if k.nk else None, k.nk, _abi.i32ptr(k.ks), _abi.dptr(colmajor(invmat))))
        self.h = h

    def energies(self, q, pos, enc=0.0, static=0.0) -> np.ndarray:
        q = np.ascontiguousarray(q, dtype=np.float64)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, len(q), 3)
        out = np.full(len(pos), np.nan)
        _abi.check(self.lib, self.lib.ceg_recip_energy(self.h, _abi.dptr(pos.reshape(-1)), _abi.dptr(q), len(q), len(pos), enc, static, _abi.dptr(out)))
        return out

    def energies_chunked(self, q, pos, chunk, enc=0.0, static=0.0) -> np.ndarray:
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, len(q), 3)
        return np.concatenate([self.energies(q, pos[b:b + chunk], enc, static) for b in range(0, len(pos), chunk)])

    def energies_device(self, q, d_pos: int, n: int, d_out: int, enc=0.0, static=0.0, stream: int = 0) -> None:
        q = np.ascontiguousarray(q, dtype=np.float64)
        _abi.check(self.lib, self.lib.ceg_recip_energy_device(self.h, C.c_void_p(d_pos), _abi.dptr(q), len(q), n, enc, static, C.c_void_p(d_out),
                                                              C.c_void_p(stream) if stream else None))

    def set_structure_factor(self, sf) -> None:
        re_, im_ = np.ascontiguousarray(np.asarray(sf).real), np.ascontiguousarray(np.asarray(sf).imag)
        _abi.check(self.lib, self.lib.ceg_recip_set_structure_factor(self.h, _abi.dptr(re_), _abi.dptr(im_)))

    def reference(self, q, pos, enc=0.0, static=0.0, sf=None):
        k = self.k
        return reference(self.invmat, k.ijk, k.kf, k.sf if sf is None else sf, q, pos, enc, static)

    def bound(self, q, pos, enc=0.0, static=0.0, sf=None):
        k = self.k
        return bound(self.invmat, k.ks, k.kf, k.sf if sf is None else sf, q, pos, enc, static)

    def close(self) -> None:
        if self.h:
            self.lib.ceg_recip_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------- geometry and molecules
def general_cell() -> np.ndarray:
    """invmat of a triclinic cell (27, 31, 36 A; 77, 104, 95 degrees) turned by a rotation about (1, 2, 3): all nine entries of the
    matrix and of its inverse are non-zero."""
    from ceg_hip.hostmirror.utils import mat_from_parameters
    mat = np.asarray(mat_from_parameters((27.0, 31.0, 36.0), (77.0, 104.0, 95.0)), dtype=np.float64)
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = 0.7
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    inv = np.linalg.inv(R @ mat)
    assert np.all(np.abs(inv) > 1e-4) and np.all(np.abs(R @ mat) > 1e-2)
    return inv


def molecule(natoms: int, seed: int):
    """(charges [natoms] of order 1 e, model geometry [natoms, 3] within +-3 A)."""
    rng = np.random.default_rng(1000 + seed)
    return rng.uniform(-1.2, 1.2, natoms), rng.uniform(-3.0, 3.0, (natoms, 3))


def placements(model, n: int, seed: int, spread=60.0) -> np.ndarray:
    rng = np.random.default_rng(2000 + seed)
    return rng.uniform(-spread, spread, (n, 1, 3)) + np.asarray(model)[None]


# ---------------------------------------------------------------------------------------------- the variant matrix
# name -> (ks, rho, natoms, (c_in_lds, waves)): every k_recip<C_IN_LDS, WAVES>.  tests/test_recip_cases_host.py asserts, through
# ceg_recip_launch_shape, that each row selects the variant it names.
VARIANTS = {
    "lds-8": ((8, 8, 8), 1.0, 3, (True, 8)),            # stride 43
    "lds-4": ((8, 8, 8), 1.0, 8, (True, 4)),            # 8 x 8 x 43 table entries per workgroup would pass 40 KiB
    "lds-2": ((8, 8, 8), 1.0, 16, (True, 2)),
    "lds-1": ((18, 18, 18), 0.45, 16, (True, 1)),       # stride 93: 23.8 KB of tables, the constants of the small set beside them
    "global-8": ((18, 18, 18), 1.0, 3, (False, 8)),     # about 12 000 k-vectors: 290 KB of constants stay in global memory
    "global-4": ((18, 18, 18), 0.62, 6, (False, 4)),    # about 2 900 k-vectors: still 70 KB of constants, and a reference of 64
    "global-2": ((18, 18, 18), 0.62, 12, (False, 2)),   # placements x 16 atoms that takes 1.5 s instead of 6.5 s
    "global-1": ((18, 18, 18), 0.62, 16, (False, 1)),
}
N_RAGGED = 517                                           # per_wave = 1 in every variant, the last workgroup ragged
_KSETS = {}


def variant_kset(name: str) -> KSet:
    ks, rho, _natoms, _v = VARIANTS[name]
    key = (ks, rho)
    if key not in _KSETS:
        _KSETS[key] = kset(ks, rho, seed=len(_KSETS) + 11)
    return _KSETS[key]


def tail(per_wave: int, waves: int) -> int:
    """r of n = 2048 per_wave waves + r: the last workgroup then holds a wave with a partial range and, with more than one wave,
    a wave whose range is empty (and with four or more, a full one in front)."""
    if waves >= 4:
        return per_wave + per_wave // 2          # wave 0 full, wave 1 half, waves 2.. empty
    return per_wave // 2                         # wave 0 half, wave 1 (if any) empty


def big_n(per_wave: int, waves: int) -> int:
    return 2048 * per_wave * waves + tail(per_wave, waves)


def per_wave_one_chunk(waves: int) -> int:
    """A batch size below 2 x 2048 placements per wave of a workgroup: per_wave = 1; odd, so its last workgroup is ragged."""
    return 2048 * waves + 37


def check_subset(n: int, per_wave: int, waves: int, at_least=64, seed=5) -> np.ndarray:
    """Indices compared with the reference: the first and the last 2 per_wave waves placements and random ones in between."""
    edge = min(2 * per_wave * waves, n)
    idx = set(range(edge)) | set(range(n - edge, n))
    rng = np.random.default_rng(seed)
    while len(idx) < min(at_least, n):
        idx.add(int(rng.integers(0, n)))
    return np.array(sorted(idx))


# ---------------------------------------------------------------------------------------------- k-space edges
def box400() -> KSet:
    """The largest legal box, stride 134 + 133 + 133 = 400, sparsely filled: the rows i = 0..133 and i = 1..133 in full and the
    corners j, k = +-66 at three i."""
    ijk = [(i, 1, 0) for i in range(134)] + [(i, 0, 0) for i in range(1, 134)]
    ijk += [(i, j, k) for i in (1, 70, 133) for j in (-66, 66) for k in (-66, 66)] + [(0, 66, -66), (0, 66, 66), (0, 0, 66), (133, -66, 0)]
    return with_constants((133, 66, 66), ijk, 8)


def window_kset(natoms: int, ks=(8, 8, 8)) -> KSet:
    """A k-set whose dynamic LDS -- tables + constants -- lies in (64 KiB - LDS_STATIC, 64 KiB]: the launch budget counts the dynamic
    part alone, so here the workgroup asks for more than 64 KiB in all."""
    for rho in np.arange(1.0, 1.74, 0.01):
        k = kset(ks, float(rho), seed=7)
        _w, c, _pw, lds = launch_shape(k, natoms, 130)
        if c and 65536 - LDS_STATIC < lds <= 65536:
            return k
    raise AssertionError("no k-set in the window")


def edge_ksets() -> dict:
    segs = kset(SEGMENT_KS, seed=6)
    e = {
        "nk0-box0": with_constants((0, 0, 0), np.empty((0, 3)), 1),
        "nk0-box3": with_constants((3, 3, 3), np.empty((0, 3)), 1),
        "nk1": with_constants((3, 3, 3), [[2, -1, 3]], 2),
        "kx0": kset((0, 5, 5), seed=3),
        "ky0": kset((5, 0, 5), seed=4),
        "kz0": kset((5, 5, 0), seed=5),
        "line": kset((6, 0, 0), seed=6),
        "row21": with_constants((20, 1, 1), [[i, 1, -1] for i in range(21)], 7),
        "holes-dups-shuffled": kset((7, 5, 4), holes=12, dups=9, shuffle=True, seed=9),
        "tab-64k": with_constants((101, 38, 38), [[i, j, 38] for j in (-38, 0, 38) for i in range(1, 102, 4)], 10),
    }
    for nseg in (64, 65, 128, 129):
        e[f"seg{nseg}"] = trimmed_to_segments(segs, nseg)
    return e
