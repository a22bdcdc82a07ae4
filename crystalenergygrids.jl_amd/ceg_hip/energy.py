"""``energy_point`` / ``energy_grid`` for many placements at once, entirely on the GPU (SURVEY §8f
rows f1 + f2): Van der Waals and real-space Coulomb terms by batched interpolation of the
device-resident grids (:mod:`ceg_hip.interp`), reciprocal-space Ewald term by ``ceg_recip_*``.
Reference: ``energy_point`` ``src/grids.jl:311-327``, ``energy_grid`` ``src/grids.jl:346-424``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np

from . import _abi
from .hostmirror.ewald import EwaldFramework, ewald_context_constants
from .grids import CrystalEnergySetup, _matT
from .interp import GridInterpolator


class ReciprocalEwald:
    """Device-resident k-space tables of an :class:`EwaldFramework` (``ceg_recip_*``)."""

    def __init__(self, ef: EwaldFramework, device: int = 0):
        if ef.alpha == 0.0:
            raise ValueError("Ewald summation is not defined for this framework (alpha == 0)")
        self._lib = _abi.load_library()
        self.ef = ef
        ijk = np.ascontiguousarray(ef.kvec_ijk, dtype=np.int32)
        kf = np.ascontiguousarray(ef.kfactors, dtype=np.float64)
        re = np.ascontiguousarray(ef.StoreRigidChargeFramework.real, dtype=np.float64)
        im = np.ascontiguousarray(ef.StoreRigidChargeFramework.imag, dtype=np.float64)
        ks = np.asarray(ef.kspace.ks, dtype=np.int32)
        inv = _matT(ef.invmat)
        h = C.c_void_p()
        rc = self._lib.ceg_recip_create(C.byref(h), device, _abi.i32ptr(ijk.reshape(-1)), _abi.dptr(kf), _abi.dptr(re),
                                        _abi.dptr(im), len(kf), _abi.i32ptr(ks), _abi.dptr(inv))
        _abi.check(self._lib, rc)
        self._h = h

    def energies(self, molecule, positions) -> np.ndarray:
        """compute_ewald for ``molecule`` (a RASPASystem; charges + internal geometry) placed at
        ``positions[n, natoms, 3]`` -> K, float64[n]."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, len(molecule), 3)
        q = np.ascontiguousarray(molecule.atomic_charge, dtype=np.float64)
        enc, static = ewald_context_constants(self.ef, ((molecule,),))
        out = np.empty(len(pos), dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_recip_energy(self._h, _abi.dptr(pos.reshape(-1)), _abi.dptr(q), len(q), len(pos),
                                                         enc, static, _abi.dptr(out)))
        return out

    def launch_shape(self, natoms: int, n: int):
        """``ceg_recip_launch_shape`` (host side only): the launch :meth:`energies` gives ``n`` placements of a molecule of
        ``natoms`` atoms -> (waves per workgroup, constants in LDS (bool), placements per wave, dynamic LDS bytes)."""
        ijk = np.ascontiguousarray(self.ef.kvec_ijk, dtype=np.int32).reshape(-1)
        ks = np.asarray(self.ef.kspace.ks, dtype=np.int32)
        out = np.zeros(4, dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_recip_launch_shape(_abi.i32ptr(ijk), len(ijk) // 3, _abi.i32ptr(ks), int(natoms), int(n),
                                                               _abi.i32ptr(out)))
        return int(out[0]), bool(out[1]), int(out[2]), int(out[3])

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ceg_recip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReducedEnergyGrid(NamedTuple):
    """What :meth:`GpuEnergySetup.energy_grid_reduced` returns; an output that was not asked for is None."""
    mean: Optional[np.ndarray]
    min: Optional[np.ndarray]
    argmin: Optional[np.ndarray]


class GpuEnergySetup:
    """A :class:`CrystalEnergySetup` whose grids and k-space tables live on the GPU."""

    def __init__(self, setup: CrystalEnergySetup, device: int = 0):
        self.setup = setup
        self.vdw = [GridInterpolator(g, device) if g.ewald_precision == math.inf else None for g in setup.grids]
        self.has_coulomb = setup.coulomb.ewald_precision != -math.inf
        self.coulomb = GridInterpolator(setup.coulomb, device) if self.has_coulomb else None
        self.recip = ReciprocalEwald(setup.ewald, device) if self.has_coulomb else None

    def energy_points(self, positions) -> np.ndarray:
        """``energy_point(setup, positions[p])`` for every placement p -> float64[n, 2] (vdw, coulomb).
        ``positions[n, natoms, 3]`` in Å.  Blocking spheres short-circuit to (1e100, 0) like the
        reference (grids.jl:312-314)."""
        s = self.setup
        natoms = len(s.atomsidx)
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, natoms, 3)
        n = len(pos)
        vdw = np.zeros(n)
        for a in range(natoms):
            it = self.vdw[s.atomsidx[a]]
            if it is not None:                       # zero grid -> 0 K (grids.jl:213)
                vdw += it(pos[:, a])
        out = np.zeros((n, 2))
        out[:, 0] = vdw
        if self.has_coulomb:
            direct = np.zeros(n)
            for a in range(natoms):
                direct += s.charges[a] * self.coulomb(pos[:, a])
            out[:, 1] = direct + self.recip.energies(s.molecule, pos)
        if not s.block.empty:
            blocked = np.array([any(s.block[p] for p in mol) for mol in pos])
            out[blocked] = (1e100, 0.0)
        return out

    def energy_grid(self, step: float) -> np.ndarray:
        """``energy_grid(setup, step)`` for a mono-atomic guest or ``num_rotate == 0`` (grids.jl:346-424):
        float64[numA, numB, numC] of ``sum(energy_point)`` on the fractional lattice of the unit cell."""
        s = self.setup
        a, b, c = s.framework.mat[:, 0], s.framework.mat[:, 1], s.framework.mat[:, 2]
        numA = int(math.floor(np.linalg.norm(a) / step)) + 1
        numB = int(math.floor(np.linalg.norm(b) / step)) + 1
        numC = int(math.floor(np.linalg.norm(c) / step)) + 1
        stepA, stepB, stepC = a / numA, b / numB, c / numC
        iA, iB, iC = np.meshgrid(np.arange(numA), np.arange(numB), np.arange(numC), indexing="ij")
        ofs = iA[..., None] * stepA + iB[..., None] * stepB + iC[..., None] * stepC          # grids.jl:396
        base = np.asarray(s.molecule.position, dtype=np.float64).reshape(-1, 3)
        pos = ofs.reshape(-1, 1, 3) + base[None, :, :]
        e = self.energy_points(pos)
        return (e[:, 0] + e[:, 1]).reshape(numA, numB, numC)

    def _egrid_arguments(self, step: float, rotations):
        """Lattice (grids.jl:378-384) and every argument ``ceg_energy_grid`` and ``ceg_energy_grid_reduced`` share, up to and
        including ``static_contribution`` -> (args, objects the pointers in args refer to, nrot, (numA, numB, numC))."""
        s = self.setup
        a, b, c = s.framework.mat[:, 0], s.framework.mat[:, 1], s.framework.mat[:, 2]
        numA = int(math.floor(np.linalg.norm(a) / step)) + 1
        numB = int(math.floor(np.linalg.norm(b) / step)) + 1
        numC = int(math.floor(np.linalg.norm(c) / step)) + 1
        steps = np.ascontiguousarray(np.stack([a / numA, b / numB, c / numC]).reshape(-1))      # columns stepA, stepB, stepC
        num = np.array([numA, numB, numC], dtype=np.int32)
        rot = np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)
        nrot = len(rot)
        rot_cm = np.ascontiguousarray(rot.transpose(0, 2, 1).reshape(-1))                       # column-major
        base = np.ascontiguousarray(np.asarray(s.molecule.position, dtype=np.float64).reshape(-1, 3))
        natoms = len(base)
        q = np.ascontiguousarray(s.charges, dtype=np.float64)
        handles = (C.c_void_p * natoms)(*[self.vdw[i]._h if self.vdw[i] is not None else None for i in s.atomsidx])
        enc = static = 0.0
        if self.has_coulomb:
            enc, static = ewald_context_constants(s.ewald, ((s.molecule,),))
        if s.block.empty:
            bargs = (None, None, None, None, None, None)
            keep = ()
        else:
            cs = s.block.csetup
            mask = np.ascontiguousarray(s.block.block, dtype=np.uint8)
            keep = (mask, np.ascontiguousarray(cs.dims, dtype=np.int32), np.ascontiguousarray(cs.size, dtype=np.float64),
                    np.ascontiguousarray(cs.shift, dtype=np.float64), _matT(cs.cell.mat), _matT(cs.cell.invmat))
            bargs = (keep[0].ctypes.data, _abi.i32ptr(keep[1]), _abi.dptr(keep[2]), _abi.dptr(keep[3]), _abi.dptr(keep[4]), _abi.dptr(keep[5]))
        args = (handles, self.coulomb._h if self.has_coulomb else None, self.recip._h if self.has_coulomb else None,
                _abi.dptr(base.reshape(-1)), _abi.dptr(q), natoms, _abi.dptr(rot_cm), nrot, _abi.dptr(steps),
                _abi.i32ptr(num), *bargs, enc, static)
        return args, (handles, base, q, rot_cm, steps, num, keep), nrot, (numA, numB, numC)

    def energy_grid_rotations(self, step: float, rotations, out_device_ptr: Optional[int] = None, stream: int = 0) -> np.ndarray:
        """``energy_grid(setup, step, num_rotate)`` for a polyatomic guest (grids.jl:346-424) in ONE device pass
        (``ceg_energy_grid``): float64[nrot, numA, numB, numC] of ``sum(energy_point)`` with the molecule turned by
        ``rotations[k]`` (3x3, applied as ``r @ p``, grids.jl:389; e.g. from :func:`ceg_hip.hostmirror.lebedev.rotation_matrices`)
        on the lattice of :meth:`energy_grid`.  At the reference's default ``num_rotate = 40`` its ``get_rotation_matrices``
        (lebedev.jl:109-123) yields 43 orientations for a linear symmetric guest such as CO2 (the 86-point Lebedev grid halved)
        and 70 for a non-linear one (5 z-rotations x 14 points).  The array is a view of the buffer in Julia's memory order of
        ``allvals`` (rotation fastest).  With ``out_device_ptr`` (device memory for nrot*numA*numB*numC doubles) the result stays on the
        device, the call is asynchronous on ``stream`` and the lattice shape is returned instead."""
        lib = _abi.load_library()
        args, keep, nrot, (numA, numB, numC) = self._egrid_arguments(step, rotations)
        on_device = out_device_ptr is not None
        buf = None if on_device else np.empty(nrot * numA * numB * numC, dtype=np.float64)
        _abi.check(lib, lib.ceg_energy_grid(*args, C.c_void_p(int(out_device_ptr)) if on_device else buf.ctypes.data, 1 if on_device else 0,
                                            C.c_void_p(stream) if stream else None))
        del keep
        if on_device:
            return (nrot, numA, numB, numC)
        return buf.reshape(numC, numB, numA, nrot).transpose(3, 2, 1, 0)

    def energy_grid_reduced(self, step: float, rotations, temperatures=(), weights=None, want_min: bool = True,
                            want_argmin: bool = False, out_device_ptrs=None, stream: int = 0):
        """The rotation axis of :meth:`energy_grid_rotations` collapsed on the device (``ceg_energy_grid_reduced``): per lattice
        point the reference's ``meanBoltzmann`` (utils.jl:415-443) at each of ``temperatures`` (K, at most 8) with the optional
        ``weights[nrot]`` (its third argument, e.g. the Lebedev weights), the minimum over the orientations and the 0-based index
        of the first orientation that attains it.  The nrot*numA*numB*numC elements never leave the device.

        -> :class:`ReducedEnergyGrid` ``(mean, min, argmin)``: float64[ntemps, numA, numB, numC] (None without temperatures),
        float64[numA, numB, numC] (None unless ``want_min``), int32[numA, numB, numC] (None unless ``want_argmin``).  With
        ``out_device_ptrs = (mean, min, argmin)`` (device addresses in the layout of the C ABI, None where an output is not
        wanted; ``want_min`` / ``want_argmin`` are then not looked at) the results stay on the device, the call is asynchronous
        on ``stream`` and the lattice shape is returned instead."""
        lib = _abi.load_library()
        args, keep, nrot, (numA, numB, numC) = self._egrid_arguments(step, rotations)
        temps = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=np.float64)).reshape(-1))
        ntemps = len(temps)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if len(w) != nrot:
                raise ValueError(f"{len(w)} weights for {nrot} rotations")
        points = numA * numB * numC
        on_device = out_device_ptrs is not None
        if on_device:
            outs = [C.c_void_p(int(p)) if p else None for p in out_device_ptrs]
            p_mean = C.cast(outs[0], _abi.c_double_p) if outs[0] is not None else None
        else:
            mean = np.empty(ntemps * points, dtype=np.float64) if ntemps else None
            mn = np.empty(points, dtype=np.float64) if want_min else None
            amin = np.empty(points, dtype=np.int32) if want_argmin else None
            p_mean = _abi.dptr(mean) if mean is not None else None
            outs = [None, mn.ctypes.data if mn is not None else None, amin.ctypes.data if amin is not None else None]
        _abi.check(lib, lib.ceg_energy_grid_reduced(*args, _abi.dptr(temps) if ntemps else None, ntemps,
                                                    _abi.dptr(w) if w is not None else None, p_mean, outs[1], outs[2],
                                                    1 if on_device else 0, C.c_void_p(stream) if stream else None))
        del keep
        if on_device:
            return (numA, numB, numC)

        def lattice(x, lead=()):
            return None if x is None else x.reshape(lead + (numC, numB, numA)).transpose(*range(len(lead)), *(len(lead) + i for i in (2, 1, 0)))
        return ReducedEnergyGrid(lattice(mean, (ntemps,)), lattice(mn), lattice(amin))

    def close(self) -> None:
        for it in self.vdw:
            if it is not None:
                it.close()
        if self.coulomb is not None:
            self.coulomb.close()
        if self.recip is not None:
            self.recip.close()


class PairEnergies:
    """Device-resident guest atoms + pair table (``ceg_pairs_*``): batched single_contribution_vdw."""

    def __init__(self, ff, mat, invmat, device: int = 0):
        from .hostmirror.constants import COULOMBIC_CONVERSION_FACTOR
        self._lib = _abi.load_library()
        self.ff = ff
        rules, offsets = ff.pair_table()
        self._keep = (rules, offsets)
        h = C.c_void_p()
        rc = self._lib.ceg_pairs_create(C.byref(h), device, _abi.dptr(_matT(mat)), _abi.dptr(_matT(invmat)), ff.cutoff ** 2,
                                        rules.ctypes.data, _abi.i32ptr(offsets), ff.nkinds, COULOMBIC_CONVERSION_FACTOR)
        _abi.check(self._lib, rc)
        self._h = h

    def set_atoms(self, positions, kinds, molecule) -> None:
        """positions[N,3]; kinds 1-based ff indices; molecule ids (non-negative)."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32) - 1)
        mol = np.ascontiguousarray(molecule, dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_pairs_set_atoms(self._h, _abi.dptr(pos.reshape(-1)), _abi.i32ptr(k), _abi.i32ptr(mol), len(pos)))

    def energies(self, trial, trial_kinds, exclude_molecule: int = -1) -> np.ndarray:
        tk = np.ascontiguousarray(np.asarray(trial_kinds, dtype=np.int32) - 1)
        t = np.ascontiguousarray(trial, dtype=np.float64).reshape(-1, len(tk), 3)
        out = np.empty(len(t), dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_pairs_energy(self._h, _abi.dptr(t.reshape(-1)), _abi.i32ptr(tk), len(tk), len(t),
                                                         exclude_molecule, _abi.dptr(out)))
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ceg_pairs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuMonteCarloEnergy:
    """``movement_energy`` (montecarlo.jl:563-579) of a :class:`ceg_hip.hostmirror.montecarlo.MonteCarloSetup` for
    many trial placements at once: framework terms by batched grid interpolation, guest-guest terms by
    ``ceg_pairs_*``, reciprocal term by ``ceg_recip_*`` against the structure factor of everything else."""

    def __init__(self, mc, device: int = 0):
        from .hostmirror import montecarlo as M
        self.mc, self._M = mc, M
        self.interp = [GridInterpolator(g, device) if (g is not None and g.ewald_precision == math.inf) else None for g in mc.grids]
        self.has_coulomb = mc.coulomb.ewald_precision != -math.inf
        self.coulomb = GridInterpolator(mc.coulomb, device) if self.has_coulomb else None
        self.recip = ReciprocalEwald(mc.ewald, device) if mc.ewald.alpha != 0.0 else None
        self.pairs = PairEnergies(mc.ff, mc.mat, mc.invmat, device)
        self.refresh()

    def refresh(self) -> None:
        """Upload the current guest atoms (call after the host-side state changed)."""
        mc = self.mc
        pos, kinds, mol = [], [], []
        for m, (i, j, ids, p) in enumerate(mc.molecules()):
            pos.append(p)
            kinds += list(ids)
            mol += [m] * len(ids)
        self.pairs.set_atoms(np.concatenate(pos) if pos else np.empty((0, 3)), kinds, mol)

    def movement_energies(self, idx, positions) -> np.ndarray:
        """-> float64[n, 4]: (framework vdw, framework direct, inter, reciprocal) of molecule ``idx``
        (0-based (kind, molecule)) at each of ``positions[n, natoms, 3]``."""
        mc, M = self.mc, self._M
        i, j = idx
        ids = mc.ffidx[i]
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, len(ids), 3)
        out = np.zeros((len(pos), 4))
        if mc.grids:
            for a, ix in enumerate(ids):
                it = self.interp[ix - 1]
                if it is not None:
                    out[:, 0] += it(pos[:, a])
                if self.has_coulomb:
                    c = self.coulomb(pos[:, a])
                    out[:, 1] += np.where(c == 1e100, c, float(mc.charges[ix]) * c)
        out[:, 2] = self.pairs.energies(pos, ids, exclude_molecule=mc.flat_index(i, j))
        if self.recip is not None:
            rest = M.ewald_rest(mc, idx)
            lib = self.recip._lib
            _abi.check(lib, lib.ceg_recip_set_structure_factor(self.recip._h, _abi.dptr(np.ascontiguousarray(rest.real)),
                                                               _abi.dptr(np.ascontiguousarray(rest.imag))))
            q = np.ascontiguousarray([mc.charges[ix] for ix in ids], dtype=np.float64)
            rec = np.empty(len(pos))
            _abi.check(lib, lib.ceg_recip_energy(self.recip._h, _abi.dptr(pos.reshape(-1)), _abi.dptr(q), len(q), len(pos), 0.0, 0.0,
                                                 _abi.dptr(rec)))
            out[:, 3] = rec
        return out

    def baseline_energy(self):
        """baseline_energy (montecarlo.jl:530-542) with the framework and guest-guest sums on the GPU
        (each pair is seen from both molecules, hence the 1/2) and the many-molecule reciprocal sum on
        the host."""
        mc, M = self.mc, self._M
        reciprocal = M.compute_ewald_mc(mc)
        fv = fd = inter = 0.0
        for i, j, ids, p in mc.molecules():
            e = self.movement_energies((i, j), p[None])[0]
            fv += e[0]; fd += e[1]; inter += e[2]
        return M.BaselineEnergyReport(fv, fd, 0.5 * inter, reciprocal, mc.tailcorrection)

    def close(self) -> None:
        for it in self.interp:
            if it is not None:
                it.close()
        if self.coulomb is not None:
            self.coulomb.close()
        if self.recip is not None:
            self.recip.close()
        self.pairs.close()


class DeviceMonteCarlo:
    """Device-resident energy state of a :class:`ceg_hip.hostmirror.montecarlo.MonteCarloSetup` (``ceg_mc_*``, BASELINE config 5):
    ``movement_energy`` (montecarlo.jl:563-579) of a batch of trial placements in ONE launch, ``update_mc!``
    (montecarlo.jl:615-628) applied on the device.  The MC driver (proposals, acceptance) stays with the caller.

    ``grids_from``: another instance on the same device and framework whose grid interpolators this one uses instead of uploading
    its own (the chains of an isotherm share one framework); the interpolators are released when the last instance using them
    is closed.  ``upload_guests=False`` (a setup without molecules only): the handle as ``ceg_mc_create`` leaves it, an empty box,
    without a call of ``ceg_mc_set_guests``."""

    def __init__(self, mc, device: int = 0, grids_from: Optional["DeviceMonteCarlo"] = None, upload_guests: bool = True):
        from .hostmirror.constants import COULOMBIC_CONVERSION_FACTOR
        self._lib = _abi.load_library()
        self.mc = mc
        self._group = None
        ff = mc.ff
        nk = ff.nkinds
        if grids_from is not None:
            if len(grids_from.interp) != nk:
                raise ValueError("grids_from: another force field (number of kinds differs)")
            self.interp, self.coulomb, self._grid_users = grids_from.interp, grids_from.coulomb, grids_from._grid_users
        else:
            self.interp = [GridInterpolator(g, device) if (g is not None and g.ewald_precision == math.inf) else None
                           for g in (mc.grids if mc.grids else [None] * nk)]
            has_coulomb = bool(mc.grids) and mc.coulomb.ewald_precision != -math.inf
            self.coulomb = GridInterpolator(mc.coulomb, device) if has_coulomb else None
            self._grid_users = [0]
        self._grid_users[0] += 1
        handles = (C.c_void_p * nk)(*[it._h if it is not None else None for it in self.interp])
        charge = np.ascontiguousarray([0.0 if (k + 1 >= len(mc.charges) or np.isnan(mc.charges[k + 1])) else float(mc.charges[k + 1])
                                       for k in range(nk)], dtype=np.float64)
        rules, offsets = ff.pair_table()
        self._keep = (rules, offsets, handles, charge)
        ef = mc.ewald
        if ef.alpha != 0.0:
            ijk = np.ascontiguousarray(ef.kvec_ijk, dtype=np.int32).reshape(-1)
            kf = np.ascontiguousarray(ef.kfactors, dtype=np.float64)
            re = np.ascontiguousarray(ef.StoreRigidChargeFramework.real, dtype=np.float64)
            im = np.ascontiguousarray(ef.StoreRigidChargeFramework.imag, dtype=np.float64)
            ks = np.asarray(ef.kspace.ks, dtype=np.int32)
            einv = _matT(ef.invmat)
            kargs = (_abi.i32ptr(ijk), _abi.dptr(kf), _abi.dptr(re), _abi.dptr(im), len(kf), _abi.i32ptr(ks), _abi.dptr(einv))
        else:
            kargs = (None, None, None, None, 0, None, None)
        h = C.c_void_p()
        rc = self._lib.ceg_mc_create(C.byref(h), device, handles, self.coulomb._h if self.coulomb is not None else None, _abi.dptr(charge), nk,
                                     _abi.dptr(_matT(mc.mat)), _abi.dptr(_matT(mc.invmat)), ff.cutoff ** 2, rules.ctypes.data,
                                     _abi.i32ptr(offsets), COULOMBIC_CONVERSION_FACTOR, *kargs)
        _abi.check(self._lib, rc)
        self._h = h
        if upload_guests:
            self.refresh()
        elif any(len(kind) for kind in mc.positions):
            raise ValueError("upload_guests=False needs a setup without molecules")
        else:
            self._slot = [[] for _ in mc.positions]

    def neighbour_cells(self):
        """-> (bins per axis, capacity per cell) of the guest neighbour cells, or None when the guest-guest sum runs the exhaustive
        loop (MC cells of a few cutoffs, i.e. every fixture of the reference; energy.jl:340-349 is the reference's own switch)."""
        nb = np.zeros(3, dtype=np.int32)
        cap = C.c_int32(0)
        rc = self._lib.ceg_mc_neighbour_cells(self._h, _abi.i32ptr(nb), C.byref(cap))
        if rc < 0:
            _abi.check(self._lib, rc)
        return (tuple(int(x) for x in nb), int(cap.value)) if rc == 1 else None

    def cell_lists(self, nslots: Optional[int] = None):
        """``ceg_mc_cell_lists``: the host's cell lists of the handle -> (int32[nslots] cell, int32[nslots] entry in that cell) per atom
        slot, -1 where the slot is in no cell, or None when the handle keeps no neighbour cells.  ``nslots`` defaults to the atom slots
        of the guests on the device (:meth:`state`)."""
        if nslots is None:
            nslots = len(self.state()[0])
        cell_of, idx_of = np.full(int(nslots), -1, dtype=np.int32), np.full(int(nslots), -1, dtype=np.int32)
        rc = self._lib.ceg_mc_cell_lists(self._h, _abi.i32ptr(cell_of), _abi.i32ptr(idx_of), int(nslots))
        if rc < 0:
            _abi.check(self._lib, rc)
        return (cell_of, idx_of) if rc == 1 else None

    def refresh(self) -> None:
        """Upload the guests of ``self.mc`` (initial state, or to resynchronise with the host side)."""
        pos, kinds, first = [], [], [0]
        self._slot = [[] for _ in self.mc.positions]          # [kind][index in kind] -> molecule index on the device
        for i, j, ids, p in self.mc.molecules():
            self._slot[i].append(len(first) - 1)
            pos.append(np.asarray(p, dtype=np.float64).reshape(-1, 3))
            kinds += [k - 1 for k in ids]
            first.append(first[-1] + len(ids))
        pos = np.ascontiguousarray(np.concatenate(pos) if pos else np.empty((0, 3)), dtype=np.float64)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        first = np.ascontiguousarray(first, dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_mc_set_guests(self._h, _abi.dptr(pos.reshape(-1)), _abi.i32ptr(kinds), _abi.i32ptr(first), len(first) - 1))

    def trial(self, idx, positions) -> np.ndarray:
        """-> float64[n + 1, 4]: row 0 movement_energy of molecule ``idx`` (0-based (kind, molecule)) where it is now, row 1 + t at
        ``positions[t]``; columns (framework vdw, framework direct, inter, reciprocal)."""
        mol = self._slot[idx[0]][idx[1]]
        m = len(self.mc.ffidx[idx[0]])
        t = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, m, 3)
        out = np.empty((len(t) + 1, 4), dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_mc_trial(self._h, mol, _abi.dptr(t.reshape(-1)) if len(t) else None, len(t), _abi.dptr(out.reshape(-1))))
        return out

    def trial_device(self, idx, d_trial: int, n: int, d_out: int, stream: int = 0) -> None:
        """``ceg_mc_trial_device``: ``n`` trial placements at device address ``d_trial`` (float64[n, m, 3]) -> rows at device address
        ``d_out`` (float64[n + 1, 4]), enqueued on ``stream``; nothing is copied or synchronised."""
        _abi.check(self._lib, self._lib.ceg_mc_trial_device(self._h, self._slot[idx[0]][idx[1]], C.c_void_p(d_trial), int(n), C.c_void_p(d_out),
                                                            C.c_void_p(stream) if stream else None))

    def trial_insert_device(self, i: int, d_trial: int, n: int, d_out: int, stream: int = 0) -> None:
        """``ceg_mc_trial_insert_device``: rows float64[n, 4] at ``d_out`` for a NEW molecule of kind ``i``."""
        k = np.ascontiguousarray([ix - 1 for ix in self.mc.ffidx[i]], dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_mc_trial_insert_device(self._h, _abi.i32ptr(k), len(k), C.c_void_p(d_trial), int(n), C.c_void_p(d_out),
                                                                   C.c_void_p(stream) if stream else None))

    def accept(self, idx, positions) -> None:
        """update_mc!(mc, idx, positions) on the device (asynchronous).  The host-side ``mc`` is NOT touched."""
        p = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        _abi.check(self._lib, self._lib.ceg_mc_accept(self._h, self._slot[idx[0]][idx[1]], _abi.dptr(p)))

    def trial_insert(self, i: int, positions) -> np.ndarray:
        """movement_energy of a NEW molecule of kind ``i`` at each of ``positions[n, m, 3]`` -> float64[n, 4]."""
        k = np.ascontiguousarray([ix - 1 for ix in self.mc.ffidx[i]], dtype=np.int32)
        t = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, len(k), 3)
        out = np.empty((len(t), 4), dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_mc_trial_insert(self._h, _abi.i32ptr(k), len(k), _abi.dptr(t.reshape(-1)), len(t), _abi.dptr(out.reshape(-1))))
        return out

    def insert(self, i: int, positions) -> int:
        """add_one_system! on the device: a molecule of kind ``i`` joins (index in its kind returned, = append)."""
        k = np.ascontiguousarray([ix - 1 for ix in self.mc.ffidx[i]], dtype=np.int32)
        p = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        mol = C.c_int32(-1)
        _abi.check(self._lib, self._lib.ceg_mc_insert(self._h, _abi.i32ptr(k), len(k), _abi.dptr(p), C.byref(mol)))
        self._slot[i].append(int(mol.value))
        return len(self._slot[i]) - 1

    def remove(self, idx) -> int:
        """remove_one_system!(mc, i, j) on the device; the host-side indices behave like the reference's (montecarlo.jl:798-808):
        the last molecule of kind ``i`` takes index ``j``; returns its old index."""
        i, j = idx
        d = self._slot[i][j]
        last = len(self._slot[i]) - 1
        self._slot[i][j] = self._slot[i][last]
        self._slot[i].pop()
        moved = C.c_int32(-1)
        _abi.check(self._lib, self._lib.ceg_mc_remove(self._h, d, C.byref(moved)))
        if moved.value != d:                         # the device moved its last molecule into the hole
            for kind in self._slot:
                for q, v in enumerate(kind):
                    if v == moved.value:
                        kind[q] = d
        return last

    def ewald_constants(self):
        """``(energy_net_charges, static_contribution)`` of the EwaldContext (ewald.jl:497-544) for the species counts of the DEVICE
        state (``_slot``), not for ``mc.positions``: right after ``sweep_gcmc(..., positions=False)`` has changed the counts.  The
        molecules are rigid, so the intramolecular term of a species comes from ``mc.models`` (or, without a model, from any molecule
        of that species whose coordinates the host holds).  ``(0.0, 0.0)`` without Ewald summation.  The pair is kept for the
        counts it was computed for: a run that asks again with the same counts pays for it once."""
        from .hostmirror.ewald import ewald_context_constants
        from .hostmirror.raspa import RASPASystem
        mc = self.mc
        if mc.ewald.alpha == 0.0:
            return 0.0, 0.0
        key = (id(mc.ewald), tuple(len(kind) for kind in self._slot))
        kept = getattr(self, "_ewald_constants", None)
        if kept is not None and kept[0] == key:
            return kept[1]
        systems = []
        for i, kind in enumerate(self._slot):
            if not kind:
                continue
            m = len(mc.ffidx[i])
            shape = np.asarray(mc.models[i], dtype=np.float64).reshape(-1, 3) if len(getattr(mc, "models", ())) > i else None
            if shape is None or len(shape) != m:
                shape = next((np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in mc.positions[i] if p is not None), None)
            if shape is None:
                raise ValueError(f"species {i}: neither a model nor a molecule with coordinates on the host (pull_positions() first)")
            q = np.array([mc.charges[ix] for ix in mc.ffidx[i]], dtype=np.float64)
            systems.append([RASPASystem(mc.mat, shape, [""] * m, np.zeros(m), q, True)] * len(kind))
        self._ewald_constants = (key, ewald_context_constants(mc.ewald, systems))
        return self._ewald_constants[1]

    def _baseline_report(self, rec):
        """One ``ceg_mc_baseline_t`` record into the reference's report: the two constants and the tail correction stay on the host."""
        from .hostmirror import montecarlo as M
        reciprocal = 0.0
        if self.mc.ewald.alpha != 0.0:
            enc, static = self.ewald_constants()
            reciprocal = 2 * (float(rec["recip_framework"]) + enc) + float(rec["recip_guests"]) + static
        return M.BaselineEnergyReport(float(rec["framework_vdw"]), float(rec["framework_direct"]), float(rec["inter"]), reciprocal,
                                      self.mc.tailcorrection)

    def baseline_record(self, refresh: bool = False) -> np.ndarray:
        """``ceg_mc_baseline``: the raw ``_abi.MC_BASELINE_DTYPE`` record (framework, guest-guest and the two k-space sums, the
        molecules and atoms summed) in two launches, four with ``refresh`` (every structure factor recomputed from the positions
        first, as ``compute_ewald(::IncrementalEwaldContext)`` does)."""
        rec = np.zeros(1, dtype=_abi.MC_BASELINE_DTYPE)
        _abi.check(self._lib, self._lib.ceg_mc_baseline(self._h, _abi.MC_BASELINE_REFRESH if refresh else 0, rec.ctypes.data))
        return rec[0]

    def baseline_energy(self, route: str = "rows", refresh: bool = False):
        """baseline_energy (montecarlo.jl:530-542) from the device-resident state.

        ``route="rows"`` (the default): framework and guest-guest terms from row 0 of one trial launch per molecule (every pair is
        seen from both sides, hence the 1/2), the reciprocal term from the total guest structure factor kept on the device and the
        two EwaldContext constants (ewald.jl:497-544).  ``route="device"``: ``ceg_mc_baseline`` -- the whole state walked once on the
        device, every pair once; ``refresh`` (this route only) recomputes the structure factors from the positions first."""
        if route == "device":
            return self._baseline_report(self.baseline_record(refresh))
        if route != "rows":
            raise ValueError(f"unknown route {route!r} (rows or device)")
        if refresh:
            raise ValueError("refresh belongs to route='device'")
        from .hostmirror import montecarlo as M
        from .hostmirror.ewald import ewald_context_constants
        mc = self.mc
        fv = fd = inter = 0.0
        for i, kind in enumerate(self._slot):
            m = len(mc.ffidx[i])
            for j in range(len(kind)):
                row = self.trial((i, j), np.empty((0, m, 3)))[0]
                fv += row[0]; fd += row[1]; inter += row[2]
        reciprocal = 0.0
        ef = mc.ewald
        if ef.alpha != 0.0:
            _pos, a = self.state()
            enc, static = ewald_context_constants(ef, [k for k in M._ewald_systems(mc) if k])
            f = ef.StoreRigidChargeFramework
            reciprocal = (2 * (float((ef.kfactors * (f.real * a.real + f.imag * a.imag)).sum()) + enc)
                          + float((ef.kfactors * (a.real ** 2 + a.imag ** 2)).sum()) + static)
        return M.BaselineEnergyReport(fv, fd, 0.5 * inter, reciprocal, mc.tailcorrection)

    def state(self):
        """(positions[natoms, 3], total guest structure factor complex[nk]) read back from the device."""
        natoms = sum(len(ids) for _i, _j, ids, _p in self.mc.molecules())
        nk = len(self.mc.ewald.kfactors) if self.mc.ewald.alpha != 0.0 else 0
        pos = np.empty((natoms, 3)); re = np.empty(max(nk, 1)); im = np.empty(max(nk, 1))
        _abi.check(self._lib, self._lib.ceg_mc_get_state(self._h, _abi.dptr(pos.reshape(-1)) if natoms else None, _abi.dptr(re), _abi.dptr(im)))
        # device molecule order -> the host's (kind, index) order
        sizes = {}
        for i, kind in enumerate(self._slot):
            for d in kind:
                sizes[d] = len(self.mc.ffidx[i])
        start, o = {}, 0
        for d in sorted(sizes):
            start[d] = o
            o += sizes[d]
        host = [pos[start[d]:start[d] + sizes[d]] for kind in self._slot for d in kind]
        return (np.concatenate(host) if host else pos), (re[:nk] + 1j * im[:nk])

    def pull_positions(self) -> None:
        """``mc.positions`` from the device (after ``sweep_gcmc(..., positions=False)``): kind by kind in device molecule order."""
        pos, _sf = self.state()
        sizes = [len(self.mc.ffidx[i]) for i, kind in enumerate(self._slot) for _d in kind]
        split = iter(np.split(pos, np.cumsum(sizes)[:-1]) if sizes else [])
        self.mc.positions = [[next(split).copy() for _d in kind] for kind in self._slot]

    def close(self) -> None:
        if getattr(self, "_group", None) is not None:
            raise RuntimeError(f"this chain is a member of {self._group!r}: close the group first")
        if getattr(self, "_h", None):
            self._lib.ceg_mc_destroy(self._h)
            self._h = None
            self._grid_users[0] -= 1
            if self._grid_users[0] == 0:
                for it in self.interp:
                    if it is not None:
                        it.close()
                if self.coulomb is not None:
                    self.coulomb.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MonteCarloDrift(RuntimeError):
    """The drift check at the end of ``run_montecarlo!`` (simulation.jl:850-853) failed: recorded and actual energy differ."""


class MonteCarloHalted(RuntimeError):
    """A sweep halted a chain on a full neighbour cell (:meth:`DeviceMonteCarloGroup.halted`): ``chain`` and the absolute ``step``."""

    def __init__(self, chain: int, step: int):
        super().__init__(f"chain {chain} halted at step {step} on a full neighbour cell: raise the capacity with device_cells(capacity=...)")
        self.chain, self.step = chain, step


class MonteCarloRun(NamedTuple):
    """What :meth:`DeviceMonteCarloGroup.run_montecarlo` returns"""
    initial_energies: np.ndarray      # [ninit, K] K, after every initialisation cycle
    energies: np.ndarray              # [ncycles, K] K, after every production cycle
    cycles: np.ndarray                # [ninit + ncycles, K] _abi.MC_CYCLE_RECORD_DTYPE
    stats: tuple                      # (the init call's stats or None, the production call's or None)
    baselines: tuple                  # baseline_energies() at the start, at the first production cycle, at the end
    recorded: np.ndarray              # [K] K, what the drift check compared with the final baseline (energies[-1] + the swaps' bookkeeping)


class Isotherm(NamedTuple):
    """What :meth:`DeviceMonteCarloGroup.make_isotherm` returns (``make_isotherm``'s isotherm, loadings, energies, per chain)"""
    isotherm: np.ndarray              # [K] mean of the chain's loadings
    loadings: list                    # [K] of float64[ncycles[c]]: count[0] / Π after each of the chain's own production cycles
    energies: list                    # [K] of float64[ncycles[c]] K, after each of the chain's own production cycles
    drift_ok: np.ndarray              # [K] bool: isapprox(recorded, actual, rtol=1e-9) (simulation.jl:850-853)
    recorded: np.ndarray              # [K] K
    actual: np.ndarray                # [K] K, the final baseline_energy
    run: MonteCarloRun


class ParallelTemperingRun(NamedTuple):
    """What :meth:`DeviceMonteCarloGroup.run_parallel_tempering` returns; "by rung": entry ``[j, r]`` belongs to the chain that sat on
    rung ``r`` during cycle ``j``"""
    exchanges: np.ndarray             # [ninit + ncycles, K] _abi.MC_EXCHANGE_RECORD_DTYPE, per chain
    cycles_by_rung: np.ndarray        # [ninit + ncycles, K] _abi.MC_CYCLE_RECORD_DTYPE, re-sorted by rung
    exchanges_by_rung: np.ndarray     # [ninit + ncycles, K] the exchange records re-sorted by rung
    chain_of_rung: np.ndarray         # [ninit + ncycles, K] the chain on rung r during cycle j
    acceptance: np.ndarray            # [K - 1] accepted / attempted of the rung pair (r, r + 1) over the production cycles (NaN: never tried)
    pair_counts: np.ndarray           # [K, 2] attempted, accepted of the production cycles (row K - 1 is zeros)
    rungs: np.ndarray                 # [K] the rung of every chain at the end
    recorded: np.ndarray              # [K] K, the device's energy of every chain at the end, held against the final baseline
    baselines: tuple                  # baseline_energies() at the start, at the first production cycle, at the end
    stats: tuple                      # (the init call's stats or None, the production call's or None)


class DeviceMonteCarloGroup:
    """K :class:`DeviceMonteCarlo` chains on one device stepped in lockstep (``ceg_mc_group_*``): one launch evaluates the trials
    of every chain, one launch applies every accepted move -- the way ``make_isotherm`` (parameterinputs.jl:316-329) runs one
    ``run_gcmc`` per pressure, with the launch cost shared by the chains.  With ``trial`` / ``accept`` the acceptance rule stays
    with the caller; ``sweep`` runs whole sweeps of translations and rotations on the device, ``sweep_gcmc`` whole sweeps of all six
    move kinds of ``MCMoves``, insertions and deletions included; ``sweep_cycles`` / ``sweep_gcmc_cycles`` run either over whole cycles
    with the temperature schedule and the step-size adaptation of ``run_montecarlo!`` on the device, and ``run_montecarlo`` composes
    the reference's whole run from them.  While
    grouped the chains' own methods remain usable (insert, remove, single trials ...) and are ordered with the group calls; the
    group and its chains are driven from one thread.  Usable as a context manager; ``close()`` gives the chains back."""

    MAX_CHAINS = 256          # CEG_MC_GROUP_MAX

    def __init__(self, chains):
        self.chains = list(chains)
        if not self.chains:
            raise ValueError("a group needs at least one chain")
        self._lib = self.chains[0]._lib
        hs = (C.c_void_p * len(self.chains))(*[c._h for c in self.chains])
        g = C.c_void_p()
        _abi.check(self._lib, self._lib.ceg_mc_group_create(C.byref(g), hs, len(self.chains)))
        self._h = g
        for c in self.chains:
            c._group = self
        self._blocks = None           # what set_blocks installed: (species blocks, atom blocks)
        self.sampler = None           # what set_sampler installed (its geometry and tables, for the host restatement)
        self.chain_plan = None        # what set_chain_plan installed: (phiPV_div_k [K, nspecies] or None, stop_step [K] or None)
        self.tempering = None         # what set_tempering installed: (every, capacity)
        self.recorder = None          # what set_recorder installed: dict(every, origin, capacity, track_min, max_atoms, max_molecules)

    def __repr__(self):
        return f"DeviceMonteCarloGroup(k={len(self.chains)})"

    @staticmethod
    def _carries_blocks(mc) -> bool:
        return any(b is not None and not b.empty for b in list(getattr(mc, "speciesblocks", None) or []) + list(getattr(mc, "atomblocks", None) or []))

    def set_blocks(self, species_blocks, atom_blocks=None) -> None:
        """``ceg_mc_group_set_blocks``: the block pockets that :meth:`sweep_gcmc` tests (``inblockpocket`` and the retry loop of
        ``choose_step!``, simulation.jl:271-326).  ``species_blocks``: one :class:`ceg_hip.grids.BlockFile` (or None: empty) per
        species; ``atom_blocks``: one per force-field index (``mc.atomblocks``: entry ``ix - 1`` for the atoms of ff index ``ix``), looked
        up at ``point + delta / 2`` (montecarlo.jl:636), or None for no atom blocks.  The masks are copied to the device once and stay
        until they are replaced or cleared with ``set_blocks(None)``."""
        species_blocks, atom_blocks = list(species_blocks or []), list(atom_blocks or [])
        table = np.zeros(len(species_blocks) + len(atom_blocks), dtype=_abi.MC_BLOCK_DTYPE)
        keep = []
        for t, b, half in zip(table, species_blocks + atom_blocks, [False] * len(species_blocks) + [True] * len(atom_blocks)):
            if b is None:             # (no grid for this ff index: never blocked; a geometry that passes the checks)
                t["dims"], t["size"], t["mat"], t["invmat"] = 1, 1.0, np.eye(3).reshape(-1), np.eye(3).reshape(-1)
                continue
            cs = b.csetup
            t["dims"], t["size"], t["shift"] = cs.dims, cs.size, cs.shift
            t["mat"], t["invmat"] = np.asarray(cs.cell.mat, dtype=np.float64).T.reshape(-1), np.asarray(cs.cell.invmat, dtype=np.float64).T.reshape(-1)
            if half:
                t["offset"] = (np.asarray(cs.size, dtype=np.float64) / np.asarray(cs.dims, dtype=np.float64)) / 2.0
            if not b.empty:
                mask = np.ascontiguousarray(b.block, dtype=np.uint8)
                if mask.shape != tuple(int(d) + 1 for d in cs.dims):
                    raise ValueError(f"a block mask of shape {mask.shape} on a lattice of {tuple(int(d) + 1 for d in cs.dims)} points")
                keep.append(mask)
                t["mask"] = mask.ctypes.data
        ns = len(species_blocks)
        _abi.check(self._lib, self._lib.ceg_mc_group_set_blocks(self._h, table[:ns].ctypes.data if ns else None, ns,
                                                                table[ns:].ctypes.data if atom_blocks else None, len(atom_blocks)))
        self._blocks = (species_blocks, atom_blocks) if len(table) else None

    def block_counts(self):
        """``ceg_mc_group_block_counts``: per chain, the pocket-blocked steps of the last :meth:`sweep_gcmc` and the sum of the attempt
        indices its proposals used -> (int64[K], int64[K])."""
        pocket, attempts = np.zeros(len(self.chains), dtype=np.int64), np.zeros(len(self.chains), dtype=np.int64)
        _abi.check(self._lib, self._lib.ceg_mc_group_block_counts(self._h, _abi.i64ptr(pocket), _abi.i64ptr(attempts)))
        return pocket, attempts

    def device_cells(self, on: bool = True, capacity: Optional[int] = None) -> None:
        """``ceg_mc_group_set_device_cells``: :meth:`sweep`, :meth:`sweep_gcmc` and their ``_cycles`` forms take the chains that keep
        their guests in neighbour cells (:meth:`DeviceMonteCarlo.neighbour_cells`); their cell lists are kept on the device during
        a sweep.  ``capacity``: such chains get at least that many entries per cell.  ``on=False``: such chains are refused again."""
        _abi.check(self._lib, self._lib.ceg_mc_group_set_device_cells(self._h, 1 if on else 0, int(capacity or 0)))

    def halted(self) -> np.ndarray:
        """``ceg_mc_group_halted`` -> int64[K]: the absolute step at which the last sweep call halted the chain on a full cell (nothing
        of that step was applied; continue from it after ``device_cells(capacity=...)``), -1 where it did not."""
        out = np.full(len(self.chains), -1, dtype=np.int64)
        _abi.check(self._lib, self._lib.ceg_mc_group_halted(self._h, _abi.i64ptr(out)))
        return out

    def _raise_if_halted(self) -> None:
        h = self.halted()
        for c in np.nonzero(h >= 0)[0]:
            raise MonteCarloHalted(int(c), int(h[c]))

    @staticmethod
    def chain_plan_arrays(k: int, phiPV_div_k=None, stop_step=None):
        """The two arrays of a chain plan for ``k`` chains as ``ceg_mc_group_set_chain_plan`` takes them -> (float64 ``[k, nspecies]``
        or None, int64 ``[k]`` or None).  ``phiPV_div_k``: ``[k, nspecies]``, or ``[k]`` for one species; ``stop_step``: ``[k]`` integers.
        Needs no device; the values themselves are checked by the library (a stop < 0 at once, a ``phiPV_div_k`` by the GCMC sweep)."""
        phi = stop = None
        if phiPV_div_k is not None:
            phi = np.asarray(phiPV_div_k, dtype=np.float64)
            if phi.ndim == 1:
                phi = phi[:, None]
            if phi.ndim != 2 or phi.shape[0] != k or not 1 <= phi.shape[1] <= _abi.GCMC_MAX_SPECIES:
                raise ValueError(f"phiPV_div_k: [{k}, nspecies] with 1 <= nspecies <= {_abi.GCMC_MAX_SPECIES}, got shape {phi.shape}")
            phi = np.ascontiguousarray(phi)
        if stop_step is not None:
            given = np.asarray(stop_step)
            if given.shape != (k,) or given.dtype.kind not in "iu":
                raise ValueError(f"stop_step: one integer step per chain ({k})")
            if given.dtype.kind == "u" and given.size and int(given.max()) > np.iinfo(np.int64).max:
                raise ValueError("stop_step: a step beyond 2^63 - 1")
            stop = np.ascontiguousarray(given, dtype=np.int64)
        return phi, stop

    def set_chain_plan(self, phiPV_div_k=None, stop_step=None) -> None:
        """``ceg_mc_group_set_chain_plan``: what differs between the chains of an isotherm (``make_isotherm``, parameterinputs.jl:305-334).
        ``phiPV_div_k[c][i]`` (K) replaces the species table's value for chain ``c`` in the swap rules of :meth:`sweep_gcmc` /
        :meth:`sweep_gcmc_cycles`; chain ``c`` takes no part in the absolute steps ``s >= stop_step[c]`` of any sweep: its state, its
        statistics and its share of a sampler's map stay those of its own last step, and its log records are zero but for
        ``molecule == -2``, ``kind == -1`` (and ``species == -1``).  Either may be None; ``set_chain_plan()`` removes the plan.  It stays
        installed until it is replaced or removed; what is installed is kept in ``self.chain_plan``."""
        phi, stop = self.chain_plan_arrays(len(self.chains), phiPV_div_k, stop_step)
        if phi is None and stop is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_set_chain_plan(self._h, None))
            self.chain_plan = None
            return
        plan = _abi.McChainPlan(phi.shape[1] if phi is not None else 0, 0, phi.ctypes.data if phi is not None else None,
                                stop.ctypes.data if stop is not None else None)
        _abi.check(self._lib, self._lib.ceg_mc_group_set_chain_plan(self._h, C.addressof(plan)))
        self.chain_plan = (phi, stop)

    def baseline_records(self, refresh: bool = False) -> np.ndarray:
        """``ceg_mc_group_baseline``: one ``_abi.MC_BASELINE_DTYPE`` record per chain, all chains in one pass (two launches, four with
        ``refresh``); member ``c`` gets the bytes :meth:`DeviceMonteCarlo.baseline_record` gives for that chain."""
        rec = np.zeros(len(self.chains), dtype=_abi.MC_BASELINE_DTYPE)
        _abi.check(self._lib, self._lib.ceg_mc_group_baseline(self._h, _abi.MC_BASELINE_REFRESH if refresh else 0, rec.ctypes.data))
        return rec

    def baseline_energies(self, refresh: bool = False):
        """baseline_energy (montecarlo.jl:530-542) of every chain -> list of ``BaselineEnergyReport``; the two Ewald constants come
        from each chain's current species counts, the tail correction from its setup."""
        return [chain._baseline_report(r) for chain, r in zip(self.chains, self.baseline_records(refresh))]

    def trial(self, moves):
        """One trial per chain: ``moves[c]`` is ``("move", idx, positions[n, m, 3])`` (rows: n + 1, row 0 where the molecule is now;
        n = 0 gives the deletion energy), ``("insert", i, positions[n, m, 3])`` (n rows of a new molecule of kind ``i``; one kind
        per call) or None (idle).  -> list of float64[rows, 4] (None for idle chains)."""
        k = len(self.chains)
        if len(moves) != k:
            raise ValueError(f"{len(moves)} moves for {k} chains")
        mol = np.full(k, -2, dtype=np.int32)
        n = np.zeros(k, dtype=np.int32)
        kinds, parts, nrows = None, [], []
        for c, (chain, mv) in enumerate(zip(self.chains, moves)):
            if mv is None:
                nrows.append(0)
                continue
            what, idx, positions = mv
            if what == "move":
                mol[c] = chain._slot[idx[0]][idx[1]]
                m = len(chain.mc.ffidx[idx[0]])
            elif what == "insert":
                mol[c] = -1
                k_i = [ix - 1 for ix in chain.mc.ffidx[idx]]
                if kinds is not None and k_i != kinds:
                    raise ValueError("one inserted species per group call")
                kinds, m = k_i, len(k_i)
            else:
                raise ValueError(f"unknown move {what!r}")
            t = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, m, 3)
            n[c] = len(t)
            parts.append(t.reshape(-1))
            nrows.append(len(t) + (1 if what == "move" else 0))
        trial = np.ascontiguousarray(np.concatenate(parts) if parts else np.empty(0), dtype=np.float64)
        out = np.empty((sum(nrows), 4), dtype=np.float64)
        ik = np.ascontiguousarray(kinds if kinds is not None else [0], dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_mc_group_trial(self._h, _abi.i32ptr(mol), _abi.i32ptr(n), _abi.i32ptr(ik),
                                                           len(kinds) if kinds is not None else 0,
                                                           _abi.dptr(trial) if len(trial) else None, _abi.dptr(out.reshape(-1))))
        rows, o = [], 0
        for mv, r in zip(moves, nrows):
            rows.append(None if mv is None else out[o:o + r])
            o += r
        return rows

    def accept(self, accepted) -> None:
        """update_mc! on every chain whose entry is ``(idx, positions[m, 3])`` (None: nothing for that chain); asynchronous."""
        k = len(self.chains)
        if len(accepted) != k:
            raise ValueError(f"{len(accepted)} entries for {k} chains")
        mol = np.full(k, -1, dtype=np.int32)
        parts = []
        for c, (chain, a) in enumerate(zip(self.chains, accepted)):
            if a is None:
                continue
            idx, positions = a
            mol[c] = chain._slot[idx[0]][idx[1]]
            parts.append(np.ascontiguousarray(positions, dtype=np.float64).reshape(-1))
        p = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(1), dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_mc_group_accept(self._h, _abi.i32ptr(mol), _abi.dptr(p)))

    def sweep(self, nsteps: int, seed: int, first_step: int = 0, *, temperature, dmax, thetamax, p_rotation=0.5, stream_id=None,
              bead=None, degrees: bool = False, log: bool = False):
        """``ceg_mc_group_sweep``: ``nsteps`` Markov steps of every chain on the device -- molecule and move drawn from the
        counter-based stream of :mod:`ceg_hip.mcrng`, ``movement_energy`` before and after, the Metropolis rule of
        ``compute_accept_move`` (montecarlo.jl:702-712), ``update_mc!`` -- with one synchronisation at the end.

        ``temperature`` (K), ``dmax`` (A), ``thetamax`` (radians, or degrees with ``degrees=True``) and ``p_rotation``: one value for
        all chains or one per chain.  ``stream_id``: one distinct id per chain (default: the chain's position).  ``bead``: per
        chain, the 0-based atom each kind rotates about (default :func:`ceg_hip.mcrng.default_beads`, i.e. ``mc.bead``).
        Step ``s`` of the call is the absolute step ``first_step + s`` of the stream: continue a run with ``first_step`` advanced.

        -> stats (structured array [K]: trials / acceptances per move kind, blocked trials, ``delta`` = sum of after - before over
        the accepted moves), and with ``log=True`` also the log [nsteps, K] (molecule in the DEVICE's molecule order, move kind,
        accepted flag, ``u``, the two rows, the proposed positions).  The host-side ``mc.positions`` are NOT touched: read
        :meth:`DeviceMonteCarlo.state`."""
        return self._sweep(nsteps, None, seed, first_step, temperature=temperature, dmax=dmax, thetamax=thetamax, p_rotation=p_rotation,
                           stream_id=stream_id, bead=bead, degrees=degrees, log=log)

    def _cycles(self, ncycles: int, steps_per_cycle: int, temperature, adapt, cycle0: int, prior):
        """The ``ceg_mc_cycles_t`` of a ``*_cycles`` call -> (struct, what it points to, the per-chain temperature of the sweep's own
        parameters or None with a table, the records [ncycles, K] to fill)."""
        k = len(self.chains)
        names = {"dmax": _abi.MC_ADAPT_DMAX, "thetamax": _abi.MC_ADAPT_THETAMAX}
        bits = int(adapt) if isinstance(adapt, (int, np.integer)) else sum(names[a] for a in set(adapt))
        table = None
        if np.ndim(temperature) == 2:
            table = np.ascontiguousarray(temperature, dtype=np.float64)
            if table.shape != (int(ncycles), k):
                raise ValueError(f"temperature: a scalar, one per chain ({k}) or a table [{int(ncycles)}, {k}]")
            temperature = None
        pr = None
        if prior is not None:
            pr = np.ascontiguousarray(prior, dtype=np.int64)
            if pr.shape != (k, 4):
                raise ValueError(f"prior: [{k}, 4] translation trials, accepted, rotation trials, accepted")
        fits = 0 <= int(ncycles) * k <= _abi.MC_CYCLES_MAX_RECORDS            # (beyond it the library refuses the call: nothing to hold)
        records = np.zeros((int(ncycles) if fits else 1, k), dtype=_abi.MC_CYCLE_RECORD_DTYPE)
        cyc = _abi.McCycles(int(ncycles), int(steps_per_cycle), int(cycle0), bits, 0, table.ctypes.data if table is not None else None,
                            pr.ctypes.data if pr is not None else None)
        return cyc, (table, pr), temperature, records

    def sweep_cycles(self, ncycles: int, steps_per_cycle: int, seed: int, first_step: int = 0, *, temperature, dmax, thetamax,
                     adapt=("dmax", "thetamax"), cycle0: int = 1, prior=None, p_rotation=0.5, stream_id=None, bead=None, degrees: bool = False,
                     log: bool = False):
        """``ceg_mc_group_sweep_cycles``: ``ncycles`` whole cycles of ``steps_per_cycle`` steps of :meth:`sweep` in one call, with the
        end-of-cycle block of ``run_montecarlo!`` (simulation.jl:727-728, 818-827) on the device: ``temperature`` -- a scalar, one per
        chain or a table ``[ncycles, K]`` whose row ``j`` is in force during cycle ``j`` (``simu.temperatures``) -- and the adaptation
        of ``dmax`` / ``thetamax`` from the cumulative acceptance ratios after every cycle (``adapt``: the names to adapt, or the
        ``CEG_MC_ADAPT_*`` bits).  ``cycle0``: the reference's ``counter_cycle`` of the first cycle of this call; ``prior`` ``[K, 4]``: the
        translation trials, accepted, rotation trials, accepted before this call.  To continue a run pass ``first_step`` and ``cycle0``
        advanced, ``prior`` = the last record's counters and ``dmax`` / ``thetamax`` = its ``dmax_next`` / ``thetamax_next``
        (:func:`ceg_hip.mcrng.cycle_records` restates the records).  The other arguments as :meth:`sweep`.

        -> (stats, cycles ``_abi.MC_CYCLE_RECORD_DTYPE`` [ncycles, K][, log [ncycles * steps_per_cycle, K]])."""
        cycles = self._cycles(ncycles, steps_per_cycle, temperature, adapt, cycle0, prior)
        return self._sweep(int(ncycles) * int(steps_per_cycle), cycles, seed, first_step, temperature=cycles[2], dmax=dmax, thetamax=thetamax,
                           p_rotation=p_rotation, stream_id=stream_id, bead=bead, degrees=degrees, log=log)

    def _sweep(self, nsteps, cycles, seed, first_step, *, temperature, dmax, thetamax, p_rotation, stream_id, bead, degrees, log):
        """:meth:`sweep` (``cycles`` None) and :meth:`sweep_cycles` (``cycles`` from :meth:`_cycles`; ``temperature`` None with a table)"""
        from . import mcrng
        k = len(self.chains)

        def per_chain(x, what):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (k,)) if np.ndim(x) == 0 else x, dtype=np.float64)
            if a.shape != (k,):
                raise ValueError(f"{what}: one value or one per chain ({k})")
            return a

        T = None if temperature is None else per_chain(temperature, "temperature")
        dm, pr = per_chain(dmax, "dmax"), per_chain(p_rotation, "p_rotation")
        th = per_chain(thetamax, "thetamax")
        if degrees:
            th = np.ascontiguousarray(np.deg2rad(th))
        sid = np.ascontiguousarray(np.arange(k) if stream_id is None else stream_id, dtype=np.uint32)
        if sid.shape != (k,):
            raise ValueError(f"stream_id: one per chain ({k})")
        beads = []
        for c, chain in enumerate(self.chains):
            if self._carries_blocks(chain.mc):
                raise NotImplementedError("plain sweeps do not test block pockets (inblockpocket of choose_step!), and this setup has some: "
                                          "sweep_gcmc does")
            per_kind = mcrng.default_beads(chain.mc) if bead is None else list(bead[c])
            by_device = {d: per_kind[i] for i, kind in enumerate(chain._slot) for d in kind}
            beads += [by_device[d] for d in sorted(by_device)]
        beads = np.ascontiguousarray(beads if beads else [0], dtype=np.int32)
        params = _abi.SweepParams(int(seed), int(first_step), sid.ctypes.data, T.ctypes.data if T is not None else None, dm.ctypes.data,
                                  th.ctypes.data, pr.ctypes.data, beads.ctypes.data)
        stats = np.zeros(k, dtype=_abi.SWEEP_STATS_DTYPE)
        records = np.zeros((max(int(nsteps), 0), k), dtype=_abi.SWEEP_RECORD_DTYPE) if log else None
        log_ptr = records.ctypes.data if log and records.size else None
        if cycles is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_sweep(self._h, C.addressof(params), int(nsteps), stats.ctypes.data, log_ptr))
            return (stats, records) if log else stats
        _abi.check(self._lib, self._lib.ceg_mc_group_sweep_cycles(self._h, C.addressof(params), C.addressof(cycles[0]), stats.ctypes.data,
                                                                  cycles[3].ctypes.data if cycles[3].size else None, log_ptr))
        return (stats, cycles[3], records) if log else (stats, cycles[3])

    def gcmc_species(self, moves, phiPV_div_k, self_reciprocal=None, bead=None) -> np.ndarray:
        """The species table of ``ceg_mc_group_sweep_gcmc`` (``_abi.GCMC_SPECIES_DTYPE``) from the first chain's setup: one species
        per kind of ``mc`` -- atom kinds, ``mc.models``, ``mc.bead``, the tail-correction rows -- with ``moves[i]`` a
        :class:`ceg_hip.mcrng.MoveTable` and ``phiPV_div_k[i]`` in K.  ``self_reciprocal[i]`` defaults to ``ctx.energies[i]``
        (ewald.jl:497-544): ``COULOMBIC_CONVERSION_FACTOR alpha / sqrt(pi) * sum(q^2)``."""
        from . import mcrng
        from .hostmirror.constants import COULOMBIC_CONVERSION_FACTOR
        mc = self.chains[0].mc
        ns = len(mc.ffidx)
        if ns > _abi.GCMC_MAX_SPECIES:
            raise ValueError(f"at most {_abi.GCMC_MAX_SPECIES} species")
        if len(moves) != ns or len(phiPV_div_k) != ns:
            raise ValueError(f"moves and phiPV_div_k: one entry per species ({ns})")
        beads = mcrng.default_beads(mc) if bead is None else list(bead)
        table = np.zeros(ns, dtype=_abi.GCMC_SPECIES_DTYPE)
        for i, ids in enumerate(mc.ffidx):
            m = len(ids)
            model = np.asarray(mc.models[i] if len(mc.models) > i else np.zeros((m, 3)), dtype=np.float64).reshape(-1, 3)
            if len(model) != m or m > 16:
                raise ValueError(f"species {i}: the model needs {m} <= 16 atoms")
            t = table[i]
            t["m"], t["bead"] = m, beads[i]
            t["kinds"][:m] = [ix - 1 for ix in ids]
            t["model"][:m] = model
            t["cumulative"] = moves[i].cumulatives
            t["phiPV_div_k"] = phiPV_div_k[i]
            if self_reciprocal is not None:
                t["self_reciprocal"] = self_reciprocal[i]
            elif mc.ewald.alpha != 0.0:
                q = np.array([0.0 if np.isnan(mc.charges[ix]) else mc.charges[ix] for ix in ids])
                t["self_reciprocal"] = float((q ** 2).sum()) * (COULOMBIC_CONVERSION_FACTOR / math.sqrt(math.pi) * mc.ewald.alpha)
            if mc.tail_cross is not None:
                t["tail_framework"] = mc.tail_framework[i]
                t["tail_cross"][:ns] = np.asarray(mc.tail_cross)[i, :ns]
        return table

    def sweep_gcmc(self, nsteps: int, seed: int, first_step: int = 0, *, temperature, dmax, thetamax, moves=None, phiPV_div_k=None,
                   max_molecules, species=None, self_reciprocal=None, stream_id=None, bead=None, degrees: bool = False, log: bool = False,
                   positions: bool = True):
        """``ceg_mc_group_sweep_gcmc``: ``nsteps`` steps of every chain with all six move kinds of ``MCMoves`` (translation,
        rotation, random_translation, random_rotation, random_reinsertion, swap) proposed, decided and applied on the device; the
        molecule table changes on the device and is read back once, at the end.

        ``moves[i]`` / ``phiPV_div_k[i]`` per species (kind of ``mc``), or a ready ``species`` table (:meth:`gcmc_species`);
        ``max_molecules``: one value or one per chain; the other arguments as :meth:`sweep`.

        Block pockets: the masks of :meth:`set_blocks`, or else ``mc.speciesblocks`` / ``mc.atomblocks`` of the first chain's setup where
        it carries any, are tested as ``choose_step!`` tests them (``inblockpocket``, the 1000-attempt retry loop); :meth:`block_counts`
        reports the pocket-blocked steps and the attempts.

        -> stats (``_abi.GCMC_STATS_DTYPE`` [K]) and with ``log=True`` the log [nsteps, K] (``_abi.GCMC_RECORD_DTYPE``).  Afterwards
        every chain's ``mc.positions`` holds the final state, species by species in device molecule order, and its (kind, index)
        addressing follows it; ``mc.tailcorrection`` and ``mc.sums`` are NOT updated.  ``positions=False`` skips the read-back of
        the coordinates (one synchronisation and copy per chain): ``mc.positions`` then holds one ``None`` per molecule, which is
        all the device entry points need, until :meth:`DeviceMonteCarlo.pull_positions` fills them in -- for runs of many sweeps
        that look at the coordinates only now and then."""
        return self._sweep_gcmc(nsteps, None, seed, first_step, temperature=temperature, dmax=dmax, thetamax=thetamax, moves=moves,
                                phiPV_div_k=phiPV_div_k, max_molecules=max_molecules, species=species, self_reciprocal=self_reciprocal,
                                stream_id=stream_id, bead=bead, degrees=degrees, log=log, positions=positions)

    def sweep_gcmc_cycles(self, ncycles: int, steps_per_cycle: int, seed: int, first_step: int = 0, *, temperature, dmax, thetamax,
                          adapt=("dmax", "thetamax"), cycle0: int = 1, prior=None, moves=None, phiPV_div_k=None, max_molecules, species=None,
                          self_reciprocal=None, stream_id=None, bead=None, degrees: bool = False, log: bool = False, positions: bool = True):
        """``ceg_mc_group_sweep_gcmc_cycles``: :meth:`sweep_cycles` for :meth:`sweep_gcmc` -- a whole GCMC production run of K chains
        in one call.  A temperature table must be constant per chain where a species swaps (simulation.jl:688).  The host mirrors are
        rebuilt and the coordinates read back once, at the end.  -> (stats, cycles[, log])."""
        cycles = self._cycles(ncycles, steps_per_cycle, temperature, adapt, cycle0, prior)
        return self._sweep_gcmc(int(ncycles) * int(steps_per_cycle), cycles, seed, first_step, temperature=cycles[2], dmax=dmax, thetamax=thetamax,
                                moves=moves, phiPV_div_k=phiPV_div_k, max_molecules=max_molecules, species=species, self_reciprocal=self_reciprocal,
                                stream_id=stream_id, bead=bead, degrees=degrees, log=log, positions=positions)

    def _sweep_gcmc(self, nsteps, cycles, seed, first_step, *, temperature, dmax, thetamax, moves, phiPV_div_k, max_molecules, species,
                    self_reciprocal, stream_id, bead, degrees, log, positions):
        """:meth:`sweep_gcmc` (``cycles`` None) and :meth:`sweep_gcmc_cycles`, as :meth:`_sweep`"""
        k = len(self.chains)

        def per_chain(x, what, dtype=np.float64):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), (k,)) if np.ndim(x) == 0 else x, dtype=dtype)
            if a.shape != (k,):
                raise ValueError(f"{what}: one value or one per chain ({k})")
            return a

        T = None if temperature is None else per_chain(temperature, "temperature")
        dm, th = per_chain(dmax, "dmax"), per_chain(thetamax, "thetamax")
        if degrees:
            th = np.ascontiguousarray(np.deg2rad(th))
        cap = per_chain(max_molecules, "max_molecules", np.int32)
        sid = np.ascontiguousarray(np.arange(k) if stream_id is None else stream_id, dtype=np.uint32)
        if sid.shape != (k,):
            raise ValueError(f"stream_id: one per chain ({k})")
        table = np.ascontiguousarray(species if species is not None else self.gcmc_species(moves, phiPV_div_k, self_reciprocal, bead))
        given = []
        mc0 = self.chains[0].mc
        if self._blocks is None and self._carries_blocks(mc0):          # the setup's own masks, unless the caller installed some
            self.set_blocks(mc0.speciesblocks or [None] * len(mc0.ffidx), mc0.atomblocks)
        for chain in self.chains:
            by_device = {d: i for i, kind in enumerate(chain._slot) for d in kind}
            given += [by_device[d] for d in sorted(by_device)]
        given = np.ascontiguousarray(given if given else [0], dtype=np.int32)
        out = np.full(max(int(np.clip(cap, 0, None).sum()), 1), -1, dtype=np.int32)
        params = _abi.GcmcParams(int(seed), int(first_step), sid.ctypes.data, T.ctypes.data if T is not None else None, dm.ctypes.data,
                                 th.ctypes.data, len(table), 0, table.ctypes.data, given.ctypes.data, cap.ctypes.data, out.ctypes.data)
        stats = np.zeros(k, dtype=_abi.GCMC_STATS_DTYPE)
        records = np.zeros((max(int(nsteps), 0), k), dtype=_abi.GCMC_RECORD_DTYPE) if log else None
        log_ptr = records.ctypes.data if log and records.size else None
        if cycles is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_sweep_gcmc(self._h, C.addressof(params), int(nsteps), stats.ctypes.data, log_ptr))
        else:
            _abi.check(self._lib, self._lib.ceg_mc_group_sweep_gcmc_cycles(self._h, C.addressof(params), C.addressof(cycles[0]), stats.ctypes.data,
                                                                           cycles[3].ctypes.data if cycles[3].size else None, log_ptr))
        # the chains' host side from the reported table: _slot[i] = the device indices of species i in device order
        offsets = np.concatenate([[0], np.cumsum(np.clip(cap, 0, None))])
        for c, chain in enumerate(self.chains):
            spec = out[offsets[c]:offsets[c] + int(stats[c]["nmol"])]
            chain._slot = [[int(d) for d in np.nonzero(spec == i)[0]] for i in range(len(chain.mc.positions))]
            chain.mc.positions = [[None] * len(kind) for kind in chain._slot]
            if positions:
                chain.pull_positions()
        if cycles is not None:
            return (stats, cycles[3], records) if log else (stats, cycles[3])
        return (stats, records) if log else stats

    def numsteps(self, moves=None):
        """The reference's steps per cycle (``numsteps``, simulation.jl:683-700) of every chain: 50 per leading species with a swap
        probability > 0, then the molecule count of the first species without one.  ``moves``: one :class:`ceg_hip.mcrng.MoveTable`
        per species, or None (no swaps)."""
        out = []
        for chain in self.chains:
            n = 0
            for i, kind in enumerate(chain._slot):
                if moves is None or moves[i].swap == 0:
                    n += len(kind)
                    break
                n += 50
            out.append(n)
        return out

    def run_montecarlo(self, temperatures, ncycles: int, ninit: int = 0, *, seed: int = 0, steps_per_cycle: Optional[int] = None, gcmc=None,
                       dmax=1.3, thetamax=math.radians(30.0), adapt=("dmax", "thetamax"), p_rotation=0.5, stream_id=None, bead=None,
                       positions: bool = True, check_drift: bool = True):
        """The shape of ``run_montecarlo!`` (simulation.jl:640-860) for the K chains: ``baseline_energy``, the ``ninit`` cycles in one
        :meth:`sweep_cycles` / :meth:`sweep_gcmc_cycles` call, ``baseline_energy`` again (the precise energy at the first production
        cycle, :788-790), the ``ncycles`` production cycles in one call that continues ``cycle0``, the counters and the step sizes, the
        final ``baseline_energy`` and the reference's drift check ``isapprox(recorded, actual, rtol=1e-9)`` (:850-853), raised as
        :class:`MonteCarloDrift` where it fails (``check_drift=False``: not checked; the caller compares ``recorded`` with
        ``baselines[2]``).

        ``temperatures``: a scalar, one per chain, or ``[ninit + ncycles, K]`` (``simu.temperatures`` per chain).  ``steps_per_cycle``
        defaults to :meth:`numsteps` of the first chain; a chain whose ``numsteps`` differs is refused (it belongs in another group).
        ``gcmc``: None for translations and rotations only, else the keywords of :meth:`sweep_gcmc` that describe the species
        (``moves`` and ``phiPV_div_k``, or ``species``; ``max_molecules``; ``self_reciprocal``).  ``dmax`` / ``thetamax`` (radians) start
        at the reference's 1.3 A and 30 degrees (``MoveStatistics(1.3u"Å", 30.0u"°")``).

        -> :class:`MonteCarloRun`: ``initial_energies`` [ninit, K] and ``energies`` [ncycles, K] (the baseline of the phase + the
        records' deltas, K), ``cycles`` [ninit + ncycles, K], ``stats`` (the init call's or None, the production call's or None),
        ``baselines`` (start, first production cycle, end), each a list of ``BaselineEnergyReport``, and ``recorded`` [K], the energy
        the drift check holds against the final baseline.

        Swaps: the records' ``delta_swaps`` sums what ``compute_accept_move_swap`` calls ``diff``, +-(E - self_reciprocal) + tc, while
        the state gains or loses E and the two Ewald constants move with the species counts.  ``recorded`` is therefore
        ``energies[-1]`` plus, per species, (count now - count at the first production cycle) * self_reciprocal, minus the tail
        correction's change as the species table holds it, plus the change of ``2 energy_net_charges + static_contribution`` and of
        ``mc.tailcorrection`` -- all functions of the counts alone.  Without swaps it is ``energies[-1]``.

        A chain that keeps its guests in neighbour cells takes part after :meth:`device_cells`, with or without ``gcmc``.
        If a sweep call halts a chain on a full cell, :class:`MonteCarloHalted` names chain and step; the states are those the call
        left (the halted chain as before that step).  Continuing a run in the middle of a cycle is out of scope: raise the capacity
        with ``device_cells(capacity=...)`` and start the run again."""
        from . import mcrng
        k = len(self.chains)
        ninit, ncycles = int(ninit), int(ncycles)
        if ninit < 0 or ncycles < 0:
            raise ValueError("ninit and ncycles must be >= 0")
        moves = table = None
        if gcmc is not None:                         # the species table once, for both calls and for the bookkeeping of the swaps
            gcmc = dict(gcmc)
            given = gcmc.pop("species", None)
            described = (gcmc.pop("moves", None), gcmc.pop("phiPV_div_k", None), gcmc.pop("self_reciprocal", None))
            table = np.ascontiguousarray(given if given is not None else self.gcmc_species(described[0], described[1], described[2], bead))
            gcmc["species"] = table
            moves = [mcrng.MoveTable(cumulatives=row["cumulative"]) for row in table]
        per_chain = self.numsteps(moves)
        L = per_chain[0] if steps_per_cycle is None else int(steps_per_cycle)
        if steps_per_cycle is None and any(n != L for n in per_chain):
            raise ValueError(f"the chains' steps per cycle differ ({per_chain}): chains whose cycle lengths differ belong in different groups")
        if L < 1:
            raise ValueError("empty simulation: no step per cycle (simulation.jl:718)")
        T = np.asarray(temperatures, dtype=np.float64)
        if T.ndim == 2 and T.shape != (ninit + ncycles, k):
            raise ValueError(f"temperatures: a scalar, one per chain ({k}) or a table [{ninit + ncycles}, {k}]")
        dm = np.broadcast_to(np.asarray(dmax, dtype=np.float64), (k,)).copy()
        th = np.broadcast_to(np.asarray(thetamax, dtype=np.float64), (k,)).copy()
        prior = np.zeros((k, 4), dtype=np.int64)
        done = [0]                                   # cycles run so far
        common = dict(adapt=adapt, stream_id=stream_id, bead=bead)

        def retail(before):                          # mc.tailcorrection follows the species counts (modify_species!, montecarlo.jl:814,858)
            from .hostmirror.montecarlo import modify_species_dryrun
            for chain, old in zip(self.chains, before):
                mc = chain.mc
                if mc.tail_cross is None:
                    continue
                counts = list(old)
                for i, kind in enumerate(chain._slot):
                    while counts[i] != len(kind):
                        num = 1 if counts[i] < len(kind) else -1
                        mc.tailcorrection += modify_species_dryrun(mc.tail_framework, mc.tail_cross, counts, i, num)
                        counts[i] += num

        def phase(n, last):
            rows = T[done[0]:done[0] + n] if T.ndim == 2 else T
            args = dict(temperature=rows, dmax=dm, thetamax=th, cycle0=1 + done[0], prior=prior, **common)
            if gcmc is None:
                stats, cyc = self.sweep_cycles(n, L, seed, done[0] * L, p_rotation=p_rotation, **args)
            else:
                before = [[len(kind) for kind in chain._slot] for chain in self.chains]
                stats, cyc = self.sweep_gcmc_cycles(n, L, seed, done[0] * L, positions=positions and last, **gcmc, **args)
                retail(before)
            self._raise_if_halted()                  # (a chain with neighbour cells whose cell filled up: device_cells)
            if n > 0:
                dm[:], th[:] = cyc[-1]["dmax_next"], cyc[-1]["thetamax_next"]
                for q, name in enumerate(("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")):
                    prior[:, q] = cyc[-1][name]
            done[0] += n
            return stats, cyc

        start = self.baseline_energies()
        base = np.array([float(r) for r in start])
        if self.recorder is not None:                # the recorder's energies are the reference's `energy`: the baseline + the deltas
            self.recorder_rebase(base)
        stats_init = stats = None
        cycles = np.zeros((0, k), dtype=_abi.MC_CYCLE_RECORD_DTYPE)
        initial_energies = np.zeros((0, k))
        production = start
        if ninit > 0:
            stats_init, cycles = phase(ninit, ncycles == 0)
            initial_energies = base[None, :] + cycles["delta_moves"] + cycles["delta_swaps"]
            production = self.baseline_energies()
            base = np.array([float(r) for r in production])
            if self.recorder is not None:            # (the precise energy at the first production cycle, simulation.jl:788-790)
                self.recorder_rebase(base)
        energies = np.zeros((0, k))
        recorded = base.copy()
        if ncycles > 0:
            counts0 = [[len(kind) for kind in chain._slot] for chain in self.chains]
            consts0 = [chain.ewald_constants() for chain in self.chains]
            tail0 = [chain.mc.tailcorrection for chain in self.chains]
            stats, cyc = phase(ncycles, True)
            energies = base[None, :] + cyc["delta_moves"] + cyc["delta_swaps"]
            cycles = np.concatenate([cycles, cyc])
            recorded = energies[-1].copy()
            for c, chain in enumerate(self.chains if table is not None else []):
                counts, ns = list(counts0[c]), len(table)
                for i, kind in enumerate(chain._slot):
                    while counts[i] != len(kind):
                        num = 1 if counts[i] < len(kind) else -1
                        recorded[c] += num * float(table[i]["self_reciprocal"]) - mcrng.tail_change(table[i]["tail_framework"], table[i]["tail_cross"][:ns],
                                                                                                     counts, i, num)
                        counts[i] += num
                (enc0, static0), (enc1, static1) = consts0[c], chain.ewald_constants()
                recorded[c] += ((2 * enc1 + static1) - (2 * enc0 + static0)) + (chain.mc.tailcorrection - tail0[c])
        end = start
        if ninit + ncycles > 0:                      # (not a single-point computation, simulation.jl:849)
            end = self.baseline_energies()
            for c, (rec, actual) in enumerate(zip(recorded, (float(r) for r in end)) if check_drift else ()):
                if not abs(rec - actual) <= 1e-9 * max(abs(rec), abs(actual)):
                    raise MonteCarloDrift(f"chain {c}: energy deviation observed between actual ({actual!r}) and recorded ({rec!r}): "
                                          "the simulation results are wrong")
        return MonteCarloRun(initial_energies, energies, cycles, (stats_init, stats), (start, production, end), recorded)

    def set_tempering(self, every: Optional[int], energies=None, rungs=None, capacity: int = 1024) -> None:
        """``ceg_mc_group_set_tempering``: from now on :meth:`sweep_cycles` and :meth:`sweep_gcmc_cycles` exchange replicas between
        neighbouring rungs of the temperature ladder at the end of every cycle ``cc`` with ``cc % every == 0`` (the rule of
        ``run_parallel_tempering``, simulation.jl:533), on the device.  Temperatures, not configurations, are exchanged: the
        ``temperature`` argument of those calls is then indexed by RUNG (non-decreasing), and the chain on rung ``r`` runs at entry ``r``.
        ``energies``: the total energy of every chain now (K; default: the totals of :meth:`baseline_energies`); ``rungs``: the rung of
        every chain, a permutation (default: chain ``c`` on rung ``c``); ``capacity``: the cycles of exchange records kept.
        ``every=None`` removes the state.  Any other call that moves a chain (``sweep``, ``accept``, ``insert`` ...) makes the stored
        energies stale: install the state again.  :func:`ceg_hip.mcrng.exchange_round` restates a cycle end."""
        if every is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_set_tempering(self._h, None))
            self.tempering = None
            return
        k = len(self.chains)
        if energies is None:
            energies = [float(r) for r in self.baseline_energies()]
        E = np.ascontiguousarray(energies, dtype=np.float64)
        if E.shape != (k,):
            raise ValueError(f"energies: one per chain ({k})")
        R = None
        if rungs is not None:
            R = np.ascontiguousarray(rungs, dtype=np.int32)
            if R.shape != (k,):
                raise ValueError(f"rungs: one per chain ({k})")
        spec = _abi.McTempering(int(every), int(capacity), R.ctypes.data if R is not None else None, E.ctypes.data)
        _abi.check(self._lib, self._lib.ceg_mc_group_set_tempering(self._h, C.addressof(spec)))
        self.tempering = (int(every), int(capacity))

    def tempering_read(self):
        """``ceg_mc_group_tempering_read`` -> (rungs int32[K], energies float64[K] -- as of the end of the last ``*_cycles`` call --,
        pair counts int64[K, 2]: attempted and accepted exchanges of the rung pair (r, r + 1), records
        ``_abi.MC_EXCHANGE_RECORD_DTYPE`` [cycles, K] of every cycle since :meth:`set_tempering`)."""
        if self.tempering is None:
            raise RuntimeError("the group has no tempering state (set_tempering)")
        k = len(self.chains)
        rung, energy, pairs = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.float64), np.zeros((k, 2), dtype=np.int64)
        n = C.c_int64(0)
        _abi.check(self._lib, self._lib.ceg_mc_group_tempering_read(self._h, None, None, None, None, C.byref(n)))
        records = np.zeros((max(int(n.value), 0), k), dtype=_abi.MC_EXCHANGE_RECORD_DTYPE)
        _abi.check(self._lib, self._lib.ceg_mc_group_tempering_read(self._h, _abi.i32ptr(rung), _abi.dptr(energy), _abi.i64ptr(pairs.reshape(-1)),
                                                                    records.ctypes.data if records.size else None, C.byref(n)))
        return rung, energy, pairs, records

    def run_parallel_tempering(self, ladder, ncycles: int, ninit: int = 0, *, every: int = 1, seed: int = 0, steps_per_cycle: Optional[int] = None,
                               gcmc=None, dmax=1.3, thetamax=math.radians(30.0), adapt=("dmax", "thetamax"), p_rotation=0.5, stream_id=None,
                               bead=None, rungs=None, positions: bool = True, check_drift: bool = True) -> ParallelTemperingRun:
        """The shape of ``run_parallel_tempering`` (simulation.jl:461-622) for the K chains, composed like :meth:`run_montecarlo`:
        ``baseline_energy`` and :meth:`set_tempering`, the ``ninit`` cycles in one :meth:`sweep_cycles` call, ``baseline_energy`` again and
        the state installed again with the precise energies (the rungs carried over), the ``ncycles`` production cycles in one call, and
        for every chain the device's recorded energy against the final ``baseline_energy`` at the reference's rtol 1e-9 (:614),
        raised as :class:`MonteCarloDrift` where it fails (``check_drift=False``: not checked).

        ``ladder``: the temperatures BY RUNG, non-decreasing: one per rung, or a table ``[ninit + ncycles, K]``.  ``every``: an exchange
        round after every cycle ``cc`` with ``cc % every == 0``.  ``rungs``: the rung of every chain at the start (default: chain ``c`` on
        rung ``c``).  ``gcmc``: as in :meth:`run_montecarlo`, with displacement moves only (exchanges under swaps are refused).  Step
        sizes and counters stay with the chain, not the rung.  Afterwards no tempering state is installed.

        -> :class:`ParallelTemperingRun`: the exchange records per chain, the cycle and exchange records re-sorted by rung, the
        acceptance ratio of every rung pair over the production cycles, the final rungs and energies."""
        k = len(self.chains)
        ninit, ncycles = int(ninit), int(ncycles)
        if ninit < 0 or ncycles < 0:
            raise ValueError("ninit and ncycles must be >= 0")
        L = self.numsteps(None)[0] if steps_per_cycle is None else int(steps_per_cycle)
        if steps_per_cycle is None and any(n != L for n in self.numsteps(None)):
            raise ValueError("the chains' steps per cycle differ: chains whose cycle lengths differ belong in different groups")
        if L < 1:
            raise ValueError("empty simulation: no step per cycle (simulation.jl:718)")
        T = np.asarray(ladder, dtype=np.float64)
        if T.shape not in ((k,), (ninit + ncycles, k)):
            raise ValueError(f"ladder: one temperature per rung ({k}) or a table [{ninit + ncycles}, {k}]")
        dm = np.broadcast_to(np.asarray(dmax, dtype=np.float64), (k,)).copy()
        th = np.broadcast_to(np.asarray(thetamax, dtype=np.float64), (k,)).copy()
        prior = np.zeros((k, 4), dtype=np.int64)
        done = [0]

        def phase(n, last):
            rows = T[done[0]:done[0] + n] if T.ndim == 2 else T
            args = dict(temperature=rows, dmax=dm, thetamax=th, cycle0=1 + done[0], prior=prior, adapt=adapt, stream_id=stream_id, bead=bead)
            if gcmc is None:
                stats, cyc = self.sweep_cycles(n, L, seed, done[0] * L, p_rotation=p_rotation, **args)
            else:
                stats, cyc = self.sweep_gcmc_cycles(n, L, seed, done[0] * L, positions=positions and last, **dict(gcmc), **args)
            self._raise_if_halted()
            dm[:], th[:] = cyc[-1]["dmax_next"], cyc[-1]["thetamax_next"]
            for q, name in enumerate(("translation_trials", "translation_accepted", "rotation_trials", "rotation_accepted")):
                prior[:, q] = cyc[-1][name]
            done[0] += n
            return stats, cyc

        start = self.baseline_energies()
        production = end = start
        stats_init = stats = None
        cycles = [np.zeros((0, k), dtype=_abi.MC_CYCLE_RECORD_DTYPE)]
        exchanges = [np.zeros((0, k), dtype=_abi.MC_EXCHANGE_RECORD_DTYPE)]
        rung = np.arange(k, dtype=np.int32) if rungs is None else np.ascontiguousarray(rungs, dtype=np.int32)
        recorded = np.array([float(r) for r in start])
        pairs = np.zeros((k, 2), dtype=np.int64)
        try:
            if ninit > 0:
                self.set_tempering(every, recorded, rung, capacity=ninit)
                stats_init, cyc = phase(ninit, ncycles == 0)
                rung, recorded, pairs, rec = self.tempering_read()
                cycles.append(cyc); exchanges.append(rec)
                production = end = self.baseline_energies()
            if ncycles > 0:
                self.set_tempering(every, [float(r) for r in production], rung, capacity=ncycles)
                stats, cyc = phase(ncycles, True)
                rung, recorded, pairs, rec = self.tempering_read()
                cycles.append(cyc); exchanges.append(rec)
                end = self.baseline_energies()
        finally:
            if self.tempering is not None:
                self.set_tempering(None)
        for c, (rec, actual) in enumerate(zip(recorded, (float(r) for r in end)) if check_drift and ninit + ncycles > 0 else ()):
            if not abs(rec - actual) <= 1e-9 * max(abs(rec), abs(actual)):
                raise MonteCarloDrift(f"chain {c}: energy deviation observed between actual ({actual!r}) and recorded ({rec!r}): "
                                      "the simulation results are wrong")
        cycles, exchanges = np.concatenate(cycles), np.concatenate(exchanges)
        chain_of_rung = np.argsort(exchanges["rung"], axis=1).astype(np.int32)
        with np.errstate(invalid="ignore", divide="ignore"):
            acceptance = pairs[:-1, 1] / pairs[:-1, 0]
        return ParallelTemperingRun(exchanges, np.take_along_axis(cycles, chain_of_rung, axis=1), np.take_along_axis(exchanges, chain_of_rung, axis=1),
                                    chain_of_rung, acceptance, pairs, rung, recorded, (start, production, end), (stats_init, stats))

    def make_isotherm(self, phiPV_div_k, ncycles, ninit: int = 0, *, temperature, max_molecules, moves=None, species=None, self_reciprocal=None,
                      seed: int = 0, steps_per_cycle: Optional[int] = None, supercell=(1, 1, 1), dmax=1.3, thetamax=math.radians(30.0),
                      adapt=("dmax", "thetamax"), stream_id=None, bead=None, positions: bool = True):
        """``make_isotherm`` (parameterinputs.jl:305-334) on the device sweeps: chain ``c`` is the ``run_gcmc`` of one pressure, with its own
        ``phiPV_div_k[c]`` (``[K, nspecies]`` K, e.g. from :func:`ceg_hip.mcrng.phiPV_div_k`) and its own run length ``ncycles[c]`` (e.g.
        from :func:`ceg_hip.mcrng.isotherm_ncycles`); all chains run the same ``ninit`` cycles first.  Composed from what exists: a chain
        plan (:meth:`set_chain_plan`) with ``stop_step[c] = (ninit + ncycles[c]) * steps_per_cycle``, a series-only sampler with one frame
        per production cycle, and :meth:`run_montecarlo` over ``max(ncycles)`` production cycles -- baseline, ``ninit`` cycles, baseline,
        production, baseline.  The call is as long as the longest chain; the others stop at their own last step and stay stopped.

        ``temperature``: a scalar or one per chain (constant, as ``make_isotherm`` asserts).  ``moves`` (one
        :class:`ceg_hip.mcrng.MoveTable` per species; ``run_gcmc`` passes the first through ``MoveTable.for_gcmc``) or a ready ``species``
        table, whose own ``phiPV_div_k`` is not read.  ``supercell``: the unit cells of the MC cell, whose product is the ``Π`` the
        loadings are divided by (parameterinputs.jl:244).  The other arguments as :meth:`run_montecarlo`.

        Refuses to run with a sampler of the caller's installed (``RuntimeError``); a chain plan of the caller's is replaced.  Afterwards
        neither a sampler nor a plan is installed.

        -> :class:`Isotherm`: per chain the mean loading, the loadings ``count[0] / Π`` and the energies (K) after each of its OWN
        production cycles, the outcome of the reference's drift check at rtol 1e-9 (``drift_ok``, with ``recorded`` and ``actual``), and the
        underlying :class:`MonteCarloRun`."""
        k = len(self.chains)
        if self.sampler is not None:
            raise RuntimeError("make_isotherm installs a sampler of its own: remove yours first (set_sampler(None))")
        n = np.asarray(ncycles)
        if n.shape != (k,) or n.dtype.kind not in "iu" or (n < 0).any():
            raise ValueError(f"ncycles: one run length >= 0 per chain ({k})")
        ninit = int(ninit)
        if ninit < 0:
            raise ValueError("ninit must be >= 0")
        phi, _ = self.chain_plan_arrays(k, phiPV_div_k, None)
        if phi is None:
            raise ValueError("phiPV_div_k: one row per chain")
        pi = int(np.prod([int(x) for x in supercell]))
        if len(supercell) != 3 or pi < 1:
            raise ValueError("supercell: three integers >= 1")
        if species is None:
            if moves is None:
                raise ValueError("moves or species")
            species = self.gcmc_species(moves, list(phi[0]), self_reciprocal, bead)
        species = np.ascontiguousarray(species)
        from . import mcrng
        L = int(steps_per_cycle) if steps_per_cycle is not None else self.numsteps([mcrng.MoveTable(cumulatives=row["cumulative"]) for row in species])[0]
        longest = int(n.max())
        try:
            self.set_chain_plan(phi, (ninit + n.astype(np.int64)) * L)
            self.set_sampler(L, from_step=ninit * L, series_capacity=longest)
            run = self.run_montecarlo(temperature, longest, ninit, seed=seed, steps_per_cycle=steps_per_cycle, dmax=dmax, thetamax=thetamax,
                                      gcmc=dict(species=species, max_molecules=max_molecules), adapt=adapt, stream_id=stream_id, bead=bead,
                                      positions=positions, check_drift=False)
            series = self.sampler_read()[1]
        finally:
            self.set_sampler(None)
            self.set_chain_plan()
        loadings = [series["count"][:int(n[c]), c, 0] / pi for c in range(k)]
        actual = np.array([float(r) for r in run.baselines[2]])
        drift_ok = np.abs(run.recorded - actual) <= 1e-9 * np.maximum(np.abs(run.recorded), np.abs(actual))
        return Isotherm(np.array([x.mean() if len(x) else np.nan for x in loadings]), loadings, [run.energies[:int(n[c]), c] for c in range(k)],
                        drift_ok, run.recorded, actual, run)

    def set_sampler(self, every: Optional[int], from_step: int = 0, step: Optional[float] = None, dims=None, supercell=(1, 1, 1), channels=None,
                    chain_map=None, symmetries=(), series_capacity: int = 0) -> None:
        """``ceg_mc_group_set_sampler``: from now on :meth:`sweep` and :meth:`sweep_gcmc` take a frame after every absolute step ``s``
        with ``s >= from_step`` and ``(s + 1) % every == 0`` -- one more launch that bins every atom of every chain as
        ``bin_trajectory`` does (averageclusters.jl:154-202) and appends one record per chain (molecule counts, running energy
        change) to the series; :meth:`sampler_read` fetches both.  ``every=None`` removes the sampler.

        The map lives on the unit cell: the MC cell with its columns divided by ``supercell``.  ``dims = (na, nb, nc)``, or from
        ``step`` (A) as ``floor(cell_lengths(unit cell) / step)`` (:169); neither: no map, the series only.  ``channels``: the channel
        of every force-field kind -- a dict from kind (0-based index, or the force field's symbol) to channel, kinds not named are
        not binned; or one entry per kind with -1 for "not binned"; default: every kind into channel 0.  ``chain_map``: the map of
        every chain, -1 for a chain that is not binned (default: all chains pooled in map 0).  ``symmetries``: operations
        ``(R[3, 3], t[3])`` on the fractional coordinates of the unit cell, each adding one count per atom (:185-188).
        ``series_capacity``: the frames the series can hold; a sweep (or :meth:`sample`) whose frames would not fit is refused.
        What was installed is kept in ``self.sampler`` (``unit_invmat``, ``dims``, ``channels``, ``chain_map``, ``symmetries``,
        ``supercell``) for :func:`ceg_hip.mcrng.bin_positions`."""
        if every is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_set_sampler(self._h, None))
            self.sampler = None
            return
        k = len(self.chains)
        mc = self.chains[0].mc
        nkinds = mc.ff.nkinds
        supercell = tuple(int(x) for x in supercell)
        if len(supercell) != 3 or min(supercell) < 1:
            raise ValueError("supercell: three integers >= 1")
        unit = np.asarray(mc.mat, dtype=np.float64) / np.asarray(supercell, dtype=np.float64)[None, :]
        unit_invmat = np.linalg.inv(unit)
        if dims is None and step is not None:
            dims = np.floor(np.linalg.norm(unit, axis=0) / float(step)).astype(np.int64)
        with_map = dims is not None
        dims = np.ascontiguousarray(dims if with_map else (0, 0, 0), dtype=np.int32)
        if dims.shape != (3,):
            raise ValueError("dims: (na, nb, nc)")
        if channels is None:
            kind_channel = np.zeros(nkinds, dtype=np.int32)
        elif isinstance(channels, dict):
            kind_channel = np.full(nkinds, -1, dtype=np.int32)
            for key, ch in channels.items():
                kind_channel[mc.ff.sdict[key] - 1 if isinstance(key, str) else int(key)] = ch
        else:
            kind_channel = np.ascontiguousarray(channels, dtype=np.int32)
            if kind_channel.shape != (nkinds,):
                raise ValueError(f"channels: one entry per force-field kind ({nkinds})")
        cmap = np.ascontiguousarray(np.zeros(k) if chain_map is None else chain_map, dtype=np.int32)
        if cmap.shape != (k,):
            raise ValueError(f"chain_map: one entry per chain ({k})")
        if with_map and (cmap.max() < 0 or kind_channel.max(initial=-1) < 0):
            raise ValueError("a map needs at least one chain with a map (chain_map >= 0) and one kind with a channel (channels >= 0)")
        sym = np.zeros((len(symmetries), 3, 4), dtype=np.float64)
        for q, op in enumerate(symmetries):
            if len(op) == 2:
                sym[q, :, :3], sym[q, :, 3] = np.asarray(op[0], dtype=np.float64).reshape(3, 3), np.asarray(op[1], dtype=np.float64).reshape(3)
            else:
                sym[q] = np.asarray(op, dtype=np.float64).reshape(3, 4)
        spec = _abi.MC_SAMPLER(int(every), int(from_step), int(series_capacity), (C.c_int32 * 3)(*[int(d) for d in dims]),
                               int(cmap.max()) + 1 if with_map else 0, int(kind_channel.max()) + 1 if with_map else 0, nkinds, len(sym), 0,
                               (C.c_double * 9)(*unit_invmat.T.reshape(-1)), cmap.ctypes.data, kind_channel.ctypes.data, sym.ctypes.data if len(sym) else None)
        _abi.check(self._lib, self._lib.ceg_mc_group_set_sampler(self._h, C.addressof(spec)))
        self.sampler = dict(every=int(every), from_step=int(from_step), series_capacity=int(series_capacity), dims=tuple(int(d) for d in dims),
                            nmaps=int(spec.nmaps), nchannels=int(spec.nchannels), unit_invmat=unit_invmat, supercell=supercell,
                            channels=kind_channel, chain_map=cmap, symmetries=sym)

    def _sampler(self):
        s = getattr(self, "sampler", None)
        if s is None:
            raise RuntimeError("no sampler installed: set_sampler first")
        return s

    def sample(self) -> None:
        """``ceg_mc_group_sample``: one frame of the resident state, now (asynchronous, ordered with the group's other calls) -- for
        runs driven through :meth:`trial` / :meth:`accept`.  Its records carry ``step == -1``."""
        self._sampler()
        _abi.check(self._lib, self._lib.ceg_mc_group_sample(self._h))

    def sampler_read(self):
        """``ceg_mc_group_sampler_read`` -> ``(bins, series, total)``: ``bins`` int64 ``[nmaps, nchannels, nc, nb, na]`` (``None`` without
        a map), ``series`` ``[frames, K]`` of ``_abi.MC_SAMPLE_RECORD_DTYPE``, and ``total[map] = frames * (1 + nsym) * prod(supercell) *
        chains on that map``: the ``total`` of ``bin_trajectories`` over the chains' trajectories (averageclusters.jl:196,233-234), so that
        ``bins[map, channel] / total[map]`` is the density map."""
        s = self._sampler()
        frames = C.c_int64(0)
        _abi.check(self._lib, self._lib.ceg_mc_group_sampler_read(self._h, None, None, C.byref(frames)))
        k = len(self.chains)
        na, nb, nc = s["dims"]
        bins = np.zeros((s["nmaps"], s["nchannels"], nc, nb, na), dtype=np.int64) if s["nmaps"] else None
        series = np.zeros((int(frames.value), k), dtype=_abi.MC_SAMPLE_RECORD_DTYPE)
        _abi.check(self._lib, self._lib.ceg_mc_group_sampler_read(self._h, _abi.i64ptr(bins.reshape(-1)) if bins is not None else None,
                                                                  series.ctypes.data if series.size else None, None))
        per_frame = (1 + len(s["symmetries"])) * int(np.prod(s["supercell"]))
        total = np.array([int(frames.value) * per_frame * int((s["chain_map"] == m).sum()) for m in range(s["nmaps"])], dtype=np.int64)
        return bins, series, total

    def sampler_reset(self) -> None:
        """``ceg_mc_group_sampler_reset``: bins, series and frame count back to zero."""
        self._sampler()
        _abi.check(self._lib, self._lib.ceg_mc_group_sampler_reset(self._h))

    def set_recorder(self, every: Optional[int], origin: int = 0, capacity: int = 1024, energies=None, track_min: bool = False,
                     max_atoms: Optional[int] = None, max_molecules: Optional[int] = None) -> None:
        """``ceg_mc_group_set_recorder``: from now on :meth:`sweep_cycles` and :meth:`sweep_gcmc_cycles` copy every chain's configuration
        into device memory at the end of every cycle ``cc`` with ``cc >= origin and (cc - origin) % every == 0`` (``every=0``: no
        periodic frames) -- the trajectory ``run_montecarlo!`` writes every ``printevery`` cycles (simulation.jl:784-799) -- and, with
        ``track_min``, keep per chain the lowest-energy configuration seen at any cycle end (``RMinimumEnergy``,
        parameterinputs.jl:86-108), with no host round trip; :meth:`recorder_read` / :meth:`recorder_minimum` read everything once,
        after the run.  ``energies``: the total energy of every chain now (K; default: the totals of :meth:`baseline_energies`);
        ``capacity``: the frames kept; ``max_atoms`` / ``max_molecules``: the room of a frame per chain, by default what the largest
        chain holds now -- for GCMC pass the sweep's ``max_molecules``, and ``max_atoms`` follows from the largest species.
        ``every=None`` removes the recorder.  :meth:`run_montecarlo` rebases an installed recorder at its two baselines.  Any other call
        that moves a chain (``sweep``, ``accept``, ``insert``, :meth:`restore` ...) makes the running energies stale:
        :meth:`recorder_rebase`.  ``track_min`` is refused under GCMC swaps (``delta_swaps`` is the rule's ``diff``, not the state's
        energy change).  :func:`ceg_hip.mcrng.snapshot_cycles` / :func:`ceg_hip.mcrng.track_minimum` restate the schedule and the rule."""
        if every is None:
            _abi.check(self._lib, self._lib.ceg_mc_group_set_recorder(self._h, None))
            self.recorder = None
            return
        k = len(self.chains)
        if energies is None:
            energies = [float(r) for r in self.baseline_energies()]
        E = np.ascontiguousarray(energies, dtype=np.float64)
        if E.shape != (k,):
            raise ValueError(f"energies: one per chain ({k})")
        largest = max((len(ids) for chain in self.chains for ids in chain.mc.ffidx), default=1)
        if max_molecules is None:
            max_molecules = max(sum(len(kind) for kind in chain._slot) for chain in self.chains)
            if max_atoms is None:
                max_atoms = max(sum(len(chain.mc.ffidx[i]) * len(kind) for i, kind in enumerate(chain._slot)) for chain in self.chains)
        elif max_atoms is None:
            max_atoms = int(max_molecules) * largest
        max_atoms, max_molecules = max(int(max_atoms), 1), max(int(max_molecules), 1)
        spec = _abi.McRecorder(int(every), int(origin), int(capacity), max_atoms, max_molecules, 1 if track_min else 0, 0, E.ctypes.data)
        _abi.check(self._lib, self._lib.ceg_mc_group_set_recorder(self._h, C.addressof(spec)))
        self.recorder = dict(every=int(every), origin=int(origin), capacity=int(capacity), track_min=bool(track_min), max_atoms=max_atoms,
                             max_molecules=max_molecules)

    def _recorder(self):
        r = getattr(self, "recorder", None)
        if r is None:
            raise RuntimeError("no recorder installed: set_recorder first")
        return r

    def snapshot(self) -> None:
        """``ceg_mc_group_snapshot``: one frame of the resident state, now (asynchronous, ordered with the group's other calls).  Its
        records carry ``cycle == step == -1`` and the recorder's running energy; the species of its molecules are -1."""
        self._recorder()
        _abi.check(self._lib, self._lib.ceg_mc_group_snapshot(self._h))

    def recorder_rebase(self, energies) -> None:
        """``ceg_mc_group_recorder_rebase``: replace the recorder's running energies (K, one per chain) -- the precise energy at the
        first production cycle (simulation.jl:788-790).  The minimum is neither tested nor reset."""
        self._recorder()
        E = np.ascontiguousarray(energies, dtype=np.float64)
        if E.shape != (len(self.chains),):
            raise ValueError(f"energies: one per chain ({len(self.chains)})")
        _abi.check(self._lib, self._lib.ceg_mc_group_recorder_rebase(self._h, _abi.dptr(E)))

    @staticmethod
    def _recorder_bodies(records, xyz, kind, first, species):
        """[n, K] records and the four padded arrays -> per record (positions, kinds, mol_first, species) trimmed to the counts (empty
        where the record carries no body)"""
        out = []
        for f in range(records.shape[0]):
            row = []
            for c in range(records.shape[1]):
                r = records[f, c]
                na, nm = (0, 0) if r["flags"] & _abi.MC_SNAPSHOT_NO_BODY else (int(r["natoms"]), int(r["nmol"]))
                row.append((xyz[f, c, :na].copy(), kind[f, c, :na].copy(), first[f, c, :nm + 1].copy(), species[f, c, :nm].copy()))
            out.append(row)
        return out

    def recorder_read(self, first_frame: int = 0, nframes: Optional[int] = None):
        """``ceg_mc_group_recorder_read`` -> ``(records, frames)``: ``records`` ``[n, K]`` of ``_abi.MC_SNAPSHOT_RECORD_DTYPE`` for the
        frames ``first_frame .. first_frame + nframes`` (default: all from ``first_frame``), and ``frames[f][c]`` = (positions
        ``[natoms, 3]``, kinds int32 ``[natoms]`` 0-based, mol_first int32 ``[nmol + 1]``, species int32 ``[nmol]``) of chain ``c`` in
        molecule order -- what ``ceg_mc_get_state`` returns and ``ceg_mc_set_guests`` takes (:meth:`restore`).  A record with flag 1
        (the chain did not fit ``max_atoms`` / ``max_molecules``) has the true counts and an empty body."""
        s = self._recorder()
        taken = C.c_int64(0)
        _abi.check(self._lib, self._lib.ceg_mc_group_recorder_read(self._h, 0, 0, None, None, None, None, None, C.byref(taken)))
        first_frame = int(first_frame)
        n = int(taken.value) - first_frame if nframes is None else int(nframes)
        k, ma, mm = len(self.chains), s["max_atoms"], s["max_molecules"]
        records = np.zeros((max(n, 0), k), dtype=_abi.MC_SNAPSHOT_RECORD_DTYPE)
        xyz, kind = np.zeros((max(n, 0), k, ma, 3)), np.zeros((max(n, 0), k, ma), dtype=np.int32)
        first, species = np.zeros((max(n, 0), k, mm + 1), dtype=np.int32), np.zeros((max(n, 0), k, mm), dtype=np.int32)
        some = n > 0
        _abi.check(self._lib, self._lib.ceg_mc_group_recorder_read(self._h, first_frame, n, records.ctypes.data if some else None,
                                                                   _abi.dptr(xyz.reshape(-1)) if some else None, _abi.i32ptr(kind.reshape(-1)) if some else None,
                                                                   _abi.i32ptr(first.reshape(-1)) if some else None,
                                                                   _abi.i32ptr(species.reshape(-1)) if some else None, None))
        return records, self._recorder_bodies(records, xyz, kind, first, species)

    def recorder_minimum(self):
        """``ceg_mc_group_recorder_min`` -> ``(mink int64[K], mine float64[K], records [K], bodies)``: per chain the cycle at whose end
        the lowest energy was seen (-1: the state at :meth:`set_recorder`), that energy, its record and ``bodies[c]`` = (positions,
        kinds, mol_first, species) as :meth:`recorder_read` gives them."""
        s = self._recorder()
        k, ma, mm = len(self.chains), s["max_atoms"], s["max_molecules"]
        mink, mine = np.zeros(k, dtype=np.int64), np.zeros(k)
        records = np.zeros((1, k), dtype=_abi.MC_SNAPSHOT_RECORD_DTYPE)
        xyz, kind = np.zeros((1, k, ma, 3)), np.zeros((1, k, ma), dtype=np.int32)
        first, species = np.zeros((1, k, mm + 1), dtype=np.int32), np.zeros((1, k, mm), dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_mc_group_recorder_min(self._h, _abi.i64ptr(mink), _abi.dptr(mine), records.ctypes.data, _abi.dptr(xyz.reshape(-1)),
                                                                  _abi.i32ptr(kind.reshape(-1)), _abi.i32ptr(first.reshape(-1)), _abi.i32ptr(species.reshape(-1))))
        return mink, mine, records[0], self._recorder_bodies(records, xyz, kind, first, species)[0]

    def restore(self, chain_index: int, frame) -> None:
        """Put a frame of :meth:`recorder_read` / :meth:`recorder_minimum` -- (positions, kinds, mol_first, species) -- back into chain
        ``chain_index`` through ``ceg_mc_set_guests`` and refresh the chain's host side (``mc.positions``, the molecule order, the tail
        correction where the counts change).  Species of -1 (a frame of the plain entry point) are taken from the molecules' kinds.
        The recorder's and a tempering state's energies of that chain are stale afterwards."""
        chain = self.chains[int(chain_index)]
        mc = chain.mc
        pos, kinds, first, species = frame
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        first = np.ascontiguousarray(first, dtype=np.int32)
        if len(first) < 1 or first[-1] != len(kinds) or len(pos) != len(kinds):
            raise ValueError("the frame has no body (a record with flag 1?) or its arrays disagree")
        nmol = len(first) - 1
        by_kinds = {}
        for i, ids in enumerate(mc.ffidx):
            by_kinds.setdefault(tuple(int(q) - 1 for q in ids), i)
        spec = []
        for j in range(nmol):
            i = int(species[j]) if len(species) > j and species[j] >= 0 else by_kinds.get(tuple(int(q) for q in kinds[first[j]:first[j + 1]]))
            if i is None or not 0 <= i < len(mc.ffidx) or tuple(int(q) - 1 for q in mc.ffidx[i]) != tuple(int(q) for q in kinds[first[j]:first[j + 1]]):
                raise ValueError(f"molecule {j} of the frame matches no species of the chain")
            spec.append(i)
        _abi.check(self._lib, self._lib.ceg_mc_set_guests(chain._h, _abi.dptr(pos.reshape(-1)) if len(pos) else None, _abi.i32ptr(kinds) if len(kinds) else None,
                                                          _abi.i32ptr(first), nmol))
        before = [len(kind) for kind in chain._slot]
        chain._slot = [[j for j in range(nmol) if spec[j] == i] for i in range(len(mc.positions))]
        mc.positions = [[pos[first[j]:first[j + 1]].copy() for j in kind] for kind in chain._slot]
        if mc.tail_cross is not None:                # mc.tailcorrection follows the species counts (modify_species!, montecarlo.jl:814,858)
            from .hostmirror.montecarlo import modify_species_dryrun
            counts = list(before)
            for i, kind in enumerate(chain._slot):
                while counts[i] != len(kind):
                    num = 1 if counts[i] < len(kind) else -1
                    mc.tailcorrection += modify_species_dryrun(mc.tail_framework, mc.tail_cross, counts, i, num)
                    counts[i] += num

    def close(self) -> None:
        if getattr(self, "_h", None):
            rc = self._lib.ceg_mc_group_destroy(self._h)
            self._h = None
            for c in self.chains:
                c._group = None
            _abi.check(self._lib, rc)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
