"""Site hopping on the device (``ceg_site_group_*``, ``csrc/ceg_site.hip``): the reference's second Monte-Carlo model
(``src/sitehopping.jl``), in which a mobile species hops between a finite set of sites and all physics is folded into two tables,
``frameworkenergies[n]`` and ``interactions[n, n]``.

:class:`SiteHopping` holds the tables, a population and the tail correction; :class:`DeviceSiteHoppingGroup` keeps K chains on one
copy of the tables on the device and runs whole cycles of all of them inside one kernel; :func:`run_montecarlo` and
:func:`run_random_quenching` are ``run_montecarlo!(::SiteHopping, ...; groupcycles, restartgroupcycle)`` (simulation.jl:863-1010) and
``run_random_quenching`` on top of it.  With ``groupcycles = G`` a cycle is G m hops accepted or rejected as one move, and with
``restartgroupcycle`` it first restarts from a fresh random population (basin hopping): ``DeviceSiteHoppingGroup.sweep_grouped``,
every cycle, decision, restore and restart inside one kernel (``mcrng.site_grouped_replay``).  Sites are 0-based here (the reference's are 1-based).  The step itself is specified in
``include/ceg_hip.h`` and restated in :mod:`ceg_hip.mcrng` (``site_step``, ``site_replay``).  :func:`run_parallel_tempering` is the
reference's routine of that name (simulation.jl:461-634) on ``DeviceSiteHoppingGroup.set_tempering``: ladders of rungs that exchange
configurations per step inside the sweep kernel (``mcrng.site_ladder_replay``).

:func:`build_site_tables` is the reference's constructor (sitehopping.jl:41-82): both tables from a guest-free
:class:`ceg_hip.energy.DeviceMonteCarlo` of the mobile species in three launches (``ceg_site_tables``)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _abi, mcrng


class SiteHopping:
    """``SiteHopping`` of the reference, without the geometry: ``frameworkenergies`` float64[n] (K), ``interactions`` float64[n, n] (K,
    symmetric, the diagonal 1e100), ``population`` uint16[m] (0-based sites, no site twice) and ``tailcorrection`` (K).

    ``population`` may be an integer m: then it is ``mcrng.site_random_population(seed, stream_id, n, m)``, the ``randperm`` start of
    sitehopping.jl:85-88 drawn from the Philox stream."""

    def __init__(self, frameworkenergies, interactions, population, tailcorrection: float = 0.0, *, seed: int = 0, stream_id: int = 0):
        self.frameworkenergies = np.ascontiguousarray(frameworkenergies, dtype=np.float64).reshape(-1)
        n = len(self.frameworkenergies)
        self.interactions = np.ascontiguousarray(interactions, dtype=np.float64)
        if self.interactions.shape != (n, n):
            raise ValueError(f"interactions must be [{n}, {n}]")
        if n > 65535:
            raise ValueError("Cannot handle more than 65535 different sites")                  # sitehopping.jl:25
        if isinstance(population, (int, np.integer)):
            population = mcrng.site_random_population(seed, stream_id, n, int(population))
        self.population = check_population(population, n)
        self.tailcorrection = float(tailcorrection)

    @classmethod
    def from_setup(cls, mc, sites, population, *, species: int = 0, tailcorrection: Optional[float] = None, device: int = 0, seed: int = 0,
                   stream_id: int = 0) -> "SiteHopping":
        """``SiteHopping(sites, framework, forcefield, syst_mol, population)`` (sitehopping.jl:23-96): ``mc`` is the
        ``MonteCarloSetup`` of the mobile species alone WITHOUT molecules (``setup_montecarlo(..., [(molecule, 0)], blockfiles=[False])``),
        or a guest-free ``DeviceMonteCarlo`` of it; the tables are built on the device (:func:`build_site_tables`).  The tail
        correction depends on the number of molecules and is the caller's (default: the setup's own)."""
        from .energy import DeviceMonteCarlo
        dev = mc if isinstance(mc, DeviceMonteCarlo) else DeviceMonteCarlo(mc, device, upload_guests=False)
        try:
            fw, _rec, it = build_site_tables(dev, sites, species)
        finally:
            if dev is not mc:
                dev.close()
        tail = float(getattr(dev.mc, "tailcorrection", 0.0)) if tailcorrection is None else float(tailcorrection)
        sh = cls(fw, it, population, tail, seed=seed, stream_id=stream_id)
        sh.sites = np.ascontiguousarray(sites, dtype=np.float64).reshape(len(fw), -1, 3)
        return sh

    @property
    def nsites(self) -> int:
        return len(self.frameworkenergies)

    def baseline_energy(self) -> float:
        """``baseline_energy(sh)`` (sitehopping.jl:105-112) on the host, in extended precision."""
        return float(mcrng.site_baseline(self.frameworkenergies, self.interactions, self.population, self.tailcorrection))

    def __repr__(self):
        return f"SiteHopping setup with {len(self.population)} molecules among {self.nsites} sites"


def ewald_offsets(mc, species: int, shape):
    """The count-dependent constants of the ``EwaldContext`` (ewald.jl:497-544) that the tables carry: with
    ``c(N) = 2 energy_net_charges(N) + static_contribution(N)`` for N molecules of ``species`` alone, ``(c(1), c(2) - 2 c(1))``;
    ``shape`` float64[m_atoms, 3]: the rigid molecule (any site).  ``(0.0, 0.0)`` without Ewald summation."""
    from .hostmirror.ewald import ewald_context_constants
    from .hostmirror.raspa import RASPASystem
    if mc.ewald.alpha == 0.0:
        return 0.0, 0.0
    shape = np.asarray(shape, dtype=np.float64).reshape(-1, 3)
    m = len(shape)
    q = np.array([mc.charges[ix] for ix in mc.ffidx[species]], dtype=np.float64)
    one = RASPASystem(mc.mat, shape, [""] * m, np.zeros(m), q, True)

    def c(count):
        enc, static = ewald_context_constants(mc.ewald, [[one] * count])
        return 2.0 * enc + static
    return c(1), c(2) - 2.0 * c(1)


def build_site_tables(dev, sites, species: int = 0, on_device: bool = False):
    """``ceg_site_tables``: (framework[n], recip[n], interactions[n, n]) in K for the ``sites`` float64[n, m_atoms, 3] (Cartesian A) of
    species ``species`` of ``dev``, a :class:`ceg_hip.energy.DeviceMonteCarlo` that holds no guest (``upload_guests=False`` on a setup
    without molecules).  ``framework[i] = Number(baseline_energy({s_i}).er)``, ``recip[i]`` its inter + reciprocal part
    (``ewaldenergies[i]``), ``interactions[i, j]`` = inter + reciprocal of ``baseline_energy({s_i, s_j}).er`` minus ``recip[i]`` minus
    ``recip[j]``, the diagonal 1e100.  ``on_device``: three float64 torch tensors on the handle's device (``ceg_site_tables_device``),
    which :class:`DeviceSiteHoppingGroup` reads in place."""
    mc = dev.mc
    kinds = np.ascontiguousarray([ix - 1 for ix in mc.ffidx[species]], dtype=np.int32)
    pos = np.ascontiguousarray(sites, dtype=np.float64).reshape(-1, len(kinds), 3)
    n = len(pos)
    off1, off2 = ewald_offsets(mc, species, pos[0]) if n else (0.0, 0.0)
    lib = dev._lib
    if on_device:
        import torch
        fw, rec = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
        it = torch.empty((n, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _abi.check(lib, lib.ceg_site_tables_device(dev._h, _abi.i32ptr(kinds), len(kinds), _abi.dptr(pos.reshape(-1)), n, off1, off2,
                                                   C.c_void_p(fw.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(it.data_ptr())))
        return fw, rec, it
    fw, rec, it = np.empty(n), np.empty(n), np.empty((n, n))
    _abi.check(lib, lib.ceg_site_tables(dev._h, _abi.i32ptr(kinds), len(kinds), _abi.dptr(pos.reshape(-1)), n, off1, off2, _abi.dptr(fw),
                                        _abi.dptr(rec), _abi.dptr(it.reshape(-1))))
    return fw, rec, it


def check_population(population, n: int) -> np.ndarray:
    """-> uint16[m]; raises where a site is outside ``0..n-1`` or used twice."""
    p = np.asarray(population)
    if p.ndim != 1 or (p.size and (p.min() < 0 or p.max() >= n)):
        raise ValueError(f"Cannot populate site {int(p.max()) if p.size else -1} among {n} sites")   # sitehopping.jl:93
    if len(np.unique(p)) != len(p):
        raise ValueError("a site is populated twice")
    return np.ascontiguousarray(p, dtype=np.uint16)


class DeviceSiteHoppingGroup:
    """K chains of m molecules on one copy of the tables, resident on ``device`` (``ceg_site_group_t``).

    ``populations``: integer [K, m] (0-based sites).  ``frameworkenergies`` / ``interactions`` may be torch tensors on that device
    (float64, contiguous): the group then reads them in place and keeps a reference."""

    def __init__(self, frameworkenergies, interactions, populations, tailcorrection: float = 0.0, device: int = 0):
        self._lib = _abi.load_library()
        self._h = None
        self.rungs = None                 # set_tempering
        pops = np.ascontiguousarray(populations)
        if pops.ndim != 2:
            raise ValueError("populations must be [K, m]")
        if pops.size and (pops.min() < 0 or pops.max() > 65535):
            raise ValueError("sites must fit UInt16")
        pops = np.ascontiguousarray(pops, dtype=np.uint16)
        self.k, self.m = (int(x) for x in pops.shape)
        on_device = hasattr(frameworkenergies, "data_ptr")
        if on_device != hasattr(interactions, "data_ptr"):
            raise ValueError("both tables on the device or both on the host")
        if on_device:
            import torch
            for t in (frameworkenergies, interactions):
                if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or (t.device.index or 0) != device:
                    raise ValueError("device tables must be contiguous float64 tensors on the group's device")
            self.n = int(frameworkenergies.numel())
            if tuple(interactions.shape) != (self.n, self.n):
                raise ValueError(f"interactions must be [{self.n}, {self.n}]")
            torch.cuda.synchronize(device)
            self._keep = (frameworkenergies, interactions)
            fw, it = C.c_void_p(frameworkenergies.data_ptr()), C.c_void_p(interactions.data_ptr())
        else:
            f = np.ascontiguousarray(frameworkenergies, dtype=np.float64).reshape(-1)
            i = np.ascontiguousarray(interactions, dtype=np.float64)
            self.n = len(f)
            if i.shape != (self.n, self.n):
                raise ValueError(f"interactions must be [{self.n}, {self.n}]")
            self._keep = (f, i)
            fw, it = C.c_void_p(f.ctypes.data), C.c_void_p(i.ctypes.data)
        self.tailcorrection = float(tailcorrection)
        h = C.c_void_p()
        _abi.check(self._lib, self._lib.ceg_site_group_create(int(device), self.n, self.m, self.k, fw, it, 1 if on_device else 0,
                                                              C.c_void_p(pops.ctypes.data), self.tailcorrection, C.byref(h)))
        self._h = h

    @classmethod
    def from_setups(cls, setups, device: int = 0) -> "DeviceSiteHoppingGroup":
        """One chain per :class:`SiteHopping`; all must share the tables of the first."""
        first = setups[0]
        for sh in setups[1:]:
            if sh.frameworkenergies is not first.frameworkenergies and not (
                    np.array_equal(sh.frameworkenergies, first.frameworkenergies) and np.array_equal(sh.interactions, first.interactions)):
                raise ValueError("the chains of a group share one pair of tables")
            if sh.tailcorrection != first.tailcorrection or len(sh.population) != len(first.population):
                raise ValueError("the chains of a group share the tail correction and the number of molecules")
        return cls(first.frameworkenergies, first.interactions, np.stack([sh.population for sh in setups]), first.tailcorrection, device)

    def _sweep(self, ncycles, seed, first_step, temperature, steps_per_cycle, cycle0, stream_id, log, restart=None):
        """The arguments and buffers that ``sweep_cycles`` and ``sweep_grouped`` (``restart`` not None) share, and the call."""
        ncycles = int(ncycles)
        spc = self.m if steps_per_cycle is None else int(steps_per_cycle)
        T = np.asarray(temperature, dtype=np.float64)
        T = np.ascontiguousarray(np.broadcast_to(T if T.ndim == 2 else T.reshape(1, -1), (max(ncycles, 0), self.k)), dtype=np.float64)
        ids = None if stream_id is None else np.ascontiguousarray(stream_id, dtype=np.uint32)
        if ids is not None and ids.shape != (self.k,):
            raise ValueError("stream_id must be [K]")
        params = _abi.SiteParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step), ids.ctypes.data if ids is not None else None)
        cycles = _abi.SiteCycles(ncycles, spc, int(cycle0), T.ctypes.data if T.size else None)
        stats = np.zeros(self.k, dtype=_abi.SITE_STATS_DTYPE)
        recs = np.zeros((max(ncycles, 0), self.k), dtype=_abi.SITE_CYCLE_RECORD_DTYPE)
        steps = np.zeros((max(ncycles, 0) * spc, self.k), dtype=_abi.SITE_RECORD_DTYPE) if log else None
        out = (stats.ctypes.data, recs.ctypes.data if recs.size else None, steps.ctypes.data if (steps is not None and steps.size) else None)
        if restart is None:
            _abi.check(self._lib, self._lib.ceg_site_group_sweep_cycles(self._h, C.byref(params), C.byref(cycles), *out))
            return stats, recs, steps
        grouped = np.zeros((max(ncycles, 0), self.k), dtype=_abi.SITE_GROUPED_RECORD_DTYPE)
        _abi.check(self._lib, self._lib.ceg_site_group_sweep_grouped(self._h, C.byref(params), C.byref(cycles), int(restart), *out,
                                                                     grouped.ctypes.data if grouped.size else None))
        return stats, recs, steps, grouped

    def sweep_cycles(self, ncycles: int, seed: int, first_step: int = 0, *, temperature, steps_per_cycle: Optional[int] = None, cycle0: int = 0,
                     stream_id=None, log: bool = False):
        """``ceg_site_group_sweep_cycles``: ``ncycles`` cycles of ``steps_per_cycle`` (default m, as the reference) steps of every chain.
        ``temperature``: a scalar, [K] or [ncycles, K].  -> (stats [K] ``_abi.SITE_STATS_DTYPE``, cycle records [ncycles, K]
        ``_abi.SITE_CYCLE_RECORD_DTYPE``, log [ncycles * steps_per_cycle, K] ``_abi.SITE_RECORD_DTYPE`` or None)."""
        return self._sweep(ncycles, seed, first_step, temperature, steps_per_cycle, cycle0, stream_id, log)

    def sweep_grouped(self, ncycles: int, seed: int, first_step: int = 0, *, temperature, steps_per_cycle: Optional[int] = None, cycle0: int = 0,
                      stream_id=None, restart: int = 0, log: bool = False):
        """``ceg_site_group_sweep_grouped``: ``ncycles`` grouped cycles of ``steps_per_cycle`` (default m; ``groupcycles = G`` of the
        reference is G m) steps of every chain: the hops of a cycle are accepted or rejected as one move against the energy at its
        start, and with ``restart`` (0 or 1, as the library takes it) every cycle begins from a fresh random population (the rule:
        ``include/ceg_hip.h``, restated as ``mcrng.site_grouped_replay``).  Arguments as :meth:`sweep_cycles`.  -> (stats, cycle
        records, log or None, grouped records [ncycles, K] ``_abi.SITE_GROUPED_RECORD_DTYPE``).  Refused while tempering is installed."""
        return self._sweep(ncycles, seed, first_step, temperature, steps_per_cycle, cycle0, stream_id, log, restart=restart)

    def stats(self) -> np.ndarray:
        """The counters, ``delta`` and the running energy of every chain now (a call of no cycles)."""
        return self.sweep_cycles(0, 0, temperature=1.0)[0]

    def baseline_energies(self) -> np.ndarray:
        """``baseline_energy`` (sitehopping.jl:105-112) of every chain, one launch -> float64[K]."""
        out = np.empty(self.k, dtype=np.float64)
        _abi.check(self._lib, self._lib.ceg_site_group_baseline(self._h, _abi.dptr(out)))
        return out

    def rebase(self) -> None:
        """Every chain's running energy becomes its baseline (the reference's ``idx_cycle == 0`` step)."""
        _abi.check(self._lib, self._lib.ceg_site_group_rebase(self._h))

    def populations(self) -> np.ndarray:
        out = np.empty((self.k, self.m), dtype=np.uint16)
        _abi.check(self._lib, self._lib.ceg_site_group_get_populations(self._h, out.ctypes.data))
        return out

    def set_populations(self, populations) -> None:
        """Replaces every chain's population (validated as at creation) and rebases."""
        p = np.asarray(populations)
        if p.shape != (self.k, self.m) or (p.size and (p.min() < 0 or p.max() > 65535)):
            raise ValueError("populations must be [K, m] of sites that fit UInt16")
        p = np.ascontiguousarray(p, dtype=np.uint16)
        _abi.check(self._lib, self._lib.ceg_site_group_set_populations(self._h, p.ctypes.data))

    def set_recorder(self, every: Optional[int], origin: int = 0, capacity: int = 1024, track_min: bool = False) -> None:
        """Frames of every chain's population and energy at the cycle ends where ``mcrng.snapshot_due(cc, origin, every)`` holds, and
        with ``track_min`` the population of the lowest cycle-end energy (``RMinimumEnergy``), both written inside the sweep kernel.
        ``every=None`` removes the recorder; ``every=0`` with ``track_min`` keeps the minimum only."""
        if every is None:
            _abi.check(self._lib, self._lib.ceg_site_group_set_recorder(self._h, None))
            return
        spec = _abi.SiteRecorder(int(every), int(origin), int(capacity), 1 if track_min else 0, 0)
        _abi.check(self._lib, self._lib.ceg_site_group_set_recorder(self._h, C.byref(spec)))

    def recorder_read(self, first_frame: int = 0, nframes: Optional[int] = None):
        """-> (records [nframes, K] ``_abi.SITE_FRAME_RECORD_DTYPE``, populations uint16[nframes, K, m])"""
        held = C.c_int64(0)
        _abi.check(self._lib, self._lib.ceg_site_group_recorder_read(self._h, 0, 0, None, None, C.byref(held)))
        if nframes is None:
            nframes = held.value - int(first_frame)
        recs = np.zeros((max(int(nframes), 0), self.k), dtype=_abi.SITE_FRAME_RECORD_DTYPE)
        pops = np.zeros((max(int(nframes), 0), self.k, self.m), dtype=np.uint16)
        _abi.check(self._lib, self._lib.ceg_site_group_recorder_read(self._h, int(first_frame), int(nframes), recs.ctypes.data if recs.size else None,
                                                                     pops.ctypes.data if pops.size else None, C.byref(held)))
        return recs, pops

    def recorder_minimum(self):
        """-> (mink int64[K] (-1: the state at installation), mine float64[K], populations uint16[K, m])"""
        mink, mine = np.zeros(self.k, dtype=np.int64), np.zeros(self.k, dtype=np.float64)
        pops = np.zeros((self.k, self.m), dtype=np.uint16)
        _abi.check(self._lib, self._lib.ceg_site_group_recorder_min(self._h, _abi.i64ptr(mink), _abi.dptr(mine), pops.ctypes.data))
        return mink, mine, pops

    def set_tempering(self, rungs: Optional[int], p: float = 0.1, pair_cdf=None, ladder_stream=None) -> None:
        """``ceg_site_group_set_tempering``: the K chains become K / ``rungs`` ladders (chain ``l * rungs + r`` is rung r of ladder
        l) that exchange configurations per step inside the sweep kernel, by the rule of ``include/ceg_hip.h`` restated in
        :mod:`ceg_hip.mcrng`.  ``pair_cdf`` float64[rungs - 1] (default ``mcrng.site_exchange_cdf(rungs, p)``, the reference's
        ``randsubseq(1:(Npt-1), 0.1)``), ``ladder_stream`` uint32[K / rungs] (default: the ladder's index).  The temperatures of
        later sweeps must rise strictly with the rung inside every ladder.  ``rungs=None`` removes the tempering."""
        if rungs is None:
            _abi.check(self._lib, self._lib.ceg_site_group_set_tempering(self._h, None))
            self.rungs = None
            return
        rungs = int(rungs)
        valid = 2 <= rungs <= _abi.SITE_MAX_RUNGS and self.k % rungs == 0          # (else the library refuses, whatever the tables)
        if pair_cdf is None:
            cdf = mcrng.site_exchange_cdf(rungs, p) if valid else np.zeros(0)
        else:
            cdf = np.ascontiguousarray(pair_cdf, dtype=np.float64).reshape(-1)
        ls = None if ladder_stream is None else np.ascontiguousarray(ladder_stream, dtype=np.uint32).reshape(-1)
        if valid and (len(cdf) != rungs - 1 or (ls is not None and len(ls) != self.k // rungs)):
            raise ValueError("pair_cdf must be [rungs - 1] and ladder_stream [K / rungs]")
        spec = _abi.SiteTempering(rungs, 0, cdf.ctypes.data if cdf.size else None, ls.ctypes.data if ls is not None else None, 0)
        _abi.check(self._lib, self._lib.ceg_site_group_set_tempering(self._h, C.byref(spec)))
        self.rungs = rungs

    def tempering_read(self):
        """-> (attempted int64[K / R, R - 1], accepted int64[K / R, R - 1] per pair of rungs, replica int32[K]: per rung, the rung on
        which the configuration now there sat when tempering was installed)"""
        R = getattr(self, "rungs", None)
        if not R:
            _abi.check(self._lib, self._lib.ceg_site_group_tempering_read(self._h, None, None, None))     # raises: nothing installed
            raise RuntimeError("the group has no tempering")
        att, acc = (np.zeros((self.k // R, R - 1), dtype=np.int64) for _ in range(2))
        rep = np.zeros(self.k, dtype=np.int32)
        _abi.check(self._lib, self._lib.ceg_site_group_tempering_read(self._h, _abi.i64ptr(att.reshape(-1)), _abi.i64ptr(acc.reshape(-1)), _abi.i32ptr(rep)))
        return att, acc, rep

    def close(self) -> None:
        if self._h is not None:
            self._lib.ceg_site_group_destroy(self._h)
            self._h = None
            self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SiteHoppingDrift(RuntimeError):
    """The running energy of a chain left its baseline by more than the tolerance (simulation.jl:1003-1007)."""


class SiteHoppingRun(NamedTuple):
    energies: np.ndarray          # float64[nframes, K] (K): the baseline at idx_cycle 0, then every printevery cycles
    populations: np.ndarray       # uint16[nframes, K, m]
    cycles: np.ndarray            # int64[nframes] idx_cycle of the frames (0, printevery, 2 printevery, ...)
    initial_energy: np.ndarray    # float64[K] baseline before the first cycle
    final_energy: np.ndarray      # float64[K] baseline after the last cycle
    records: np.ndarray           # [ninit + ncycles, K] _abi.SITE_CYCLE_RECORD_DTYPE
    stats: np.ndarray             # [K] _abi.SITE_STATS_DTYPE
    minimum: Optional[tuple]      # track_min: (idx_cycle int64[K] (0: the start of production), energy float64[K], populations uint16[K, m])
    grouped: Optional[np.ndarray] = None      # groupcycles: [ninit + ncycles, K] _abi.SITE_GROUPED_RECORD_DTYPE


def run_montecarlo(group: DeviceSiteHoppingGroup, temperatures, ncycles: int, ninit: int = 0, *, printevery: int = 1, seed: int = 0,
                   first_step: int = 0, stream_id=None, drift_rtol: float = 1e-9, track_min: bool = False, groupcycles: Optional[int] = None,
                   restartgroupcycle: bool = False) -> SiteHoppingRun:
    """``run_montecarlo!(::SiteHopping, simu; groupcycles, restartgroupcycle)`` (simulation.jl:863-1010) for every chain of ``group``:
    baseline, ``ninit`` initialisation cycles, a rebase (the reference's precise energy at ``idx_cycle == 0``), ``ncycles``
    production cycles of m steps with a frame every ``printevery`` cycles, then the drift check: ``|energy - baseline| <=
    drift_rtol max(|baseline|, 1)`` per chain, else :class:`SiteHoppingDrift`.

    ``temperatures``: [ninit + ncycles] or [ninit + ncycles, K].  The frames are ``idx_cycle`` 0 (the state after the
    initialisation), then ``printevery``, ``2 printevery``, ...; ``printevery == 0``: frame 0 and, if ``ncycles > 0``, the last cycle.
    The device counts cycles from 0: the initialisation cycles are 0..ninit-1, production cycle ``idx_cycle`` is
    ``ninit - 1 + idx_cycle``.  The absolute steps run on from ``first_step``.  ``track_min``: ``RMinimumEnergy`` over the production
    cycle ends, from the state at ``idx_cycle == 0`` on (strict <: a tie keeps the earlier cycle).

    ``groupcycles = G``: the initialisation and the production cycles are grouped cycles of G m steps
    (:meth:`DeviceSiteHoppingGroup.sweep_grouped`), each accepted or rejected as one move; ``restartgroupcycle`` restarts every one
    of them from a fresh random population.  The counters of the records and stats then count cycles, and ``run.grouped`` holds the
    grouped records.  Not on a tempered group (the reference's ``run_parallel_tempering`` has no group cycles)."""
    ncycles, ninit = int(ncycles), int(ninit)
    if groupcycles is None:
        if restartgroupcycle:
            raise ValueError("restartgroupcycle needs groupcycles")
        spc = group.m

        def sweep(count, first, temps, cycle0):
            s, r, _l = group.sweep_cycles(count, seed, first, temperature=temps, cycle0=cycle0, stream_id=stream_id)
            return s, r, None
    else:
        if int(groupcycles) < 1:
            raise ValueError("groupcycles >= 1")
        if group.rungs:
            raise ValueError("group cycles on a tempered group: run_parallel_tempering has none")
        spc = int(groupcycles) * group.m

        def sweep(count, first, temps, cycle0):
            s, r, _l, g = group.sweep_grouped(count, seed, first, temperature=temps, steps_per_cycle=spc, cycle0=cycle0, stream_id=stream_id,
                                              restart=bool(restartgroupcycle))
            return s, r, g
    T = np.asarray(temperatures, dtype=np.float64)
    if T.ndim == 0:
        T = np.full(ninit + ncycles, float(T))
    T = np.broadcast_to(T.reshape(ninit + ncycles, -1), (ninit + ncycles, group.k))
    e0 = group.baseline_energies()
    recs, grecs = [], []
    if ninit:
        _s, r, gr = sweep(ninit, first_step, T[:ninit], 0)
        recs.append(r)
        grecs.append(gr)
    group.rebase()
    every = int(printevery) if printevery > 0 else max(ncycles, 1)
    nframes = ncycles // every
    frames_e, frames_p, frames_c = [group.baseline_energies()], [group.populations()], [0]
    stats = minimum = None
    if track_min and not ncycles:
        minimum = (np.zeros(group.k, dtype=np.int64), frames_e[0].copy(), frames_p[0].copy())
    if ncycles:
        group.set_recorder(every, origin=ninit - 1 + every, capacity=nframes, track_min=track_min)
        stats, r, gr = sweep(ncycles, first_step + ninit * spc, T[ninit:], ninit)
        recs.append(r)
        grecs.append(gr)
        fr, fp = group.recorder_read()
        if track_min:
            mink, mine, best = group.recorder_minimum()
            minimum = (np.where(mink < 0, 0, mink - (ninit - 1)), mine, best)
        group.set_recorder(None)
        for f in range(len(fr)):
            frames_e.append(fr[f]["energy"].copy())
            frames_p.append(fp[f])
            frames_c.append(int(fr[f]["cycle"][0]) - (ninit - 1))
    if stats is None:
        stats = group.stats()
    final = group.baseline_energies()
    drift = np.abs(stats["energy"] - final)
    bad = np.nonzero(~(drift <= drift_rtol * np.maximum(np.abs(final), 1.0)))[0]
    if len(bad):
        c = int(bad[0])
        raise SiteHoppingDrift(f"chain {c}: running energy {stats['energy'][c]!r} against baseline {final[c]!r}")
    records = np.concatenate(recs) if recs else np.zeros((0, group.k), dtype=_abi.SITE_CYCLE_RECORD_DTYPE)
    grouped = None
    if groupcycles is not None:
        grouped = np.concatenate(grecs) if grecs else np.zeros((0, group.k), dtype=_abi.SITE_GROUPED_RECORD_DTYPE)
    return SiteHoppingRun(np.array(frames_e), np.array(frames_p, dtype=np.uint16), np.array(frames_c, dtype=np.int64), e0, final, records, stats, minimum,
                          grouped)


class QuenchingRun(NamedTuple):
    start: np.ndarray             # uint16[N, m] the random populations the quenches began from
    run: SiteHoppingRun           # run.minimum: the lowest cycle-end energy of each quench (RMinimumEnergy)


def run_random_quenching(sh: SiteHopping, N: int, temperatures, ncycles: int, *, seed: int = 0, printevery: int = 0, device: int = 0,
                         groupcycles: Optional[int] = None, restartgroupcycle: bool = False) -> QuenchingRun:
    """``run_random_quenching``: N independent quenches of ``sh``'s tables from random populations, as the chains of one group.
    Chain c starts from ``mcrng.site_random_population(seed, c, n, m)`` (purpose 11 of stream c) and runs on stream c.
    ``temperatures`` [ncycles] (the quench's schedule, shared) or [ncycles, N].  ``groupcycles`` / ``restartgroupcycle`` are passed
    through to :func:`run_montecarlo` (simulation.jl:450)."""
    n, m = sh.nsites, len(sh.population)
    start = np.stack([mcrng.site_random_population(seed, c, n, m) for c in range(int(N))])
    with DeviceSiteHoppingGroup(sh.frameworkenergies, sh.interactions, start, sh.tailcorrection, device) as g:
        run = run_montecarlo(g, temperatures, int(ncycles), 0, printevery=printevery, seed=seed, track_min=True, groupcycles=groupcycles,
                             restartgroupcycle=restartgroupcycle)
    return QuenchingRun(start, run)


class ParallelTemperingRun(NamedTuple):
    temperatures: np.ndarray      # float64[Npt] sorted: the rungs
    energies: np.ndarray          # float64[N_print, K] by rung (K = ladders * Npt; chain l * Npt + r is rung r of ladder l): the matrix the reference returns
    populations: np.ndarray       # uint16[N_print, K, m] by rung
    cycles: np.ndarray            # int64[N_print] idx_cycle of the frames
    hops_attempted: np.ndarray    # int64[K] per rung, initialisation included
    hops_accepted: np.ndarray     # int64[K]
    pairs_attempted: np.ndarray   # int64[ladders, Npt - 1] exchanges of rungs j and j + 1
    pairs_accepted: np.ndarray    # int64[ladders, Npt - 1]
    replica: np.ndarray           # int32[K] per rung: the rung its configuration started on
    run: SiteHoppingRun           # everything run_montecarlo returns, by rung


def run_parallel_tempering(sh: SiteHopping, temperatures, ncycles: int, ninit: int = 0, *, printevery: int = 1, seed: int = 0, device: int = 0,
                           ladders: int = 1, p: float = 0.1) -> ParallelTemperingRun:
    """``run_parallel_tempering(sh0, simu, temperatures)`` (simulation.jl:461-634): ``Npt = len(temperatures)`` copies of ``sh`` at the
    sorted temperatures; at every step the first pair of ``randsubseq(1:(Npt-1), p)`` may exchange configurations
    (``DeviceSiteHoppingGroup.set_tempering``; the rule is restated in :mod:`ceg_hip.mcrng`), every other rung hops.  ``ladders``
    independent ladders run side by side: ladder l draws its exchanges from stream l, its rung r hops on stream ``l * Npt + r``.

    Every rung starts from ``sh``'s population and baseline.  The frames follow the reference's ``report_now``: ``idx_cycle`` 0, then
    every ``printevery`` cycles (``printevery == 0``: frame 0 and the last cycle), ``N_print`` rows in all.  At the end the drift
    check of :612-616 is applied per rung at rtol 1e-9 (:class:`SiteHoppingDrift`).

    The reference's own routine appears to fail for ``ninit > 0`` (:512 and :567 read ``energy`` and ``sh`` outside their scope), so
    this wrapper runs the ``ninit`` cycles (with exchanges) and rebases every rung at ``idx_cycle`` 0, as
    ``run_montecarlo!(::SiteHopping)`` does.  Not covered: a schedule that attempts more than the first pair, and the output files
    (the reference's routine has no ``groupcycles``)."""
    Ts = np.sort(np.asarray(temperatures, dtype=np.float64).reshape(-1))
    npt, ladders = len(Ts), int(ladders)
    if ladders < 1:
        raise ValueError("ladders >= 1")
    k = ladders * npt
    start = np.tile(np.asarray(sh.population, dtype=np.uint16), (k, 1))
    with DeviceSiteHoppingGroup(sh.frameworkenergies, sh.interactions, start, sh.tailcorrection, device) as g:
        g.set_tempering(npt, p)
        run = run_montecarlo(g, np.tile(Ts, (int(ninit) + int(ncycles), ladders)), int(ncycles), int(ninit), printevery=printevery, seed=seed,
                             drift_rtol=1e-9)
        att, acc, rep = g.tempering_read()
    return ParallelTemperingRun(Ts, run.energies, run.populations, run.cycles, run.stats["attempted"].copy(), run.stats["accepted"].copy(), att, acc, rep, run)
