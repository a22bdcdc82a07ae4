"""ctypes view of ``include/ceg_hip.h`` (types + function prototypes).

This is the Python twin of the ``ccall`` stubs in ``julia/CEGHip.jl``: plain pointers
and sizes only.  Loading is strict: if ``libceg_hip.so`` is missing the import of the
product path fails loudly -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

RULE_DTYPE = np.dtype([('kind', '<i4'), ('_pad', '<i4'), ('p', '<f8', (3,)), ('shift', '<f8')],
                      align=True)
assert RULE_DTYPE.itemsize == 40

PKG_DIR = Path(__file__).resolve().parent.parent          # crystalenergygrids.jl_amd/
REPO_DIR = PKG_DIR.parent
LIB_PATH = PKG_DIR / "csrc" / "libceg_hip.so"

class GridHeader(C.Structure):
    """``ceg_grid_header_t``"""
    _fields_ = [("spacing", C.c_double), ("dims", C.c_int32 * 3), ("has_mat", C.c_int32),
                ("size", C.c_double * 3), ("shift", C.c_double * 3), ("delta", C.c_double * 3), ("unitcell", C.c_double * 3),
                ("num_unitcell", C.c_int32 * 3), ("_pad", C.c_int32), ("ewald_precision", C.c_double), ("mat", C.c_double * 9)]


class SweepParams(C.Structure):
    """``ceg_mc_sweep_params_t``"""
    _fields_ = [("seed", C.c_uint64), ("first_step", C.c_uint64), ("stream_id", C.c_void_p), ("temperature", C.c_void_p),
                ("dmax", C.c_void_p), ("thetamax", C.c_void_p), ("p_rotation", C.c_void_p), ("bead", C.c_void_p)]


# ``ceg_mc_sweep_stats_t`` and ``ceg_mc_sweep_record_t`` as structured arrays
SWEEP_STATS_DTYPE = np.dtype([('translation_trials', '<i8'), ('translation_accepted', '<i8'), ('rotation_trials', '<i8'),
                              ('rotation_accepted', '<i8'), ('blocked', '<i8'), ('delta', '<f8')], align=True)
SWEEP_RECORD_DTYPE = np.dtype([('molecule', '<i4'), ('kind', '<i4'), ('accepted', '<i4'), ('_pad', '<i4'), ('u', '<f8'),
                               ('rows', '<f8', (2, 4)), ('positions', '<f8', (16, 3))], align=True)
assert SWEEP_STATS_DTYPE.itemsize == 48 and SWEEP_RECORD_DTYPE.itemsize == 472

GCMC_MAX_SPECIES = 8         # CEG_MC_GCMC_MAX_SPECIES


class GcmcParams(C.Structure):
    """``ceg_mc_gcmc_params_t``"""
    _fields_ = [("seed", C.c_uint64), ("first_step", C.c_uint64), ("stream_id", C.c_void_p), ("temperature", C.c_void_p),
                ("dmax", C.c_void_p), ("thetamax", C.c_void_p), ("nspecies", C.c_int32), ("_pad", C.c_int32), ("species", C.c_void_p),
                ("molecule_species", C.c_void_p), ("max_molecules", C.c_void_p), ("molecule_species_out", C.c_void_p)]


# ``ceg_mc_gcmc_species_t``, ``ceg_mc_gcmc_stats_t`` and ``ceg_mc_gcmc_record_t`` as structured arrays
GCMC_SPECIES_DTYPE = np.dtype([('m', '<i4'), ('bead', '<i4'), ('kinds', '<i4', (16,)), ('model', '<f8', (16, 3)), ('cumulative', '<f8', (5,)),
                               ('phiPV_div_k', '<f8'), ('self_reciprocal', '<f8'), ('tail_framework', '<f8'),
                               ('tail_cross', '<f8', (GCMC_MAX_SPECIES,))], align=True)
GCMC_STATS_DTYPE = np.dtype([('trials', '<i8', (7,)), ('accepted', '<i8', (7,)), ('blocked', '<i8'), ('capacity', '<i8'), ('spent', '<i8'),
                             ('delta_moves', '<f8'), ('delta_swaps', '<f8'), ('count', '<i4', (GCMC_MAX_SPECIES,)), ('nmol', '<i4'),
                             ('_pad', '<i4')], align=True)
GCMC_RECORD_DTYPE = np.dtype([('species', '<i4'), ('molecule', '<i4'), ('kind', '<i4'), ('accepted', '<i4'), ('n_species', '<i4'),
                              ('flags', '<i4'), ('u', '<f8'), ('tc', '<f8'), ('rows', '<f8', (2, 4)), ('positions', '<f8', (16, 3))], align=True)
assert (C.sizeof(GcmcParams), GCMC_SPECIES_DTYPE.itemsize, GCMC_STATS_DTYPE.itemsize, GCMC_RECORD_DTYPE.itemsize) == (88, 584, 192, 488)
# ``ceg_mc_block_t`` (``mask``: the address of a uint8 array in host memory, 0 = empty; ``mat`` / ``invmat`` column-major)
MC_BLOCK_DTYPE = np.dtype([('mask', '<u8'), ('dims', '<i4', (3,)), ('_pad', '<i4'), ('size', '<f8', (3,)), ('shift', '<f8', (3,)),
                           ('offset', '<f8', (3,)), ('mat', '<f8', (9,)), ('invmat', '<f8', (9,))], align=True)
assert MC_BLOCK_DTYPE.itemsize == 240
# ``ceg_mc_baseline_t`` (one record per chain) and the flag of ``ceg_mc_baseline`` / ``ceg_mc_group_baseline``
MC_BASELINE_DTYPE = np.dtype([('framework_vdw', '<f8'), ('framework_direct', '<f8'), ('inter', '<f8'), ('recip_framework', '<f8'),
                              ('recip_guests', '<f8'), ('nmol', '<i4'), ('natoms', '<i4')], align=True)
assert MC_BASELINE_DTYPE.itemsize == 48
MC_BASELINE_REFRESH = 1      # CEG_MC_BASELINE_REFRESH
MC_SAMPLER_MAX_SYM = 191     # CEG_MC_SAMPLER_MAX_SYM


class MC_SAMPLER(C.Structure):
    """``ceg_mc_sampler_t`` (``unit_invmat`` column-major; the three arrays in host memory, copied by ``ceg_mc_group_set_sampler``)"""
    _fields_ = [("every", C.c_int64), ("from_step", C.c_int64), ("series_capacity", C.c_int64), ("dims", C.c_int32 * 3),
                ("nmaps", C.c_int32), ("nchannels", C.c_int32), ("nkinds", C.c_int32), ("nsym", C.c_int32), ("_pad", C.c_int32),
                ("unit_invmat", C.c_double * 9), ("chain_map", C.c_void_p), ("kind_channel", C.c_void_p), ("sym", C.c_void_p)]


# ``ceg_mc_sample_record_t``: one record per (frame, chain) of the sampler's series
MC_SAMPLE_RECORD_DTYPE = np.dtype([('step', '<i8'), ('nmol', '<i4'), ('natoms', '<i4'), ('count', '<i4', (GCMC_MAX_SPECIES,)),
                                   ('delta_moves', '<f8'), ('delta_swaps', '<f8')], align=True)
assert (C.sizeof(MC_SAMPLER), MC_SAMPLE_RECORD_DTYPE.itemsize) == (152, 64)
MC_ADAPT_DMAX, MC_ADAPT_THETAMAX = 1, 2      # CEG_MC_ADAPT_*
MC_CYCLES_MAX_RECORDS = 16777216             # CEG_MC_CYCLES_MAX_RECORDS


class McCycles(C.Structure):
    """``ceg_mc_cycles_t`` (``temperatures`` [ncycles][K] and ``prior`` [K][4] in host memory, either may be NULL)"""
    _fields_ = [("ncycles", C.c_int64), ("steps_per_cycle", C.c_int64), ("cycle0", C.c_int64), ("adapt", C.c_int32), ("_pad", C.c_int32),
                ("temperatures", C.c_void_p), ("prior", C.c_void_p)]


# ``ceg_mc_cycle_record_t``: one record per (cycle, chain) of ``ceg_mc_group_sweep_cycles`` / ``ceg_mc_group_sweep_gcmc_cycles``
MC_CYCLE_RECORD_DTYPE = np.dtype([('temperature', '<f8'), ('dmax', '<f8'), ('thetamax', '<f8'), ('dmax_next', '<f8'), ('thetamax_next', '<f8'),
                                  ('delta_moves', '<f8'), ('delta_swaps', '<f8'), ('translation_trials', '<i8'), ('translation_accepted', '<i8'),
                                  ('rotation_trials', '<i8'), ('rotation_accepted', '<i8'), ('nmol', '<i4'), ('_pad', '<i4')], align=True)
assert (C.sizeof(McCycles), MC_CYCLE_RECORD_DTYPE.itemsize) == (48, 96)


class McChainPlan(C.Structure):
    """``ceg_mc_chain_plan_t`` (``phiPV_div_k`` [K][nspecies] and ``stop_step`` [K] in host memory, either may be NULL)"""
    _fields_ = [("nspecies", C.c_int32), ("_pad", C.c_int32), ("phiPV_div_k", C.c_void_p), ("stop_step", C.c_void_p)]


assert C.sizeof(McChainPlan) == 24
MC_STOPPED = -2              # record.molecule of a step a chain sat out (its stop_step reached)


class McTempering(C.Structure):
    """``ceg_mc_tempering_t`` (``rung`` [K] int32, may be NULL, and ``energy`` [K] float64 in host memory)"""
    _fields_ = [("every", C.c_int64), ("record_capacity", C.c_int64), ("rung", C.c_void_p), ("energy", C.c_void_p)]


# ``ceg_mc_exchange_record_t``: one record per (cycle, chain) while a tempering state is installed
MC_EXCHANGE_RECORD_DTYPE = np.dtype([('rung', '<i4'), ('rung_next', '<i4'), ('partner', '<i4'), ('accepted', '<i4'), ('energy', '<f8'),
                                     ('temperature_next', '<f8'), ('u', '<f8'), ('threshold', '<f8')], align=True)
assert (C.sizeof(McTempering), MC_EXCHANGE_RECORD_DTYPE.itemsize) == (32, 48)
MC_RECORDER_MAX_BYTES = 8 << 30      # CEG_MC_RECORDER_MAX_BYTES
MC_SNAPSHOT_NO_BODY, MC_SNAPSHOT_STOPPED = 1, 2      # flags of a snapshot record


class McRecorder(C.Structure):
    """``ceg_mc_recorder_t`` (``energy`` [K] float64 in host memory, copied by ``ceg_mc_group_set_recorder``)"""
    _fields_ = [("every", C.c_int64), ("origin", C.c_int64), ("frame_capacity", C.c_int64), ("max_atoms", C.c_int32),
                ("max_molecules", C.c_int32), ("track_min", C.c_int32), ("_pad", C.c_int32), ("energy", C.c_void_p)]


# ``ceg_mc_snapshot_record_t``: one record per (frame, chain) of the recorder, and one per chain for the minimum
MC_SNAPSHOT_RECORD_DTYPE = np.dtype([('cycle', '<i8'), ('step', '<i8'), ('energy', '<f8'), ('nmol', '<i4'), ('natoms', '<i4'),
                                     ('flags', '<i4'), ('_pad', '<i4')], align=True)
assert (C.sizeof(McRecorder), MC_SNAPSHOT_RECORD_DTYPE.itemsize) == (48, 40)

SITE_MAX_MOLECULES = 4096    # CEG_SITE_MAX_MOLECULES
SITE_FRAME_TAKEN, SITE_FRAME_DROPPED, SITE_NEW_MINIMUM = 1, 2, 4      # flags of a site cycle record
SITE_GROUP_ACCEPTED, SITE_GROUP_RESTARTED = 8, 16                     # and those a grouped cycle adds (ceg_site_group_sweep_grouped)


class SiteParams(C.Structure):
    """``ceg_site_params_t`` (``stream_id`` [K] uint32 in host memory, or NULL)"""
    _fields_ = [("seed", C.c_uint64), ("first_step", C.c_uint64), ("stream_id", C.c_void_p)]


class SiteCycles(C.Structure):
    """``ceg_site_cycles_t`` (``temperature`` [ncycles][K] float64 in host memory)"""
    _fields_ = [("ncycles", C.c_int64), ("steps_per_cycle", C.c_int64), ("cycle0", C.c_int64), ("temperature", C.c_void_p)]


class SiteRecorder(C.Structure):
    """``ceg_site_recorder_t``"""
    _fields_ = [("every", C.c_int64), ("origin", C.c_int64), ("frame_capacity", C.c_int64), ("track_min", C.c_int32), ("_pad", C.c_int32)]


class SiteTempering(C.Structure):
    """``ceg_site_tempering_t`` (``pair_cdf`` [R-1] float64 and ``ladder_stream`` [K/R] uint32 in host memory, the latter or NULL)"""
    _fields_ = [("rungs", C.c_int32), ("_pad", C.c_int32), ("pair_cdf", C.c_void_p), ("ladder_stream", C.c_void_p), ("_reserved", C.c_int64)]


assert C.sizeof(SiteTempering) == 32
SITE_MAX_RUNGS = 16          # a ladder is one workgroup of 16 waves at the most

SITE_STATS_DTYPE = np.dtype([('attempted', '<i8'), ('accepted', '<i8'), ('delta', '<f8'), ('energy', '<f8')], align=True)
SITE_CYCLE_RECORD_DTYPE = np.dtype([('cycle', '<i8'), ('temperature', '<f8'), ('energy', '<f8'), ('delta', '<f8'), ('attempted', '<i8'),
                                    ('accepted', '<i8'), ('flags', '<i4'), ('_pad', '<i4')], align=True)
SITE_RECORD_DTYPE = np.dtype([('molecule', '<i4'), ('old_site', '<i4'), ('new_site', '<i4'), ('accepted', '<i4'), ('before', '<f8'),
                              ('after', '<f8'), ('u', '<f8')], align=True)
SITE_FRAME_RECORD_DTYPE = np.dtype([('cycle', '<i8'), ('energy', '<f8')], align=True)
assert (C.sizeof(SiteParams), C.sizeof(SiteCycles), C.sizeof(SiteRecorder), SITE_STATS_DTYPE.itemsize, SITE_CYCLE_RECORD_DTYPE.itemsize,
        SITE_RECORD_DTYPE.itemsize, SITE_FRAME_RECORD_DTYPE.itemsize) == (24, 32, 32, 32, 56, 40, 16)
SITE_GROUPED_RECORD_DTYPE = np.dtype([('before', '<f8'), ('restart_energy', '<f8'), ('after', '<f8'), ('u', '<f8'), ('accepted', '<i4'),
                                      ('restarted', '<i4'), ('hops_accepted', '<i8')], align=True)       # ceg_site_grouped_record_t
assert SITE_GROUPED_RECORD_DTYPE.itemsize == 48

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)

# name -> (restype, argtypes); every symbol include/ceg_hip.h declares
PROTOTYPES = {
    "ceg_abi_version": (C.c_int, []),
    "ceg_device_count": (C.c_int, []),
    "ceg_last_error": (C.c_char_p, []),
    "ceg_grid_vdw": (C.c_int, [
        c_double_p, c_int64_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double,
        C.c_void_p, c_int32_p, C.c_int32,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, c_float_p, C.c_int32]),
    "ceg_grid_coulomb": (C.c_int, [
        c_double_p, c_double_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, c_float_p, C.c_int32]),
    "ceg_grid_vdw_device": (C.c_int, [
        c_double_p, c_int64_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double,
        C.c_void_p, c_int32_p, C.c_int32,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_int32]),
    "ceg_grid_coulomb_device": (C.c_int, [
        c_double_p, c_double_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_int32]),
    "ceg_grid_vdw_file": (C.c_int, [
        c_double_p, c_int64_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double,
        C.c_void_p, c_int32_p, C.c_int32,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, c_float_p, C.c_int32,
        C.c_char_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]),
    "ceg_grid_coulomb_file": (C.c_int, [
        c_double_p, c_double_p, C.c_int64, c_double_p, c_double_p,
        C.c_int32, C.c_double, C.c_double, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, c_float_p, C.c_int32,
        C.c_char_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]),
    "ceg_release_cached_buffers": (C.c_int, []),
    "ceg_host_grid_alloc": (c_float_p, [c_int32_p]),
    "ceg_host_grid_free": (C.c_int, [c_float_p]),
    "ceg_plan_create": (C.c_int, [
        C.POINTER(C.c_void_p), C.c_int32,
        c_double_p, c_int64_p, c_double_p, C.c_int64,
        c_double_p, c_double_p, C.c_int32, C.c_double, C.c_double,
        C.c_void_p, c_int32_p, C.c_int32, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p]),
    "ceg_plan_destroy": (C.c_int, [C.c_void_p]),
    "ceg_image_cache_stats": (C.c_int, [c_int64_p, c_int64_p, c_int64_p]),
    "ceg_plan_can_cull": (C.c_int, [C.c_void_p]),
    "ceg_plan_uniform_class": (C.c_int, [C.c_void_p]),
    "ceg_uniform_class": (C.c_int, [c_int64_p, c_double_p, C.c_int64, C.c_void_p, c_int32_p, C.c_int32, C.c_double, c_double_p]),
    "ceg_plan_ew2_fine": (C.c_int, [C.c_void_p]),
    "ceg_ew2_table": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int32, c_double_p, C.c_int64, c_int32_p, c_int32_p, c_int32_p, c_double_p]),
    "ceg_plan_num_images": (C.c_int64, [C.c_void_p]),
    "ceg_plan_copy_images": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "ceg_plan_build_vdw": (C.c_int, [
        C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32,
        C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ceg_plan_build_coulomb": (C.c_int, [
        C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32,
        C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "ceg_plan_build_fused": (C.c_int, [
        C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
        C.c_int32, C.c_void_p]),
    "ceg_plan_create_multi": (C.c_int, [
        C.POINTER(C.c_void_p), C.c_int32,
        c_double_p, c_int64_p, c_double_p, C.c_int64,
        c_double_p, c_double_p, C.c_int32, C.c_double, C.c_double,
        C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p]),
    "ceg_plan_num_probes": (C.c_int, [C.c_void_p]),
    "ceg_grids_multi": (C.c_int, [
        c_double_p, c_int64_p, c_double_p, C.c_int64, c_double_p, c_double_p, C.c_int32, C.c_double, C.c_double,
        C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, C.c_double,
        c_int32_p, c_double_p, c_double_p, c_double_p,
        C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_void_p), c_float_p, C.c_int32]),
    "ceg_plan_build_multi": (C.c_int, [
        C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "ceg_plan_eval_points": (C.c_int, [
        C.c_void_p, C.c_int32, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    "ceg_interp_create": (C.c_int, [
        C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32,
        c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32]),
    "ceg_interp_create_from_file": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_char_p, C.c_int32, C.c_double, c_double_p, c_double_p, C.c_void_p]),
    "ceg_interp_set_higherorder": (C.c_int, [C.c_void_p, C.c_int32]),
    "ceg_interp_destroy": (C.c_int, [C.c_void_p]),
    "ceg_interp_points": (C.c_int, [C.c_void_p, c_double_p, C.c_int64, c_double_p]),
    "ceg_interp_points_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ceg_scale_grid_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p]),
    "ceg_recip_create": (C.c_int, [
        C.POINTER(C.c_void_p), C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p, C.c_int64,
        c_int32_p, c_double_p]),
    "ceg_recip_destroy": (C.c_int, [C.c_void_p]),
    "ceg_recip_layout": (C.c_int, [c_int32_p, C.c_int64, c_int32_p, c_int32_p, c_int32_p, C.c_void_p, C.c_void_p]),
    "ceg_recip_launch_shape": (C.c_int, [c_int32_p, C.c_int64, c_int32_p, C.c_int32, C.c_int64, c_int32_p]),
    "ceg_recip_energy": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_int32, C.c_int64, C.c_double, C.c_double, c_double_p]),
    "ceg_block_from_grid": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, c_int32_p, C.c_double, C.c_void_p]),
    "ceg_block_spheres": (C.c_int, [C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_double,
                                    c_double_p, c_double_p, C.c_int32, C.c_void_p]),
    "ceg_recip_set_structure_factor": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "ceg_pairs_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, c_double_p, c_double_p, C.c_double, C.c_void_p, c_int32_p,
                                   C.c_int32, C.c_double]),
    "ceg_pairs_destroy": (C.c_int, [C.c_void_p]),
    "ceg_pairs_set_atoms": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_int32_p, C.c_int64]),
    "ceg_pairs_energy": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, C.c_int32, C.c_int64, C.c_int32, c_double_p]),
    "ceg_pairs_energy_device": (C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "ceg_pairs_neighbour_cells": (C.c_int, [C.c_void_p, c_int32_p]),
    "ceg_mc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, c_double_p, C.c_int32, c_double_p,
                                c_double_p, C.c_double, C.c_void_p, c_int32_p, C.c_double, c_int32_p, c_double_p, c_double_p, c_double_p,
                                C.c_int64, c_int32_p, c_double_p]),
    "ceg_mc_destroy": (C.c_int, [C.c_void_p]),
    "ceg_mc_set_guests": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_int32_p, C.c_int32]),
    "ceg_mc_trial": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    "ceg_mc_trial_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ceg_mc_trial_insert_device": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ceg_mc_accept": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "ceg_mc_get_state": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "ceg_mc_neighbour_cells": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p]),
    "ceg_mc_trial_insert": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, c_double_p, C.c_int64, c_double_p]),
    "ceg_mc_insert": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, c_double_p, c_int32_p]),
    "ceg_mc_remove": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p]),
    "ceg_mc_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32]),
    "ceg_mc_group_destroy": (C.c_int, [C.c_void_p]),
    "ceg_mc_group_trial": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, C.c_int32, c_double_p, c_double_p]),
    "ceg_mc_group_accept": (C.c_int, [C.c_void_p, c_int32_p, c_double_p]),
    "ceg_mc_group_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ceg_mc_group_sweep_gcmc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ceg_mc_group_sweep_cycles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ceg_mc_group_sweep_gcmc_cycles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ceg_mc_group_set_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "ceg_mc_group_block_counts": (C.c_int, [C.c_void_p, c_int64_p, c_int64_p]),
    "ceg_mc_group_set_chain_plan": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_mc_group_set_device_cells": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "ceg_mc_group_halted": (C.c_int, [C.c_void_p, c_int64_p]),
    "ceg_mc_cell_lists": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, C.c_int64]),
    "ceg_mc_group_set_tempering": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_mc_group_tempering_read": (C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_int64_p, C.c_void_p, c_int64_p]),
    "ceg_mc_group_set_recorder": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_mc_group_snapshot": (C.c_int, [C.c_void_p]),
    "ceg_mc_group_recorder_rebase": (C.c_int, [C.c_void_p, c_double_p]),
    "ceg_mc_group_recorder_read": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p]),
    "ceg_mc_group_recorder_min": (C.c_int, [C.c_void_p, c_int64_p, c_double_p, C.c_void_p, c_double_p, c_int32_p, c_int32_p, c_int32_p]),
    "ceg_mc_group_set_sampler": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_mc_group_sample": (C.c_int, [C.c_void_p]),
    "ceg_mc_group_sampler_read": (C.c_int, [C.c_void_p, c_int64_p, C.c_void_p, c_int64_p]),
    "ceg_mc_group_sampler_reset": (C.c_int, [C.c_void_p]),
    "ceg_mc_baseline": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_mc_group_baseline": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_energy_grid": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, c_double_p, c_double_p, C.c_int32,
                                  c_double_p, C.c_int32, c_double_p, c_int32_p,
                                  C.c_void_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                  C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_energy_grid_reduced": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, c_double_p, c_double_p, C.c_int32,
                                          c_double_p, C.c_int32, c_double_p, c_int32_p,
                                          C.c_void_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                          C.c_double, C.c_double, c_double_p, C.c_int32, c_double_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_site_tables": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, c_double_p, C.c_int32, C.c_double, C.c_double, c_double_p, c_double_p, c_double_p]),
    "ceg_site_tables_device": (C.c_int, [C.c_void_p, c_int32_p, C.c_int32, c_double_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "ceg_site_group_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double,
                                        C.POINTER(C.c_void_p)]),
    "ceg_site_group_destroy": (C.c_int, [C.c_void_p]),
    "ceg_site_group_sweep_cycles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ceg_site_group_sweep_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ceg_site_group_baseline": (C.c_int, [C.c_void_p, c_double_p]),
    "ceg_site_group_rebase": (C.c_int, [C.c_void_p]),
    "ceg_site_group_get_populations": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_site_group_set_populations": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_site_group_set_recorder": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_site_group_recorder_read": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, c_int64_p]),
    "ceg_site_group_recorder_min": (C.c_int, [C.c_void_p, c_int64_p, c_double_p, C.c_void_p]),
    "ceg_site_group_set_tempering": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ceg_site_group_tempering_read": (C.c_int, [C.c_void_p, c_int64_p, c_int64_p, c_int32_p]),
    "ceg_recip_energy_device": (C.c_int, [C.c_void_p, C.c_void_p, c_double_p, C.c_int32, C.c_int64, C.c_double, C.c_double,
                                          C.c_void_p, C.c_void_p]),
    "ceg_grid_local_minima": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, c_int32_p, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_int64,
                                        c_int64_p, c_double_p, C.c_void_p]),
    "ceg_grid_components": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, c_int32_p, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, c_int64_p, C.c_void_p]),
    "ceg_grid_site_proximity": (C.c_int, [C.c_int32, c_int32_p, c_double_p, c_double_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p]),
    "ceg_grid_site_density": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, c_int32_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_grid_basins": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, c_int32_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_double,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p,
                                  C.c_int32, C.c_void_p]),
    "ceg_grid_smooth": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, c_int32_p, c_double_p, C.c_int32, c_double_p,
                                  C.c_int32, c_double_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ceg_grid_ranked": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, c_int32_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                  c_int64_p, C.c_void_p]),
    "ceg_grid_site_nearest": (C.c_int, [C.c_int32, c_int32_p, c_double_p, C.c_int32, C.c_double, c_double_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, c_int64_p,
                                        C.c_void_p]),
    "ceg_coalesce_ranked": (C.c_int, [c_int32_p, c_double_p, c_double_p, C.c_int64, c_int32_p, c_double_p, C.c_int32, C.c_double, C.c_double,
                                      C.c_double, C.c_double, c_double_p, c_double_p, C.c_int64, c_int64_p]),
    "ceg_grid_coalesce": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                    c_int32_p, c_double_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_int32, C.c_int64, c_int64_p, C.c_void_p]),
    "ceg_grid_site_partition": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, c_int32_p, c_double_p, C.c_int32, C.c_double,
                                          c_double_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, c_int32_p, c_int64_p,
                                          C.c_void_p]),
    "ceg_cluster_closer_than": (C.c_int, [c_double_p, c_double_p, C.c_int64, c_double_p, C.c_int32, C.c_double, C.c_double, c_int64_p]),
}
BASINS_MAX_OWNERS = 16                           # CEG_BASINS_MAX_OWNERS
COMPONENTS_NONZERO, COMPONENTS_BAND = 0, 1      # CEG_COMPONENTS_*
SITE_PROXIMITY_MAX_SITES = 2048                  # CEG_SITE_PROXIMITY_MAX_SITES

ALGO_AUTO, ALGO_BRUTEFORCE, ALGO_CULLED = 0, 1, 2
EGRID_MAX_TEMPS = 8          # CEG_EGRID_MAX_TEMPS


class CegError(RuntimeError):
    """Non-zero status from libceg_hip (message from ``ceg_last_error``)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libceg_hip error {code}: {msg}")
        self.code = code


_lib = None


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen ``libceg_hip.so`` and bind every prototype.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else Path(os.environ.get("CEG_HIP_LIB", LIB_PATH))
    if not p.exists():
        raise ImportError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the grid build.")
    if "torch" not in sys.modules and not os.environ.get("CEG_HIP_NO_TORCH"):
        # PyTorch ships its own HIP runtime; when this package hands device memory to / takes it from torch (plan builds into
        # tensors, ceg_grid_*_device, torch.distributed ranks) that runtime must be the one the process loads first, or torch's
        # lazy initialisation later finds no device.  A pure C-ABI user without torch is unaffected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(str(p))
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.ceg_abi_version() != 1:
        raise ImportError("libceg_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, code: int) -> None:
    if code != 0:
        raise CegError(code, (lib.ceg_last_error() or b"").decode())


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(c_double_p)


def i32ptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(c_int32_p)


def i64ptr(a: np.ndarray):
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(c_int64_p)


def fptr(a: np.ndarray):
    assert a.dtype == np.float32
    return a.ctypes.data_as(c_float_p)
