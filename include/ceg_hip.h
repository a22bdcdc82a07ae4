/*
 * ceg_hip.h -- C ABI of libceg_hip.so, the MI355X (gfx950) energy-grid builder.
 *
 * Drop-in boundary for the grid-build hot path of CrystalEnergyGrids.jl.  The
 * reference has no FFI of its own (it is 100 % Julia); the boundary is placed
 * at the two loop nests that fill the grid array:
 *
 *     create_grid_vdw      src/grids.jl:144-150   (calls src/probes.jl:71-92)
 *     create_grid_coulomb  src/grids.jl:171-177   (calls src/probes.jl:94-117)
 *
 * Everything above those loops (CIF / force-field parsing, ProbeSystem,
 * GridCoordinatesSetup, initialize_ewald, unit constants, the .grid writer)
 * stays in the host language and hands this library plain arrays.
 *
 * Conventions
 *   - all pointers are borrowed for the duration of the call; nothing is retained
 *     except inside a ceg_plan_t, which copies what it needs to the device;
 *   - 3x3 matrices are column-major (Julia SMatrix order);
 *   - return value 0 = ok, <0 = error, message via ceg_last_error() (thread-local);
 *   - no physical constants live in the library: lambda / threshold / alpha are
 *     arguments computed by the host (src/grids.jl:141-143,168-170, src/ewald.jl:198-204);
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     returns CEG_ERR_NO_DEVICE.
 */
#ifndef CEG_HIP_H
#define CEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CEG_ABI_VERSION 1

#if defined(__GNUC__)
#define CEG_API __attribute__((visibility("default")))
#else
#define CEG_API
#endif

/* error codes */
#define CEG_OK                 0
#define CEG_ERR_INVALID       -1   /* bad argument (null pointer, negative size, ...)        */
#define CEG_ERR_NO_DEVICE     -2   /* no HIP device / requested device not present           */
#define CEG_ERR_HIP           -3   /* a HIP runtime call failed                              */
#define CEG_ERR_RULE          -4   /* rule kind not valid in a VdW grid (mirrors the Julia
                                      error()/throw sites of src/interactions.jl:442-467)    */
#define CEG_ERR_UNSUPPORTED   -5

/* Interaction kinds.  Numeric values = order of `@enum InteractionKind`,
 * src/interactions.jl:23-33. */
enum ceg_kind {
    CEG_HARDSPHERE            = 0,
    CEG_COULOMB_EWALD_DIRECT  = 1,
    CEG_COULOMB               = 2,
    CEG_LENNARDJONES          = 3,
    CEG_BUCKINGHAM            = 4,
    CEG_MONOMIAL              = 5,
    CEG_EXPONENTIAL           = 6,
    CEG_UNDEFINED_INTERACTION = 7,
    CEG_NOINTERACTION         = 8
};

/* One InteractionRule (src/interactions.jl:232-237): kind, params (<=3), shift.
 * An InteractionRuleSum (src/interactions.jl:557-583) is a run of these. */
typedef struct ceg_rule {
    int32_t kind;
    int32_t _pad;
    double  p[3];
    double  shift;
} ceg_rule_t;

/* Algorithm selector for the build entry points. */
enum ceg_algo {
    CEG_ALGO_AUTO       = 0,  /* culled when the supercell allows it, else brute force   */
    CEG_ALGO_BRUTEFORCE = 1,  /* every atom tested for every point, literal min-image
                                 routine (src/utils.jl:210-246); reference loop shape    */
    CEG_ALGO_CULLED     = 2   /* lattice-image list + spatial bins; same selection rule
                                 as the reference, evaluated per image                   */
};

/* ---- library / device info ------------------------------------------------ */
CEG_API int         ceg_abi_version(void);
CEG_API int         ceg_device_count(void);         /* number of HIP devices, 0 if none   */
CEG_API const char* ceg_last_error(void);           /* thread-local, never NULL           */

/* ---- one-shot host API ---------------------------------------------------- */
/*
 * Fills `grid` exactly like the loop nest of create_grid_vdw (src/grids.jl:144-150):
 * for every (i,j,k) in 0:dims[0] x 0:dims[1] x 0:dims[2],
 *   pos   = abc_to_xyz(i,j,k)                       src/coordinates.jl:72-76
 *   deriv = compute_derivatives_vdw(probe, pos)     src/probes.jl:71-92
 *   _set_gridpoint!(grid,i,j,k,delta,lambda,threshold,deriv)  src/grids.jl:118-135
 *
 *  pos       [3*natoms]  cartesian A, supercell-tiled ProbeSystem.positions (src/probes.jl:29-55)
 *  atomkind  [natoms]    1-based force-field index   (src/probes.jl:23,54)
 *  mat,invmat            supercell matrix / inverse  (src/probes.jl:27-28), column-major
 *  ortho,safemin2        from prepare_periodic_distance_computations (src/utils.jl:146-155)
 *  cutoff2               forcefield.cutoff^2         (src/probes.jl:75)
 *  rules,rule_offset     rules[rule_offset[k-1] .. rule_offset[k]) = flattened
 *                        forcefield.interactions[k, probe] (src/forcefields.jl:302-304);
 *                        rule_offset has nkinds+1 entries
 *  dims,size,shift,delta GridCoordinatesSetup fields (src/coordinates.jl:32-41), A
 *  lambda,threshold      1/GRID_TO_KELVIN, GRID_TO_KELVIN*1e7 (src/grids.jl:141-143,148)
 *  grid      [(dims[2]+1)*(dims[1]+1)*(dims[0]+1)*8] float, host memory,
 *            column-major [z,y,x,channel] (src/grids.jl:126-133)
 *  ngpus     1..ceg_device_count(): x-slabs are spread over that many devices
 */
CEG_API int ceg_grid_vdw(const double* pos, const int64_t* atomkind, int64_t natoms,
                 const double mat[9], const double invmat[9],
                 int32_t ortho, double safemin2, double cutoff2,
                 const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                 const int32_t dims[3], const double size[3], const double shift[3],
                 const double delta[3],
                 double lambda, double threshold,
                 float* grid, int32_t ngpus);

/*
 * Same for create_grid_coulomb (src/grids.jl:171-177) with
 * compute_derivatives_ewald (src/probes.jl:94-117) / derivatives_ewald
 * (src/ewald.jl:299-312).
 *  charge [natoms] e, alpha = ewald.alpha in 1/A,
 *  lambda = COULOMBIC_CONVERSION_FACTOR/GRID_TO_KELVIN, threshold = 1e7/lambda
 *  (src/grids.jl:169-170).
 */
CEG_API int ceg_grid_coulomb(const double* pos, const double* charge, int64_t natoms,
                     const double mat[9], const double invmat[9],
                     int32_t ortho, double safemin2, double cutoff2, double alpha,
                     const int32_t dims[3], const double size[3], const double shift[3],
                     const double delta[3],
                     double lambda, double threshold,
                     float* grid, int32_t ngpus);

/*
 * The same two builds with the .grid file written on the way ("device -> file"):
 * `header` (the bytes of _create_grid_common, src/grids.jl:108-116, + the Ewald precision for a Coulomb
 * grid, :180) is written first, every finished chunk of the payload is written at its offset while later
 * chunks are still being computed, `trailer` (the cell matrix, :154/:182) goes after the payload.  The
 * library does not interpret header or trailer -- the host produces them with the reference's own writer.
 * `grid` may be NULL (file only) or a host array that is filled as by ceg_grid_vdw / ceg_grid_coulomb.
 */
CEG_API int ceg_grid_vdw_file(const double* pos, const int64_t* atomkind, int64_t natoms,
                 const double mat[9], const double invmat[9],
                 int32_t ortho, double safemin2, double cutoff2,
                 const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                 const int32_t dims[3], const double size[3], const double shift[3],
                 const double delta[3], double lambda, double threshold,
                 float* grid, int32_t ngpus,
                 const char* path, const void* header, int64_t header_bytes,
                 const void* trailer, int64_t trailer_bytes);
CEG_API int ceg_grid_coulomb_file(const double* pos, const double* charge, int64_t natoms,
                     const double mat[9], const double invmat[9],
                     int32_t ortho, double safemin2, double cutoff2, double alpha,
                     const int32_t dims[3], const double size[3], const double shift[3],
                     const double delta[3], double lambda, double threshold,
                     float* grid, int32_t ngpus,
                     const char* path, const void* header, int64_t header_bytes,
                     const void* trailer, int64_t trailer_bytes);

/* Page-locked result arrays.  ceg_grid_vdw / ceg_grid_coulomb / ceg_grids_multi into an ordinary host array go through a pinned
 * ring and a second pass by host threads; when `grid` was allocated HERE, every chunk is copied D2H straight to its place and the
 * call is bounded by the PCIe transfer alone (256^3: 10.3 instead of 13.4 ms for a VdW grid).  The memory is page-locked host memory,
 * [8*(dims[0]+1)*(dims[1]+1)*(dims[2]+1)] floats in the layout above, owned by the library: hand it back with ceg_host_grid_free
 * (it returns to the per-process cache, so the page-locking is paid once; ceg_release_cached_buffers unpins idle arrays).  In Julia:
 * `unsafe_wrap(Array, ptr, (dz+1, dy+1, dx+1, 8))`.  NULL on failure (ceg_last_error). */
CEG_API float* ceg_host_grid_alloc(const int32_t dims[3]);
CEG_API int    ceg_host_grid_free(float* grid);

/* The one-shot entry points keep, per process, one idle device output slab per GPU and one pinned
 * staging ring (page-locking / hipMalloc of 0.5 GB cost as much as the build itself).  This frees
 * whatever is idle; safe to call at any time, never required. */
CEG_API int ceg_release_cached_buffers(void);

/* The same builds with the assembled grid left in DEVICE memory: d_grid [8*(dims[0]+1)*(dims[1]+1)*(dims[2]+1)] floats on
 * `target_device`, layout as above -- for callers that feed the grid consumers (ceg_scale_grid_device + ceg_interp_create with
 * grid_on_device = 1, then ceg_mc_create) without a trip through host memory.  The x-slabs are spread over `ngpus` devices starting
 * at the target; the target's slab is built in place, the others travel chunk by chunk with hipMemcpyPeerAsync (xGMI inside a
 * node) while later chunks are still being computed: the single-process counterpart of the all-gather that bench.py / the
 * torch.distributed ranks do with RCCL.  Synchronous: d_grid is complete on return. */
CEG_API int ceg_grid_vdw_device(const double* pos, const int64_t* atomkind, int64_t natoms,
                                const double mat[9], const double invmat[9], int32_t ortho, double safemin2, double cutoff2,
                                const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                                const int32_t dims[3], const double size[3], const double shift[3], const double delta[3],
                                double lambda, double threshold, float* d_grid, int32_t target_device, int32_t ngpus);
CEG_API int ceg_grid_coulomb_device(const double* pos, const double* charge, int64_t natoms,
                                    const double mat[9], const double invmat[9], int32_t ortho, double safemin2, double cutoff2,
                                    double alpha,
                                    const int32_t dims[3], const double size[3], const double shift[3], const double delta[3],
                                    double lambda, double threshold, float* d_grid, int32_t target_device, int32_t ngpus);

/* ---- resident-plan API (device buffers, caller-owned stream) ---------------- */
/*
 * A plan is one ProbeSystem + one GridCoordinatesSetup made resident on one
 * device: atom table, rule table, lattice-image list and spatial bins.  It is
 * what a multi-process driver (one rank per GPU) uses: each rank builds its
 * own x-slab [i_begin, i_end) into device memory on its own stream and the
 * slabs are then exchanged by the caller (RCCL all-gather).
 *
 * rules/rule_offset/nkinds/atomkind may be NULL/0 for a Coulomb-only plan;
 * charge may be NULL for a VdW-only plan.
 */
typedef struct ceg_plan ceg_plan_t;

CEG_API int ceg_plan_create(ceg_plan_t** plan, int32_t device,
                    const double* pos, const int64_t* atomkind, const double* charge,
                    int64_t natoms,
                    const double mat[9], const double invmat[9],
                    int32_t ortho, double safemin2, double cutoff2,
                    const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                    double alpha,
                    const int32_t dims[3], const double size[3], const double shift[3],
                    const double delta[3]);
CEG_API int ceg_plan_destroy(ceg_plan_t* plan);
/* The lattice-image list + bins of a plan (the ~1 ms host part of plan creation for a 10 k-atom framework) are kept on the device
 * and shared between plans that need exactly the same list -- same framework, cell, cutoff, grid box, per-atom kind flags and
 * charges --, which is what the K + 1 one-shot calls of one setup_RASPA and every later call on the same framework are; the
 * last CEG_HIP_IMAGE_CACHE (default 6, 0 = off) lists are kept, ceg_release_cached_buffers drops them.  Counters since load: */
CEG_API int ceg_image_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries);

/* 1 if the culled algorithm is valid for this plan (every perpendicular width of
 * `mat` is >= 2*cutoff, which ProbeSystem guarantees, src/probes.jl:24), else 0. */
CEG_API int ceg_plan_can_cull(const ceg_plan_t* plan);

/* Uniform class of the plan's VdW-active atoms (of probe 0 on a multi-probe plan), what ceg_plan_build_vdw / _fused and
 * ceg_plan_eval_points run with: 0 per-candidate Lennard-Jones records; 1 every kind that is present and has a rule with the probe
 * carries ONE bit-identical Lennard-Jones rule (4 eps, sigma, shift are applied once per tile of grid points); 2 as 1, and every
 * atom of those kinds carries one bit-identical charge (applied once per tile in the fused build).  CEG_HIP_UNIFORM_CLASS=0 | 1 in
 * the environment at plan creation caps it.  Results agree with class 0 to rounding (the constants multiply a sum, not each term). */
CEG_API int ceg_plan_uniform_class(const ceg_plan_t* plan);
/* The same classification on a caller's tables, without a device (diagnostics, CPU tests): atomkind 1-based as in
 * ceg_plan_create, charge may be NULL.  Returns 0 / 1 / 2 or a negative error; constants (may be NULL) receives
 * {4 eps, sigma^6, shift, q}, zeros where not applicable. */
CEG_API int ceg_uniform_class(const int64_t* atomkind, const double* charge, int64_t natoms, const ceg_rule_t* rules,
                              const int32_t* rule_offset, int32_t nkinds, double cutoff2, double constants[4]);

/* 1 if the plan holds the fine r^2-indexed table of the real-space Ewald functions (64 intervals per octave of r^2, two degree-5
 * polynomials per interval) beside the ordinary one (32 per octave, degree 6), else 0.  The fused builds of uniform class 1 / 2 and
 * the Coulomb build and point evaluation of a single-probe plan then read the fine table (one Horner step per function and one
 * 16-byte read fewer per pair); every other launch, ceg_plan_build_multi included, keeps the ordinary table.  A plan has none
 * without an Ewald term, when cutoff^2 lies more than 352 intervals above the radius of the exact path (12 A: 330), or with
 * CEG_HIP_EW2_FINE=0 in the environment at plan creation (one library runs both paths: tests, A/B).  Results of the two tables agree
 * within the fit's error: below 1.5e-11 of the pair term at a 12 A cutoff, where the ordinary table is at 1e-11. */
CEG_API int ceg_plan_ew2_fine(const ceg_plan_t* plan);
/* The table such a plan builds, without a device (diagnostics, CPU tests): fine = 0 the ordinary layout, 1 the fine one; r_exact2 the
 * squared radius of the exact path (4.0 unless a hard sphere reaches further).  Interval k (0-based) covers the r^2 whose high
 * 32 bits shifted right by 20 - log2(intervals per octave) equal base + k; its record is stride doubles, the coefficients of B0(s) =
 * erfc(alpha sqrt(s))/sqrt(s) and then of C(s) = 2 alpha/sqrt(pi) exp(-alpha^2 s) in ascending powers of t = s - (start of the
 * interval).  Returns 1 when a plan would use the table, 0 when it would not -- the range needs more intervals than the kernels hold
 * (352 fine, 176 ordinary: no table is built, stride = 0, ni receives the number needed), the fit misses 5e-11 somewhere (the table is built and
 * returned all the same), or the arguments are out of range (stride = 0, ni = 0) --, negative on error.  table (NULL = query) receives
 * ni * stride doubles, capacity is its size in doubles; worst receives the largest relative error of the fit at 17 points per
 * interval.  Any output may be NULL. */
CEG_API int ceg_ew2_table(double alpha, double r_exact2, double cutoff2, int32_t fine, double* table, int64_t capacity, int32_t* base,
                          int32_t* ni, int32_t* stride, double* worst);

/* number of lattice images kept by the culled algorithm (0 before first use) */
CEG_API int64_t ceg_plan_num_images(const ceg_plan_t* plan);
/* The plan's lattice-image list copied to the host (diagnostics / tests: the list is built on the device since round 4 and must be
 * byte-identical to the host build, CEG_HIP_IMAGES_ON_HOST=1): xyzq [4 n] (position + charge), kind [n] (kind | 1 << 25 when the kind
 * has a VdW rule; -1 without rules), atom [n] (index of the framework atom), bin_start [nb0 nb1 nb2 + 1]; any output may be NULL. */
CEG_API int ceg_plan_copy_images(const ceg_plan_t* plan, double* xyzq, int32_t* kind, int32_t* atom, int32_t* bin_start, int32_t nb[3]);

/*
 * Build x-planes i in [i_begin, i_end) (0 <= i_begin <= i_end <= dims[0]+1).
 * Element (k,j,i,c) is written at
 *     d_out[c*channel_stride + ((i - i_origin)*(dims[1]+1) + j)*(dims[2]+1) + k]
 * so the same call serves a full grid buffer (i_origin = 0, channel_stride =
 * full grid points) or a compact slab (i_origin = i_begin, channel_stride =
 * slab points).  d_out is DEVICE memory on the plan's device; `stream` is a
 * hipStream_t (NULL = default stream).  The call is asynchronous.
 */
CEG_API int ceg_plan_build_vdw(ceg_plan_t* plan, double lambda, double threshold,
                       int32_t i_begin, int32_t i_end,
                       float* d_out, int64_t channel_stride, int32_t i_origin,
                       int32_t algo, void* stream);
CEG_API int ceg_plan_build_coulomb(ceg_plan_t* plan, double lambda, double threshold,
                           int32_t i_begin, int32_t i_end,
                           float* d_out, int64_t channel_stride, int32_t i_origin,
                           int32_t algo, void* stream);
/* VdW and Coulomb grids of the same slab in one pass over the atoms (shared
 * geometry work).  Same semantics as the two calls above. */
CEG_API int ceg_plan_build_fused(ceg_plan_t* plan,
                         double lambda_vdw, double threshold_vdw,
                         double lambda_coulomb, double threshold_coulomb,
                         int32_t i_begin, int32_t i_end,
                         float* d_out_vdw, float* d_out_coulomb,
                         int64_t channel_stride, int32_t i_origin,
                         int32_t algo, void* stream);

/*
 * Multi-probe plans: ALL the grids of one setup from one pass.  setup_RASPA (src/raspa.jl:497-520) asks for one
 * create_grid_vdw per distinct guest atom plus one create_grid_coulomb, all on the same framework, cutoff and grid geometry;
 * here the K probes' rule tables go into ONE plan (one lattice-image list, one set of bins and function tables) and
 * ceg_plan_build_multi computes the requested grids together: per candidate image one staging, one distance, one 1/r^2, K
 * Lennard-Jones evaluations with K accumulator sets, one real-space Ewald evaluation.
 *
 *   nprobes       1 .. 4 (CEG_MAX_PROBES)
 *   rules[q], rule_offset[q]   the flattened column ff.interactions[:, probe_q] as for ceg_plan_create (same nkinds for all).
 *                 Every probe may be of any rule class ceg_plan_create takes (round 4: Na + the C and O of CO2 are one plan).  The
 *                 probes that are Lennard-Jones-only against the framework kinds that are present (at most one LJ rule per kind;
 *                 NoInteraction / CoulombEwaldDirect count as none) share accumulating loops -- two of them with the Coulomb grid,
 *                 up to four in a VdW launch --; a probe of another class (a Buckingham / hard-sphere cation) is launched alone with
 *                 the kernel of its class, or fused with the Coulomb grid when no Lennard-Jones pair takes that place: all from the
 *                 plan's one image list, bins and function tables.  The exact-path radius of the plan is the largest any probe
 *                 asks for (hard spheres); CEG_ERR_UNSUPPORTED only if that reaches the cutoff.  charge may be NULL (VdW grids only).
 *   d_out_vdw     [nprobes] device pointers, NULL entries are skipped; d_out_coulomb may be NULL.  Layout, channel_stride,
 *                 i_begin / i_end / i_origin, lambda / threshold and the asynchronous stream semantics as ceg_plan_build_*.
 *
 * Every grid is bit-identical to the one the same call produces when it is asked for that grid alone (identical per-pair
 * arithmetic whatever the grouping into launches; candidates that contribute exact zeros may be staged in one launch and
 * dropped in another, which leaves the FP64 sums unchanged); against a single-probe plan of ceg_plan_create the
 * values agree to the last bits of the FP64 sums (a VdW-only single-probe plan lists fewer images, which reorders the sums).
 * The ordinary ceg_plan_build_vdw / _coulomb / _fused calls work on a multi-probe plan too and use probe 0.
 */
#define CEG_MAX_PROBES 4
CEG_API int ceg_plan_create_multi(ceg_plan_t** plan, int32_t device,
                          const double* pos, const int64_t* atomkind, const double* charge, int64_t natoms,
                          const double mat[9], const double invmat[9],
                          int32_t ortho, double safemin2, double cutoff2,
                          int32_t nprobes, const ceg_rule_t* const* rules, const int32_t* const* rule_offset, int32_t nkinds,
                          double alpha,
                          const int32_t dims[3], const double size[3], const double shift[3], const double delta[3]);
CEG_API int ceg_plan_num_probes(const ceg_plan_t* plan);    /* 0 for an ordinary plan */
/* One-shot form (what the Julia binding calls once per setup_RASPA): host arrays out, grids_vdw [nprobes] (NULL entries skipped),
 * grid_coulomb may be NULL; the x-slabs are spread over `ngpus` devices and every device pipelines compute / D2H / host copy as
 * ceg_grid_vdw does.  Probes of any rule class, as for ceg_plan_create_multi. */
CEG_API int ceg_grids_multi(const double* pos, const int64_t* atomkind, const double* charge, int64_t natoms,
                    const double mat[9], const double invmat[9], int32_t ortho, double safemin2, double cutoff2,
                    int32_t nprobes, const ceg_rule_t* const* rules, const int32_t* const* rule_offset, int32_t nkinds, double alpha,
                    const int32_t dims[3], const double size[3], const double shift[3], const double delta[3],
                    double lambda_vdw, double threshold_vdw, double lambda_coulomb, double threshold_coulomb,
                    float* const* grids_vdw, float* grid_coulomb, int32_t ngpus);
CEG_API int ceg_plan_build_multi(ceg_plan_t* plan,
                         double lambda_vdw, double threshold_vdw,
                         double lambda_coulomb, double threshold_coulomb,
                         int32_t i_begin, int32_t i_end,
                         float* const* d_out_vdw, float* d_out_coulomb,
                         int64_t channel_stride, int32_t i_origin, void* stream);

/*
 * Raw FP64 results of compute_derivatives_vdw / compute_derivatives_ewald
 * (src/probes.jl:71-117) at arbitrary cartesian points, before
 * _set_gridpoint!: out[8*p + 0..7] = value, d1x, d1y, d1z, d2xy, d2xz, d2yz, d3.
 * points/out are HOST memory; synchronous.  which: 0 = vdw, 1 = coulomb.
 */
CEG_API int ceg_plan_eval_points(ceg_plan_t* plan, int32_t which, int32_t algo,
                         const double* points, int64_t npoints, double* out);

/* ---- grid consumer: batched tricubic interpolation --------------- */
/*
 * interpolate_grid (src/grids.jl:212-273) for many points at once on a device-resident
 * EnergyGrid: offsetpoint/wrap_atom (src/coordinates.jl:58-66), 8 corners x 8 channels gather
 * (grids.jl:227-244), the VdW "any corner value > 5e6 -> 1e100 K" rule (:245-248) and the
 * tricubic polynomial (:252-258, evaluated as the equivalent tensor product of cubic Hermite
 * bases instead of the 64x64 COEFF product).  This is what framework_interactions
 * (src/montecarlo.jl:490-504) and energy_grid (src/grids.jl:394-419) call per atom.
 *
 *  grid        [8*(dims[0]+1)*(dims[1]+1)*(dims[2]+1)] float, layout as above, ALREADY in K
 *              (i.e. after parse_grid's `grid .*= GRID_TO_KELVIN`, grids.jl:78);
 *              host memory if grid_on_device == 0, else a device pointer; either way the handle
 *              keeps its own node-major copy ([x][y][z][8]), the input is not referenced later
 *  mat,invmat  UNIT-cell matrix of csetup.cell (not the supercell), column-major
 *  is_vdw      1 for a VdW grid (ewald_precision == Inf): enables the 5e6 rule
 */
typedef struct ceg_interp ceg_interp_t;

/* What parse_grid (src/grids.jl:61-94) reads from a .grid file besides the payload. */
typedef struct ceg_grid_header {
    double  spacing;
    int32_t dims[3];
    int32_t has_mat;            /* 1 if the file ends with the 9 x f64 cell matrix (grids.jl:154,182), then in `mat` */
    double  size[3], shift[3], delta[3], unitcell[3];
    int32_t num_unitcell[3];
    int32_t _pad;
    double  ewald_precision;    /* Inf for a VdW grid (grids.jl:92) */
    double  mat[9];             /* column-major */
} ceg_grid_header_t;

CEG_API int ceg_interp_create(ceg_interp_t** handle, int32_t device,
                              const float* grid, int32_t grid_on_device,
                              const int32_t dims[3], const double size[3], const double shift[3],
                              const double mat[9], const double invmat[9], int32_t is_vdw);
/* A cached grid straight from its file ("Retrieved ... grid", src/raspa.jl:426-438 -> parse_grid, src/grids.jl:61-94): header
 * parsed, payload streamed file -> pinned ring -> device, multiplied by `scale` (GRID_TO_KELVIN, grids.jl:78: each product formed
 * in Float64 and rounded to Float32) on the device, node-major copy made -- no host array, no second upload.
 *  iscoulomb   the file carries the Ewald precision after the header (136 bytes instead of 128); VdW grids get the 5e6 rule
 *  mat,invmat  both NULL: the cell matrix stored at the end of the file is used (its inverse is formed here); else the unit-cell
 *              matrix and its inverse as for ceg_interp_create (parse_grid's `mat` argument)
 *  header_out  may be NULL */
CEG_API int ceg_interp_create_from_file(ceg_interp_t** handle, int32_t device, const char* path, int32_t iscoulomb, double scale,
                                const double* mat, const double* invmat, ceg_grid_header_t* header_out);
/* EnergyGrid.higherorder (grids.jl:21-29): 1 (default) the tricubic branch; 0 the "no derivatives" branch of interpolate_grid
 * (:259-269) -- channel 1 at the 8 corners, trilinear weights, no blocking rule, with the reference's index order for that branch
 * (it addresses the [z, y, x, channel] array as [x, y, z, 1]); an index beyond its axis (a BoundsError in Julia) gives NaN. */
CEG_API int ceg_interp_set_higherorder(ceg_interp_t* handle, int32_t higherorder);
CEG_API int ceg_interp_destroy(ceg_interp_t* handle);
/* points [3*n] cartesian A, out [n] K; host memory, synchronous */
CEG_API int ceg_interp_points(ceg_interp_t* handle, const double* points, int64_t npoints, double* out);
/* device memory on the handle's device, asynchronous on `stream` */
CEG_API int ceg_interp_points_device(ceg_interp_t* handle, const double* d_points, int64_t npoints,
                                     double* d_out, void* stream);
/* in-place `grid .*= scale` in Float32 on device memory (parse_grid, grids.jl:78), so a grid
 * that was just built by ceg_plan_build_* can be interpolated without leaving the GPU */
CEG_API int ceg_scale_grid_device(float* d_grid, int64_t nfloats, double scale, int32_t device, void* stream);

/* ---- grid consumer: batched reciprocal-space Ewald energy --------- */
/*
 * The `coulomb_reciprocal` term of energy_point (src/grids.jl:319-325): compute_ewald(ctx)
 * (src/ewald.jl:555-577) for a context holding ONE rigid molecule, evaluated for many placements of
 * that molecule at once:
 *   E = 2*(sum_k kf_k Re(conj(S_f(k)) S_a(k)) + energy_net_charges) + sum_k kf_k |S_a(k)|^2
 *       + static_contribution,      S_a(k) = sum_atoms q exp(2 pi i k.f),  f = invmat * position
 * With ceg_interp_* this completes energy_point / energy_grid on the device.
 *
 *  kvec_ijk  [3*nk] integer k-vectors in the order of kspace.kindices (src/ewald.jl:213-236)
 *  kfactors  [nk]   (src/ewald.jl:247-259);  sf_re, sf_im [nk] = StoreRigidChargeFramework (:267-271)
 *  ks        (kx, ky, kz);  invmat: inverse of the SUPERCELL matrix (eframework.invmat), column-major
 */
typedef struct ceg_recip ceg_recip_t;

CEG_API int ceg_recip_create(ceg_recip_t** handle, int32_t device, const int32_t* kvec_ijk,
                             const double* kfactors, const double* sf_re, const double* sf_im, int64_t nk,
                             const int32_t ks[3], const double invmat[9]);
CEG_API int ceg_recip_destroy(ceg_recip_t* handle);
/* Host side only (works without a device): the row / segment layout ceg_recip_create gives these k-vectors.  The kernel walks
 * them as rows (j, k) x i = i0..i1 -- the structure of the reference's kspace.kindices (src/ewald.jl:213-236) --, cut into segments
 * dealt to the 64 lanes in `nrounds` rounds; round r runs to its longest segment, `nslots` = the sum of those lengths.
 *  slot_of [nk]            (may be NULL) slot * 64 + lane of every k-vector
 *  desc    [nrounds * 64]  (may be NULL; size it from a first call) i0 | (j + ky) << 9 | (k + kz) << 18 | round length << 27 */
CEG_API int ceg_recip_layout(const int32_t* kvec_ijk, int64_t nk, const int32_t ks[3], int32_t* nrounds, int32_t* nslots,
                             int64_t* slot_of, int32_t* desc);
/* Host side only (works without a device): the launch ceg_recip_energy* would give these k-vectors, a molecule of `natoms` atoms
 * and `n` placements -- for diagnostics and for tests that must know which kernel variant they exercise.
 *  out = { waves per workgroup (8, 4, 2, 1), 1 when the k-vector constants are staged in LDS else 0,
 *          placements a wave walks (1, 2, 4, 8), dynamic LDS bytes }
 * Refusals as at the launch: natoms > 16 and tables above 64 KiB CEG_ERR_UNSUPPORTED; the k-space checks of ceg_recip_create. */
CEG_API int ceg_recip_launch_shape(const int32_t* kvec_ijk, int64_t nk, const int32_t ks[3], int32_t natoms, int64_t n,
                                   int32_t out[4]);
/* positions [n][natoms][3] A, charges [natoms] e, out [n] K -- host memory, synchronous.
 * energy_net_charges / static_contribution: the two EwaldContext constants (src/ewald.jl:497-544). */
CEG_API int ceg_recip_energy(ceg_recip_t* handle, const double* positions, const double* charges,
                             int32_t natoms, int64_t n, double energy_net_charges,
                             double static_contribution, double* out);
/* positions / out in device memory (charges on the host), asynchronous on `stream` */
CEG_API int ceg_recip_energy_device(ceg_recip_t* handle, const double* d_positions, const double* charges,
                                    int32_t natoms, int64_t n, double energy_net_charges,
                                    double static_contribution, double* d_out, void* stream);

/* replace the structure factor the placements are summed against (same nk).  With
 * sf = framework + all other guests ("rest" of single_contribution_ewald, src/ewald.jl:718-737) and
 * energy_net_charges = static_contribution = 0, ceg_recip_energy* returns single_contribution_ewald
 * of the moved molecule for every trial placement. */
CEG_API int ceg_recip_set_structure_factor(ceg_recip_t* handle, const double* sf_re, const double* sf_im);

/* ---- energy_grid for a rigid molecule in many orientations (SURVEY 8f, rows f1 + f2 on a lattice) ---- */
/*
 * energy_grid (src/grids.jl:346-424) of a CrystalEnergySetup: for every point (iA, iB, iC) of the lattice
 * iA*stepA + iB*stepB + iC*stepC (:382-384, :396) and every orientation k of the molecule, sum(energy_point(...)) (:311-327) with the
 * atoms at offset + rotations[k] * base[a] (:389, :409): 1e100 when an atom sits on a blocked node of the BlockFile, else
 *   sum_a interpolate_grid(vdw grid of atom a) + sum_a q_a interpolate_grid(coulomb grid) + compute_ewald of the molecule there.
 * The atom positions are generated on the device and never stored; the reciprocal term uses the lattice: the structure factor of
 * the molecule is (phase of the offset) x (structure factor of the rotated molecule), so all placements share one real matrix
 * product over the k-vectors (csrc/ceg_egrid.hip) instead of one table build and one k-space walk per placement.
 *
 *  vdw_grids     [natoms] handle of the VdW grid of each atom (setup.grids[atomsidx[i]]); NULL = zero grid -> 0 K
 *  coulomb_grid  NULL: setup.coulomb.ewald_precision == -Inf, the Coulomb terms are 0 (grids.jl:317)
 *  recip         NULL iff coulomb_grid is NULL; the structure factor it currently holds is the one summed against
 *  base          [natoms][3] A: position(molecule);  charges [natoms] e: setup.charges;  natoms 1 .. 16
 *  rotations     [nrot][9] column-major, applied as r * p (grids.jl:389); ANY 3x3 matrix, not checked for orthogonality;  nrot >= 1
 *  steps         stepA, stepB, stepC as columns (grids.jl:382-384);  num = numA, numB, numC
 *  block         NULL = no blocking; else the BlockFile mask [block_dims[0]+1][block_dims[1]+1][block_dims[2]+1] (z fastest, 1 =
 *                blocked) as ceg_block_* writes it, host memory, with the csetup of the BlockFile (coordinates.jl:58-70, 83-101):
 *                block_dims / block_size / block_shift as for the grids, block_mat / block_invmat the unit cell
 *  energy_net_charges, static_contribution   the two EwaldContext constants, as ceg_recip_energy
 *  out           nrot*numA*numB*numC doubles in Julia's memory order of `allvals`: element (k, iA, iB, iC), 0-based, at
 *                k + nrot*(iA + numA*(iB + numB*iC)).  out_on_device = 1: device memory on the handles' device, asynchronous on
 *                `stream`.  out_on_device = 0: host memory, synchronous; the lattice travels in slabs of iC of at most
 *                CEG_HIP_EGRID_SLAB_BYTES (default 256 MiB; at least one iC plane), so the device holds one slab besides the
 *                tables.  The result does not depend on the slab size, nor on where `out` lives, bit for bit.
 * All handles must live on one device (CEG_ERR_INVALID otherwise); natoms > 16 -> CEG_ERR_UNSUPPORTED.
 * Not covered: the MonteCarloSetup variant (energy_point_mc!, guests retained), the num_rotate < 0 random-offset mode
 * (grids.jl:404-406), the scratchspace cache (:349-354, host business) and the Lebedev tables (an artifact the reference
 * downloads): the rotation matrices are an input.  What the reference does with `allvals` next -- meanBoltzmann over the
 * rotation axis, the minimum over the orientations -- is ceg_energy_grid_reduced below, which never moves the elements.
 */
CEG_API int ceg_energy_grid(ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid, ceg_recip_t* recip,
                            const double* base, const double* charges, int32_t natoms,
                            const double* rotations, int32_t nrot, const double steps[9], const int32_t num[3],
                            const uint8_t* block, const int32_t block_dims[3], const double block_size[3], const double block_shift[3],
                            const double block_mat[9], const double block_invmat[9],
                            double energy_net_charges, double static_contribution,
                            double* out, int32_t out_on_device, void* stream);

/*
 * The same elements collapsed over the rotation axis on the device, per lattice point (iA, iB, iC):
 *   min     the smallest of the nrot elements;  argmin  the 0-based index of the first orientation that attains it (findmin)
 *   mean_t  meanBoltzmann(allvals, T_t, weights) (src/utils.jl:415-443), what output_cube (src/output.jl:207-209) and compute_levels
 *           (src/basins.jl:842-869) make of the array:  m = min - 30 T_t,  f_k = exp((m - x_k)/T_t) w_k  (w_k = 1 without weights),
 *           mean = sum_k(f_k x_k) / sum_k(f_k), evaluated as min + sum_k(f_k (x_k - min)) / sum_k(f_k): a single orientation, or
 *           equal elements, give the element itself bit for bit
 * A blocked element (1e100) has f = 0 and drops out of the mean; where every orientation is blocked min is 1e100 exactly and the
 * mean is what the formula gives, about 1e100.  A NaN element makes min and every mean of its point NaN, argmin the first NaN.
 *
 *  every argument up to static_contribution: as ceg_energy_grid
 *  temperatures  [ntemps] K, each finite and > 0;  ntemps 0 .. CEG_EGRID_MAX_TEMPS (all of them share one pass over the elements)
 *  weights       NULL or [nrot]: meanBoltzmann's third argument (the Lebedev weights get_rotation_matrices returns), host memory
 *  out_mean      [ntemps][numA*numB*numC], NULL iff ntemps == 0;  out_min, out_argmin  [numA*numB*numC] each, either may be NULL.
 *                Element (iA, iB, iC) at iA + numA*(iB + numB*iC): every output is an Array{Float64,3} (Int32 for argmin) in
 *                Julia's memory order, temperature t at offset t*numA*numB*numC.
 *                out_on_device = 0: host memory, synchronous; the lattice is worked through in slabs of iC of at most
 *                CEG_HIP_EGRID_SLAB_BYTES of elements, the device holds one slab and its reduced outputs, and only those are copied
 *                back.  out_on_device = 1: device memory, asynchronous on `stream`; the slab of elements (same cap) comes from the
 *                stream-ordered allocator, the caller provides no room for the elements.
 * The order in which the elements of a point are combined is fixed by the kernel and depends on nrot alone: the result does not
 * depend on the slab size, on where the outputs live, nor on which other temperatures are asked for, bit for bit; min and argmin
 * are exactly those of ceg_energy_grid's elements.
 * CEG_ERR_INVALID: ntemps out of range, a temperature that is not finite and > 0, out_mean missing with ntemps > 0 (or given with
 * ntemps == 0), no output requested at all; every refusal of ceg_energy_grid holds as it stands.  Nothing is launched on a bad
 * argument.
 */
#define CEG_EGRID_MAX_TEMPS 8
CEG_API int ceg_energy_grid_reduced(ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid, ceg_recip_t* recip,
                                    const double* base, const double* charges, int32_t natoms,
                                    const double* rotations, int32_t nrot, const double steps[9], const int32_t num[3],
                                    const uint8_t* block, const int32_t block_dims[3], const double block_size[3], const double block_shift[3],
                                    const double block_mat[9], const double block_invmat[9],
                                    double energy_net_charges, double static_contribution,
                                    const double* temperatures, int32_t ntemps, const double* weights,
                                    double* out_mean, double* out_min, int32_t* out_argmin,
                                    int32_t out_on_device, void* stream);

/* ---- guest-guest pair energies for trial placements ---------------- */
/*
 * single_contribution_vdw (src/energy.jl:397-427, the exhaustive variant :407-427) of a rigid
 * molecule against all other guest atoms of the system, for many trial placements at once:
 *   E = sum_{atom k2 of the molecule} sum_{guest atom l1 not of the excluded molecule, d2 < cutoff2}
 *           ff[kind(l1), kind(k2)](d2)
 * d2 by unsafe_periodic_distance2! (src/utils.jl:294-302: wrap to the nearest image of the MC cell, no
 * image search); rule energies as src/interactions.jl:367-406 (sum rules: :589-595), which includes the
 * CoulombEwaldDirect pair term q_i q_j erfc(alpha r)/r that carries the real-space guest-guest Ewald sum.
 *
 *  mat, invmat   MC cell (= supercell) matrix and inverse, column-major
 *  rules, rule_offset[nkinds*nkinds + 1]   rule run of the pair (a, b), 0-based kinds, at index
 *                a*nkinds + b (the table is symmetric); kinds rejected as for the grids -> CEG_ERR_RULE
 *                only for UndefinedInteraction (every other kind has an energy form)
 *  coulombic     COULOMBIC_CONVERSION_FACTOR in K A / e^2 (src/constants.jl), an argument like lambda
 */
typedef struct ceg_pairs ceg_pairs_t;

CEG_API int ceg_pairs_create(ceg_pairs_t** handle, int32_t device, const double mat[9], const double invmat[9],
                             double cutoff2, const ceg_rule_t* rules, const int32_t* rule_offset,
                             int32_t nkinds, double coulombic);
CEG_API int ceg_pairs_destroy(ceg_pairs_t* handle);
/* the guest atoms currently in the system: positions [3*natoms] A, kinds [natoms] 0-based ff index,
 * molecule [natoms] id of the molecule each atom belongs to (any non-negative labelling) */
CEG_API int ceg_pairs_set_atoms(ceg_pairs_t* handle, const double* positions, const int32_t* kinds,
                                const int32_t* molecule, int64_t natoms);
/* trial [n][m][3] A, trial_kinds [m]; atoms with molecule id == exclude_molecule are skipped (-1: none);
 * out [n] K.  Host memory, synchronous. */
CEG_API int ceg_pairs_energy(ceg_pairs_t* handle, const double* trial, const int32_t* trial_kinds, int32_t m,
                             int64_t n, int32_t exclude_molecule, double* out);
/* trial / out in device memory, asynchronous on `stream` */
CEG_API int ceg_pairs_energy_device(ceg_pairs_t* handle, const double* d_trial, const int32_t* trial_kinds,
                                    int32_t m, int64_t n, int32_t exclude_molecule, double* d_out, void* stream);
/* 1 when the atoms are kept sorted by neighbour cell (MC cells much larger than the cutoff sphere: the reference's
 * CellListMap branch, energy.jl:399-404; CEG_HIP_MC_CELLS=1|0 forces the choice at create time), with the bins per
 * fractional axis; 0 for the exhaustive loop.  Same sums either way. */
CEG_API int ceg_pairs_neighbour_cells(ceg_pairs_t* handle, int32_t nb[3]);

/* ---- device-resident Monte-Carlo energy state (BASELINE config 5: f1 + f2 + f3 in one launch) ---- */
/*
 * movement_energy (src/montecarlo.jl:563-579) of one rigid molecule of a MonteCarloSetup for a batch of trial
 * placements, from state that lives on the device: guest atoms, pair table, k-space tables, the framework
 * structure factor, the per-molecule structure factors sums[:, ij+1] and their total sums[:, 1] of the reference's
 * IncrementalEwaldContext (src/ewald.jl:584-652).  One kernel launch evaluates, per placement,
 *   framework_interactions    (montecarlo.jl:490-504)  sum_atoms interpolate_grid(vdw grid of the atom's kind) and
 *                                                      sum_atoms charge * interpolate_grid(coulomb grid) (1e100 kept)
 *   single_contribution_vdw   (energy.jl:407-427)      against every guest atom of the OTHER molecules
 *   single_contribution_ewald (ewald.jl:704-738)       2 sum kf Re(conj(rest) S) + sum kf |S|^2,
 *                                                      rest = framework + sums[:,1] - sums[:,ij+1]
 * and ceg_mc_accept applies update_mc! / update_ewald_context! (montecarlo.jl:615-628, ewald.jl:757-773) on the
 * device: no host-built structure factor is uploaded between moves.  Molecules are rigid, <= 16 atoms.
 *
 *  vdw_grids    [nkinds] interpolation handles by 0-based force-field index, NULL where the kind has no grid / a zero grid;
 *               coulomb_grid NULL when the framework carries no charges.  The handles must outlive this object.
 *  kind_charge  [nkinds] e;  mat, invmat: MC cell (= supercell), column-major;  rules / rule_offset / coulombic as ceg_pairs_create
 *  kvec_ijk, kfactors, sf_re, sf_im, nk, ks, ewald_invmat as ceg_recip_create (nk = 0: no Ewald summation)
 *
 * Threading: a handle is NOT thread-safe -- one Markov chain, one caller at a time (the reference's update_mc! is not either);
 * different handles may be driven from different threads.  A chain group (ceg_mc_group_*, below) and all its members are driven
 * from ONE thread: while a handle is grouped its calls share the group's stream and staging.
 * Errors: accept / insert / remove keep a host mirror (molecule table, free atom slots, neighbour-cell lists) in step with the
 * device state.  If one of them fails after it has started to change either side (kernel launch failure, allocation failure
 * while growing the arrays or rebuilding the cells) the handle is marked inconsistent: every later call except
 * ceg_mc_set_guests and ceg_mc_destroy returns CEG_ERR_HIP, and ceg_mc_set_guests rebuilds both sides from scratch.
 */
typedef struct ceg_mc ceg_mc_t;

/* A new handle is an EMPTY BOX and usable as it is: ceg_mc_trial_insert / _insert_device, ceg_mc_insert and ceg_mc_get_state need no
 * ceg_mc_set_guests first (a GCMC isotherm starts there); ceg_mc_set_guests with nmol = 0 gives the same state. */
CEG_API int ceg_mc_create(ceg_mc_t** handle, int32_t device, ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid,
                          const double* kind_charge, int32_t nkinds, const double mat[9], const double invmat[9],
                          double cutoff2, const ceg_rule_t* rules, const int32_t* rule_offset, double coulombic,
                          const int32_t* kvec_ijk, const double* kfactors, const double* sf_re, const double* sf_im,
                          int64_t nk, const int32_t ks[3], const double ewald_invmat[9]);
CEG_API int ceg_mc_destroy(ceg_mc_t* handle);
/* the guests currently in the system, molecule j = atoms [mol_first[j], mol_first[j+1]) (mol_first[0] = 0):
 * positions [3*natoms] A, kinds [natoms] 0-based ff index.  Computes every sums[:, ij+1] and sums[:, 1] on the device
 * (compute_ewald(::IncrementalEwaldContext), ewald.jl:630-652).  Synchronous. */
CEG_API int ceg_mc_set_guests(ceg_mc_t* handle, const double* positions, const int32_t* kinds,
                              const int32_t* mol_first, int32_t nmol);
/* trial [n][m][3] A placements of molecule `molecule` (m = its atom count); out [(n+1)][4] K:
 * row 0 = movement_energy where the molecule is now, row 1+t = at trial t; columns framework vdw, framework direct,
 * guest-guest, reciprocal.  Host memory; one launch + one stream synchronisation (small batches travel through pinned,
 * device-mapped buffers). */
CEG_API int ceg_mc_trial(ceg_mc_t* handle, int32_t molecule, const double* trial, int64_t n, double* out);
/* The same with the trial placements and the result rows in DEVICE memory (like ceg_recip_energy_device / ceg_pairs_energy_device):
 * for callers that generate trials on the device or evaluate large batches repeatedly -- a 65 536-placement call through the host
 * entry point spends a third of its time moving 4.7 MB in and 2.1 MB out of pageable memory.  Enqueued on `stream` (a hipStream_t,
 * NULL = the null stream), ordered behind everything this handle has enqueued so far; later accept / insert / remove calls are
 * ordered behind it; no synchronisation: the rows are valid when `stream` has reached this point.  Always the wave-per-placement
 * kernels.  ceg_mc_trial_insert_device: the GCMC counterpart (see ceg_mc_trial_insert). */
CEG_API int ceg_mc_trial_device(ceg_mc_t* handle, int32_t molecule, const double* d_trial, int64_t n, double* d_out, void* stream);
CEG_API int ceg_mc_trial_insert_device(ceg_mc_t* handle, const int32_t* kinds, int32_t m, const double* d_trial, int64_t n, double* d_out, void* stream);
/* the molecule now sits at positions [m][3]: update_mc! on the device.  Asynchronous; later calls on this handle are
 * ordered behind it. */
CEG_API int ceg_mc_accept(ceg_mc_t* handle, int32_t molecule, const double* positions);
/* GCMC swaps (gcmc.jl / mcmoves.jl evaluate them with the same movement_energy):
 * trial_insert: movement_energy of a molecule that is NOT in the system (kinds [m] 0-based ff indices) at each of n trial
 *   placements trial [n][m][3]: nothing excluded from the pair sum, rest = framework + sums[:, 1]
 *   (single_contribution_ewald with ij < 0, ewald.jl:704-728); out [n][4], no current-position row.  Synchronous.
 * insert: add_one_system! (ewald.jl:775-792): the molecule becomes index nmol (returned in *molecule_out); asynchronous.
 * remove: remove_one_system! (ewald.jl:794-810, :404-413): sums[:, 1] -= sums[:, ij+1]; the LAST molecule takes index
 *   `molecule` (*moved_out = its old index, = `molecule` when it was the last one); asynchronous. */
CEG_API int ceg_mc_trial_insert(ceg_mc_t* handle, const int32_t* kinds, int32_t m, const double* trial, int64_t n, double* out);
CEG_API int ceg_mc_insert(ceg_mc_t* handle, const int32_t* kinds, int32_t m, const double* positions, int32_t* molecule_out);
CEG_API int ceg_mc_remove(ceg_mc_t* handle, int32_t molecule, int32_t* moved_out);
/* read back (any pointer may be NULL): positions [3*natoms] in molecule order, total guest structure factor sums[:, 1] as re / im [nk] */
CEG_API int ceg_mc_get_state(ceg_mc_t* handle, double* positions, double* sf_total_re, double* sf_total_im);
/* The guest-guest sum runs over neighbour cells (the reference's CellListMap branch, energy.jl:341-349,399-404) when the MC
 * cell is large enough for that to pay: fractional bins of the cell kept current on the device by accept / insert / remove.
 * Returns 1 with the bin counts and the per-cell capacity when the cells are in use, 0 (and zeros) for the exhaustive loop;
 * the energies are the same sums either way.  Environment: CEG_HIP_MC_CELLS=1|0 forces the choice, CEG_HIP_MC_BIN = bin width, A. */
CEG_API int ceg_mc_neighbour_cells(ceg_mc_t* handle, int32_t nb[3], int32_t* capacity);
/* ---- chain groups: one Markov step of K chains per launch (make_isotherm's chains, src/parameterinputs.jl:316-329) ----
 * K handles on ONE device stepped in lockstep: one launch evaluates the trials of every chain, one launch applies every accepted
 * move; with trial / accept the acceptance rule stays with the caller (ceg_mc_group_sweep, below, runs whole sweeps of
 * translations and rotations on the device).  A batch-1 ceg_mc_trial is mostly launch and completion latency; a group pays
 * it once per step for all K chains.
 *
 * create: 1 <= k <= CEG_MC_GROUP_MAX handles, all on one device, each at most once, none already in a group, each after
 *   ceg_mc_set_guests (CEG_ERR_INVALID otherwise).  Synchronises every member's stream; until destroy, every member's own
 *   asynchronous work (accept, insert, remove, the _device trials) runs on the group's stream, so per-handle calls stay legal
 *   and are ordered with the group calls.  ceg_mc_destroy of a grouped handle returns CEG_ERR_INVALID.
 * destroy: synchronises the group and gives every member its own stream back (the handles stay valid).
 * trial (host memory, synchronous): for chain c
 *   molecule[c] >= 0  displacement of that molecule: n[c] + 1 rows as ceg_mc_trial lays them out (n[c] = 0: row 0 alone, the
 *                     deletion energy);
 *   molecule[c] == -1 insertion of a molecule of kinds insert_kinds[0..insert_m) (one species per call): n[c] rows as ceg_mc_trial_insert;
 *   molecule[c] == -2 the chain is idle in this step.
 *   trial holds the placements [n[c]][m_c][3] packed in chain order, out the rows [.][4] packed in chain order.  A chain's rows come
 *   from the kernel body of ceg_mc_trial / ceg_mc_trial_insert with its three-workgroup split (the single-handle path up to 256
 *   rows): columns 0, 2, 3 bit-identical, column 1 (framework direct) to ~1e-12 relative, where the compiler fuses a few
 *   multiply-adds of the interpolation differently.  More placements or rows than the group's mapped staging holds (1 MiB
 *   each way: 32 768 rows) -> CEG_ERR_UNSUPPORTED: large batches belong on ceg_mc_trial_device.
 * accept (asynchronous): update_mc! for every chain with molecule[c] >= 0 (negative: nothing for that chain), positions [m_c][3]
 *   of the accepted chains only, packed in chain order.  If the call fails after it has changed a chain's host mirror, every chain
 *   it touched is marked inconsistent (see Errors above).
 * A call that would use a chain marked inconsistent returns CEG_ERR_HIP, with the chain's index in ceg_last_error(). */
#define CEG_MC_GROUP_MAX 256
typedef struct ceg_mc_group ceg_mc_group_t;

CEG_API int ceg_mc_group_create(ceg_mc_group_t** group, ceg_mc_t* const* chains, int32_t k);
CEG_API int ceg_mc_group_destroy(ceg_mc_group_t* group);
CEG_API int ceg_mc_group_trial(ceg_mc_group_t* group, const int32_t* molecule, const int32_t* n,
                               const int32_t* insert_kinds, int32_t insert_m, const double* trial, double* out);
CEG_API int ceg_mc_group_accept(ceg_mc_group_t* group, const int32_t* molecule, const double* positions);

/* ---- sweeps: S Markov steps of all K chains of a group with no host round trip between steps ----
 * The inner loop of run_montecarlo! (src/simulation.jl:727-781) for rigid translations and rotations: choose a molecule and a move,
 * build the trial placement from the resident positions, movement_energy before and after, compute_accept_move
 * (src/montecarlo.jl:702-712), update_mc!.  Proposal, decision and update run on the device; the rows are those of
 * ceg_mc_group_trial (the same kernel body, three workgroups per row), the update is that of ceg_mc_group_accept.  Per step two
 * launches are enqueued back to back on the group's stream (one more where fast and exact-pair chains are mixed); a chain's
 * per-step inputs and rows stay in device memory and the host synchronises once, at the end.
 *
 * Random stream: Philox4x32-10, multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85.
 *   key = (seed low word, seed high word); counter = (step low, step high, stream id of the chain, purpose), step = first_step + s
 *   the absolute 64-bit step number.  Known answers (counter; key) -> output:
 *     0 0 0 0; 0 0                                            -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff x4; ffffffff x2                                -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0  -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   U(a, b) = (((uint64)a << 21) | (b >> 11)) * 2^-53 in [0, 1).  One block (w0..w3) per (step, stream, purpose); every workgroup
 *   that takes part in a chain's step regenerates it, nothing random is stored.  For stream c at step s:
 *     purpose 0, selection: molecule j = min(floor(U(w0,w1) nmol), nmol - 1); a rotation iff molecule j has more than one atom
 *       and U(w2,w3) < p_rotation[c], else a translation;
 *     purposes 1 and 2, geometry: translation (random_translation, src/mcmoves.jl:139-146, scalar branch)
 *       r = ((2U(w0,w1)-1) dmax, (2U(w2,w3)-1) dmax, (2U(w0',w1')-1) dmax), primed words from purpose 2, added to every atom;
 *       rotation (random_rotation, :147-164) theta = thetamax (2U(w0,w1)-1) rad, axis = min(floor(3 U(w2,w3)), 2), the matrices of
 *       :155-161, about atom `bead` of the molecule: ref + R (p - ref);
 *     purpose 3, acceptance: u = U(w0,w1).
 * Rule: b, a = the four columns of the row before / after summed left to right; a trial whose framework VdW column is >= 1e90 is
 *   blocked and rejected; otherwise accepted if a < b or u < exp((b - a) / T).  A chain without molecules is idle.
 *
 * params: seed, first_step; per chain stream_id (pairwise distinct), temperature K (finite, > 0), dmax A and thetamax rad (finite,
 *   >= 0), p_rotation in [0, 1]; bead: one 0-based atom index per molecule of every chain, packed in chain order (molecule order of
 *   ceg_mc_set_guests / ceg_mc_insert).  A violation, nsteps < 0 or a missing pointer -> CEG_ERR_INVALID; a member that keeps its
 *   guests in neighbour cells -> CEG_ERR_UNSUPPORTED unless ceg_mc_group_set_device_cells, below, is on (its update needs the cell lists); a member marked
 *   inconsistent -> CEG_ERR_HIP.  A refused call launches nothing and leaves every chain as it was.  nsteps == 0: zeros.
 * stats_out [K]: trials and acceptances per move kind (a blocked trial counts as a trial of its kind and in `blocked`), delta =
 *   FP64 sum of a - b over the accepted moves.
 * log_out [nsteps][K] or NULL (production): per (step, chain) the molecule and move kind (0 translation, 1 rotation; both -1 for
 *   an idle chain), the accepted flag, u, the rows before / after and the proposed positions (unused entries zero).
 * Synchronous.  Afterwards every per-handle and group entry point works on the moved state; the molecule table does not change.
 * Not covered: swap / reinsertion / random_* moves (ceg_mc_group_sweep_gcmc, below), the inblockpocket test of choose_step! (a group with
 * masks installed by ceg_mc_group_set_blocks is refused with CEG_ERR_UNSUPPORTED rather than swept without them), and the adaptation of
 * dmax / thetamax (src/simulation.jl:820-825): ceg_mc_group_sweep_cycles, below, runs it at every cycle end. */
typedef struct ceg_mc_sweep_params {
    uint64_t seed, first_step;
    const uint32_t* stream_id;                 /* [K] */
    const double *temperature, *dmax, *thetamax, *p_rotation;      /* [K] each */
    const int32_t* bead;                       /* [sum of the chains' molecule counts] */
} ceg_mc_sweep_params_t;
typedef struct ceg_mc_sweep_stats {
    int64_t translation_trials, translation_accepted, rotation_trials, rotation_accepted, blocked;
    double delta;
} ceg_mc_sweep_stats_t;
typedef struct ceg_mc_sweep_record {
    int32_t molecule, kind, accepted, _pad;
    double u;
    double rows[2][4];
    double positions[16][3];
} ceg_mc_sweep_record_t;

CEG_API int ceg_mc_group_sweep(ceg_mc_group_t* group, const ceg_mc_sweep_params_t* params, int64_t nsteps,
                               ceg_mc_sweep_stats_t* stats_out, ceg_mc_sweep_record_t* log_out);

/* ---- GCMC sweeps: all six move kinds of src/mcmoves.jl:1-8, the molecule table owned by the device ----
 * The inner loop of run_montecarlo! (src/simulation.jl:730-781) with choose_step! (:271-326): species, move kind and molecule drawn
 * per step, the proposal built on the device, movement_energy rows from the kernel body of ceg_mc_group_trial (displacement and
 * insertion rows alike), compute_accept_move / compute_accept_move_swap (src/montecarlo.jl:702-712, src/gcmc.jl:77-88), then
 * update_mc! / add_one_system! / remove_one_system! with the semantics of ceg_mc_accept / ceg_mc_insert / ceg_mc_remove -- all on the
 * device, two launches per step (three where fast and exact-pair chains are mixed), one synchronisation per sweep.
 * ceg_mc_group_sweep, its stream and its results are unchanged; this entry point shares purposes 1-3 of its stream and adds 4-8.
 *
 * Move kinds (record.kind, index of stats.trials / stats.accepted): 0 translation, 1 rotation, 2 random_translation, 3 random_rotation,
 *   4 random_reinsertion, 5 swap_insertion, 6 swap_deletion.
 * Random stream (Philox4x32-10, key, counter and U(a, b) as for ceg_mc_group_sweep), stream c at the absolute step s:
 *   purpose 4, selection: species i = min(floor(U(w0,w1) nspecies), nspecies - 1); move kind = the first k in 0..4 with
 *     U(w2,w3) < cumulative[k] of species i, else swap;
 *   purpose 5, molecule: with N_i the molecules of species i, j = min(floor(U(w0,w1) N_i), N_i - 1): the j-th molecule of species i
 *     counted in device molecule order; a swap is a deletion iff U(w2,w3) < 0.5, else an insertion;
 *   purposes 1 and 2: translation and rotation exactly as ceg_mc_group_sweep draws them (dmax, thetamax of the chain, atom `bead` of
 *     the species);
 *   purposes 6, 7, 8: random_translation (mcmoves.jl:143) r = mat (U3 - 0.5) with U3 = (U(w0,w1), U(w2,w3)) of purpose 6 and U(w0,w1)
 *     of purpose 7, r_x = (mat[0] a + mat[3] b) + mat[6] c etc. (mat column-major, the MC cell); random_rotation theta =
 *     pi (2 U(w2,w3) - 1) from purpose 7, axis = min(floor(3 U(w0,w1)), 2) from purpose 8, the matrices of mcmoves.jl:155-161 about
 *     atom `bead`; random_reinsertion: t = p + r for every atom, then t_bead + R (t - t_bead); swap_insertion: the same pair applied
 *     to the species' model positions (simulation.jl:300-305).  A rotation of a one-atom molecule is the identity;
 *   purpose 3, acceptance: u = U(w0,w1).
 * A step whose species has N_i == 0 and whose move is not an insertion is SPENT (simulation.jl:282): nothing is evaluated, nothing
 *   is counted but stats.spent.
 * Rows: displacement kinds rows[0] / rows[1] = movement_energy before / after; deletion rows[0] = movement_energy where the molecule
 *   is, rows[1] = zeros; insertion rows[0] = zeros, rows[1] = the row of ceg_mc_trial_insert at the proposed placement.
 * Rule: displacements as ceg_mc_group_sweep (framework VdW of the trial row >= 1e90: blocked, rejected).  Swaps, all in FP64 and in
 *   this order: E = ((row[0] + row[1]) + row[2]) + row[3]; tc = modify_species_dryrun(i, +-1) (src/tailcorrection.jl:86-96) on the
 *   chain's current counts: d = tail_framework[i]; for j = 0..nspecies-1 in order: d += (j == i) ? (double)(n + 2 N_j) tail_cross[i][j]
 *   : (double)(2 N_j) tail_cross[i][j]; tc = d (double)n with n = +1 / -1;
 *   insertion: diff = (E - self_reciprocal) + tc, accepted iff u < ((phiPV_div_k / T) / (N_i + 1)) exp(-diff / T); an insertion whose
 *     framework VdW column is >= 1e90 is blocked and rejected;
 *   deletion:  diff = -(E - self_reciprocal) + tc, accepted iff u < ((N_i T) / phiPV_div_k) exp(-diff / T).
 * Update: an accepted insertion becomes molecule nmol (the last); after an accepted deletion of molecule d the LAST molecule takes
 *   index d.  Atom slots: the slots of a deleted molecule go on a per-species stack the next insertion of that species pops; with an
 *   empty stack the insertion takes fresh slots at the high-water mark.
 * Capacity: an insertion proposed while the chain holds max_molecules molecules is counted as a swap_insertion trial and in
 *   stats.capacity, is not evaluated (rows zero) and is rejected: a caller that sees capacity > 0 knows the sweep was truncated.
 *
 * params: seed, first_step, stream_id, temperature, dmax, thetamax as ceg_mc_sweep_params_t.  species [nspecies], 1 <= nspecies <=
 *   CEG_MC_GCMC_MAX_SPECIES, shared by the chains: m atoms (1..16) of kinds[m], model positions (mc.models[i]), bead (0-based),
 *   cumulative[5] (the MCMoves tuple: non-decreasing, in [0, 1]; swap probability = 1 - cumulative[4]), phiPV_div_k K (finite, > 0
 *   where the swap probability is > 0), self_reciprocal K (ctx.energies[i], simulation.jl:768,770), tail_framework and
 *   tail_cross[0..nspecies) (zeros: no tail correction).  molecule_species: the species of every current molecule, packed in chain
 *   order and device molecule order (atom count and kinds must match the handle's molecule).  max_molecules [K] >= the chain's count.
 *   molecule_species_out (may be NULL): the final table, chain c at offset sum of max_molecules[0..c), stats[c].nmol entries.
 *   Violations -> CEG_ERR_INVALID; a member with neighbour cells -> CEG_ERR_UNSUPPORTED; a member marked inconsistent -> CEG_ERR_HIP;
 *   each decided before anything is launched or changed.
 * stats_out [K]; log_out [nsteps][K] or NULL.  record.molecule: device index (an insertion: the index it takes if accepted; -1 for a
 *   spent step); record.flags: 1 spent, 2 blocked, 4 capacity; record.n_species = N_i before the move; record.tc = the tail-correction
 *   change of a swap (0 otherwise).  stats.delta_moves = sum of a - b over accepted displacements, stats.delta_swaps = sum of diff over
 *   accepted swaps.
 * Synchronous.  Afterwards the handles' host mirrors (molecule table, free atom slots, high-water mark) are rebuilt from the device and
 *   every per-handle and group entry point works on the new state.
 * Not covered: the fugacity coefficient and the accessible-volume factor of GCMCData (phiPV_div_k
 *   comes from the caller, as the reference takes it from Clapeyron), and chains that keep their guests in neighbour cells.  One
 *   phiPV_div_k per chain and a last step per chain (an isotherm's pressures): ceg_mc_group_set_chain_plan, below.
 *
 * Block pockets (ceg_mc_group_set_blocks): the inblockpocket test and the 1000-attempt retry loop of choose_step!
 * (src/simulation.jl:271-326, src/montecarlo.jl:631-640), resolved inside the trial launch of the step (no launch is added).
 *   Masks: a block is a byte mask [dims[0]+1][dims[1]+1][dims[2]+1], z fastest, 1 = blocked, as ceg_block_from_grid / ceg_block_spheres
 *     write it, with its own dims, size, shift, mat, invmat (column-major) and offset[3].  The lookup of a point p (BlockFile getindex,
 *     src/coordinates.jl:58-66,97-101) runs in FP64 without contraction: q = p + offset; abc = invmat q summed left to right;
 *     abc -= floor(abc); w = mat abc; index_c = rint((w_c - shift_c) * dims_c / size_c + 1) - 1 (ties to even), clamped to [0, dims_c] for
 *     memory safety only.  A NULL mask is BlockFile.empty: never blocked.  Species blocks: one per species, offset = 0.  Atom blocks
 *     (atomblocks of src/montecarlo.jl:181-186): one per atom kind (0-based, the index used in species.kinds), offset_c =
 *     (size_c / dims_c) / 2, the csetup.Delta ./ 2 of montecarlo.jl:636.
 *   inblockpocket(i, pos) is true iff for some atom a the species block of i holds pos[a], or atom blocks are installed and the atom
 *     block of kinds[a] holds pos[a].
 *   Random stream: attempt t = 0..999 of a retried proposal draws purposes 6, 7, 8 with counter word 3 = purpose | (t << 8); attempt 0
 *     is the block a group without masks draws.  Purposes 0-5 are never retried.
 *   Per move kind, after the selection (spent and capacity steps are decided first and are unchanged):
 *     0 translation, 1 rotation, 3 random_rotation: one proposal; if inblockpocket, the step is pocket-blocked;
 *     2 random_translation, 4 random_reinsertion: the first attempt t with !inblockpocket is the proposal; none in 1000: pocket-blocked;
 *     5 swap_insertion: the first attempt t whose bead atom lies outside the species block (species block and bead only,
 *       simulation.jl:310-316) is the proposal; if inblockpocket of that whole placement, the step is pocket-blocked; none in 1000:
 *       pocket-blocked;
 *     6 swap_deletion: no test.
 *   A pocket-blocked step is counted in stats.trials[kind], in stats.blocked and in the chain's pocket counter
 *     (ceg_mc_group_block_counts); no energy row is evaluated (both rows of the record are zero); it is rejected, the state untouched.
 *   Record: flags bit 3 (value 8) = pocket-blocked; flags >> 16 = the index of the attempt used (0 where the kind is not retried, 999
 *     on exhaustion); positions = the proposal that was tested (zeros on exhaustion).  With no masks installed every record is
 *     bit-identical to that of a group that never heard of masks.
 *   With masks installed the call returns CEG_ERR_INVALID, before anything is launched, if params->nspecies differs from the nspecies
 *     of the masks, or if atom blocks are installed and some species.kinds[a] >= nkinds. */
#define CEG_MC_GCMC_MAX_SPECIES 8
typedef struct ceg_mc_gcmc_species {
    int32_t m, bead;
    int32_t kinds[16];
    double model[16][3];
    double cumulative[5];
    double phiPV_div_k, self_reciprocal, tail_framework;
    double tail_cross[CEG_MC_GCMC_MAX_SPECIES];
} ceg_mc_gcmc_species_t;
typedef struct ceg_mc_gcmc_params {
    uint64_t seed, first_step;
    const uint32_t* stream_id;                 /* [K] */
    const double *temperature, *dmax, *thetamax;      /* [K] each */
    int32_t nspecies, _pad;
    const ceg_mc_gcmc_species_t* species;      /* [nspecies] */
    const int32_t* molecule_species;           /* [sum of the chains' molecule counts] */
    const int32_t* max_molecules;              /* [K] */
    int32_t* molecule_species_out;             /* [sum of max_molecules] or NULL */
} ceg_mc_gcmc_params_t;
typedef struct ceg_mc_gcmc_stats {
    int64_t trials[7], accepted[7];
    int64_t blocked, capacity, spent;
    double delta_moves, delta_swaps;
    int32_t count[CEG_MC_GCMC_MAX_SPECIES];
    int32_t nmol, _pad;
} ceg_mc_gcmc_stats_t;
typedef struct ceg_mc_gcmc_record {
    int32_t species, molecule, kind, accepted;
    int32_t n_species, flags;
    double u, tc;
    double rows[2][4];
    double positions[16][3];
} ceg_mc_gcmc_record_t;

CEG_API int ceg_mc_group_sweep_gcmc(ceg_mc_group_t* group, const ceg_mc_gcmc_params_t* params, int64_t nsteps,
                                    ceg_mc_gcmc_stats_t* stats_out, ceg_mc_gcmc_record_t* log_out);

/* Block pockets of a group (semantics: above).  set_blocks copies the masks (host memory) to the group's device once; they stay until
 * they are replaced, cleared with (NULL, 0, NULL, 0) or the group is destroyed.  Synchronises the group.  CEG_ERR_INVALID: dims <= 0,
 * a geometry entry that is not finite, size <= 0, nspecies outside [0, CEG_MC_GCMC_MAX_SPECIES], nkinds < 0, or a missing array.
 * block_counts: per chain, the pocket-blocked steps of the last ceg_mc_group_sweep_gcmc and the sum of the attempt indices it used
 * (zeros before any sweep and after a sweep without masks); either pointer may be NULL. */
typedef struct ceg_mc_block {
    const uint8_t* mask;                       /* host memory; NULL = empty */
    int32_t dims[3], _pad;
    double size[3], shift[3], offset[3], mat[9], invmat[9];
} ceg_mc_block_t;
CEG_API int ceg_mc_group_set_blocks(ceg_mc_group_t* group, const ceg_mc_block_t* species_blocks, int32_t nspecies,
                                    const ceg_mc_block_t* atom_blocks, int32_t nkinds);
CEG_API int ceg_mc_group_block_counts(ceg_mc_group_t* group, int64_t* pocket_out /*[K]*/, int64_t* attempts_out /*[K]*/);

/* ---- sampler of a group: density maps and the per-cycle series, taken on the device while a sweep runs ----
 * What a run produces besides its final state: the counts of bin_trajectory (src/averageclusters.jl:154-202), the input of
 * average_clusters and of the site analysis, and the series of GCMCRecorder (Ns after every cycle, src/parameterinputs.jl:232-249)
 * and of run_montecarlo! (the running energy, src/simulation.jl:784-799).  With a sampler installed, both sweeps take a FRAME after
 * every absolute step s with s >= from_step and (s + 1) % every == 0, in step order: one more launch (k_mcg_sample) enqueued on the
 * group's stream behind the accept launch of that step.  A frame bins every occupied atom slot of every chain and appends one record
 * per chain to the series.  The sampler only reads chain state: statistics, logs and final states of a sweep are byte-identical
 * with and without it, and with no sampler installed a sweep enqueues exactly the launches it enqueues without this section.
 *
 * Bins: int64 [nmaps][nchannels][nc][nb][na], a fastest -- one (map, channel) block is a Julia Array{Int,3}(na, nb, nc).  Zeroed by
 *   set_sampler and by sampler_reset; frames accumulate.  dims = (0, 0, 0): no map, the series only.
 * Bin of a position p, in FP64 without contraction and in this order (I = unit_invmat, column-major; n = dims):
 *     y_r = (I[r] p_x + I[r+3] p_y) + I[r+6] p_z;   u_r = y_r - floor(y_r);   i_r = (int)ceil(u_r n_r) + (u_r == 0) - 1
 *   (averageclusters.jl:182-184, 0-based), then clamped to [0, n_r - 1] for memory safety only.  The map lives on the UNIT cell (the
 *   MC cell with its columns divided by the supercell): folding a supercell image onto it is the "- floor".
 *   Every symmetry operation q adds one count more (:185-188): y'_r = ((R_r0 y_0 + R_r1 y_1) + R_r2 y_2) + t_r on the unfloored y, with
 *   sym[q][r] = (R_r0, R_r1, R_r2, t_r), then the same index rule, into the same (map, channel).
 * What is binned: the occupied atom slots (molecule >= 0 in the atom record) of the chains with chain_map[c] >= 0, into map
 *   chain_map[c] and channel kind_channel[kind]; an atom of kind >= nkinds or with kind_channel[kind] == -1 is skipped.
 * Atomics: integer atomics only, so bins and records do not depend on the order in which workgroups or lanes arrive.
 * Series: one 64-byte record per (frame, chain), binned or not; series_out is [frames][K].  step: the step the frame follows;
 *   nmol: the chain's molecules; natoms: the occupied atom slots counted in the atom records (an empty chain: 0, 0, nothing binned);
 *   count: molecules per species during a GCMC sweep, zeros otherwise; delta_moves, delta_swaps: the sums of the sweep's statistics
 *   as they stand after that step's accept launch (a plain sweep: its `delta` and 0; ceg_mc_group_sample: zeros).  During a GCMC sweep
 *   molecule count, high-water mark of the slots and count[] are read from the device's own table, otherwise from the chains' views.
 * A sweep whose frames (countable from first_step, nsteps, every, from_step) exceed what is left of series_capacity, or whose steps
 *   reach beyond 2^63 - 1, returns CEG_ERR_INVALID before anything is launched or changed.
 * set_sampler: installs (replacing the earlier one; NULL removes it); synchronises the group.  CEG_ERR_INVALID with nothing changed
 *   -- the earlier sampler stays -- for: every < 1; from_step or series_capacity < 0; dims neither all zero nor all >= 1; with a map:
 *   nmaps or nchannels < 1, nkinds < 0, an entry of chain_map outside [-1, nmaps) or of kind_channel outside [-1, nchannels), a
 *   unit_invmat or sym entry that is not finite, a missing array, more than CEG_MC_SAMPLER_MAX_BINS bins over all maps and channels (8 GiB of counts); with or
 *   without a map: nsym outside [0, CEG_MC_SAMPLER_MAX_SYM].  Without a map, nmaps, nchannels, nkinds, unit_invmat and the arrays
 *   are ignored.
 * A frame whose launch fails is not counted, and a sweep that fails after it has enqueued frames takes none of them: the frame
 *   count, the series and `total` never include a record that was not written.
 * sample: one frame of the resident state, now (step = -1): asynchronous, ordered on the group's stream behind everything enqueued
 *   so far; for the host-driven trial / accept route.  Members that keep neighbour cells are accepted: the atom records are
 *   authoritative.  No sampler or a full series -> CEG_ERR_INVALID; a member marked inconsistent -> CEG_ERR_HIP.
 * sampler_read: synchronises the group; bins_out (all bins), series_out ([frames][K]) and frames_out may each be NULL.
 * sampler_reset: zeroes bins, series and the frame count. */
#define CEG_MC_SAMPLER_MAX_SYM 191
#define CEG_MC_SAMPLER_MAX_BINS 1073741824
typedef struct ceg_mc_sampler {
    int64_t every;             /* >= 1: a frame after absolute step s iff s >= from_step && (s + 1) % every == 0 */
    int64_t from_step;         /* >= 0 (the ninit cycles of a run are not sampled) */
    int64_t series_capacity;   /* >= 0 frames kept in the series */
    int32_t dims[3];           /* na, nb, nc >= 1; all three 0: no density map, series only */
    int32_t nmaps, nchannels, nkinds, nsym, _pad;
    double  unit_invmat[9];    /* inverse of the UNIT cell the map lives on (MC cell ./ supercell), column-major */
    const int32_t* chain_map;    /* [K]      map of chain c in [0, nmaps), or -1: not binned */
    const int32_t* kind_channel; /* [nkinds] channel of atoms of ff kind k in [0, nchannels), or -1: not binned */
    const double*  sym;          /* [nsym][3][4] rows (R_r0 R_r1 R_r2 t_r), fractional, unit cell; nsym <= MAX_SYM */
} ceg_mc_sampler_t;
typedef struct ceg_mc_sample_record {   /* 64 bytes */
    int64_t step;              /* absolute step the frame follows; -1 for ceg_mc_group_sample */
    int32_t nmol, natoms;      /* molecules, occupied atom slots */
    int32_t count[CEG_MC_GCMC_MAX_SPECIES];  /* GCMC sweep: molecules per species; otherwise zeros */
    double  delta_moves, delta_swaps;        /* the sweep's stats sums as they stand after that step */
} ceg_mc_sample_record_t;
CEG_API int ceg_mc_group_set_sampler(ceg_mc_group_t* group, const ceg_mc_sampler_t* spec);
CEG_API int ceg_mc_group_sample(ceg_mc_group_t* group);
CEG_API int ceg_mc_group_sampler_read(ceg_mc_group_t* group, int64_t* bins_out, ceg_mc_sample_record_t* series_out, int64_t* frames_out);
CEG_API int ceg_mc_group_sampler_reset(ceg_mc_group_t* group);

/* ---- cycles: whole cycles of run_montecarlo! on the device, temperature schedule and step-size adaptation included ----
 * The end-of-cycle block of the main loop (src/simulation.jl:727-728, 818-827): `temperature = simu.temperatures[counter_cycle]` and
 * the adaptation of statistics.dmax / statistics.θmax from the cumulative acceptance ratios.  ceg_mc_group_sweep_cycles /
 * ceg_mc_group_sweep_gcmc_cycles run ncycles * steps_per_cycle steps from params->first_step: checks, refusals, random stream, rows,
 * rule, update, stats, log and final state are those of ceg_mc_group_sweep / ceg_mc_group_sweep_gcmc over that many steps, and the
 * launches of every step are the ones that entry point enqueues, sampler frames included.  The one addition is one more launch
 * (k_mcg_cycle_end, one workgroup, one lane per chain) after the last step of each cycle, behind that step's accept launch and behind
 * its sampler frame if there is one.  It reads the chain's counters, writes the cycle's record and stores the next cycle's
 * temperature, dmax and thetamax into the chain's parameters in device memory, where the next step's launches read them: stream
 * order alone makes them visible.  The two sweeps themselves are unchanged, byte for byte and launch for launch.
 *
 * Temperature: with a table, row j ([K] values, K) is in force during cycle j of the call; params->temperature is then not read and
 *   may be NULL.  Every entry must be finite and > 0.  ceg_mc_group_sweep_gcmc_cycles: if any species has a swap probability > 0
 *   (cumulative[4] < 1), every chain's column must be constant -- the reference refuses GCMC with a varying temperature
 *   (simulation.jl:688) and phiPV_div_k belongs to one temperature -- else CEG_ERR_INVALID.  Without a table params->temperature holds
 *   throughout.
 * Adaptation, at the end of cycle j of the call with cc = cycle0 + j (the reference's counter_cycle), from the CUMULATIVE counters =
 *   prior + this call's stats as they stand then.  A blocked or pocket-blocked trial counts as a trial of its kind; translation and
 *   rotation are kinds 0 and 1 only (the random_* kinds do not count, as in MoveStatistics).  All in FP64, without contraction, IEEE
 *   division and square root, in this order, with clamp(x, lo, hi) = x > hi ? hi : (x < lo ? lo : x):
 *     translation (CEG_MC_ADAPT_DMAX, only if translation_trials > 0):
 *       r = (double)accepted / (double)trials;  q = 10.0 / (double)(99 + cc);  s = sqrt(q);
 *       f = (r - 0.25) * s;  g = 1.0 + f;  dmax = clamp(dmax * g, 0.1, 3.0)
 *     rotation (CEG_MC_ADAPT_THETAMAX, only if rotation_trials > 0), in radians as this ABI holds thetamax:
 *       r = (double)accepted / (double)trials;  a = (r - 0.5) / (double)cc;  b = a * 2.0943951023931953;      (120 degrees)
 *       thetamax = clamp(thetamax + b, 0.17453292519943295, 3.141592653589793)                               (10 and 180 degrees)
 *   With zero trials of a kind (the reference's NaN ratio), with the bit clear, or for a chain that holds no molecule at the cycle
 *   end, the value is carried over unchanged.  This is a restatement in radians: the reference works in degrees, so the result is
 *   NOT bit-equal to the reference's degree arithmetic (it agrees to rounding).
 * cycles: ncycles >= 0, steps_per_cycle >= 1, cycle0 >= 1 (the counter_cycle of the first cycle of THIS call), adapt (CEG_MC_ADAPT_*
 *   bits), temperatures ([ncycles][K] or NULL), prior ([K][4]: translation trials, accepted, rotation trials, accepted BEFORE this
 *   call; NULL: zeros).
 * cycles_out [ncycles][K]: per (cycle, chain) the temperature, dmax and thetamax in force during the cycle, the two step sizes after
 *   the adaptation at its end, the call's stats sums as they stand at the end of the cycle (plain sweep: its delta and 0), the four
 *   cumulative counters (prior + this call) and the chain's molecule count.  log_out [ncycles * steps_per_cycle][K] or NULL.
 * Refusals, all CEG_ERR_INVALID before anything is launched or changed: a NULL `cycles`; ncycles < 0, steps_per_cycle < 1 or
 *   cycle0 < 1; unknown adapt bits; a table entry that is not finite and > 0 (or a varying column where GCMC forbids it); a prior
 *   entry < 0 or accepted > trials; cycles_out NULL with ncycles > 0; ncycles * steps_per_cycle, or first_step plus it, beyond
 *   2^63 - 1; 99 + cycle0 + ncycles not representable; more than CEG_MC_CYCLES_MAX_RECORDS records (ncycles * K) in one call.
 *   Everything the underlying sweep refuses is refused likewise.  ncycles == 0: zero stats, nothing launched.
 * Continuation: a run split over several calls gives the bytes of the one-call run if each call passes first_step advanced, cycle0
 *   advanced, prior = the summed counters (the last record's) and dmax / thetamax = the last record's dmax_next / thetamax_next.
 * Synchronous.  Not covered: one steps_per_cycle applies to the whole group (chains whose reference cycle lengths differ belong in
 *   different groups; chains whose run LENGTHS differ stop at their own last step with ceg_mc_group_set_chain_plan, below); the baseline_energy at cycle 0 inside the run (a caller
 *   composes it from two calls around ceg_mc_group_baseline).  The positions every `printevery` cycles and the minimum-energy
 *   configuration: ceg_mc_group_set_recorder, below. */
#define CEG_MC_ADAPT_DMAX     1
#define CEG_MC_ADAPT_THETAMAX 2
#define CEG_MC_CYCLES_MAX_RECORDS 16777216
typedef struct ceg_mc_cycles {          /* 48 bytes */
    int64_t ncycles;                    /* >= 0 */
    int64_t steps_per_cycle;            /* >= 1; the call runs ncycles * steps_per_cycle steps from params->first_step */
    int64_t cycle0;                     /* >= 1: the reference's counter_cycle of the first cycle of THIS call */
    int32_t adapt, _pad;                /* CEG_MC_ADAPT_* bits */
    const double*  temperatures;        /* [ncycles][K] K, or NULL: params->temperature throughout */
    const int64_t* prior;               /* [K][4] translation trials, accepted, rotation trials, accepted BEFORE this call; NULL: zeros */
} ceg_mc_cycles_t;
typedef struct ceg_mc_cycle_record {    /* 96 bytes */
    double  temperature, dmax, thetamax;        /* in force during the cycle */
    double  dmax_next, thetamax_next;           /* after the adaptation at its end */
    double  delta_moves, delta_swaps;           /* the call's stats sums as they stand at the end of the cycle (plain sweep: delta, 0) */
    int64_t translation_trials, translation_accepted, rotation_trials, rotation_accepted;  /* prior + this call, at the end of the cycle */
    int32_t nmol, _pad;
} ceg_mc_cycle_record_t;
CEG_API int ceg_mc_group_sweep_cycles(ceg_mc_group_t* group, const ceg_mc_sweep_params_t* params, const ceg_mc_cycles_t* cycles,
                                      ceg_mc_sweep_stats_t* stats_out, ceg_mc_cycle_record_t* cycles_out /*[ncycles][K]*/,
                                      ceg_mc_sweep_record_t* log_out /*[ncycles * steps_per_cycle][K] or NULL*/);
CEG_API int ceg_mc_group_sweep_gcmc_cycles(ceg_mc_group_t* group, const ceg_mc_gcmc_params_t* params, const ceg_mc_cycles_t* cycles,
                                           ceg_mc_gcmc_stats_t* stats_out, ceg_mc_cycle_record_t* cycles_out,
                                           ceg_mc_gcmc_record_t* log_out);

/* ---- chain plan: a fugacity term and a last step per chain (make_isotherm, src/parameterinputs.jl:305-334) ----
 * An isotherm is one run_gcmc per pressure.  The pressure of a chain enters its run in one number, phiPV_div_k of
 * compute_accept_move_swap (src/gcmc.jl:77-88, built at src/simulation.jl:701-715), and in its run length, ncycles =
 * ceil(simu.ncycles (1 + 1e3 / P)) (parameterinputs.jl:319).  The plan gives a group both per chain, so that one lockstep call runs
 * the chains of an isotherm: it is as long as the longest chain, and the others stop at their own last step and stay stopped.
 *
 * set_chain_plan copies both arrays (host memory) to the group's device memory and synchronises the group.  The plan stays installed
 *   until it is replaced, removed with NULL, or the group is destroyed.
 * phiPV_div_k [K][nspecies] K, or NULL: entry [c][i] replaces species[i].phiPV_div_k for chain c in both swap rules of
 *   ceg_mc_group_sweep_gcmc and ceg_mc_group_sweep_gcmc_cycles (the table's own value is then neither read nor checked).  Nothing else
 *   changes: the FP64 expressions and their order are the ones documented for ceg_mc_group_sweep_gcmc ("Rule").  Entries of species
 *   with no swap probability are not read.  The plain sweeps ignore the array.
 * stop_step [K] absolute steps, or NULL: chain c takes no part in the absolute steps s >= stop_step[c] of any of the four sweep entry
 *   points.  For such a step no row is evaluated (the chain is in no trial launch: the grid shrinks), nothing of the chain's state
 *   changes, and its statistics, spent / blocked / capacity and pocket counters count nothing.  Its log record is zero bytes except
 *   molecule = -2 (ceg_mc_group_trial's "idle in this step"), kind = -1 and, in the GCMC record, species = -1.
 *   Sampler: a frame taken after such a step does not bin the chain (a pooled map would otherwise count the frozen chain again and
 *     again); the chain's series record of the frame is still written, from its frozen state, so series_out stays [frames][K].
 *   Cycle end: the record of a cycle whose last step is >= stop_step[c] is still written, with the counters as they stand; dmax and
 *     thetamax are carried over without adaptation, as for a chain with no molecules.
 *   stop_step[c] <= first_step is legal: the chain sits the whole call out.  The random stream is keyed by the absolute step, so a
 *   stopped chain can be continued later from first_step = stop_step[c], and the continuation gives the bytes of the uninterrupted run.
 * Refusals, all CEG_ERR_INVALID before anything is launched or changed, the earlier plan staying installed: set_chain_plan with
 *   nspecies outside [0, CEG_MC_GCMC_MAX_SPECIES], phiPV_div_k given with nspecies < 1, or a stop_step < 0; a GCMC sweep with a plan
 *   whose phiPV_div_k has an nspecies other than params->nspecies, or with an entry that is not finite and > 0 for a species whose swap
 *   probability is > 0.
 * With no plan installed, or a plan whose two pointers are NULL, every sweep enqueues the launches and produces the bytes (log,
 *   statistics, records, maps, states) it produces without this section.
 * Not covered: the fugacity coefficient (phi comes from the caller, as the reference takes it from Clapeyron); one steps_per_cycle
 *   applies to the whole group.  (Chains that keep their guests in neighbour cells take part with ceg_mc_group_set_device_cells, below.) */
typedef struct ceg_mc_chain_plan {      /* 24 bytes */
    int32_t nspecies, _pad;
    const double*  phiPV_div_k;         /* [K][nspecies] in K, or NULL: every chain uses the species table's value */
    const int64_t* stop_step;           /* [K] absolute steps, or NULL: no chain ever stops */
} ceg_mc_chain_plan_t;
CEG_API int ceg_mc_group_set_chain_plan(ceg_mc_group_t* group, const ceg_mc_chain_plan_t* plan);   /* NULL removes it */

/* ---- device cells: the sweeps on chains that keep their guests in neighbour cells ----
 * A handle whose MC cell is several cut-offs wide keeps its guest atoms in neighbour cells (ceg_mc_neighbour_cells), and the host
 * holds which atom slot sits at which entry of which cell.  The sweeps refuse such a chain (CEG_ERR_UNSUPPORTED) unless device cells
 * are switched on for the group; then all four sweep entry points take it: its trial rows walk the cells (the body of ceg_mc_trial /
 * ceg_mc_trial_insert with cells), and the cell operations of an accepted step are worked out in the accept launch on a device copy
 * of the lists (cell and entry per atom slot, atom slot per entry), exactly as ceg_mc_accept / ceg_mc_insert / ceg_mc_remove work
 * them out on the host: a displacement, atom by atom in order, refreshes where the bin is unchanged, else takes out (the last entry
 * into the hole) and puts in (append); an insertion puts the atoms of the new slot run in, in order; a deletion takes the molecule's
 * atoms out in order and then refreshes the atoms of the last molecule where that one takes over the index.
 * The copy is uploaded before a sweep where the host's lists have changed, and the host's lists are rebuilt from it after a sweep
 * that accepted a move (both cost time per call, not per step: prefer long calls), so every
 * host-driven call works on the chain afterwards as on any other.  Log, statistics and states are those of the host-driven route
 * with the same proposals, byte for byte; chains without cells in the same group run the kernels and give the bytes they gave before.
 * A full cell halts the chain: an accepted displacement or insertion that would put an atom into a cell already holding `capacity` entries is
 *   not applied -- nothing of the step is written: atoms, structure factors, cells, lists, statistics -- and from that absolute
 *   step on the chain behaves as if the chain plan had stopped it there (log records with molecule = -2, no sampler bins, cycle
 *   records written with the step sizes carried over; in a GCMC sweep nothing of the molecule table, the counts or the freed slots changes).  The call returns CEG_OK; ceg_mc_group_halted reports the step.  The caller
 *   raises the capacity (set_device_cells with a larger min_capacity) and continues from first_step = that step: proposals and
 *   decisions depend on (seed, absolute step, stream id) only and a larger capacity changes no order of entries, so the result is
 *   that of a run that had the capacity from the start.  Continuing in the middle of a cycle of the *_cycles entry points is not
 *   covered.
 * Every index read from the device's lists is range-checked before it is used; a failed check halts the chain in the same way and
 *   the call returns CEG_ERR_HIP with the chain marked inconsistent.
 * Not covered: growing the capacity inside a call; continuing a halted chain in the middle of a cycle. */
/* on != 0: the sweeps of this group take chains that keep their guests in neighbour cells; their cell lists are kept on the
   device during a sweep.  min_capacity > 0: their cells are rebuilt with at least that many entries per cell (never fewer
   than rebuild_cells would choose).  on == 0: as before (such chains are refused).  Synchronises the group's stream. */
CEG_API int ceg_mc_group_set_device_cells(ceg_mc_group_t* group, int32_t on, int32_t min_capacity);
/* per chain the absolute step at which the last sweep call halted it on a full cell, -1 if it did not */
CEG_API int ceg_mc_group_halted(ceg_mc_group_t* group, int64_t* halted_step_out /* [K] */);
/* the host's cell lists of a handle: cell and entry of every atom slot (-1: in no cell); returns 0 without neighbour cells */
CEG_API int ceg_mc_cell_lists(ceg_mc_t* handle, int32_t* cell_of, int32_t* idx_of, int64_t nslots);

/* ---- tempering: replica exchange between the chains of a group at cycle ends (run_parallel_tempering, src/simulation.jl:461-622) ----
 * K chains of one group on a ladder of temperatures exchange with their neighbours on the ladder at the end of a cycle, inside
 * ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles, with no host round trip.  What is exchanged is the TEMPERATURE, not the
 * configuration: a chain keeps its state, random stream, step sizes, statistics and log; what moves is the RUNG of the ladder it
 * sits on.  The rule is the reference's (:533): compute_accept_move(E_i, E_{i+1}, inv(inv(T_i) - inv(T_{i+1}))).
 * One more launch per cycle (k_mcg_exchange, one workgroup, one lane per chain) follows k_mcg_cycle_end on the group's stream; plain
 * loads and stores, stream order is the only synchronisation.  The two plain sweeps (ceg_mc_group_sweep / _sweep_gcmc) ignore an
 * installed tempering state.
 *
 * set_tempering copies `rung` and `energy` (host memory) to the group's device memory and synchronises the group; NULL removes the
 *   state.  every >= 1; record_capacity >= 0 cycles of records kept; rung [K] a permutation of 0..K-1 (NULL: chain c on rung c);
 *   energy [K] the total energy of every chain NOW (e.g. ceg_mc_group_baseline's total), finite.
 * While installed, for both *_cycles entry points:
 *   Temperatures by rung: every temperature the caller passes is indexed by rung -- params->temperature[r] and column r of
 *     cycles->temperatures -- and the chain on rung r runs at it.  Every row must be non-decreasing in r.
 *   Energy at the end of cycle j of a call: energy at the call's start + the call's delta_moves as it stands then, and in the GCMC
 *     entry point (that + delta_moves) + delta_swaps; FP64, in this order, no contraction.  After the last cycle of a call it becomes
 *     the next call's start value.  The rungs likewise persist on the device; the host's copy is refreshed at the end of each call.
 *   Round: with cc = cycle0 + j, an exchange round happens iff cc % every == 0; parity = (cc / every) & 1; the rung pairs are
 *     (r, r + 1) for r = parity, parity + 2, ... with r + 1 < K.  A pair is attempted only if neither chain is stopped at the cycle's
 *     last step (last_step >= its stop: the chain plan's, or the step at which a full cell halted it); else both get partner = -1,
 *     accepted = -1.
 *   Rule: a the chain on the lower rung, b on the upper, T_a and T_b the temperatures in force during the ended cycle (the cycle
 *     record's).  In FP64, without contraction, IEEE division:
 *       ia = 1 / T_a;  ib = 1 / T_b;  d = ia - ib;  Tp = 1 / d;  x = (E_a - E_b) / Tp;  e = exp(x);   accept iff E_b < E_a || u < e
 *     Equal temperatures give Tp = +inf, e = 1 and an accepted exchange; NaN energies reject.  exp is the device library's.
 *   Draw: u = U(w0, w1) of the Philox block (seed of the call, absolute last step of the cycle, stream id of chain a, purpose 9).
 *   After the round -- at EVERY cycle end, round or not -- chain c's temperature for the next cycle is row_{j+1}[rung_next[c]]: the
 *     table's next row, or params->temperature where there is no table; after the call's last cycle the ended cycle's row.  One
 *     ceg_mc_exchange_record_t is written per (cycle, chain).
 *   Sampler: a density map's chain_map is indexed by rung (chain c is binned into chain_map[rung[c]], the rung it held during the
 *     frame's cycle), so maps belong to temperatures; the series records stay per chain.  A frame of ceg_mc_group_sample is binned
 *     by the rungs as they stand on the device then.
 * tempering_read synchronises the group and copies what is asked for (each pointer may be NULL): the rung and the energy of every
 *   chain, attempted and accepted exchanges of the rung pair (r, r + 1) in row r (row K - 1 is zeros), the records of all cycles since
 *   set_tempering and their number.
 * Refusals, all CEG_ERR_INVALID before anything is launched or changed, the earlier state staying: set_tempering with every < 1, a
 *   negative (or absurd, > 2^32) record_capacity, a rung that is no permutation, a missing or non-finite energy; a *_cycles call whose
 *   ncycles exceeds what is left of record_capacity, with a row that decreases, or -- ceg_mc_group_sweep_gcmc_cycles -- with any
 *   species whose swap probability is > 0 (phiPV_div_k belongs to one temperature).
 * A sweep that fails (CEG_ERR_HIP) once its steps have been enqueued takes none of its records and marks the tempering state stale:
 *   the next *_cycles call is refused (CEG_ERR_INVALID) until set_tempering is called again.  A failure before that (the device
 *   cannot be selected, an allocation or the copy of the call's block fails) has launched and changed nothing: the state stays.
 * Continuation: a run split over several calls (first_step, cycle0, prior and the step sizes advanced as for the cycles above; with
 *   a table each call gets its own rows) gives the one-call run's logs, states, rungs, partners, draws, decisions and pair counts.
 *   Two entries cannot be equal in their bytes, by the definitions above.  Energy: a later call starts from the ROUNDED sum of the
 *   earlier one and its delta_moves starts at zero, so the same terms are added in another association; energies, and the
 *   thresholds computed from them, agree to rounding (one rounding of at most half an ulp of the largest partial sum per step; a
 *   decision could differ only where u lies that close to the threshold).  temperature_next of a call's last cycle: the call cannot
 *   see the row that follows, so it is the ENDED cycle's row at the chain's next rung; the next call starts every chain at its rung's
 *   entry of its own first row, so the temperatures the chains run at are the one-call run's.
 * Not enforced: any other call that moves a chain (the plain sweeps, accept, insert, remove, set_guests) makes the stored energies
 *   stale; the caller installs the state again.
 * With no tempering installed every entry point enqueues exactly the launches and produces the bytes it produces without this section.
 * Not covered: step sizes and the cumulative counters stay with the chain, not the rung; exchanges under GCMC swaps; any pair
 *   schedule other than the alternating one; exchanging configurations; SiteHopping. */
typedef struct ceg_mc_tempering {       /* 32 bytes */
    int64_t every;                      /* >= 1: a round at the end of every cycle cc with cc % every == 0 */
    int64_t record_capacity;            /* >= 0: cycles of records kept */
    const int32_t* rung;                /* [K] a permutation of 0..K-1, or NULL: chain c on rung c */
    const double*  energy;              /* [K] K: the total energy of every chain now, finite */
} ceg_mc_tempering_t;
typedef struct ceg_mc_exchange_record { /* 48 bytes */
    int32_t rung, rung_next;            /* during the ended cycle, during the next */
    int32_t partner;                    /* the other chain of the pair, -1: none */
    int32_t accepted;                   /* 1, 0, or -1: no attempt */
    double  energy;                     /* of the chain at the end of the cycle */
    double  temperature_next;           /* the chain's temperature during the next cycle */
    double  u, threshold;               /* the draw and e of the rule (0 without an attempt) */
} ceg_mc_exchange_record_t;
CEG_API int ceg_mc_group_set_tempering(ceg_mc_group_t* group, const ceg_mc_tempering_t* tempering);   /* NULL removes it */
CEG_API int ceg_mc_group_tempering_read(ceg_mc_group_t* group, int32_t* rung_out /*[K]*/, double* energy_out /*[K]*/,
                                        int64_t* pair_counts_out /*[K][2]*/, ceg_mc_exchange_record_t* records_out /*[cycles][K]*/,
                                        int64_t* cycles_out);

/* ---- recorder: position snapshots and a minimum-energy record at cycle ends (src/simulation.jl:784-799, parameterinputs.jl:86-108) ----
 * The trajectory of run_montecarlo! (put!(output, o) every `printevery` cycles) and RMinimumEnergy (the lowest-energy configuration
 * seen at any cycle end) for the K chains of a group, taken inside ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles with no
 * host round trip: while a recorder is installed those two calls enqueue one more launch (k_mcg_snapshot, one workgroup per chain) at
 * the cycle ends where the recorder wants one, behind k_mcg_cycle_end and, with tempering, behind k_mcg_exchange.  The launch reads
 * chain state and writes only memory the recorder owns; everything is read once, after the run.  Plain loads and stores; stream
 * order is the only synchronisation; the bytes do not depend on the order in which workgroups or lanes arrive.
 *
 * set_recorder copies `energy` (host memory), allocates the store (frame_capacity frames, zeroed) and synchronises the group; NULL
 *   removes the recorder.  With track_min it also copies every chain's state NOW into the chain's best slot, with the given energy
 *   and mink = -1 (one launch), so it needs every member consistent.
 * Frame: at the end of cycle cc = cycle0 + j of a *_cycles call iff every > 0 && cc >= origin && (cc - origin) % every == 0.  With
 *   cycle0 counted as run_montecarlo does (1 + the cycles run so far), origin = ninit gives the reference's idx_cycle % printevery == 0.
 * Body of a frame, per (frame, chain), in four arrays [frame][chain][...]:
 *   double  xyz[max_atoms][3], int32 kind[max_atoms]   in MOLECULE order: the atoms of molecule 0, then 1, ..., each molecule's atoms
 *                                                      in slot order -- the bytes and the order of ceg_mc_get_state;
 *   int32   mol_first[max_molecules + 1]               first atom of every molecule and the atom count, as ceg_mc_set_guests takes it;
 *   int32   species[max_molecules]                     ceg_mc_group_sweep_gcmc_cycles: the species of molecule j from the device's own
 *                                                      table; -1 in the plain entry point, in ceg_mc_group_snapshot and at installation.
 *   Entries beyond the counts are zero.  During a GCMC call nmol, the high-water mark of the atom slots and the species come from the
 *   device's molecule table (the views' counts are stale there).
 * Record: one ceg_mc_snapshot_record_t per (frame, chain).  A chain whose nmol > max_molecules or natoms > max_atoms, or whose
 *   molecule table fails a range check (a molecule outside [1, 16] atoms or outside the atom slots in use), gets flags |= 1, the counts
 *   as they are in the chain (natoms: the sum of the molecules' counts) and NO body (zeros); that is not an error.  flags |= 2: the
 *   chain was stopped (chain plan) or halted (full cell) at `step`: the frame repeats the frozen state.
 * Energy at the end of cycle j of a call: energy at the call's start + the call's delta_moves as it stands then, and in the GCMC
 *   entry point (that + delta_moves) + delta_swaps; FP64, in this order, no contraction (the definition tempering uses; the recorder
 *   keeps its own copy).  After a call that ended well the value after its last cycle is the next call's start value.  Under swaps
 *   delta_swaps is compute_accept_move_swap's `diff`, not the state's energy change, so `energy` is that bookkeeping value.
 * Minimum (track_min != 0): the launch runs at EVERY cycle end and implements `if Float64(e) < Float64(record.mine)` per chain:
 *   strict, so ties keep the earlier cycle, and a NaN never wins.  The chain's record and body go to the chain's best slot (its tail
 *   zeroed; a chain that does not fit: flags 1 and a zeroed body), mine = e, mink = cc.  A chain stopped or halted at the cycle's
 *   last step is not tested.  Neither ceg_mc_group_snapshot nor recorder_rebase tests or resets the minimum.
 * snapshot: one frame of the resident state now (cycle = step = -1, energy = the recorder's running energy), asynchronous on the
 *   group's stream like ceg_mc_group_sample.
 * recorder_rebase replaces the running energies ([K], host memory, finite): the precise energy at idx_cycle == 0
 *   (simulation.jl:788-790).  Synchronises the group.
 * recorder_read synchronises and copies frames [first_frame, first_frame + nframes) of what is asked for (every pointer may be
 *   NULL): records [nframes][K], xyz [nframes][K][max_atoms][3], kind [nframes][K][max_atoms], mol_first
 *   [nframes][K][max_molecules + 1], species [nframes][K][max_molecules]; *frames_out = the frames taken so far.
 * recorder_min synchronises and copies per chain mink, mine, the best record and body ([K][...] as above), every pointer optional.
 * Refusals, all before anything is launched or changed, the earlier recorder staying installed: CEG_ERR_INVALID for every < 0,
 *   origin < 0, frame_capacity < 0, max_atoms < 1, max_molecules < 1, a missing or non-finite energy, a store (frame_capacity + 1
 *   best slot) * K * bytes per chain above CEG_MC_RECORDER_MAX_BYTES; a *_cycles call whose due frames exceed the room left, or on a
 *   stale recorder; ceg_mc_group_sweep_gcmc_cycles with track_min and any species whose swap probability is > 0; snapshot on a full
 *   store, a stale recorder or without one; a read window outside the frames taken; recorder_min without track_min or on a stale
 *   recorder.  CEG_ERR_HIP, with the chain's index in ceg_last_error(), for snapshot, or set_recorder with track_min, on a group
 *   with an inconsistent member.
 * A sweep that fails (CEG_ERR_HIP) once its steps have been enqueued takes none of its frames (they are zeroed again) and marks the
 *   recorder stale until set_recorder is called again; the frames taken before stay readable, the minimum does not (the failed
 *   call's launches may have written it).
 * With no recorder installed every entry point enqueues exactly the launches and produces the bytes it produces without this
 *   section; with one installed, no frame due and no track_min, no launch is added; logs, statistics, records and final states are
 *   the same bytes with and without it.  The two plain sweeps (ceg_mc_group_sweep / _sweep_gcmc) ignore the recorder, and like any
 *   other call that moves a chain they make its running energies stale: rebase.
 * Out of scope: the PDB / stream / zst / restart file formats of output.jl; restoring a frame on the device (the host route through
 *   ceg_mc_set_guests is the one provided); a minimum per rung; ShootingStarMinimizer's spawned quenches (a caller composes them
 *   from TRamp / TAnneal temperature tables, this minimum and ceg_mc_set_guests). */
#define CEG_MC_RECORDER_MAX_BYTES ((int64_t)8 << 30)
typedef struct ceg_mc_recorder {        /* 48 bytes */
    int64_t every;                      /* >= 0; 0: no periodic frames */
    int64_t origin;                     /* >= 0 */
    int64_t frame_capacity;             /* >= 0 frames kept */
    int32_t max_atoms, max_molecules;   /* per chain and frame, >= 1 */
    int32_t track_min, _pad;            /* != 0: RMinimumEnergy per chain */
    const double* energy;               /* [K] K: the total energy of every chain now, finite */
} ceg_mc_recorder_t;
typedef struct ceg_mc_snapshot_record { /* 40 bytes */
    int64_t cycle, step;                /* cc and the absolute last step of the cycle; -1, -1: snapshot, or the state at installation */
    double  energy;
    int32_t nmol, natoms;               /* as they are in the chain, also when they do not fit */
    int32_t flags, _pad;                /* 1: does not fit, no body; 2: the chain was stopped or halted at `step` */
} ceg_mc_snapshot_record_t;
CEG_API int ceg_mc_group_set_recorder(ceg_mc_group_t* group, const ceg_mc_recorder_t* recorder);   /* NULL removes it */
CEG_API int ceg_mc_group_snapshot(ceg_mc_group_t* group);
CEG_API int ceg_mc_group_recorder_rebase(ceg_mc_group_t* group, const double* energy /*[K]*/);
CEG_API int ceg_mc_group_recorder_read(ceg_mc_group_t* group, int64_t first_frame, int64_t nframes, ceg_mc_snapshot_record_t* records_out,
                                       double* xyz_out, int32_t* kind_out, int32_t* mol_first_out, int32_t* species_out, int64_t* frames_out);
CEG_API int ceg_mc_group_recorder_min(ceg_mc_group_t* group, int64_t* mink_out /*[K]*/, double* mine_out /*[K]*/,
                                      ceg_mc_snapshot_record_t* record_out /*[K]*/, double* xyz_out, int32_t* kind_out, int32_t* mol_first_out,
                                      int32_t* species_out);

/* ---- baseline_energy (src/montecarlo.jl:530-542) of one chain, or of every chain of a group, from the resident state ----
 * What run_montecarlo! asks for at its start, at the first production cycle, after a move that risks underflow and for its final
 * drift check (src/simulation.jl:643,789,850-853; montecarlo.jl:364).  Synchronous; `out` is host memory ([K] for a group, member
 * order).  The work is ordered on the handle's (the group's) stream behind everything enqueued so far, and takes a fixed number of
 * launches -- two, four with CEG_MC_BASELINE_REFRESH -- whatever the number of chains and molecules.
 *  framework_vdw, framework_direct  sum of framework_interactions over every atom of every molecule in the system, atom by atom as
 *                    row 0 of ceg_mc_trial computes it; the 1e100 rules are the same (a blocked VdW value is kept and summed, a
 *                    Coulomb value of exactly 1e100 is added without the charge); a NULL grid gives 0.
 *  inter             compute_vdw (src/energy.jl:355-383): every unordered pair of atoms of DIFFERENT molecules with d^2 < cutoff^2,
 *                    once, with the pair distance (fast wrap where the cell allows it, the reference's order otherwise), cutoff test
 *                    and rule energies of the trial rows: 1/2 the sum of column 2 of row 0 over the molecules.  Free atom slots are
 *                    skipped.  A handle that keeps neighbour cells is accepted: the atom records are authoritative, and the loop over
 *                    them is exhaustive.
 *  recip_framework   sum_k kf Re(conj(S_fw) S),  recip_guests  sum_k kf |S|^2,  S = sums[:, 1] as resident.  The caller composes
 *                    2 (recip_framework + energy_net_charges) + recip_guests + static_contribution (src/ewald.jl:555-577): the two
 *                    constants depend on the species counts and stay on the host, like the tail correction.  nk = 0: both 0.
 *  nmol, natoms      the molecules and the occupied atom slots that were summed.
 * CEG_MC_BASELINE_REFRESH: before the sums, every sums[:, ij+1] and sums[:, 1] is recomputed from the current positions and stored,
 *   as compute_ewald(::IncrementalEwaldContext) (src/ewald.jl:630-652) does inside the reference's baseline_energy -- the rounding
 *   accumulated by the incremental updates is gone afterwards.  Without the flag nothing in the state is written.
 * Determinism: no floating-point atomics; partial sums are combined in an order fixed by the chain's own atom-slot layout.  Repeated
 *   calls on an unchanged state return identical bytes, and ceg_mc_group_baseline returns for member c exactly the bytes
 *   ceg_mc_baseline returns for that handle alone.  An empty box gives zeros.
 * Errors: NULL handle / group / out or unknown flag bits -> CEG_ERR_INVALID before anything is launched; a handle (member) marked
 *   inconsistent -> CEG_ERR_HIP (with the chain's index in ceg_last_error() for a group) and no member's state is touched; a failure
 *   after a refresh has been launched marks the handle (every member) inconsistent. */
typedef struct ceg_mc_baseline {
    double framework_vdw, framework_direct, inter;   /* K */
    double recip_framework, recip_guests;            /* K */
    int32_t nmol, natoms;
} ceg_mc_baseline_t;
#define CEG_MC_BASELINE_REFRESH 1
CEG_API int ceg_mc_baseline(ceg_mc_t* handle, int32_t flags, ceg_mc_baseline_t* out);
CEG_API int ceg_mc_group_baseline(ceg_mc_group_t* group, int32_t flags, ceg_mc_baseline_t* out /* [K] */);

/* ---- site hopping: whole Monte-Carlo runs of K chains on two tables (src/sitehopping.jl, src/simulation.jl:863-1010) ----
 * The reference's second Monte-Carlo model: a mobile species hops between n sites; all physics sits in frameworkenergies[n] and
 * interactions[n][n] (K; symmetric, the diagonal 1e100).  A group holds one copy of the tables and K chains of m molecules each
 * (population[c][j]: the 0-based site of molecule j of chain c), all resident on one device.  ceg_site_group_sweep_cycles runs the main
 * loop of run_montecarlo!(::SiteHopping) with groupcycles = nothing for every chain: one wave per chain, all steps of all cycles inside
 * the kernel (k_site_sweep), no launch per step.  A group knows no ceg_mc_t and no ceg_mc_group_t; only the table build, at the end of
 * this section, reads one.
 *
 * The step of chain c at the absolute step s (stream = stream_id[c]; Philox and U as for ceg_mc_group_sweep, above):
 *  draws     purpose 10 (SITE_SELECT): molecule i = min(floor(U(w0, w1) m), m - 1), site new = min(floor(U(w2, w3) n), n - 1);
 *            purpose 3: u = U(w0, w1).  old = population[i].
 *  energies  before = framework[old] + R(old), after = framework[new] + R(new) (movement_energy, sitehopping.jl:114-121), with the
 *            row sum R(r) = sum over j != i of interactions[r][population[j]] in this order, a fixed function of m alone: lane
 *            l = 0..63 adds its terms j = l, l + 64, l + 128, ... (< m) in rising order onto +0.0, with +0.0 in the place of the term
 *            j == i (the same bits as leaving it out: such a sum is never -0.0); then for o = 32, 16, 8, 4, 2, 1 every lane replaces
 *            its sum by (its sum) + (the sum of lane l ^ o); R is what lane 0 then holds.  Plain FP64 adds, nothing contracted.
 *            before is recomputed at every step, which equals the reference's old_i cache: the population changes only at i itself.
 *  rule      compute_accept_move (montecarlo.jl:702-712): accepted iff after < before, or else u < exp((before - after) / T) with the
 *            device library's FP64 exp and an IEEE division.  A hop onto an occupied site meets the 1e100 of that pair and is rejected
 *            by the rule itself; a hop onto the molecule's own site has after == before, bit for bit, and is accepted as a no-op.
 *            Neither has a special case.
 *  accepted  energy = energy + (after - before), delta = delta + (after - before), population[i] = new.
 * Per chain the group keeps, in device memory between launches and calls: the population, the running energy, and since creation
 * the steps attempted, the steps accepted and `delta`, the sum of the accepted changes (ceg_site_stats_t).
 *
 * create: n in 1..65535 (sites are UInt16 in the reference), m in 1..CEG_SITE_MAX_MOLECULES, K >= 1, every site < n, no site twice
 *   within a chain (the reference's randperm never produces it, and two 1e100 terms would poison the sums), finite tailcorrection;
 *   else CEG_ERR_INVALID.  n*n*8 bytes above CEG_HIP_SITE_TABLE_LIMIT_MB MiB (environment, default 2048) -> CEG_ERR_UNSUPPORTED.
 *   tables_on_device == 0: framework [n] and interactions [n][n] are host memory and are copied once; != 0: they are device memory
 *   of `device`, which the group reads in place and never writes or frees: the caller keeps them alive until destroy.  The running
 *   energy starts as the baseline (below).  Synchronous.
 * sweep_cycles: cycles cc = cycle0 + 0 .. cycle0 + ncycles - 1 of steps_per_cycle steps each (the reference: m), the absolute steps
 *   first_step, first_step + 1, ...; temperature [ncycles][K], stream_id [K] (NULL: the chain's index), all host memory.  At the end of
 *   every cycle the chain's record goes to cycles_out [ncycles][K]; with log_out != NULL every step's record goes to
 *   log_out [ncycles * steps_per_cycle][K]; stats_out [K] receives the state after the call.  Every output may be NULL.  Synchronous.
 *   The call is cut into launches of at most CEG_HIP_SITE_STEPS_PER_LAUNCH steps per chain (environment, 1..2^30, default 4096:
 *   6 ms per launch at m = 64 and 0.11 s at m = 4096, n = 8192, K = 256, the largest shape measured), which follow each other on the
 *   group's stream with the state in device memory between them.  A run does not depend on how it is cut, by that limit or by the caller into several calls that continue
 *   first_step and cycle0: outputs and state are the same bytes.
 *   CEG_ERR_INVALID before anything is launched or changed: a missing group / params / cycles / temperature, ncycles < 0,
 *   steps_per_cycle < 1, a temperature that is not finite and > 0, cycle0 + ncycles or first_step + the steps beyond 2^63 - 1,
 *   more than CEG_MC_CYCLES_MAX_RECORDS log or cycle records.  ncycles == 0: stats only.
 * baseline: baseline_energy (sitehopping.jl:105-112) of every chain in one launch, out [K] host memory:
 *   (tailcorrection + sum_j framework[population[j]]) + sum_{i<j} interactions[population[i]][population[j]], partial sums combined in
 *   a fixed order.  rebase: sets every chain's running energy to exactly those bytes (the reference's idx_cycle == 0 step; the caller
 *   compares energy and baseline for the final drift check); the counters and delta stay.
 * set_populations: validated as at creation, replaces every chain's population and rebases.  get_populations: [K][m].
 * recorder (run_montecarlo!'s frames every printevery cycles, and RMinimumEnergy for SiteHopping, parameterinputs.jl:109), written by
 *   the chain's own wave inside k_site_sweep, no extra launch: at the end of cycle cc with every > 0, cc >= origin and
 *   (cc - origin) % every == 0 the chain's population and energy go into the next frame of the store ([frame_capacity][K]); once the
 *   store is full the frame is dropped and the chain's cycle record carries CEG_SITE_FRAME_DROPPED.  With track_min, the population
 *   of the lowest cycle-end energy so far is kept per chain, strict <, so a tie keeps the earlier cycle; installation takes the
 *   state and energy at that moment as the minimum to beat (mink = -1).  set_recorder(NULL) removes it; installing synchronises.
 *   recorder_read copies frames [first_frame, first_frame + nframes) (records [nframes][K], populations [nframes][K][m]; every
 *   pointer optional; *frames_out: the frames held); recorder_min copies mink, mine and the populations [K][m].  CEG_ERR_INVALID:
 *   every, origin or frame_capacity < 0, a store above CEG_MC_RECORDER_MAX_BYTES, a window outside the frames held, no recorder, no
 *   track_min.
 * A HIP failure once a launch has been enqueued marks the group inconsistent: every later call but destroy returns CEG_ERR_HIP.
 * tempering (run_parallel_tempering, src/simulation.jl:461-634; ceg_site_group_set_tempering): the exchange of configurations between
 *   neighbouring rungs of a temperature ladder, drawn per step inside the sweep kernel (k_site_sweep_pt: one workgroup per ladder,
 *   one wave per rung, the R populations in LDS, one workgroup barrier per step).
 *   Layout.  A group of K chains with tempering installed is L = K / R ladders of R rungs.  Chain l*R + r is rung r of ladder l.
 *     A chain index means a rung from then on.  Temperatures, streams, hop counters, cycle records, frames and the minimum belong to
 *     the rung.  Population, running `energy` and `delta` belong to the configuration and travel with it.  So energy - delta stays
 *     the baseline that the configuration started from.
 *   Temperatures.  The temperature table [ncycles][K] of ceg_site_group_sweep_cycles gives the rung temperatures.  Inside every
 *     ladder and every cycle they must be strictly increasing with the rung, because the reference sorts Ts.  Otherwise the call
 *     returns CEG_ERR_INVALID before anything is launched.
 *   Exchange draw.  At the absolute step s, every ladder takes one Philox block.  The purpose is new: SITE_EXCHANGE = 12.  The
 *     stream is the ladder's (ladder_stream[l], or l when the pointer is NULL).  v = U(w0, w1) chooses the pair.  u = U(w2, w3) is
 *     the acceptance draw.
 *   Pair table.  The pair is the first j in 0..R-2 with v < pair_cdf[j].  If there is none, the step has no exchange.
 *     pair_cdf[R-1] is host memory given by the caller.  Each entry must be finite, in [0, 1] and non-decreasing.  Otherwise the
 *     call returns CEG_ERR_INVALID.  The reference attempts at most the first element of randsubseq(1:(Npt-1), 0.1) (:528-529).
 *     That is pair_cdf[j] = 1 - q_(j+1) with q_0 = 1 and q_(i+1) = q_i * (1 - p), computed by repeated multiplication
 *     (mcrng.site_exchange_cdf).  Taking the table as input, rather than p, keeps a log off the device.  It also lets a caller
 *     or a test reach the upper pairs.
 *   Exchange attempt.  A step whose pair is j attempts the exchange of rungs j and j+1 (:531-543).  E_a and E_b are the running
 *     energies of the two rungs at the start of the step.  Tx = 1.0 / (1.0 / T_j - 1.0 / T_(j+1)), with IEEE divisions in this
 *     order.  The exchange is accepted iff E_b < E_a, or else u < exp((E_a - E_b) / Tx).  This is
 *     compute_accept_move(energypt[ipt], energypt[ipt+1], inv(inv(T) - inv(Ts[ipt+1])), sh).
 *   After the attempt.  pt_attempted[l][j] goes up by 1.  On acceptance pt_accepted[l][j] goes up by 1.  On acceptance the
 *     populations of the two rungs are exchanged, and their `energy` and `delta` with them.  The two rungs make no hop at this
 *     step.  `attempted` does not move.  Rung j logs molecule = -1, old_site = new_site = -1, before = E_a, after = E_b, u,
 *     accepted.  Rung j+1 logs molecule = -2 and the same values.  Every other rung of the ladder makes the ordinary step of
 *     k_site_sweep.  It uses its own stream and the same bits as today.
 *   Cycle ends.  Cycle records, frames and track_min work as today, per rung.  They use the population and energy that sit on
 *     the rung at that moment.  This is what the reference's simu.record(sh, energypt[ipt], ...) sees.
 *   Replica map.  The group also keeps replica[K].  It holds, per rung, the rung (0..R-1) on which the configuration now there
 *     sat when tempering was installed.  It is a permutation inside every ladder.
 *   set_tempering: rungs R in 2..16 with K % R == 0, pair_cdf as above, _reserved == 0, else CEG_ERR_INVALID with the state
 *     untouched; R populations that do not fit the LDS a workgroup may take (hipDeviceAttributeMaxSharedMemoryPerBlock) ->
 *     CEG_ERR_UNSUPPORTED with the figures.  Installing synchronises, zeroes the pair counters and sets replica to the identity;
 *     NULL removes the tempering.  set_populations resets replica as well; rebase leaves it.  While tempering is installed,
 *     sweep_cycles launches k_site_sweep_pt and takes params->stream_id per rung; without it the call is what it was.  A run does
 *     not depend on how it is cut, as above: populations (by rung), energy, delta, replica and the pair counters are in device
 *     memory between launches.  tempering_read copies the pair counters [K/R][R-1] and replica [K] (every pointer optional);
 *     CEG_ERR_INVALID with nothing installed.
 * grouped cycles (run_montecarlo!(::SiteHopping, simu; groupcycles, restartgroupcycle), src/simulation.jl:917-939, 941, 970-982;
 *   ceg_site_group_sweep_grouped): the hops of a cycle are accepted or rejected as ONE move, and with `restart` every cycle first
 *   replaces the population by a fresh randperm start (basin hopping, what run_random_quenching drives).  One kernel,
 *   k_site_sweep_grouped: one wave per chain, the population in LDS, all steps and decisions of all cycles of a launch inside it.
 *   A grouped cycle of chain c runs on stream stream_id[c] at temperature T.  Its absolute steps are s0 .. s0 + spc - 1, where
 *   spc = steps_per_cycle (G*m for the reference's groupcycles = G).  The device needs no G of its own.
 *   1. Save.  (P0, E0, D0) is the population, running `energy` and `delta` at the start of the cycle.
 *   2. Restart (only when asked for).  The population becomes the first m entries of a Fisher-Yates shuffle of 0..n-1.
 *      Entry j = 0..m-1 takes the Philox block of (seed, step s0, stream, counter word 3 = 14 | (j << 8)).  Purpose
 *      SITE_RESTART = 14 is new.  It is keyed the way the retried proposals of ceg_mc_group_sweep_gcmc key their attempts.
 *      r = j + min(floor(U(w0, w1) (n - j)), n - j - 1), and entries j and r are exchanged, for j rising.  This is the arithmetic
 *      of mcrng.site_random_population.  The device never builds the n entries: entry j ends as the value that position r_j held
 *      just before exchange j, which is found by walking down the earlier (q, r_q) pairs (mcrng.site_restart_population).
 *      Then energy = baseline_energy of that population, computed by the chain's own wave in this order, a function of m alone:
 *      F: lane l = 0..63 adds framework[pop[j]] for j = l, l + 64, ... (< m) in rising order onto +0.0.  E: for the rows
 *      i = 0, 1, .., m - 2 in rising order lane l adds interactions[pop[i]][pop[j]] for j = i + 1 + l, i + 1 + l + 64, ... (< m) in
 *      rising order onto ONE accumulator per lane that starts at +0.0 and runs through all rows.  Then F and E each meet by the xor
 *      butterfly of the row sum R (o = 32, 16, 8, 4, 2, 1), and the baseline is (tailcorrection + F) + E (mcrng.site_baseline_wave).
 *      Call this energy Er.  Without a restart, Er = E0.
 *   3. Hops.  spc ordinary steps follow, and they are the step above bit for bit: the draws, row sums, rule and log record of
 *      sweep_cycles.  `energy` moves with every accepted hop.  The group's attempted / accepted counters do not move (:946, :962).
 *      The hops accepted inside the cycle are counted separately.
 *   4. Decision.  Draw the block of (seed, s0 + spc - 1, stream, purpose SITE_GROUP = 13), and take u = U(w0, w1).  With E1 the
 *      energy after the hops, the cycle is accepted iff E1 < E0, or else u < exp((E0 - E1) / T).  This is
 *      compute_accept_move(group_energy, energy, temperature, sh) (:972), with the device library's FP64 exp and an IEEE division.
 *      A NaN E1 is rejected by the rule itself, with no special case.  attempted += 1.
 *      Accepted: accepted += 1 and delta = D0 + (E1 - E0), with or without a restart, so energy - delta stays the baseline the
 *      chain began from.  Rejected: population, `energy` and `delta` become P0, E0, D0 again.
 *   5. Cycle end.  It is as for sweep_cycles, on the state AFTER the decision: frame, strict-< minimum and the cycle record are
 *      unchanged.  `flags` gains CEG_SITE_GROUP_ACCEPTED = 8 and CEG_SITE_GROUP_RESTARTED = 16.
 *   The reference's old_i / before / after cache (:926-927, :975-980) needs no device state: `before` is recomputed at every hop,
 *   and the cache is reset wherever the population changes other than at old_i (restart, rejection).
 *   sweep_grouped is sweep_cycles plus `restart` (0 or 1) and grouped_out [ncycles][K] (optional): per cycle and chain E0, Er, E1,
 *   u, the decision, whether the cycle restarted and the hops accepted inside it.  Nothing is installed in the group, and
 *   sweep_cycles is what it was.  Validation, limits and the synchronous contract are those of sweep_cycles; in addition
 *   CEG_ERR_UNSUPPORTED while tempering is installed (run_parallel_tempering has no group cycles) and CEG_ERR_INVALID for a
 *   `restart` outside {0, 1}; in both cases nothing is launched and nothing changes.  The call is cut into launches as sweep_cycles
 *   is, and a cut may fall inside a cycle: P0, E0, D0, Er and the cycle's hop count live in device memory between launches, so
 *   outputs and state are the same bytes however the call is cut, and however the caller cuts a run into calls of whole cycles.
 *   Between calls nothing is pending.
 * Out of scope: a tempering schedule that attempts more than the first pair of randsubseq;
 *   extremal_placements; ShootingStarMinimizer; the serialised caches and output files.
 *
 * The two tables (the reference's constructor, sitehopping.jl:41-82, telescoped): ceg_site_tables (host arrays out) and
 * ceg_site_tables_device (device arrays of the handle's device out, e.g. for ceg_site_group_create with tables_on_device).
 *  handle     a ceg_mc_t of the mobile species that holds NO guest (as ceg_mc_create leaves it, or after ceg_mc_set_guests with
 *             nmol = 0) and belongs to no chain group; with guests -> CEG_ERR_UNSUPPORTED.  Nothing of the handle is written.
 *  kinds      [m_atoms] the kinds of the species' atoms, m_atoms in 1..16, as for ceg_mc_trial_insert
 *  positions  [n][m_atoms][3] Cartesian A, host memory, finite; n in 1..65535
 *  With {...} a system of exactly those placements and .er its energy report without tail correction:
 *   recip[i]           = inter + reciprocal of baseline_energy({s_i}).er                      (ewaldenergies[i]; optional, may be NULL)
 *   framework[i]       = Number(baseline_energy({s_i}).er) = framework VdW + framework direct + recip[i]
 *   interactions[i][j] = inter + reciprocal of baseline_energy({s_i, s_j}).er - recip[i] - recip[j];  [i][i] = 1e100 exactly;
 *                        [i][j] and [j][i] hold the same bits.  A site the framework grids block keeps framework[i] >= 1e90.
 *  Nothing large is subtracted on the device: with S_i the structure factor of site i over the handle's k-vectors, F the framework's,
 *   recip[i] = (2 sum_k kf Re(conj(F) S_i) + sum_k kf |S_i|^2) + offset_one and
 *   interactions[i][j] = (P_ij + 2 sum_k kf_k Re(S_i conj(S_j))) + offset_pair, P_ij the pair sum of the two molecules with the
 *   minimum image, cutoff and rule energies of row column 2 of ceg_mc_trial.  The count-dependent constants of the EwaldContext stay
 *   with the caller: with c(N) = 2 energy_net_charges(N) + static_contribution(N) for N molecules of the species (ewald.jl:497-544),
 *   offset_one = c(1) and offset_pair = c(2) - 2 c(1); both 0 without Ewald summation.
 *  Three launches for any n, on the handle's stream, then a synchronisation: k_site_points (one workgroup per site: the grids atom by
 *   atom, S_i), k_site_recip_pairs (v_mfma_f64_16x16x4 over the 16 x 16 site tiles of the upper triangle) and k_site_real_pairs (the
 *   molecule-pair sums over the same tiles, which also mirrors the triangle and sets the diagonal).
 *  CEG_ERR_UNSUPPORTED, with the figures in ceg_last_error(): n*n*8 bytes, or the structure factors (nk * n * 16 bytes), above
 *   CEG_HIP_SITE_TABLE_LIMIT_MB MiB (environment, default 2048); k-space tables of the molecule that do not fit in LDS.
 *   CEG_ERR_INVALID: a missing pointer, n or m_atoms out of range, a kind outside the pair table, a position or offset that is not
 *   finite, a handle inside a chain group. */
#define CEG_SITE_MAX_MOLECULES 4096
#define CEG_SITE_FRAME_TAKEN   1
#define CEG_SITE_FRAME_DROPPED 2
#define CEG_SITE_NEW_MINIMUM   4
#define CEG_SITE_GROUP_ACCEPTED  8      /* sweep_grouped: the cycle was accepted as one move */
#define CEG_SITE_GROUP_RESTARTED 16     /* sweep_grouped: the cycle began from a fresh random population */
typedef struct ceg_site_group ceg_site_group_t;
typedef struct ceg_site_params {        /* 24 bytes */
    uint64_t seed, first_step;
    const uint32_t* stream_id;          /* [K] or NULL */
} ceg_site_params_t;
typedef struct ceg_site_cycles {        /* 32 bytes */
    int64_t ncycles, steps_per_cycle, cycle0;
    const double* temperature;          /* [ncycles][K] */
} ceg_site_cycles_t;
typedef struct ceg_site_stats {         /* 32 bytes */
    int64_t attempted, accepted;        /* since creation */
    double delta, energy;               /* the sum of the accepted changes since creation; the running energy */
} ceg_site_stats_t;
typedef struct ceg_site_cycle_record {  /* 56 bytes */
    int64_t cycle;
    double temperature, energy, delta;
    int64_t attempted, accepted;        /* cumulative, as in the stats */
    int32_t flags, _pad;                /* CEG_SITE_FRAME_TAKEN | CEG_SITE_FRAME_DROPPED | CEG_SITE_NEW_MINIMUM | CEG_SITE_GROUP_* */
} ceg_site_cycle_record_t;
typedef struct ceg_site_record {        /* 40 bytes */
    int32_t molecule, old_site, new_site, accepted;
    double before, after, u;
} ceg_site_record_t;
typedef struct ceg_site_recorder {      /* 32 bytes */
    int64_t every, origin, frame_capacity;
    int32_t track_min, _pad;
} ceg_site_recorder_t;
typedef struct ceg_site_frame_record {  /* 16 bytes */
    int64_t cycle;
    double energy;
} ceg_site_frame_record_t;
typedef struct ceg_site_grouped_record { /* 48 bytes */
    double before, restart_energy, after, u;   /* E0, Er, E1 and the decision's draw */
    int32_t accepted, restarted;
    int64_t hops_accepted;              /* inside the cycle, whatever the decision */
} ceg_site_grouped_record_t;
typedef struct ceg_site_tempering {     /* 32 bytes */
    int32_t rungs, _pad;                /* R in 2..16, K % R == 0 */
    const double*   pair_cdf;           /* [R-1] host */
    const uint32_t* ladder_stream;      /* [K/R] host, or NULL: the ladder's index */
    int64_t _reserved;                  /* 0 */
} ceg_site_tempering_t;
CEG_API int ceg_site_tables(ceg_mc_t* handle, const int32_t* kinds, int32_t m_atoms, const double* positions, int32_t n, double offset_one,
                            double offset_pair, double* framework /*[n]*/, double* recip /*[n] or NULL*/, double* interactions /*[n][n]*/);
CEG_API int ceg_site_tables_device(ceg_mc_t* handle, const int32_t* kinds, int32_t m_atoms, const double* positions, int32_t n, double offset_one,
                                   double offset_pair, double* d_framework, double* d_recip, double* d_interactions);
CEG_API int ceg_site_group_create(int32_t device, int32_t n, int32_t m, int32_t k, const double* framework, const double* interactions,
                                  int32_t tables_on_device, const uint16_t* populations /*[K][m]*/, double tailcorrection,
                                  ceg_site_group_t** group);
CEG_API int ceg_site_group_destroy(ceg_site_group_t* group);
CEG_API int ceg_site_group_sweep_cycles(ceg_site_group_t* group, const ceg_site_params_t* params, const ceg_site_cycles_t* cycles,
                                        ceg_site_stats_t* stats_out, ceg_site_cycle_record_t* cycles_out, ceg_site_record_t* log_out);
CEG_API int ceg_site_group_sweep_grouped(ceg_site_group_t* group, const ceg_site_params_t* params, const ceg_site_cycles_t* cycles, int32_t restart,
                                         ceg_site_stats_t* stats_out, ceg_site_cycle_record_t* cycles_out, ceg_site_record_t* log_out,
                                         ceg_site_grouped_record_t* grouped_out /*[ncycles][K] or NULL*/);
CEG_API int ceg_site_group_baseline(ceg_site_group_t* group, double* out /*[K]*/);
CEG_API int ceg_site_group_rebase(ceg_site_group_t* group);
CEG_API int ceg_site_group_get_populations(ceg_site_group_t* group, uint16_t* populations_out /*[K][m]*/);
CEG_API int ceg_site_group_set_populations(ceg_site_group_t* group, const uint16_t* populations /*[K][m]*/);
CEG_API int ceg_site_group_set_recorder(ceg_site_group_t* group, const ceg_site_recorder_t* recorder);   /* NULL removes it */
CEG_API int ceg_site_group_recorder_read(ceg_site_group_t* group, int64_t first_frame, int64_t nframes, ceg_site_frame_record_t* records_out,
                                         uint16_t* populations_out, int64_t* frames_out);
CEG_API int ceg_site_group_recorder_min(ceg_site_group_t* group, int64_t* mink_out /*[K]*/, double* mine_out /*[K]*/,
                                        uint16_t* populations_out /*[K][m]*/);
CEG_API int ceg_site_group_set_tempering(ceg_site_group_t* group, const ceg_site_tempering_t* tempering);   /* NULL removes it */
CEG_API int ceg_site_group_tempering_read(ceg_site_group_t* group, int64_t* attempted /*[K/R][R-1]*/, int64_t* accepted /*[K/R][R-1]*/,
                                          int32_t* replica /*[K]*/);                       /* every pointer optional */

/* ---- blocking masks on the grid lattice ----------------------------- */
/*
 * BlockFile(g::EnergyGrid), src/grids.jl:188-204: a lattice cell (i, j, k), i < dims[0] etc., whose
 * value g.grid[k,j,i,1] exceeds `threshold` (5e6 K there) blocks its 8 corners.
 *  value   [(dims[0]+1)*(dims[1]+1)*(dims[2]+1)] float = channel 0 of the grid (host or device memory)
 *  block   [same count] uint8 out, host memory, [x][y][z] with z fastest, 1 = blocked
 */
CEG_API int ceg_block_from_grid(int32_t device, const float* value, int32_t value_on_device,
                                const int32_t dims[3], double threshold, uint8_t* block);
/*
 * The scan of parse_blockfile, src/coordinates.jl:139-152: lattice point (i, j, k) (0-based here) at
 * inverse_offsetpoint = (i, j, k) .* delta .+ shift (src/coordinates.jl:68-70) is blocked iff its
 * minimum-image distance (periodic_distance2_fromcartesian!, src/utils.jl:210-246, UNIT cell `mat`)
 * to the centre of one of the spheres is < radius.  centers [3*nspheres] are the snapped centres the
 * reference computes on the host (:128-131); radius2 [nspheres] = radius^2.
 */
CEG_API int ceg_block_spheres(int32_t device, const int32_t dims[3], const double delta[3], const double shift[3],
                              const double mat[9], const double invmat[9], int32_t ortho, double safemin2,
                              const double* centers, const double* radius2, int32_t nspheres, uint8_t* block);

/* ---- grid analysis: minima, components, site proximity maps (src/basins.jl) -------------- */
/*
 * What the reference does between an energy grid or a density map and the site model.  Common to the entry points of this section
 * (ceg_grid_basins, the last of them, says itself when it synchronises):
 *  - a grid is an Array{T,3} in Julia's memory order, first axis fastest: element (i, j, k), 0-based, at i + a*(j + b*k), dims =
 *    (a, b, c); a*b*c must fit int32 (CEG_ERR_INVALID otherwise);
 *  - every array marked "host or device" lives where its *_on_device flag says, device meaning `device`.  With device arrays the
 *    work is asynchronous on `stream` (a hipStream_t, NULL = the null stream) except where a count has to reach the caller:
 *    ceg_grid_local_minima and ceg_grid_components synchronise the stream, the two site calls do so only when an array of theirs is
 *    in host memory;
 *  - neighbours are periodic (mod1) as in the reference: an axis of length 1 makes a point its own neighbour, an axis of length 2
 *    makes both neighbours the same point; both come out as the reference's loops give them;
 *  - nothing is launched on a bad argument; no float atomics: every result is independent of the order in which waves arrive.
 *
 * ceg_grid_local_minima: local_minima(grid, tolerance; lt), basins.jl:40-99.
 *  maxima      0: lt = <;  1: lt = >.  A point is kept iff lt(value, neighbour) for all 26 periodic neighbours: strict, a NaN
 *              anywhere in the cube fails it, 1e100 and +-Inf are ordinary values.
 *  tolerance   < 0: every kept point.  >= 0: extremum = the MINIMUM of the grid over the kept points (also for maxima: :89 takes
 *              `minimum`), threshold = extremum + abs(extremum*tolerance) in FP64 in this order, and a kept point survives iff
 *              !(value > threshold) (also for maxima, :95).  The reference's `@assert min_energy < 0` (:91) is CEG_ERR_INVALID.
 *  count_out   the full count (host).  No local extremum at all, where the reference throws on an empty `minimum`: count 0, CEG_OK,
 *              extremum +Inf.
 *  ijk_out     [min(count, capacity)][3] int32, 0-based, sorted by linear index (Julia's sort! of the CartesianIndex list); host or
 *              device.  A count above the capacity is no error: compare and call again.  capacity 0: ijk_out may be NULL.
 *  extremum_out  host, optional: the minimum over the kept points (before the threshold).
 * One pass over the grid (the 3x3x3 cube of a point comes from an LDS tile with a periodic halo), then the flags are compacted in
 * linear-index order: counts per 2048 points, an exclusive scan, an emit.
 */
CEG_API int ceg_grid_local_minima(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], int32_t maxima,
                                  double tolerance, int32_t* ijk_out, int32_t ijk_on_device, int64_t capacity, int64_t* count_out,
                                  double* extremum_out, void* stream);

/*
 * ceg_grid_components: the periodic 6-connected components of the ACTIVE points of a grid.
 *  mode  CEG_COMPONENTS_NONZERO  active iff value != 0 (a NaN is active, as with iszero): local_components, basins.jl:279-313.
 *                                grid_is_int64 = 1: an int64 grid (the bins of ceg_mc_group_set_sampler), 0: FP64.  lo, hi ignored.
 *        CEG_COMPONENTS_BAND     active iff lo < value < hi, FP64 only: compute_levels, basins.jl:842-869, on a mean lattice of
 *                                ceg_energy_grid_reduced.  STRICT on both sides: the reference admits == for the point a scan starts
 *                                from and not for a neighbour, which for a value equal to a bound depends on its scan order.
 *  labels_out  [a*b*c] int32, optional, host or device: -1 for an inactive point, else the rank of the point's component when the
 *              components are ordered by their smallest linear index -- the order in which the reference's k, j, i scan finds them.
 *  count_out   the number of components (host).
 *  seed_out, size_out, sum_out   [min(count, capacity)], each optional, all host or all device (lists_on_device): the smallest linear
 *              index of the component, its number of points, the int64 sum of its values.  sum_out is for an int64 grid only
 *              (CEG_ERR_INVALID with an FP64 grid): an FP64 sum depends on the order of the additions, and the reference's is its
 *              queue's; the caller sums by label where it needs one.
 * Union-find over a parent array int32[a*b*c] (each active point united with its +i, +j, +k neighbours, the larger root hung under
 * the smaller with atomicMin until it holds), a flatten pass, ranks from the flagged roots and an exclusive scan; sizes and sums
 * by integer atomics, runs of equal labels inside a wave combined first.
 * Not covered: the unwrapped coordinates the reference's point lists carry, FP64 sums, the atol / rtol / ntol cut and the sort by
 * decreasing sum (a few numbers per component: the bindings do them from seed / size / sum).
 */
#define CEG_COMPONENTS_NONZERO 0
#define CEG_COMPONENTS_BAND    1
CEG_API int ceg_grid_components(int32_t device, const void* grid, int32_t grid_is_int64, int32_t grid_on_device, const int32_t dims[3],
                                int32_t mode, double lo, double hi, int32_t* labels_out, int32_t labels_on_device, int32_t* seed_out,
                                int32_t* size_out, int64_t* sum_out, int32_t lists_on_device, int64_t capacity, int64_t* count_out,
                                void* stream);

/*
 * ceg_grid_site_proximity: the map of site_proximity_map!, basins.jl:466-578.  For every grid point w = (i, j, k): the site s and the
 * cell offset o in {-1, 0, 1}^3 that minimise d2 = |mat * (site_s - ((w + o.*dims) ./ dims))|^2 (:526-528); the lowest site index
 * wins among equal d2; the point is assigned iff d2 < maxdist^2.
 *  mat       3x3 column-major, the cell;  sites  [nsites][3] FRACTIONAL, host memory, 0 <= nsites <= CEG_SITE_PROXIMITY_MAX_SITES.
 *            The reference first deletes the sites that snap to the voxel of an earlier one (1 + round(dims*x), :471-484): that is
 *            the caller's business (the bindings do it and return the deleted indices).
 *  site_out  [a*b*c] int32: 0 = none, else the 1-based site, as the reference's map;  offset_out  [a*b*c][3] int8, (0, 0, 0) where
 *            site_out is 0; both host or both device (out_on_device).
 * The reference reaches this map by two breadth-first passes per site with a skin of one voxel diagonal; it is the same map as long
 * as a ball does not meet its own image.  Hence CEG_ERR_INVALID unless 2*(maxdist + |mat*(1 ./ dims)|) is below the smallest
 * perpendicular width of the cell.  Under that condition an assigned point lies within half a cell of its site along every axis, so
 * the kernel tests one offset per site and axis, round(site - w/dims) clamped to {-1, 0, 1}, not 27.  (The reference also gives the
 * voxel a site snaps to to that site whatever the distances; that differs from the rule above only where maxdist, or the distance
 * to another site, is below a voxel diagonal.)
 * A gather: one thread per point, the sites in LDS.  Synchronises `stream` (the sites are read from host memory).
 */
#define CEG_SITE_PROXIMITY_MAX_SITES 2048
CEG_API int ceg_grid_site_proximity(int32_t device, const int32_t dims[3], const double mat[9], const double* sites, int32_t nsites,
                                    double maxdist, int32_t* site_out, int8_t* offset_out, int32_t out_on_device, void* stream);

/*
 * ceg_grid_site_density: the sums of closest_from_proximity, basins.jl:580-597, of an int64 density map over a proximity map, exact.
 *  bins        [a*b*c] int64, host or device;  site / offset  the map of ceg_grid_site_proximity, both host or both device
 *              (map_on_device); an entry of `site` outside 0 .. nsites is ignored
 *  rho_out     [nsites+1] int64: rho_s = the sum of the bins of the points of site s+1; entry nsites = the unattributed rest
 *  moment_out  [nsites+1][3] int64: M_c = sum of bins * (o_c*dims_c + w_c); the reference's centre is pos_c = M_c / (dims_c * rho)
 *              both host or both device (out_on_device), overwritten.
 * Integer atomics, runs of equal sites inside a wave combined first.
 */
CEG_API int ceg_grid_site_density(int32_t device, const int64_t* bins, int32_t bins_on_device, const int32_t* site, const int8_t* offset,
                                  int32_t map_on_device, const int32_t dims[3], int32_t nsites, int64_t* rho_out, int64_t* moment_out,
                                  int32_t out_on_device, void* stream);

/*
 * ceg_grid_basins: the attraction basins of local_basins(grid, minima; lt, skip, maxdist), basins.jl:195-252, as the maps from which
 * decompose_basins (:765-792) follows: for every grid point its level and the starts that own it.
 *  Definition.  u -> v is an edge when v is one of the six periodic GridNeighbors of u, lt(grid[u], grid[v]) and !skip(grid[v]).
 *    d_i(x) is the breadth-first level of x from start i along edges, D(x) = min_i d_i(x), and x belongs to basin i iff
 *    d_i(x) = D(x): the reference runs one search per start and then deletes from basin i every point that another basin reached at
 *    an earlier level (keep_shortest_distance!, :140-172).  Equal values give no edge; a NaN fails lt both ways.
 *  The one corner.  basins.jl:153 (`start == length(Q) && continue`) skips the last level of a basin when that level holds exactly
 *    one point: the point is neither checked against the earlier levels nor recorded for the later ones.  As written the reference
 *    therefore differs from the definition at points that are the sole last-level point of some basin, and only there.  This entry
 *    point follows the definition, which is what the reference's docstring promises.
 *  grid        [a*b*c] FP64, host or device, Julia's order.
 *  starts      [nstarts][3] int32, 0-based (i, j, k), host or device (starts_on_device): the list of ceg_grid_local_minima as it
 *              stands in device memory, or any other distinct points; they need not be minima.  An entry outside the grid or equal
 *              to an earlier one -> CEG_ERR_INVALID with its index in ceg_last_error().  nstarts == 0: starts may be NULL.
 *  maxima      0: lt = <;  1: lt = >.
 *  skip_above  skip(v) = v > skip_above; +Inf: nothing is skipped; a NaN value is never skipped (and never entered: it fails lt).
 *              A start whose value is skipped is dropped (:204-207): it owns nothing and its size is 0.  skip_above NaN -> INVALID.
 *  maxdist     0: no bound; > 0: levels 0 .. maxdist - 1 (the reference pushes only while current_dist < maxdist, and current_dist
 *              is 1 while the start itself is expanded, :214-226).
 *  level_out   [a*b*c] int32, optional: D(x), -1 where no basin reaches.
 *  owner_out   [a*b*c] int32, optional: the smallest index of a start that owns x, -1 for none.
 *  nowners_out [a*b*c] uint8, optional: the number of owners.        The three maps are all host or all device (maps_on_device).
 *  shared_out  [min(count, shared_capacity)][2] int32: the pairs (linear index, owner) for every owner of every point with more than
 *              one owner, sorted by index, then owner.  shared_count_out (host, optional) is the full count of pairs; a count above
 *              the capacity is no error: compare and call again.  shared_capacity 0: shared_out may be NULL.
 *  size_out    [nstarts] int32, optional: the number of points of each basin, a shared point counted once for each of its owners.
 *              shared_out and size_out are both host or both device (lists_on_device).
 *  A point with more than CEG_BASINS_MAX_OWNERS owners -> CEG_ERR_UNSUPPORTED, the linear index and the number of owners in
 *  ceg_last_error(); nothing is truncated and no output is to be used.
 * One levelled pass serves all the starts: per level one launch that claims the next frontier (compare-and-swap on the level map;
 * the claimer shows in no output) and, afterwards, one launch that pulls the owners of the level's points from their predecessors
 * one level down.  A single owner is one int32; lists of 2 .. 16 owners live in a pool and are merged in registers.  Sizes by integer
 * atomics; the pairs by counts per 2048 points, an exclusive scan and an emit.  Synchronises `stream` once per 16 levels and once
 * after the owner pass (the counts have to reach the host), and once more when an output is in host memory.  The pool starts with
 * max(a*b*c, 4096) entries (CEG_HIP_BASINS_POOL in the environment: another first size); if that is short the owner pass runs once
 * more with the bound, 16 a*b*c entries.
 * Not covered: the unwrapped coordinates of the reference's sets (a point is its wrapped index here; the reference holds whichever
 * periodic image its queue met first), clean_cluster! (a relabelling over the list of starts: the bindings do it).
 */
#define CEG_BASINS_MAX_OWNERS 16
CEG_API int ceg_grid_basins(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], const int32_t* starts,
                            int32_t starts_on_device, int64_t nstarts, int32_t maxima, double skip_above, int64_t maxdist,
                            int32_t* level_out, int32_t* owner_out, uint8_t* nowners_out, int32_t maps_on_device, int32_t* shared_out,
                            int64_t shared_capacity, int64_t* shared_count_out, int32_t* size_out, int32_t lists_on_device, void* stream);

/* ---- from a density map to the sites: smoothing, ranking, nearest-site partition (src/basins.jl:324-456, 613-731) -------------- */
/*
 * The device stages of coalescing_basins / average_clusters, and the greedy pass between them as a host function.  The conventions
 * of the grid-analysis section hold: Julia's memory order, a*b*c within int32, *_on_device flags, a full count when a capacity is
 * short (no error), nothing launched on an argument that can be refused from the host, no float atomics.  All three device entry
 * points synchronise `stream` before they return (taps, sites and counts cross the host).
 *
 * ceg_grid_smooth: imfilter(grid, Kernel.gaussian(sigma), "circular"), basins.jl:668, with the taps as an argument.
 *  grid        [a*b*c], host or device: FP64 (grid_is_int64 = 0; `scale` is ignored, x = value), or the int64 bins of the MC sampler
 *              (grid_is_int64 = 1): x = fl(scale * value), the first rounding; scale must be finite.  A bin with |value| >= 2^53
 *              -> CEG_ERR_INVALID (found by the first pass: the output is then not to be used).
 *  tapsC, lenC host arrays, lenC = 2 wC + 1 odd, 1 <= lenC <= 129; an even or non-positive length is CEG_ERR_INVALID, a longer one
 *              CEG_ERR_UNSUPPORTED with the figure in ceg_last_error().  What a Gaussian is is the caller's business.
 *  out         [a*b*c] FP64, host or device; not `grid` itself.
 *  Definition: three passes, along axis 0, then 1, then 2; y[p] = sum over t = -w .. w of taps[t + w] * x[(p + t) mod n] along the axis,
 *  t ascending, the accumulator starting at 0.0 and updated by fma(tap, x, acc); mod is the true modulus, so an axis shorter than w
 *  (or of length 1) wraps as often as needed.  Every element is that one sequence of operations whatever tile it falls in.
 *
 * ceg_grid_ranked: sortperm(vec(smoothed), rev=true) cut at `smval <= crop`, basins.jl:670, 679.
 *  Every linear index whose value is > crop, by value descending, equal values by ascending index (Julia's sortperm is stable and
 *  rev=true keeps the order of ties).  A NaN is not above anything and is dropped; the reference would visit it first.  crop >= 0 is
 *  required (CEG_ERR_INVALID otherwise, also for a NaN): it keeps -0.0 out of the keys.
 *  idx_out     [min(count, capacity)] int32;  val_out  optional, the values in the same order; both host or both device.
 *  count_out   the full count (host).
 *
 * ceg_grid_site_nearest: phase 2 of closest_to_sites, basins.jl:400-422, for every ACTIVE point and at any distance.
 *  For a point w = (i, j, k), 0-based, and a site s: buffer = site_s - (w + origin) ./ dims (an FP64 division, then a subtraction,
 *  per component), then periodic_distance_with_ofs! (utils.jl:257-280) as written: diff = buffer + 0.5, ofs = floor(diff), buffer =
 *  diff - ofs - 0.5; ref = sqrt(x*x + y*y + z*z) of mat*buffer (rows summed left to right, no contraction, correctly rounded square
 *  root); ref is returned if ortho or ref <= safemin, otherwise the first-improvement search over +1 / -1 per axis runs in the
 *  reference's order with its updates of ofs.  The point gets the site of smallest distance, the lowest index among equal ones
 *  (findmin), and that site's ofs.
 *  ortho, safemin   prepare_periodic_distance_computations(mat) (utils.jl:146-155), from the host as in the grid builds.
 *  origin      1: the reference as written (`Tuple(tovisit) ./ dims` on 1-based indices);  0: the convention of site_proximity_map!
 *              and updated_sites_with_closest.  Anything else is CEG_ERR_INVALID.
 *  sites       [nsites][3] fractional, host memory, 1 <= nsites <= CEG_SITE_PROXIMITY_MAX_SITES, finite with |x| <= 64 (so an
 *              offset fits int8).
 *  bins        optional [a*b*c] int64, host or device: a point is active iff its bin != 0.  NULL: every point is active.
 *  lin_out     [min(count, capacity)] int32, the active points in linear-index order;  site_out  int32, 0-based;  offset_out  [][3]
 *              int8;  dist_out  optional FP64.  All host or all device (out_on_device).  count_out: the full count (host).
 *
 * ceg_coalesce_ranked: the greedy pass of coalescing_basins, basins.jl:677-719, on the host (no device work, no device needed).
 *  lin, smoothed, values   [nranked]: the ranking of ceg_grid_ranked (already cut at the crop), the smoothed values and the
 *              unsmoothed grid values at those indices.
 *  maxbasins   the loop ends once that many basins exist; +Inf for no bound.
 *  value_out   [min(count, capacity)], centre_out [..][3]: the reference's `ret` at the end of the loop.  count_out: the full count.
 *  Plain IEEE FP64 in the reference's order with contraction off: pos = (i/a, j/b, k/c) on 1-based indices, the in-distance list
 *  sorted stably by distance, the submid rule, (val, pos*val/val) appended for a voxel with nothing in range and smval < atol
 *  unless val == 0, merged basins deleted in place and the new one pushed at the end.
 */
CEG_API int ceg_grid_smooth(int32_t device, const void* grid, int32_t grid_is_int64, int32_t grid_on_device, double scale,
                            const int32_t dims[3], const double* taps0, int32_t len0, const double* taps1, int32_t len1,
                            const double* taps2, int32_t len2, double* out, int32_t out_on_device, void* stream);
CEG_API int ceg_grid_ranked(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], double crop, int32_t* idx_out,
                            double* val_out, int32_t out_on_device, int64_t capacity, int64_t* count_out, void* stream);
CEG_API int ceg_grid_site_nearest(int32_t device, const int32_t dims[3], const double mat[9], int32_t ortho, double safemin,
                                  const double* sites, int32_t nsites, int32_t origin, const int64_t* bins, int32_t bins_on_device,
                                  int32_t* lin_out, int32_t* site_out, int8_t* offset_out, double* dist_out, int32_t out_on_device,
                                  int64_t capacity, int64_t* count_out, void* stream);
CEG_API int ceg_coalesce_ranked(const int32_t* lin, const double* smoothed, const double* values, int64_t nranked, const int32_t dims[3],
                                const double mat[9], int32_t ortho, double safemin, double maxdist, double atol, double maxbasins,
                                double* value_out, double* centre_out, int64_t capacity, int64_t* count_out);

/*
 * The same path with the sequential loops in the library: the greedy pass on the device, stages 2 and 3 of closest_to_sites for any
 * number of sites in one call, and cluster_closer_than! on the host.  Both device entry points synchronise `stream`.
 *
 * ceg_grid_coalesce: ceg_coalesce_ranked on the device -- the same bytes for any nranked, any number of basins and any cut into launches.
 *  lin, smoothed   [nranked] as ceg_grid_ranked leaves them, both host or both device (ranked_on_device).
 *  map         [a*b*c] the unsmoothed map, host or device: FP64 (map_is_int64 = 0, `scale` ignored) or int64 bins (val = fl(scale *
 *              bin), one rounding; scale finite).  The kernel gathers val = map[lin[r]] itself.  A bin with |value| >= 2^53 at a voxel
 *              the loop reaches -> CEG_ERR_INVALID.
 *  ortho, safemin, maxdist, atol, maxbasins   as ceg_coalesce_ranked; a NaN among them or a non-finite mat is CEG_ERR_INVALID.
 *  voxels_per_launch   the loop runs in one workgroup, in launches of at most this many ranked voxels, its state (basins, count, next
 *              rank, stop flag) kept in device memory in between; 0: the default (32768).  The result does not depend on it.
 *  value_out   [min(count, capacity)], centre_out [..][3], both host or both device (out_on_device); count_out: the full count (host).
 *  An index outside the grid -> CEG_ERR_INVALID, found on the device at the voxel the loop reaches: the outputs are then not to be used.
 *  As :695-699 are written at most one entry of the in-distance list survives -- the nearest basin with !(d > maxdist), isless on d,
 *  the lowest index among equals -- so a voxel is absorbed by that basin, or founds one (smval >= atol, counted against maxbasins), or
 *  is pushed alone as (val, pos*val/val) (smval < atol, val != 0, not counted), or is skipped.  Every voxel is compared with every
 *  basin: periodic_distance_with_ofs! in a triclinic cell is a first-improvement search, not a metric a cell index could reproduce.
 *
 * ceg_grid_site_partition: ceg_grid_site_nearest followed by stage 3 of closest_to_sites (:425-434) and the centres of
 * updated_sites_with_closest (:454), for any nsites >= 1.
 *  map         as above; a voxel is active iff its value != 0.
 *  sites       [nsites][3] fractional, host memory, finite with |x| <= 64;  origin  0 or 1, as ceg_grid_site_nearest.
 *  Every active voxel goes to its nearest site (strict <, ascending sites: the lowest index among equals).  Per site, over its voxels
 *  in linear-index order:  if (sum + rho > 1) { cap_bound = 1; skip }  sum = sum + rho;  acc[q] += (double)(w[q] + ofs[q]*dims[q]) /
 *  (double)dims[q] * rho  on the 0-based w = (i, j, k), no contraction.
 *  sums_out    [nsites];  centres_out [nsites][3] = acc / sum, NaN for a site without a voxel;  both host or both device.
 *  cap_bound_out   1 iff the cap skipped a voxel;  count_out  the number of active voxels.  Both host.
 *  Cost: a site's voxels are walked by ONE thread, because the cap makes its sum sequential: with one site, or one that takes most of
 *  the map, that walk is as long as the map has active voxels (307 k at 189^3), whatever the device.
 *  Stages: compaction in linear-index order, the nearest site with the sites streamed through LDS 2048 at a time, a stable radix sort
 *  of (site, position), the bounds of each site's run, one thread per site over its run.  Integer atomics only (the cap flag).
 *
 * ceg_cluster_closer_than: cluster_closer_than!, basins.jl:613-642, line by line on the host (no device needed), in place.
 *  rho [n], pos [n][3]: the list; on return the first *count_out entries are the list after deleteat!(ret, todelete).
 *  rho1 + rho2 > 1 is tested before the distance, d >= maxdist continues, pos1 = (rho1*pos1 + rho2*(pos2 + ofs)) / rho.
 */
CEG_API int ceg_grid_coalesce(int32_t device, const int32_t* lin, const double* smoothed, int32_t ranked_on_device, int64_t nranked,
                              const void* map, int32_t map_is_int64, int32_t map_on_device, double scale, const int32_t dims[3],
                              const double mat[9], int32_t ortho, double safemin, double maxdist, double atol, double maxbasins,
                              int64_t voxels_per_launch, double* value_out, double* centre_out, int32_t out_on_device, int64_t capacity,
                              int64_t* count_out, void* stream);
CEG_API int ceg_grid_site_partition(int32_t device, const void* map, int32_t map_is_int64, int32_t map_on_device, double scale,
                                    const int32_t dims[3], const double mat[9], int32_t ortho, double safemin, const double* sites,
                                    int32_t nsites, int32_t origin, double* sums_out, double* centres_out, int32_t out_on_device,
                                    int32_t* cap_bound_out, int64_t* count_out, void* stream);
CEG_API int ceg_cluster_closer_than(double* rho, double* pos, int64_t n, const double mat[9], int32_t ortho, double safemin, double maxdist,
                                    int64_t* count_out);

#ifdef __cplusplus
}
#endif
#endif /* CEG_HIP_H */
