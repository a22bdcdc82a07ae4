// ceg_grid_coalesce.hip -- the greedy pass of coalescing_basins (src/basins.jl:677-719 of the reference) on the device, and
// cluster_closer_than! (:613-642) as a host entry point.
//
// As :695-699 are written the loop is a nearest-basin rule (ceg_coalesce.h): every ranked voxel is compared with every basin alive, the
// nearest one in range absorbs it, and a voxel with none in range founds a basin.  That is one dependent chain, so one workgroup of
// GC_THREADS threads runs it; the parallel part is the comparison of a voxel with all the basins.
//   k_gc_greedy   per voxel: thread t takes the basins t, t + GC_THREADS, ... and keeps the nearest in range; shuffles reduce a wave, the
//                 wave results go to LDS, one barrier, and every thread reads them and takes the same decision.  The update is done by the
//                 thread that owns the basin (index mod GC_THREADS): it is the only thread that ever reads that basin again, so no second
//                 barrier is needed, and the wave results are double-buffered so that the one barrier also protects their reuse.
//                 The next voxel's index, smoothed value and map value are fetched while the current one is compared.
//   k_gc_export   the basins (val, c[3]) to the two output arrays
// The state (basins, their count, the next rank, the stop and refusal flags) lives in device memory between launches; a launch handles at
// most voxels_per_launch voxels and the result is the same bytes however the run is cut.  No scratch, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/ceg_hip.h"
#include "ceg_coalesce.h"
#include "ceg_grid_common.h"

// every expression is the reference's, operation by operation
#pragma clang fp contract(off)

namespace {

using namespace ceg_gs;

constexpr int GC_THREADS = 1024, GC_WAVES = GC_THREADS / 64;
constexpr int64_t GC_DEFAULT_VOXELS = 32768;           // per launch: see profiles/site_coalesce.txt for the time of one launch

enum { GC_BAD_INDEX = 1, GC_BAD_BIN = 2 };

struct GcState {
    int64_t next;        // the rank the next launch starts from
    int64_t count;       // basins alive
    int32_t stop;        // maxbasins was reached (:693)
    int32_t bad;         // GC_BAD_*: the outputs are not to be used
};

struct GcGeom {
    double mat[9];
    double safemin, maxdist, atol, maxbasins;
    int64_t n;
    int32_t a, b, ortho;
    double da, db, dc;
};

// the map value of voxel x and whether it may be used (an index outside the grid reads nothing)
template <typename TMAP>
__device__ __forceinline__ double gc_value(const TMAP* __restrict__ map, double scale, int64_t n, int x, int32_t* flag)
{
    *flag = 0;
    if (x < 0 || x >= n) {
        *flag = GC_BAD_INDEX;
        return 0.0;
    }
    int32_t bad = 0;
    const double v = gs_load(map, (int64_t)x, scale, &bad);
    if (bad) *flag = GC_BAD_BIN;
    return v;
}

template <typename TMAP>
__global__ __launch_bounds__(GC_THREADS) void k_gc_greedy(GcGeom G, const int32_t* __restrict__ lin, const double* __restrict__ smoothed,
                                                          const TMAP* __restrict__ map, double scale, int64_t nranked, int64_t nvox,
                                                          CegBasin* basins, GcState* state)
{
    __shared__ double s_d[2][GC_WAVES];
    __shared__ int s_i[2][GC_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (state->stop || state->bad) return;                             // uniform: every thread reads the same words
    int64_t r = state->next;
    int64_t count = state->count;
    const int64_t rend = (nranked - r < nvox) ? nranked : r + nvox;
    __syncthreads();                                                   // the state is rewritten at the end
    if (r >= rend) return;
    int32_t stop = 0, bad = 0;

    // the voxel in hand (0), and what is known of the next two
    int x0 = lin[r], f0 = 0;
    double sm0 = smoothed[r];
    double v0 = gc_value(map, scale, G.n, x0, &f0);
    int x1 = (r + 1 < rend) ? lin[r + 1] : 0;
    double sm1 = (r + 1 < rend) ? smoothed[r + 1] : 0.0;

    for (int par = 0; r < rend; ++r, par ^= 1) {
        int f1 = 0;
        const double v1 = (r + 1 < rend) ? gc_value(map, scale, G.n, x1, &f1) : 0.0;
        const int x2 = (r + 2 < rend) ? lin[r + 2] : 0;
        const double sm2 = (r + 2 < rend) ? smoothed[r + 2] : 0.0;
        if (f0) {
            bad = f0;
            break;
        }
        const int i = x0 % G.a + 1, j = (x0 / G.a) % G.b + 1, k = x0 / (G.a * G.b) + 1;                  // :681-682, 1-based
        const double pos[3] = {(double)i / G.da, (double)j / G.db, (double)k / G.dc};                    // :683

        // the nearest basin in range among this thread's
        double bd = 0.0, bofs[3] = {0.0, 0.0, 0.0};
        int bi = -1;
        for (int64_t idx = tid; idx < count; idx += GC_THREADS) {
            const CegBasin* o = basins + idx;
            double buffer[3] = {pos[0] - o->c[0], pos[1] - o->c[1], pos[2] - o->c[2]};
            double ofs[3];
            const double d = ceg_pdwo(G.mat, G.ortho != 0, G.safemin, buffer, ofs);
            if (d > G.maxdist) continue;                                                                 // :689
            if (bi < 0 || ceg_isless(d, bd)) {                      // ascending idx: the lowest index among equals stays
                bd = d;
                bi = (int)idx;
                bofs[0] = ofs[0]; bofs[1] = ofs[1]; bofs[2] = ofs[2];
            }
        }
        double wd = bd;
        int wi = bi;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double od = __shfl_xor(wd, m, 64);
            const int oi = __shfl_xor(wi, m, 64);
            if (oi >= 0 && (wi < 0 || ceg_nearer(od, oi, wd, wi))) {
                wd = od;
                wi = oi;
            }
        }
        if (lane == 0) {
            s_d[par][wave] = wd;
            s_i[par][wave] = wi;
        }
        __syncthreads();
        wd = s_d[par][0];
        wi = s_i[par][0];
#pragma unroll
        for (int w = 1; w < GC_WAVES; ++w) {
            const double od = s_d[par][w];
            const int oi = s_i[par][w];
            if (oi >= 0 && (wi < 0 || ceg_nearer(od, oi, wd, wi))) {
                wd = od;
                wi = oi;
            }
        }

        if (wi < 0) {
            const bool founds = sm0 >= G.atol;                                                          // :691
            if (founds || !(v0 == 0)) {                                                                  // :707 for the lone push
                if ((int)(count % GC_THREADS) == tid) {
                    CegBasin nb;
                    if (founds) {
                        nb.val = v0;
                        nb.c[0] = pos[0]; nb.c[1] = pos[1]; nb.c[2] = pos[2];
                    } else {
                        nb = ceg_coalesce_lone(v0, pos);
                    }
                    basins[count] = nb;
                }
                ++count;
                if (founds && (double)count >= G.maxbasins) {                                           // :693
                    stop = 1;
                    ++r;
                    break;
                }
            }
        } else if (wi == bi) {                                      // the owner: wi is among this thread's, so it is its nearest
            CegBasin o = basins[wi];
            if (ceg_coalesce_absorb(o, v0, pos, bofs)) basins[wi] = o;
        }
        x0 = x1; sm0 = sm1; v0 = v1; f0 = f1;
        x1 = x2; sm1 = sm2;
    }
    if (tid == 0) {
        state->next = r;
        state->count = count;
        state->stop = stop;
        state->bad = bad;
    }
}

__global__ __launch_bounds__(256) void k_gc_export(const CegBasin* __restrict__ basins, int64_t nout, double* __restrict__ value_out,
                                                   double* __restrict__ centre_out)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nout) return;
    const CegBasin o = basins[q];
    value_out[q] = o.val;
    centre_out[3 * q] = o.c[0];
    centre_out[3 * q + 1] = o.c[1];
    centre_out[3 * q + 2] = o.c[2];
}

}  // namespace

extern "C" int ceg_grid_coalesce(int32_t device, const int32_t* lin, const double* smoothed, int32_t ranked_on_device, int64_t nranked,
                                 const void* map, int32_t map_is_int64, int32_t map_on_device, double scale, const int32_t dims[3],
                                 const double mat[9], int32_t ortho, double safemin, double maxdist, double atol, double maxbasins,
                                 int64_t voxels_per_launch, double* value_out, double* centre_out, int32_t out_on_device, int64_t capacity,
                                 int64_t* count_out, void* stream)
{
    int64_t n = 0;
    if (nranked < 0 || (nranked > 0 && (!lin || !smoothed)) || !map || !mat || !count_out || capacity < 0 ||
        (capacity > 0 && (!value_out || !centre_out)) || voxels_per_launch < 0 || maxdist != maxdist || atol != atol || maxbasins != maxbasins ||
        safemin != safemin)
        return gerr(CEG_ERR_INVALID, "bad argument");
    if (map_is_int64 && !std::isfinite(scale)) return gerr(CEG_ERR_INVALID, "scale must be a finite number");
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(mat[q])) return gerr(CEG_ERR_INVALID, "mat must be finite");
    if (int rc = check_dims(dims, &n)) return rc;
    if (int rc = check_device(device)) return rc;
    *count_out = 0;
    if (nranked == 0) return CEG_OK;
    DevGuard guard(device);
    if (!guard.ok) return gerr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const int32_t* d_lin = (const int32_t*)ws.in(lin, ranked_on_device, sizeof(int32_t) * (size_t)nranked);
    const double* d_sm = (const double*)ws.in(smoothed, ranked_on_device, sizeof(double) * (size_t)nranked);
    const void* d_map = ws.in(map, map_on_device, 8 * (size_t)n);
    CegBasin* d_basins = (CegBasin*)ws.get(sizeof(CegBasin) * (size_t)nranked);                   // a voxel founds at most one basin
    GcState* d_state = (GcState*)ws.get(sizeof(GcState));
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    if (hipMemsetAsync(d_state, 0, sizeof(GcState), ws.st) != hipSuccess) return gerr(CEG_ERR_HIP, "hipMemsetAsync failed");
    GcGeom G{};
    for (int q = 0; q < 9; ++q) G.mat[q] = mat[q];
    G.safemin = safemin; G.maxdist = maxdist; G.atol = atol; G.maxbasins = maxbasins;
    G.n = n; G.a = dims[0]; G.b = dims[1]; G.ortho = ortho ? 1 : 0;
    G.da = (double)dims[0]; G.db = (double)dims[1]; G.dc = (double)dims[2];
    const int64_t nvox = voxels_per_launch ? voxels_per_launch : GC_DEFAULT_VOXELS;
    for (int64_t r0 = 0; r0 < nranked; r0 += nvox) {              // a launch starts from the state's rank, and does nothing once stopped
        if (map_is_int64)
            hipLaunchKernelGGL(k_gc_greedy<int64_t>, dim3(1), dim3(GC_THREADS), 0, ws.st, G, d_lin, d_sm, (const int64_t*)d_map, scale, nranked, nvox,
                               d_basins, d_state);
        else
            hipLaunchKernelGGL(k_gc_greedy<double>, dim3(1), dim3(GC_THREADS), 0, ws.st, G, d_lin, d_sm, (const double*)d_map, scale, nranked, nvox,
                               d_basins, d_state);
    }
    GcState h{};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, d_state, sizeof(GcState), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return gerr(CEG_ERR_HIP, "the greedy pass failed");
    if (h.bad == GC_BAD_INDEX) return gerr(CEG_ERR_INVALID, "a ranked index is outside the grid (the output is not to be used)");
    if (h.bad) return gerr(CEG_ERR_INVALID, "a bin with |value| >= 2^53: its conversion to FP64 would round (the output is not to be used)");
    *count_out = h.count;
    const int64_t nout = h.count < capacity ? h.count : capacity;
    if (nout == 0) return CEG_OK;
    double* d_val = (double*)ws.out(value_out, out_on_device, sizeof(double) * (size_t)nout);
    double* d_cen = (double*)ws.out(centre_out, out_on_device, sizeof(double) * 3 * (size_t)nout);
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace");
    hipLaunchKernelGGL(k_gc_export, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ws.st, d_basins, nout, d_val, d_cen);
    ws.back(value_out, out_on_device, d_val, sizeof(double) * (size_t)nout);
    ws.back(centre_out, out_on_device, d_cen, sizeof(double) * 3 * (size_t)nout);
    if (hipGetLastError() != hipSuccess || ws.failed || hipStreamSynchronize(ws.st) != hipSuccess)
        return gerr(CEG_ERR_HIP, "the copy of the basins failed");
    return CEG_OK;
}

extern "C" int ceg_cluster_closer_than(double* rho, double* pos, int64_t n, const double mat[9], int32_t ortho, double safemin, double maxdist,
                                       int64_t* count_out)
{
    if (n < 0 || (n > 0 && (!rho || !pos)) || !mat || !count_out || maxdist != maxdist || safemin != safemin)
        return gerr(CEG_ERR_INVALID, "bad argument");
    *count_out = ceg_cluster_closer_than_inplace(rho, pos, n, mat, ortho != 0, safemin, maxdist);
    return CEG_OK;
}
