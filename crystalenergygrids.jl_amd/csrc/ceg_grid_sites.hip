// ceg_grid_sites.hip -- from a density map to the list of sites (src/basins.jl of the reference, the part behind average_clusters):
//   imfilter(grid, gaussian, "circular")   basins.jl:668   ceg_grid_smooth: three separable passes.  k_gs_smooth_row (axis 0): a row
//                                                          segment of 64 points plus its halo in LDS, four rows per workgroup.
//                                                          k_gs_smooth_axis (axes 1 and 2, the array seen as [inner][n][outer]): XT
//                                                          contiguous points by a run along the axis plus 2w halo rows in LDS, loaded
//                                                          with coalesced reads; four outputs per thread share one tap load
//   sortperm(vec(smoothed), rev=true)      :670, :679  ceg_grid_ranked: the points above the crop compacted in linear-index order
//                                                          (counts per 2048 points, exclusive scan, emit), then a stable radix sort
//   closest_to_sites, phase 2              :400-422     ceg_grid_site_nearest: the active points compacted the same way, then a gather:
//                                                          one thread per point, the sites in LDS, periodic_distance_with_ofs! per pair
//   closest_to_sites, phases 2 and 3       :400-434     ceg_grid_site_partition, any number of sites: the same compaction (on the map's
//                                                          value), k_gs_nearest_tiled (the sites through LDS 2048 at a time, the best carried
//                                                          along), a stable radix sort of (site, position), k_gs_site_runs (the bounds of each
//                                                          site's run) and k_gs_site_sums: one thread per site walks its voxels in linear-index
//                                                          order, because the cap (:430) makes every step depend on the one before
//   the greedy pass                        :677-719     ceg_coalesce_ranked: host only (ceg_coalesce.h); on the device: ceg_grid_coalesce.hip
// An output element is one fixed sequence of FP64 operations whatever the tile it falls in; no float atomics (one integer atomicOr
// for the cap flag), no scratch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/ceg_hip.h"
#include "ceg_coalesce.h"
#include "ceg_grid_common.h"

// distances and the scale are the reference's expressions, operation by operation; the taps are applied by explicit fma
#pragma clang fp contract(off)

namespace {

using namespace ceg_gs;

constexpr int CHUNK = 2048;             // points of one workgroup of the compaction kernels (8 per thread)
constexpr int SEG = 64, ROWS = 4;       // k_gs_smooth_row: points of a row segment, rows per workgroup
constexpr int MAXTAPS = 129;

__device__ __forceinline__ int pmod(int x, int n)
{
    x %= n;
    return x < 0 ? x + n : x;
}

// ---- smoothing --------------------------------------------------------------------------------------------------------------------
template <typename TIN>
__global__ __launch_bounds__(256) void k_gs_smooth_row(const TIN* __restrict__ in, double scale, const double* __restrict__ taps, int w,
                                                       int a, int64_t nrows, int ntx, double* __restrict__ out, int32_t* __restrict__ bad)
{
    extern __shared__ double s_row[];                                // ROWS * (SEG + 2w)
    const int width = SEG + 2 * w;
    const int64_t bt = (int64_t)blockIdx.x;
    const int i0 = (int)(bt % ntx) * SEG;
    const int64_t r0 = (bt / ntx) * ROWS;
    for (int idx = (int)threadIdx.x; idx < ROWS * width; idx += 256) {
        const int rr = idx / width, l = idx - rr * width;
        const int64_t r = r0 + rr;
        if (r < nrows) s_row[idx] = gs_load(in, (int64_t)pmod(i0 - w + l, a) + (int64_t)a * r, scale, bad);
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & (SEG - 1), rr = (int)threadIdx.x / SEG;
    const int i = i0 + lx;
    const int64_t r = r0 + rr;
    if (i >= a || r >= nrows) return;
    const double* row = s_row + rr * width + lx;
    double acc = 0.0;
    for (int t = 0; t <= 2 * w; ++t) acc = fma(taps[t], row[t], acc);
    out[(int64_t)i + (int64_t)a * r] = acc;
}

// element (x, p, o) of [inner][n][outer] at x + inner*(p + n*o); 256 threads = XT points by NY = 256/XT lanes along the axis, each
// lane four outputs NY apart: a run of 4*NY
template <int XT>
__global__ __launch_bounds__(256) void k_gs_smooth_axis(const double* __restrict__ in, const double* __restrict__ taps, int w, int64_t inner,
                                                        int n, int64_t ntx, int ntp, double* __restrict__ out)
{
    constexpr int NY = 256 / XT, RUN = 4 * NY;
    extern __shared__ double s_t[];                                  // (RUN + 2w) * XT
    const int rows = RUN + 2 * w;
    const int64_t bt = (int64_t)blockIdx.x;
    const int64_t x0 = (bt % ntx) * XT;
    const int64_t rest = bt / ntx;
    const int p0 = (int)(rest % ntp) * RUN;
    const int64_t base = inner * (int64_t)n * (rest / ntp);
    for (int idx = (int)threadIdx.x; idx < rows * XT; idx += 256) {
        const int lr = idx / XT, lx = idx - lr * XT;
        if (x0 + lx < inner) s_t[idx] = in[base + x0 + lx + inner * (int64_t)pmod(p0 - w + lr, n)];
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % XT, ly = (int)threadIdx.x / XT;
    if (x0 + lx >= inner) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t <= 2 * w; ++t) {
        const double tp = taps[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(tp, s_t[(ly + q * NY + t) * XT + lx], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = p0 + ly + q * NY;
        if (p < n) out[base + x0 + lx + inner * (int64_t)p] = acc[q];
    }
}

// ---- compaction in linear-index order ---------------------------------------------------------------------------------------------
// SEL_VALUE_F64 / SEL_VALUE_BINS: the map value != 0, an FP64 map or int64 bins times the scale, which travels in `crop`
enum { SEL_ABOVE = 0, SEL_NONZERO = 1, SEL_ALL = 2, SEL_VALUE_F64 = 3, SEL_VALUE_BINS = 4 };

template <int SEL>
__device__ __forceinline__ bool gs_selected(const void* __restrict__ src, int64_t x, double crop)
{
    if (SEL == SEL_ABOVE) return static_cast<const double*>(src)[x] > crop;      // a NaN is not above anything
    if (SEL == SEL_NONZERO) return static_cast<const int64_t*>(src)[x] != 0;
    if (SEL == SEL_VALUE_F64) return static_cast<const double*>(src)[x] != 0;
    if (SEL == SEL_VALUE_BINS) return crop * (double)static_cast<const int64_t*>(src)[x] != 0;
    return true;
}

template <int SEL>
__global__ __launch_bounds__(256) void k_gs_chunk_count(const void* __restrict__ src, int64_t n, double crop, int32_t* __restrict__ chunkcnt)
{
    using Red = hipcub::BlockReduce<int, 256>;
    __shared__ typename Red::TempStorage tmp;
    const int64_t x0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    int mine = 0;
    for (int q = 0; q < 8; ++q)
        if (x0 + q < n && gs_selected<SEL>(src, x0 + q, crop)) ++mine;
    const int tot = Red(tmp).Sum(mine);
    if (threadIdx.x == 0) chunkcnt[blockIdx.x] = tot;
}

// the selected points below `cap`, in linear-index order: their index and, for SEL_ABOVE, their value
template <int SEL>
__global__ __launch_bounds__(256) void k_gs_emit(const void* __restrict__ src, int64_t n, double crop, const int32_t* __restrict__ chunkoff,
                                                 int64_t cap, int32_t* __restrict__ idx_out, double* __restrict__ val_out)
{
    using Scan = hipcub::BlockScan<int, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t x0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    unsigned mask = 0;
    for (int q = 0; q < 8; ++q)
        if (x0 + q < n && gs_selected<SEL>(src, x0 + q, crop)) mask |= 1u << q;
    int pre = 0;
    Scan(tmp).ExclusiveSum(__popc(mask), pre);
    int64_t pos = (int64_t)chunkoff[blockIdx.x] + pre;
    for (int q = 0; q < 8; ++q) {
        if (!((mask >> q) & 1)) continue;
        if (pos < cap) {
            idx_out[pos] = (int32_t)(x0 + q);
            if (SEL == SEL_ABOVE) val_out[pos] = static_cast<const double*>(src)[x0 + q];
        }
        ++pos;
    }
}

// ---- nearest site -----------------------------------------------------------------------------------------------------------------
struct NearGeom {
    double mat[9];
    double safemin;
    int32_t a, b, c, ns, origin, ortho;
};

__global__ __launch_bounds__(256) void k_gs_nearest(NearGeom G, const double* __restrict__ sites, const int32_t* __restrict__ lin, int64_t nout,
                                                    int32_t* __restrict__ site_out, int8_t* __restrict__ off_out, double* __restrict__ dist_out)
{
    extern __shared__ double s_sites[];
    for (int t = (int)threadIdx.x; t < 3 * G.ns; t += 256) s_sites[t] = sites[t];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nout) return;
    const int x = lin[e];
    const int i = x % G.a, j = (x / G.a) % G.b, k = x / (G.a * G.b);            // a*b*c fits int32
    const double wx = (double)(i + G.origin) / (double)G.a;                    // Tuple(tovisit) ./ dims, :415
    const double wy = (double)(j + G.origin) / (double)G.b;
    const double wz = (double)(k + G.origin) / (double)G.c;
    int best = 0, bo0 = 0, bo1 = 0, bo2 = 0;
    double bestd = INFINITY;
    for (int s = 0; s < G.ns; ++s) {
        double buf[3] = {s_sites[3 * s] - wx, s_sites[3 * s + 1] - wy, s_sites[3 * s + 2] - wz};      // :416
        int o[3];
        const double d = ceg_pdwo(G.mat, G.ortho != 0, G.safemin, buf, o);
        if (d < bestd) {                         // strict: findmin keeps the lowest site among equals
            bestd = d;
            best = s;
            bo0 = o[0]; bo1 = o[1]; bo2 = o[2];
        }
    }
    site_out[e] = best;
    off_out[3 * e] = (int8_t)bo0;
    off_out[3 * e + 1] = (int8_t)bo1;
    off_out[3 * e + 2] = (int8_t)bo2;
    if (dist_out) dist_out[e] = bestd;
}

// ---- nearest site and site sums for any number of sites ---------------------------------------------------------------------------
constexpr int SITE_TILE = 2048;          // sites of one pass through LDS (48 KiB)

// k_gs_nearest with the sites streamed through LDS SITE_TILE at a time and the best carried along: ascending sites and a strict `<`, so
// the result is the one all sites resident would give
__global__ __launch_bounds__(256) void k_gs_nearest_tiled(NearGeom G, const double* __restrict__ sites, const int32_t* __restrict__ lin, int64_t nout,
                                                          int32_t* __restrict__ site_out, int8_t* __restrict__ off_out)
{
    __shared__ double s_sites[3 * SITE_TILE];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < nout;
    const int x = live ? lin[e] : 0;
    const int i = x % G.a, j = (x / G.a) % G.b, k = x / (G.a * G.b);
    const double wx = (double)(i + G.origin) / (double)G.a;
    const double wy = (double)(j + G.origin) / (double)G.b;
    const double wz = (double)(k + G.origin) / (double)G.c;
    int best = 0, bo0 = 0, bo1 = 0, bo2 = 0;
    double bestd = INFINITY;
    for (int s0 = 0; s0 < G.ns; s0 += SITE_TILE) {
        const int cnt = G.ns - s0 < SITE_TILE ? G.ns - s0 : SITE_TILE;
        __syncthreads();
        for (int t = (int)threadIdx.x; t < 3 * cnt; t += 256) s_sites[t] = sites[3 * (int64_t)s0 + t];
        __syncthreads();
        if (!live) continue;
        for (int s = 0; s < cnt; ++s) {
            double buf[3] = {s_sites[3 * s] - wx, s_sites[3 * s + 1] - wy, s_sites[3 * s + 2] - wz};
            int o[3];
            const double d = ceg_pdwo(G.mat, G.ortho != 0, G.safemin, buf, o);
            if (d < bestd) {
                bestd = d;
                best = s0 + s;
                bo0 = o[0]; bo1 = o[1]; bo2 = o[2];
            }
        }
    }
    if (!live) return;
    site_out[e] = best;
    off_out[3 * e] = (int8_t)bo0;
    off_out[3 * e + 1] = (int8_t)bo1;
    off_out[3 * e + 2] = (int8_t)bo2;
}

__global__ __launch_bounds__(256) void k_gs_iota(int32_t* __restrict__ out, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (int32_t)e;
}

// keys sorted by site: first[s] .. last[s] is the run of site s (both stay 0 for a site without a voxel)
__global__ __launch_bounds__(256) void k_gs_site_runs(const int32_t* __restrict__ key, int64_t n, int32_t* __restrict__ first, int32_t* __restrict__ last)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int s = key[q];
    if (q == 0 || key[q - 1] != s) first[s] = (int32_t)q;
    if (q == n - 1 || key[q + 1] != s) last[s] = (int32_t)(q + 1);
}

// stage 3 of closest_to_sites (:425-434) and the centres of updated_sites_with_closest (:454): one thread per site walks the site's
// voxels in linear-index order, because the cap makes every step depend on the one before
template <typename TMAP>
__global__ __launch_bounds__(256) void k_gs_site_sums(const TMAP* __restrict__ map, double scale, int32_t a, int32_t b, int32_t c, int32_t ns,
                                                      const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ lin,
                                                      const int8_t* __restrict__ off, double* __restrict__ sums, double* __restrict__ centres,
                                                      int32_t* __restrict__ flags)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= ns) return;
    const int64_t dims[3] = {a, b, c};
    double sum = 0.0, acc[3] = {0.0, 0.0, 0.0};
    bool capped = false;
    for (int q = first[s]; q < last[s]; ++q) {
        const int e = order[q];
        const int x = lin[e];
        const double rho = gs_load(map, (int64_t)x, scale, flags + 1);      // flags[1]: a plain store of 1 by whoever sees a bad bin
        if (sum + rho > 1) {                                                     // :430
            capped = true;
            continue;
        }
        sum = sum + rho;
        const int64_t w[3] = {x % a, (x / a) % b, x / (a * b)};
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[r] += (double)(w[r] + (int64_t)off[3 * (int64_t)e + r] * dims[r]) / (double)dims[r] * rho;
    }
    if (capped) atomicOr(flags, 1);                                              // flags[0]: the one integer atomic of the call
    sums[s] = sum;
#pragma unroll
    for (int r = 0; r < 3; ++r) centres[3 * (int64_t)s + r] = acc[r] / sum;       // 0/0 = NaN for a site without a voxel
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// counts per chunk of the selected points -> exclusive offsets and the total (synchronises the stream)
template <int SEL>
int select_offsets(Workspace& ws, const void* d_src, int64_t n, double crop, int64_t* nchunk, int32_t** d_off, int64_t* total)
{
    *nchunk = (n + CHUNK - 1) / CHUNK;
    int32_t* d_cnt = (int32_t*)ws.get(sizeof(int32_t) * (size_t)(*nchunk + 1));
    *d_off = (int32_t*)ws.get(sizeof(int32_t) * (size_t)(*nchunk + 1));
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt, *d_off, (int)(*nchunk + 1), ws.st);
    void* d_tmp = ws.get(tmp_bytes);
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    int32_t last = 0;
    if (hipMemsetAsync(d_cnt + *nchunk, 0, sizeof(int32_t), ws.st) != hipSuccess) return gerr(CEG_ERR_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_gs_chunk_count<SEL>, dim3((unsigned)*nchunk), dim3(256), 0, ws.st, d_src, n, crop, d_cnt);
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, *d_off, (int)(*nchunk + 1), ws.st) != hipSuccess ||
        hipMemcpyAsync(&last, *d_off + *nchunk, sizeof(int32_t), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return gerr(CEG_ERR_HIP, "the compaction of the selected points failed");
    *total = last;
    return CEG_OK;
}

int check_taps(const double* taps, int32_t len, int axis)
{
    char msg[160];
    if (!taps || len < 1 || len % 2 == 0) {
        std::snprintf(msg, sizeof msg, "taps of axis %d: an odd number of them, at least 1 (got %d)", axis, (int)len);
        return gerr(CEG_ERR_INVALID, msg);
    }
    if (len > MAXTAPS) {
        std::snprintf(msg, sizeof msg, "taps of axis %d: %d of them, at most %d are supported", axis, (int)len, MAXTAPS);
        return gerr(CEG_ERR_UNSUPPORTED, msg);
    }
    return CEG_OK;
}

void smooth_axis(hipStream_t st, const double* d_in, const double* d_taps, int w, int64_t inner, int n, int64_t outer, double* d_out)
{
    // 64 points wide while the tile stays within 64 KiB of LDS, 32 wide for the longest halos
    if (w <= 48) {
        const int64_t ntx = (inner + 63) / 64;
        const int ntp = (n + 15) / 16;
        hipLaunchKernelGGL(k_gs_smooth_axis<64>, dim3((unsigned)(ntx * ntp * outer)), dim3(256), sizeof(double) * 64 * (size_t)(16 + 2 * w), st, d_in,
                           d_taps, w, inner, n, ntx, ntp, d_out);
    } else {
        const int64_t ntx = (inner + 31) / 32;
        const int ntp = (n + 31) / 32;
        hipLaunchKernelGGL(k_gs_smooth_axis<32>, dim3((unsigned)(ntx * ntp * outer)), dim3(256), sizeof(double) * 32 * (size_t)(32 + 2 * w), st, d_in,
                           d_taps, w, inner, n, ntx, ntp, d_out);
    }
}

}  // namespace

extern "C" int ceg_grid_smooth(int32_t device, const void* grid, int32_t grid_is_int64, int32_t grid_on_device, double scale,
                               const int32_t dims[3], const double* taps0, int32_t len0, const double* taps1, int32_t len1,
                               const double* taps2, int32_t len2, double* out, int32_t out_on_device, void* stream)
{
    int64_t n = 0;
    if (!grid || !out || (const void*)out == grid) return gerr(CEG_ERR_INVALID, "bad argument (the smoothing does not work in place)");
    if (grid_is_int64 && !std::isfinite(scale)) return gerr(CEG_ERR_INVALID, "scale must be a finite number");
    if (int rc = check_dims(dims, &n)) return rc;
    if (int rc = check_taps(taps0, len0, 0)) return rc;
    if (int rc = check_taps(taps1, len1, 1)) return rc;
    if (int rc = check_taps(taps2, len2, 2)) return rc;
    if (int rc = check_device(device)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return gerr(CEG_ERR_HIP, "hipSetDevice failed");
    const int a = dims[0], b = dims[1], c = dims[2];
    const int w0 = len0 / 2, w1 = len1 / 2, w2 = len2 / 2;
    std::vector<double> h_taps;
    h_taps.insert(h_taps.end(), taps0, taps0 + len0);
    h_taps.insert(h_taps.end(), taps1, taps1 + len1);
    h_taps.insert(h_taps.end(), taps2, taps2 + len2);
    Workspace ws((hipStream_t)stream);
    const void* d_g = ws.in(grid, grid_on_device, 8 * (size_t)n);
    const double* d_taps = (const double*)ws.in(h_taps.data(), 0, sizeof(double) * h_taps.size());
    double* d_out = (double*)ws.out(out, out_on_device, sizeof(double) * (size_t)n);
    double* d_scr = (double*)ws.get(sizeof(double) * (size_t)n);
    int32_t* d_bad = (int32_t*)ws.get(sizeof(int32_t));
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    if (hipMemsetAsync(d_bad, 0, sizeof(int32_t), ws.st) != hipSuccess) return gerr(CEG_ERR_HIP, "hipMemsetAsync failed");
    const int ntx = (a + SEG - 1) / SEG;
    const int64_t nrows = (int64_t)b * c;
    const unsigned nb0 = (unsigned)(ntx * ((nrows + ROWS - 1) / ROWS));
    const size_t lds0 = sizeof(double) * ROWS * (size_t)(SEG + 2 * w0);
    if (grid_is_int64)
        hipLaunchKernelGGL(k_gs_smooth_row<int64_t>, dim3(nb0), dim3(256), lds0, ws.st, (const int64_t*)d_g, scale, d_taps, w0, a, nrows, ntx, d_out,
                           d_bad);
    else
        hipLaunchKernelGGL(k_gs_smooth_row<double>, dim3(nb0), dim3(256), lds0, ws.st, (const double*)d_g, scale, d_taps, w0, a, nrows, ntx, d_out,
                           d_bad);
    smooth_axis(ws.st, d_out, d_taps + len0, w1, a, b, c, d_scr);
    smooth_axis(ws.st, d_scr, d_taps + len0 + len1, w2, (int64_t)a * b, c, 1, d_out);
    int32_t bad = 0;
    ws.back(out, out_on_device, d_out, sizeof(double) * (size_t)n);
    if (hipGetLastError() != hipSuccess || ws.failed || hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)                                   // the taps were read from the host
        return gerr(CEG_ERR_HIP, "the smoothing passes failed");
    if (bad) return gerr(CEG_ERR_INVALID, "a bin with |value| >= 2^53: its conversion to FP64 would round (the output is not to be used)");
    return CEG_OK;
}

extern "C" int ceg_grid_ranked(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], double crop, int32_t* idx_out,
                               double* val_out, int32_t out_on_device, int64_t capacity, int64_t* count_out, void* stream)
{
    int64_t n = 0;
    if (!grid || !count_out || capacity < 0 || (capacity > 0 && !idx_out)) return gerr(CEG_ERR_INVALID, "bad argument");
    if (!(crop >= 0)) return gerr(CEG_ERR_INVALID, "crop must be a number >= 0");
    if (int rc = check_dims(dims, &n)) return rc;
    if (int rc = check_device(device)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return gerr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const double* d_g = (const double*)ws.in(grid, grid_on_device, sizeof(double) * (size_t)n);
    int64_t nchunk = 0, total = 0;
    int32_t* d_off = nullptr;
    if (int rc = select_offsets<SEL_ABOVE>(ws, d_g, n, crop, &nchunk, &d_off, &total)) return rc;
    *count_out = total;
    const int64_t nout = total < capacity ? total : capacity;
    if (nout == 0) return CEG_OK;
    double* d_key = (double*)ws.get(sizeof(double) * (size_t)total);
    double* d_key2 = (double*)ws.get(sizeof(double) * (size_t)total);
    int32_t* d_idx = (int32_t*)ws.get(sizeof(int32_t) * (size_t)total);
    int32_t* d_idx2 = (int32_t*)ws.get(sizeof(int32_t) * (size_t)total);
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, d_key, d_key2, d_idx, d_idx2, (int)total, 0, 64, ws.st);
    void* d_tmp = ws.get(tmp_bytes);
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace");
    hipLaunchKernelGGL(k_gs_emit<SEL_ABOVE>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_g, n, crop, d_off, total, d_idx, d_key);
    // least-significant-digit radix sort: stable, so equal values keep their ascending indices, also when descending
    if (hipcub::DeviceRadixSort::SortPairsDescending(d_tmp, tmp_bytes, d_key, d_key2, d_idx, d_idx2, (int)total, 0, 64, ws.st) != hipSuccess)
        return gerr(CEG_ERR_HIP, "the radix sort failed");
    const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (hipMemcpyAsync(idx_out, d_idx2, sizeof(int32_t) * (size_t)nout, kind, ws.st) != hipSuccess ||
        (val_out && hipMemcpyAsync(val_out, d_key2, sizeof(double) * (size_t)nout, kind, ws.st) != hipSuccess))
        return gerr(CEG_ERR_HIP, "the copy of the ranking failed");
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ws.st) != hipSuccess)      // as the two other device calls of this file
        return gerr(CEG_ERR_HIP, "the ranking failed");
    return CEG_OK;
}

extern "C" int ceg_grid_site_nearest(int32_t device, const int32_t dims[3], const double mat[9], int32_t ortho, double safemin,
                                     const double* sites, int32_t nsites, int32_t origin, const int64_t* bins, int32_t bins_on_device,
                                     int32_t* lin_out, int32_t* site_out, int8_t* offset_out, double* dist_out, int32_t out_on_device,
                                     int64_t capacity, int64_t* count_out, void* stream)
{
    int64_t n = 0;
    if (!mat || !sites || !count_out || capacity < 0 || (capacity > 0 && (!lin_out || !site_out || !offset_out)) || safemin != safemin)
        return gerr(CEG_ERR_INVALID, "bad argument");
    if (origin != 0 && origin != 1) return gerr(CEG_ERR_INVALID, "origin is 0 or 1");
    if (nsites < 1) return gerr(CEG_ERR_INVALID, "at least one site");
    if (nsites > CEG_SITE_PROXIMITY_MAX_SITES) return gerr(CEG_ERR_UNSUPPORTED, "more sites than CEG_SITE_PROXIMITY_MAX_SITES");
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(mat[q])) return gerr(CEG_ERR_INVALID, "mat must be finite");
    for (int64_t q = 0; q < 3 * (int64_t)nsites; ++q)
        if (!(std::fabs(sites[q]) <= 64.0)) {
            char msg[128];
            std::snprintf(msg, sizeof msg, "site %lld: fractional coordinates must be finite with |x| <= 64", (long long)(q / 3));
            return gerr(CEG_ERR_INVALID, msg);
        }
    if (int rc = check_dims(dims, &n)) return rc;
    if (int rc = check_device(device)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return gerr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const int64_t* d_bins = bins ? (const int64_t*)ws.in(bins, bins_on_device, sizeof(int64_t) * (size_t)n) : nullptr;
    const double* d_sites = (const double*)ws.in(sites, 0, sizeof(double) * 3 * (size_t)nsites);
    int64_t nchunk = 0, total = 0;
    int32_t* d_off = nullptr;
    if (int rc = d_bins ? select_offsets<SEL_NONZERO>(ws, d_bins, n, 0.0, &nchunk, &d_off, &total)
                        : select_offsets<SEL_ALL>(ws, nullptr, n, 0.0, &nchunk, &d_off, &total))
        return rc;
    *count_out = total;
    const int64_t nout = total < capacity ? total : capacity;
    if (nout == 0) return CEG_OK;
    int32_t* d_lin = (int32_t*)ws.out(lin_out, out_on_device, sizeof(int32_t) * (size_t)nout);
    int32_t* d_site = (int32_t*)ws.out(site_out, out_on_device, sizeof(int32_t) * (size_t)nout);
    int8_t* d_ofs = (int8_t*)ws.out(offset_out, out_on_device, 3 * (size_t)nout);
    double* d_dist = (double*)ws.out(dist_out, out_on_device, sizeof(double) * (size_t)nout);
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace");
    NearGeom G{};
    for (int q = 0; q < 9; ++q) G.mat[q] = mat[q];
    G.safemin = safemin;
    G.a = dims[0]; G.b = dims[1]; G.c = dims[2]; G.ns = nsites; G.origin = origin; G.ortho = ortho ? 1 : 0;
    if (d_bins)
        hipLaunchKernelGGL(k_gs_emit<SEL_NONZERO>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_bins, n, 0.0, d_off, nout, d_lin, (double*)nullptr);
    else
        hipLaunchKernelGGL(k_gs_emit<SEL_ALL>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, (const void*)nullptr, n, 0.0, d_off, nout, d_lin,
                           (double*)nullptr);
    hipLaunchKernelGGL(k_gs_nearest, dim3((unsigned)((nout + 255) / 256)), dim3(256), sizeof(double) * 3 * (size_t)nsites, ws.st, G, d_sites, d_lin, nout,
                       d_site, d_ofs, d_dist);
    ws.back(lin_out, out_on_device, d_lin, sizeof(int32_t) * (size_t)nout);
    ws.back(site_out, out_on_device, d_site, sizeof(int32_t) * (size_t)nout);
    ws.back(offset_out, out_on_device, d_ofs, 3 * (size_t)nout);
    ws.back(dist_out, out_on_device, d_dist, sizeof(double) * (size_t)nout);
    if (hipGetLastError() != hipSuccess || ws.failed || hipStreamSynchronize(ws.st) != hipSuccess)      // `sites` was read from the host
        return gerr(CEG_ERR_HIP, "the nearest-site pass failed");
    return CEG_OK;
}

static int check_sites(const double* sites, int64_t nsites)
{
    for (int64_t q = 0; q < 3 * nsites; ++q)
        if (!(std::fabs(sites[q]) <= 64.0)) {
            char msg[128];
            std::snprintf(msg, sizeof msg, "site %lld: fractional coordinates must be finite with |x| <= 64", (long long)(q / 3));
            return gerr(CEG_ERR_INVALID, msg);
        }
    return CEG_OK;
}

extern "C" int ceg_grid_site_partition(int32_t device, const void* map, int32_t map_is_int64, int32_t map_on_device, double scale,
                                       const int32_t dims[3], const double mat[9], int32_t ortho, double safemin, const double* sites,
                                       int32_t nsites, int32_t origin, double* sums_out, double* centres_out, int32_t out_on_device,
                                       int32_t* cap_bound_out, int64_t* count_out, void* stream)
{
    int64_t n = 0;
    if (!map || !mat || !sites || !sums_out || !centres_out || !cap_bound_out || !count_out || safemin != safemin)
        return gerr(CEG_ERR_INVALID, "bad argument");
    if (map_is_int64 && !std::isfinite(scale)) return gerr(CEG_ERR_INVALID, "scale must be a finite number");
    if (origin != 0 && origin != 1) return gerr(CEG_ERR_INVALID, "origin is 0 or 1");
    if (nsites < 1) return gerr(CEG_ERR_INVALID, "at least one site");
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(mat[q])) return gerr(CEG_ERR_INVALID, "mat must be finite");
    if (int rc = check_sites(sites, nsites)) return rc;
    if (int rc = check_dims(dims, &n)) return rc;
    if (int rc = check_device(device)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return gerr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const void* d_map = ws.in(map, map_on_device, 8 * (size_t)n);
    const double* d_sites = (const double*)ws.in(sites, 0, sizeof(double) * 3 * (size_t)nsites);
    int64_t nchunk = 0, total = 0;
    int32_t* d_off = nullptr;
    if (int rc = map_is_int64 ? select_offsets<SEL_VALUE_BINS>(ws, d_map, n, scale, &nchunk, &d_off, &total)
                              : select_offsets<SEL_VALUE_F64>(ws, d_map, n, 0.0, &nchunk, &d_off, &total))
        return rc;
    *count_out = total;
    const size_t m = (size_t)(total ? total : 1);
    int32_t* d_lin = (int32_t*)ws.get(sizeof(int32_t) * m);
    int32_t* d_site = (int32_t*)ws.get(sizeof(int32_t) * m);
    int32_t* d_site2 = (int32_t*)ws.get(sizeof(int32_t) * m);
    int32_t* d_ord = (int32_t*)ws.get(sizeof(int32_t) * m);
    int32_t* d_ord2 = (int32_t*)ws.get(sizeof(int32_t) * m);
    int8_t* d_ofs = (int8_t*)ws.get(3 * m);
    int32_t* d_runs = (int32_t*)ws.get(sizeof(int32_t) * (2 * (size_t)nsites + 2));      // first[ns], last[ns], cap flag, bad-bin flag
    int32_t* d_flags = d_runs ? d_runs + 2 * (size_t)nsites : nullptr;
    double* d_sums = (double*)ws.out(sums_out, out_on_device, sizeof(double) * (size_t)nsites);
    double* d_cen = (double*)ws.out(centres_out, out_on_device, sizeof(double) * 3 * (size_t)nsites);
    int bits = 1;
    while (bits < 31 && (1ll << bits) < (int64_t)nsites) ++bits;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_site, d_site2, d_ord, d_ord2, (int)total, 0, bits, ws.st);
    void* d_tmp = ws.get(tmp_bytes);
    if (ws.failed) return gerr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    if (hipMemsetAsync(d_runs, 0, sizeof(int32_t) * (2 * (size_t)nsites + 2), ws.st) != hipSuccess) return gerr(CEG_ERR_HIP, "hipMemsetAsync failed");
    if (total > 0) {
        NearGeom G{};
        for (int q = 0; q < 9; ++q) G.mat[q] = mat[q];
        G.safemin = safemin;
        G.a = dims[0]; G.b = dims[1]; G.c = dims[2]; G.ns = nsites; G.origin = origin; G.ortho = ortho ? 1 : 0;
        const unsigned nb = (unsigned)((total + 255) / 256);
        if (map_is_int64)
            hipLaunchKernelGGL(k_gs_emit<SEL_VALUE_BINS>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_map, n, scale, d_off, total, d_lin, (double*)nullptr);
        else
            hipLaunchKernelGGL(k_gs_emit<SEL_VALUE_F64>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_map, n, 0.0, d_off, total, d_lin, (double*)nullptr);
        hipLaunchKernelGGL(k_gs_nearest_tiled, dim3(nb), dim3(256), 0, ws.st, G, d_sites, d_lin, total, d_site, d_ofs);
        hipLaunchKernelGGL(k_gs_iota, dim3(nb), dim3(256), 0, ws.st, d_ord, total);
        // least-significant-digit radix sort: stable, so the voxels of a site keep their linear-index order
        if (hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_site, d_site2, d_ord, d_ord2, (int)total, 0, bits, ws.st) != hipSuccess)
            return gerr(CEG_ERR_HIP, "the radix sort failed");
        hipLaunchKernelGGL(k_gs_site_runs, dim3(nb), dim3(256), 0, ws.st, d_site2, total, d_runs, d_runs + nsites);
    }
    const unsigned nbs = (unsigned)((nsites + 255) / 256);
    if (map_is_int64)
        hipLaunchKernelGGL(k_gs_site_sums<int64_t>, dim3(nbs), dim3(256), 0, ws.st, (const int64_t*)d_map, scale, dims[0], dims[1], dims[2], nsites, d_runs,
                           d_runs + nsites, d_ord2, d_lin, d_ofs, d_sums, d_cen, d_flags);
    else
        hipLaunchKernelGGL(k_gs_site_sums<double>, dim3(nbs), dim3(256), 0, ws.st, (const double*)d_map, scale, dims[0], dims[1], dims[2], nsites, d_runs,
                           d_runs + nsites, d_ord2, d_lin, d_ofs, d_sums, d_cen, d_flags);
    int32_t flags[2] = {0, 0};
    ws.back(sums_out, out_on_device, d_sums, sizeof(double) * (size_t)nsites);
    ws.back(centres_out, out_on_device, d_cen, sizeof(double) * 3 * (size_t)nsites);
    if (hipGetLastError() != hipSuccess || ws.failed || hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)                                   // `sites` was read from the host
        return gerr(CEG_ERR_HIP, "the site partition failed");
    if (flags[1]) return gerr(CEG_ERR_INVALID, "a bin with |value| >= 2^53: its conversion to FP64 would round (the output is not to be used)");
    *cap_bound_out = flags[0] ? 1 : 0;
    return CEG_OK;
}

extern "C" int ceg_coalesce_ranked(const int32_t* lin, const double* smoothed, const double* values, int64_t nranked, const int32_t dims[3],
                                   const double mat[9], int32_t ortho, double safemin, double maxdist, double atol, double maxbasins,
                                   double* value_out, double* centre_out, int64_t capacity, int64_t* count_out)
{
    int64_t n = 0;
    if (nranked < 0 || (nranked > 0 && (!lin || !smoothed || !values)) || !mat || !count_out || capacity < 0 ||
        (capacity > 0 && (!value_out || !centre_out)) || maxdist != maxdist || atol != atol || maxbasins != maxbasins || safemin != safemin)
        return gerr(CEG_ERR_INVALID, "bad argument");
    if (int rc = check_dims(dims, &n)) return rc;
    for (int64_t r = 0; r < nranked; ++r)
        if (lin[r] < 0 || lin[r] >= n) return gerr(CEG_ERR_INVALID, "a ranked index is outside the grid");
    const std::vector<CegBasin> ret = ceg_coalesce_greedy(lin, smoothed, values, nranked, dims, mat, ortho != 0, safemin, maxdist, atol, maxbasins);
    *count_out = (int64_t)ret.size();
    for (int64_t q = 0; q < (int64_t)ret.size() && q < capacity; ++q) {
        value_out[q] = ret[(size_t)q].val;
        for (int r = 0; r < 3; ++r) centre_out[3 * q + r] = ret[(size_t)q].c[r];
    }
    return CEG_OK;
}
