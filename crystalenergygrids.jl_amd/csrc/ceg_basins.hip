// ceg_basins.hip -- grid analysis on the device (src/basins.jl of the reference):
//   local_minima            basins.jl:40-99     k_bas_minima_flags: one pass, the 3x3x3 cube of a point served from an LDS tile with
//                                               a periodic halo; flags compacted in linear-index order (chunk counts, hipcub exclusive
//                                               scan, emit), so the list is Julia's sort! of the CartesianIndex list
//   local_components        basins.jl:279-313   union-find over a parent array int32[a*b*c]: every active point is united with its
//   compute_levels          basins.jl:842-869   +i, +j, +k periodic neighbours, the larger root always hung under the smaller one
//                                               (atomicMin, retried until it holds).  parent[x] <= x throughout, so the final root is
//                                               the component's smallest linear index whatever the arrival order of the waves; the
//                                               rank of a component = the rank of its root among the roots (same compaction)
//   site_proximity_map!     basins.jl:466-578   a gather: one thread per point, sites in LDS (see the header for why one cell offset
//   closest_from_proximity  basins.jl:580-597   per site is enough); per-site int64 sums through integer atomics
// Sizes, int64 sums and the site sums combine runs of equal labels inside a wave before the atomic (a grid row is a run of lanes), so
// one large component is not a*b*c atomics on one address.  No float atomics anywhere: the only FP64 reduction (the extremum of the
// kept minima) goes through per-workgroup partials.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/ceg_hip.h"

extern "C" void ceg_set_last_error_(const char* msg);

// the FP64 expressions of this file are the reference's, operation by operation (threshold :92, distances :526-528): no contraction
#pragma clang fp contract(off)

namespace {

int berr(int code, const char* msg)
{
    ceg_set_last_error_(msg);
    return code;
}

constexpr int TX = 32, TY = 8, TZ = 8;                      // points of a tile of k_bas_minima_flags (256 threads, TZ points each)
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;        // with the halo: 3400 doubles = 27 200 B of LDS
constexpr int CHUNK = 2048;                                  // flags of one workgroup of the compaction kernels (8 per thread)

__device__ __forceinline__ int pmod(int x, int n)
{
    x %= n;
    return x < 0 ? x + n : x;
}

// flag[x] = 1 iff lt(val, neighbour) for all 26 periodic neighbours (:50-83); per workgroup the smallest kept value and the count
__global__ __launch_bounds__(256) void k_bas_minima_flags(const double* __restrict__ g, int a, int b, int c, int ntx, int nty, int maxima,
                                                          uint8_t* __restrict__ flag, double* __restrict__ blockmin,
                                                          int32_t* __restrict__ blockcnt)
{
    __shared__ double tile[HZ * HY * HX];
    __shared__ double s_min[4];
    __shared__ int s_cnt[4];
    const int bt = (int)blockIdx.x;
    const int i0 = (bt % ntx) * TX, j0 = ((bt / ntx) % nty) * TY, k0 = (bt / (ntx * nty)) * TZ;
    for (int idx = (int)threadIdx.x; idx < HZ * HY * HX; idx += 256) {
        const int lx = idx % HX, r = idx / HX, ly = r % HY, lz = r / HY;
        const int gi = pmod(i0 + lx - 1, a), gj = pmod(j0 + ly - 1, b), gk = pmod(k0 + lz - 1, c);      // mod1 of :51-73
        tile[idx] = g[(int64_t)gi + (int64_t)a * ((int64_t)gj + (int64_t)b * gk)];
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & (TX - 1), ly = (int)threadIdx.x / TX;
    const int i = i0 + lx, j = j0 + ly;
    double mymin = INFINITY;
    int mycnt = 0;
    if (i < a && j < b) {
        for (int kk = 0; kk < TZ && k0 + kk < c; ++kk) {
            const double val = tile[((kk + 1) * HY + ly + 1) * HX + lx + 1];
            bool ok = true;
#pragma unroll
            for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        if (dz == 1 && dy == 1 && dx == 1) continue;
                        const double n = tile[((kk + dz) * HY + ly + dy) * HX + lx + dx];
                        ok = ok && (maxima ? val > n : val < n);                                       // strict; a NaN fails it
                    }
            flag[(int64_t)i + (int64_t)a * ((int64_t)j + (int64_t)b * (k0 + kk))] = ok ? 1 : 0;
            if (ok) {
                mymin = fmin(mymin, val);                                                              // `minimum` for both lt (:89)
                ++mycnt;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        mymin = fmin(mymin, __shfl_xor(mymin, d));
        mycnt += __shfl_xor(mycnt, d);
    }
    if ((threadIdx.x & 63) == 0) {
        s_min[threadIdx.x >> 6] = mymin;
        s_cnt[threadIdx.x >> 6] = mycnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blockmin[bt] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
        blockcnt[bt] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

struct MinimaHead {
    double extremum;
    int64_t kept;
};

__global__ __launch_bounds__(256) void k_bas_minima_head(const double* __restrict__ blockmin, const int32_t* __restrict__ blockcnt, int nb,
                                                         MinimaHead* __restrict__ head)
{
    using RedD = hipcub::BlockReduce<double, 256>;
    using RedI = hipcub::BlockReduce<long long, 256>;
    __shared__ typename RedD::TempStorage sd;
    __shared__ typename RedI::TempStorage si;
    double m = INFINITY;
    long long n = 0;
    for (int t = (int)threadIdx.x; t < nb; t += 256) {
        m = fmin(m, blockmin[t]);
        n += blockcnt[t];
    }
    m = RedD(sd).Reduce(m, hipcub::Min());
    n = RedI(si).Sum(n);
    if (threadIdx.x == 0) {
        head->extremum = m;
        head->kept = n;
    }
}

// flags are bytes 0 / 1, eight per thread; with use_thr the kept points with grid > threshold are cleared (:94-97)
__global__ __launch_bounds__(256) void k_bas_chunk_count(uint8_t* __restrict__ flag, const double* __restrict__ g, int use_thr, double thr,
                                                         int32_t* __restrict__ chunkcnt)
{
    using Red = hipcub::BlockReduce<int, 256>;
    __shared__ typename Red::TempStorage tmp;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t w = reinterpret_cast<const uint64_t*>(flag)[t];
    if (use_thr && w) {
        for (int q = 0; q < 8; ++q)
            if (((w >> (8 * q)) & 1) && g[t * 8 + q] > thr) w &= ~(1ull << (8 * q));
        reinterpret_cast<uint64_t*>(flag)[t] = w;
    }
    const int n = Red(tmp).Sum(__popcll(w));
    if (threadIdx.x == 0) chunkcnt[blockIdx.x] = n;
}

// MODE 0: (i, j, k) of the flagged points;  MODE 1: the flagged points are roots: their index (seed) and rankof[root] = rank
template <int MODE>
__global__ __launch_bounds__(256) void k_bas_emit(const uint8_t* __restrict__ flag, const int32_t* __restrict__ chunkoff, int a, int b,
                                                  int64_t cap, int32_t* __restrict__ out, int32_t* __restrict__ rankof)
{
    using Scan = hipcub::BlockScan<int, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t w = reinterpret_cast<const uint64_t*>(flag)[t];
    int pre = 0;
    Scan(tmp).ExclusiveSum(__popcll(w), pre);
    int64_t pos = (int64_t)chunkoff[blockIdx.x] + pre;
    for (int q = 0; q < 8; ++q) {
        if (!((w >> (8 * q)) & 1)) continue;
        const int64_t lin = t * 8 + q;
        if (MODE == 0) {
            if (pos < cap) {
                out[3 * pos] = (int32_t)(lin % a);
                out[3 * pos + 1] = (int32_t)((lin / a) % b);
                out[3 * pos + 2] = (int32_t)(lin / ((int64_t)a * b));
            }
        } else {
            rankof[lin] = (int32_t)pos;
            if (out && pos < cap) out[pos] = (int32_t)lin;
        }
        ++pos;
    }
}

// ---- components -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t pload(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; a parent two or more links above its root is pulled one link up (atomicMin: a parent only ever decreases, and only
// to a point of the same component)
__device__ __forceinline__ int32_t find_root(int32_t* P, int32_t x)
{
    int32_t p = pload(P + x);
    while (p != x) {
        const int32_t gp = pload(P + p);
        if (gp != p) atomicMin(P + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t* P, int32_t x, int32_t y)
{
    bool done = false;
    while (!done) {
        x = find_root(P, x);
        y = find_root(P, y);
        if (x == y) return;
        if (x > y) {
            const int32_t t = x;
            x = y;
            y = t;
        }
        const int32_t old = atomicMin(P + y, x);      // y was a root iff old == y; else another wave hung it meanwhile: go on from there
        done = old == y;
        y = old;
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_bas_cc_init(const T* __restrict__ g, int64_t n, double lo, double hi, int32_t* __restrict__ P)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const T v = g[x];
    const bool active = MODE == CEG_COMPONENTS_NONZERO ? v != (T)0 : ((double)v > lo && (double)v < hi);
    P[x] = active ? (int32_t)x : -1;
}

__global__ __launch_bounds__(256) void k_bas_cc_union(int32_t* __restrict__ P, int a, int b, int c)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= (int64_t)a * b * c) return;
    if (pload(P + x) < 0) return;
    const int i = (int)(x % a), j = (int)((x / a) % b), k = (int)(x / ((int64_t)a * b));
    const int64_t y0 = (i + 1 == a ? 0 : i + 1) + (int64_t)a * (j + (int64_t)b * k);
    const int64_t y1 = i + (int64_t)a * ((j + 1 == b ? 0 : j + 1) + (int64_t)b * k);
    const int64_t y2 = i + (int64_t)a * (j + (int64_t)b * (k + 1 == c ? 0 : k + 1));
    if (y0 != x && pload(P + y0) >= 0) unite(P, (int32_t)x, (int32_t)y0);
    if (y1 != x && pload(P + y1) >= 0) unite(P, (int32_t)x, (int32_t)y1);
    if (y2 != x && pload(P + y2) >= 0) unite(P, (int32_t)x, (int32_t)y2);
}

// after the unions: parent[x] = root, flag[x] = is a root
__global__ __launch_bounds__(256) void k_bas_cc_flatten(int32_t* __restrict__ P, int64_t n, uint8_t* __restrict__ flag)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    int32_t p = pload(P + x);
    if (p < 0) {
        flag[x] = 0;
        return;
    }
    int32_t r = (int32_t)x;
    while (p != r) {
        r = p;
        p = pload(P + r);
    }
    P[x] = r;                     // a reader that still sees the old parent reaches the same root
    flag[x] = r == (int32_t)x ? 1 : 0;
}

// Inclusive sums of v over the run of equal labels that ends at this lane, inside the wave; tail = last lane of its run.  Every lane
// of the wave takes part.
template <int NV>
__device__ __forceinline__ bool wave_run_sums(int label, long long (&v)[NV])
{
    const int lane = (int)threadIdx.x & 63;
    const int prev = __shfl_up(label, 1), next = __shfl_down(label, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != label);
    const int headlane = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const long long o = __shfl_up(v[q], d);
            if (lane - d >= headlane) v[q] += o;
        }
    }
    return lane == 63 || next != label;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bas_cc_labels(const T* __restrict__ g, const int32_t* __restrict__ P, const int32_t* __restrict__ rankof,
                                                       int64_t n, int64_t cap, int32_t* __restrict__ labels, int32_t* __restrict__ size,
                                                       int64_t* __restrict__ sum)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    long long v[2] = {0, 0};
    if (x < n) {
        const int32_t p = P[x];
        if (p >= 0) {
            lab = rankof[p];
            v[0] = 1;
            if (sizeof(T) == sizeof(int64_t) && sum) v[1] = (long long)g[x];
        }
        if (labels) labels[x] = lab;
    }
    const bool tail = wave_run_sums<2>(lab, v);
    if (tail && lab >= 0 && lab < cap) {
        if (size) atomicAdd(size + lab, (int32_t)v[0]);
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(sum) + lab, (unsigned long long)v[1]);
    }
}

// ---- sites ------------------------------------------------------------------------------------------------------------------------
struct ProxGeom {
    double mat[9];
    double maxdist2;
    int32_t a, b, c, ns;
};

__device__ __forceinline__ int nearest_cell(double f)      // the one offset in {-1, 0, 1} that can bring the site within half a cell
{
    const double r = rint(f);
    return r < -1.0 ? -1 : (r > 1.0 ? 1 : (int)r);
}

__global__ __launch_bounds__(256) void k_bas_proximity(ProxGeom G, const double* __restrict__ sites, int32_t* __restrict__ site_out,
                                                       int8_t* __restrict__ off_out)
{
    extern __shared__ double s_sites[];
    for (int t = (int)threadIdx.x; t < 3 * G.ns; t += 256) s_sites[t] = sites[t];
    __syncthreads();
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= (int64_t)G.a * G.b * G.c) return;
    const int i = (int)(x % G.a), j = (int)((x / G.a) % G.b), k = (int)(x / ((int64_t)G.a * G.b));
    // (J .- 1) ./ dims of :526 for the three cells an axis can take: J - 1 = w + o*dims
    const double xm = (double)(i - G.a) / G.a, x0 = (double)i / G.a, xp = (double)(i + G.a) / G.a;
    const double ym = (double)(j - G.b) / G.b, y0 = (double)j / G.b, yp = (double)(j + G.b) / G.b;
    const double zm = (double)(k - G.c) / G.c, z0 = (double)k / G.c, zp = (double)(k + G.c) / G.c;
    int best = 0, bx = 0, by = 0, bz = 0;
    double bestd2 = INFINITY;
    for (int s = 0; s < G.ns; ++s) {
        const double fx = s_sites[3 * s], fy = s_sites[3 * s + 1], fz = s_sites[3 * s + 2];
        const int ox = nearest_cell(fx - x0), oy = nearest_cell(fy - y0), oz = nearest_cell(fz - z0);
        const double vx = fx - (ox < 0 ? xm : (ox > 0 ? xp : x0));
        const double vy = fy - (oy < 0 ? ym : (oy > 0 ? yp : y0));
        const double vz = fz - (oz < 0 ? zm : (oz > 0 ? zp : z0));
        const double dx = G.mat[0] * vx + G.mat[3] * vy + G.mat[6] * vz;
        const double dy = G.mat[1] * vx + G.mat[4] * vy + G.mat[7] * vz;
        const double dz = G.mat[2] * vx + G.mat[5] * vy + G.mat[8] * vz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < bestd2) {                       // strict: the lowest site index wins among equals
            bestd2 = d2;
            best = s + 1;
            bx = ox; by = oy; bz = oz;
        }
    }
    const bool in = best > 0 && bestd2 < G.maxdist2;
    site_out[x] = in ? best : 0;
    off_out[3 * x] = (int8_t)(in ? bx : 0);
    off_out[3 * x + 1] = (int8_t)(in ? by : 0);
    off_out[3 * x + 2] = (int8_t)(in ? bz : 0);
}

__global__ __launch_bounds__(256) void k_bas_site_density(const int64_t* __restrict__ bins, const int32_t* __restrict__ site,
                                                          const int8_t* __restrict__ off, int a, int b, int c, int ns,
                                                          int64_t* __restrict__ rho, int64_t* __restrict__ moment)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    long long v[4] = {0, 0, 0, 0};
    if (x < (int64_t)a * b * c) {
        const int32_t s = site[x];
        if (s >= 0 && s <= ns) {                 // anything else is not a site of this map: ignored
            lab = s == 0 ? ns : s - 1;
            const long long val = bins[x];
            const int i = (int)(x % a), j = (int)((x / a) % b), k = (int)(x / ((int64_t)a * b));
            v[0] = val;
            v[1] = val * ((long long)off[3 * x] * a + i);
            v[2] = val * ((long long)off[3 * x + 1] * b + j);
            v[3] = val * ((long long)off[3 * x + 2] * c + k);
        }
    }
    const bool tail = wave_run_sums<4>(lab, v);
    if (tail && lab >= 0 && (v[0] | v[1] | v[2] | v[3])) {
        atomicAdd(reinterpret_cast<unsigned long long*>(rho) + lab, (unsigned long long)v[0]);
        for (int q = 0; q < 3; ++q) atomicAdd(reinterpret_cast<unsigned long long*>(moment) + 3 * lab + q, (unsigned long long)v[1 + q]);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct DevGuard {
    int prev = -1;
    bool ok = false;
    explicit DevGuard(int d)
    {
        (void)hipGetDevice(&prev);
        ok = hipSetDevice(d) == hipSuccess;
    }
    ~DevGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// stream-ordered workspace of one call: everything it handed out is freed behind the call's last launch
struct Workspace {
    hipStream_t st;
    std::vector<void*> held;
    bool failed = false;
    bool staged = false;          // an input came from host memory: the call synchronises before it returns
    explicit Workspace(hipStream_t s) : st(s) {}
    ~Workspace()
    {
        for (void* p : held) (void)hipFreeAsync(p, st);
    }
    void* get(size_t bytes)
    {
        void* p = nullptr;
        if (hipMallocAsync(&p, bytes ? bytes : 1, st) != hipSuccess) {
            failed = true;
            return nullptr;
        }
        held.push_back(p);
        return p;
    }
    // the device address of an input: itself, or a copy of the host array
    const void* in(const void* src, int on_device, size_t bytes)
    {
        if (on_device) return src;
        staged = true;
        void* p = get(bytes);
        if (p && bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) failed = true;
        return p;
    }
    // where the kernels write an output: itself, or a device buffer that back() copies to the host
    void* out(void* dst, int on_device, size_t bytes) { return (on_device || !dst) ? dst : get(bytes); }
    void back(void* dst, int on_device, const void* dev, size_t bytes)
    {
        if (dst && !on_device && bytes && hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) failed = true;
    }
};

int check_grid(int32_t device, const int32_t* dims, int64_t* n)
{
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return berr(CEG_ERR_INVALID, "dims must be three positive numbers");
    const int64_t ab = (int64_t)dims[0] * dims[1];
    if (ab > std::numeric_limits<int32_t>::max() || ab * dims[2] > std::numeric_limits<int32_t>::max())
        return berr(CEG_ERR_INVALID, "a*b*c does not fit int32");
    *n = ab * dims[2];
    if (ceg_device_count() <= 0) return berr(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ceg_device_count()) return berr(CEG_ERR_NO_DEVICE, "device not present");
    return CEG_OK;
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// chunk counts of flag[nchunk*CHUNK] -> exclusive offsets and the total (synchronises `st`)
int compact_offsets(Workspace& ws, uint8_t* d_flag, const double* d_grid, int use_thr, double thr, int64_t nchunk, int32_t** d_off, int64_t* total)
{
    int32_t* d_cnt = (int32_t*)ws.get(sizeof(int32_t) * (size_t)(nchunk + 1));
    *d_off = (int32_t*)ws.get(sizeof(int32_t) * (size_t)(nchunk + 1));
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt, *d_off, (int)(nchunk + 1), ws.st);
    void* d_tmp = ws.get(tmp_bytes);
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace");
    int32_t last = 0;
    if (hipMemsetAsync(d_cnt + nchunk, 0, sizeof(int32_t), ws.st) != hipSuccess) return berr(CEG_ERR_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_bas_chunk_count, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_flag, d_grid, use_thr, thr, d_cnt);
    if (hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, *d_off, (int)(nchunk + 1), ws.st) != hipSuccess ||
        hipMemcpyAsync(&last, *d_off + nchunk, sizeof(int32_t), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return berr(CEG_ERR_HIP, "the compaction of the flags failed");
    *total = last;
    return CEG_OK;
}

// flag array of n points padded to whole chunks, the padding zeroed
uint8_t* flag_array(Workspace& ws, int64_t n, int64_t* nchunk)
{
    *nchunk = (n + CHUNK - 1) / CHUNK;
    uint8_t* f = (uint8_t*)ws.get((size_t)(*nchunk * CHUNK));
    if (f && *nchunk * CHUNK > n && hipMemsetAsync(f + n, 0, (size_t)(*nchunk * CHUNK - n), ws.st) != hipSuccess) ws.failed = true;
    return f;
}

}  // namespace

extern "C" int ceg_grid_local_minima(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], int32_t maxima,
                                     double tolerance, int32_t* ijk_out, int32_t ijk_on_device, int64_t capacity, int64_t* count_out,
                                     double* extremum_out, void* stream)
{
    int64_t n = 0;
    if (!grid || !count_out || capacity < 0 || (capacity > 0 && !ijk_out) || (maxima != 0 && maxima != 1) || tolerance != tolerance)
        return berr(CEG_ERR_INVALID, "bad argument");
    if (int rc = check_grid(device, dims, &n)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return berr(CEG_ERR_HIP, "hipSetDevice failed");
    const int a = dims[0], b = dims[1], c = dims[2];
    const int ntx = (a + TX - 1) / TX, nty = (b + TY - 1) / TY, ntz = (c + TZ - 1) / TZ;
    const int64_t nb = (int64_t)ntx * nty * ntz;
    Workspace ws((hipStream_t)stream);
    const double* d_g = (const double*)ws.in(grid, grid_on_device, sizeof(double) * (size_t)n);
    int64_t nchunk = 0;
    uint8_t* d_flag = flag_array(ws, n, &nchunk);
    double* d_bmin = (double*)ws.get(sizeof(double) * (size_t)nb);
    int32_t* d_bcnt = (int32_t*)ws.get(sizeof(int32_t) * (size_t)nb);
    MinimaHead* d_head = (MinimaHead*)ws.get(sizeof(MinimaHead));
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace / upload the grid");
    hipLaunchKernelGGL(k_bas_minima_flags, dim3((unsigned)nb), dim3(256), 0, ws.st, d_g, a, b, c, ntx, nty, maxima, d_flag, d_bmin, d_bcnt);
    hipLaunchKernelGGL(k_bas_minima_head, dim3(1), dim3(256), 0, ws.st, d_bmin, d_bcnt, (int)nb, d_head);
    MinimaHead head{};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&head, d_head, sizeof(head), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
        hipStreamSynchronize(ws.st) != hipSuccess)
        return berr(CEG_ERR_HIP, "the scan for local extrema failed");
    *count_out = 0;
    if (extremum_out) *extremum_out = head.extremum;
    if (head.kept == 0) return CEG_OK;                       // the reference throws on the empty minimum (:89)
    double thr = 0.0;
    if (tolerance >= 0) {
        if (!(head.extremum < 0)) return berr(CEG_ERR_INVALID, "tolerance >= 0 needs a negative extremum (basins.jl:91)");
        const double prod = head.extremum * tolerance;
        thr = head.extremum + std::fabs(prod);               // :92
    }
    int32_t* d_off = nullptr;
    int64_t total = 0;
    if (int rc = compact_offsets(ws, d_flag, d_g, tolerance >= 0, thr, nchunk, &d_off, &total)) return rc;
    *count_out = total;
    const int64_t nout = total < capacity ? total : capacity;
    if (nout == 0) return CEG_OK;
    int32_t* d_ijk = (int32_t*)ws.out(ijk_out, ijk_on_device, sizeof(int32_t) * 3 * (size_t)nout);
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace");
    hipLaunchKernelGGL(k_bas_emit<0>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_flag, d_off, a, b, nout, d_ijk, (int32_t*)nullptr);
    ws.back(ijk_out, ijk_on_device, d_ijk, sizeof(int32_t) * 3 * (size_t)nout);
    if (hipGetLastError() != hipSuccess || ws.failed || (!ijk_on_device && hipStreamSynchronize(ws.st) != hipSuccess))
        return berr(CEG_ERR_HIP, "the emit of the local extrema failed");
    return CEG_OK;
}

template <typename T>
static int components_run(Workspace& ws, const T* d_g, int64_t n, const int32_t dims[3], int32_t mode, double lo, double hi, int32_t* labels_out,
                          int32_t labels_on_device, int32_t* seed_out, int32_t* size_out, int64_t* sum_out, int32_t lists_on_device,
                          int64_t capacity, int64_t* count_out)
{
    int64_t nchunk = 0;
    uint8_t* d_flag = flag_array(ws, n, &nchunk);
    int32_t* d_parent = (int32_t*)ws.get(sizeof(int32_t) * (size_t)n);
    int32_t* d_rankof = (int32_t*)ws.get(sizeof(int32_t) * (size_t)n);
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace / upload the grid");
    const unsigned nb = blocks256(n);
    if (mode == CEG_COMPONENTS_NONZERO)
        hipLaunchKernelGGL((k_bas_cc_init<T, CEG_COMPONENTS_NONZERO>), dim3(nb), dim3(256), 0, ws.st, d_g, n, lo, hi, d_parent);
    else
        hipLaunchKernelGGL((k_bas_cc_init<T, CEG_COMPONENTS_BAND>), dim3(nb), dim3(256), 0, ws.st, d_g, n, lo, hi, d_parent);
    hipLaunchKernelGGL(k_bas_cc_union, dim3(nb), dim3(256), 0, ws.st, d_parent, dims[0], dims[1], dims[2]);
    hipLaunchKernelGGL(k_bas_cc_flatten, dim3(nb), dim3(256), 0, ws.st, d_parent, n, d_flag);
    if (hipGetLastError() != hipSuccess) return berr(CEG_ERR_HIP, "the union-find launches failed");
    int32_t* d_off = nullptr;
    int64_t total = 0;
    if (int rc = compact_offsets(ws, d_flag, nullptr, 0, 0.0, nchunk, &d_off, &total)) return rc;
    *count_out = total;
    const int64_t nout = total < capacity ? total : capacity;
    const bool lists = nout > 0 && (seed_out || size_out || sum_out);
    if (!labels_out && !lists) return CEG_OK;
    int32_t* d_labels = (int32_t*)ws.out(labels_out, labels_on_device, sizeof(int32_t) * (size_t)n);
    int32_t* d_seed = lists ? (int32_t*)ws.out(seed_out, lists_on_device, sizeof(int32_t) * (size_t)nout) : nullptr;
    int32_t* d_size = lists ? (int32_t*)ws.out(size_out, lists_on_device, sizeof(int32_t) * (size_t)nout) : nullptr;
    int64_t* d_sum = lists ? (int64_t*)ws.out(sum_out, lists_on_device, sizeof(int64_t) * (size_t)nout) : nullptr;
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace");
    if ((d_size && hipMemsetAsync(d_size, 0, sizeof(int32_t) * (size_t)nout, ws.st) != hipSuccess) ||
        (d_sum && hipMemsetAsync(d_sum, 0, sizeof(int64_t) * (size_t)nout, ws.st) != hipSuccess))
        return berr(CEG_ERR_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_bas_emit<1>, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_flag, d_off, dims[0], dims[1], nout, d_seed, d_rankof);
    hipLaunchKernelGGL(k_bas_cc_labels<T>, dim3(nb), dim3(256), 0, ws.st, d_g, d_parent, d_rankof, n, nout, d_labels, d_size, d_sum);
    ws.back(labels_out, labels_on_device, d_labels, sizeof(int32_t) * (size_t)n);
    if (lists) {
        ws.back(seed_out, lists_on_device, d_seed, sizeof(int32_t) * (size_t)nout);
        ws.back(size_out, lists_on_device, d_size, sizeof(int32_t) * (size_t)nout);
        ws.back(sum_out, lists_on_device, d_sum, sizeof(int64_t) * (size_t)nout);
    }
    const bool host_out = (labels_out && !labels_on_device) || (lists && !lists_on_device);
    if (hipGetLastError() != hipSuccess || ws.failed || (host_out && hipStreamSynchronize(ws.st) != hipSuccess))
        return berr(CEG_ERR_HIP, "the labelling of the components failed");
    return CEG_OK;
}

extern "C" int ceg_grid_components(int32_t device, const void* grid, int32_t grid_is_int64, int32_t grid_on_device, const int32_t dims[3],
                                   int32_t mode, double lo, double hi, int32_t* labels_out, int32_t labels_on_device, int32_t* seed_out,
                                   int32_t* size_out, int64_t* sum_out, int32_t lists_on_device, int64_t capacity, int64_t* count_out,
                                   void* stream)
{
    int64_t n = 0;
    if (!grid || !count_out || capacity < 0 || (mode != CEG_COMPONENTS_NONZERO && mode != CEG_COMPONENTS_BAND))
        return berr(CEG_ERR_INVALID, "bad argument");
    if (mode == CEG_COMPONENTS_BAND && (grid_is_int64 || lo != lo || hi != hi))
        return berr(CEG_ERR_INVALID, "the band mode takes an FP64 grid and two bounds that are numbers");
    if (!grid_is_int64 && sum_out) return berr(CEG_ERR_INVALID, "sum_out is for an int64 grid only");
    if (int rc = check_grid(device, dims, &n)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return berr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const void* d_g = ws.in(grid, grid_on_device, 8 * (size_t)n);
    if (grid_is_int64)
        return components_run<int64_t>(ws, (const int64_t*)d_g, n, dims, mode, lo, hi, labels_out, labels_on_device, seed_out, size_out, sum_out,
                                       lists_on_device, capacity, count_out);
    return components_run<double>(ws, (const double*)d_g, n, dims, mode, lo, hi, labels_out, labels_on_device, seed_out, size_out, nullptr,
                                  lists_on_device, capacity, count_out);
}

extern "C" int ceg_grid_site_proximity(int32_t device, const int32_t dims[3], const double mat[9], const double* sites, int32_t nsites,
                                       double maxdist, int32_t* site_out, int8_t* offset_out, int32_t out_on_device, void* stream)
{
    int64_t n = 0;
    if (!mat || !site_out || !offset_out || nsites < 0 || (nsites > 0 && !sites) || !(maxdist > 0) || !std::isfinite(maxdist))
        return berr(CEG_ERR_INVALID, "bad argument");
    if (nsites > CEG_SITE_PROXIMITY_MAX_SITES) return berr(CEG_ERR_UNSUPPORTED, "more sites than CEG_SITE_PROXIMITY_MAX_SITES");
    if (dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1) {
        // the smallest perpendicular width of the cell: |det| over the area of the face the two other columns span
        const double* m = mat;
        const double cr[3][3] = {{m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]},
                                 {m[7] * m[2] - m[8] * m[1], m[8] * m[0] - m[6] * m[2], m[6] * m[1] - m[7] * m[0]},
                                 {m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]}};
        const double det = m[0] * cr[0][0] + m[1] * cr[0][1] + m[2] * cr[0][2];
        double width = INFINITY;
        for (int q = 0; q < 3; ++q) width = std::fmin(width, std::fabs(det) / std::sqrt(cr[q][0] * cr[q][0] + cr[q][1] * cr[q][1] + cr[q][2] * cr[q][2]));
        double skin[3];
        for (int r = 0; r < 3; ++r) skin[r] = m[r] / dims[0] + m[3 + r] / dims[1] + m[6 + r] / dims[2];
        const double protoskin = std::sqrt(skin[0] * skin[0] + skin[1] * skin[1] + skin[2] * skin[2]);      // :470
        if (!(std::fabs(det) > 0) || !(2.0 * (maxdist + protoskin) < width))
            return berr(CEG_ERR_INVALID, "maxdist: 2*(maxdist + voxel diagonal) must stay below the smallest width of the cell");
    }
    if (int rc = check_grid(device, dims, &n)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return berr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    ProxGeom G{};
    for (int q = 0; q < 9; ++q) G.mat[q] = mat[q];
    G.maxdist2 = maxdist * maxdist;
    G.a = dims[0]; G.b = dims[1]; G.c = dims[2]; G.ns = nsites;
    const double* d_sites = (const double*)ws.in(sites, 0, sizeof(double) * 3 * (size_t)nsites);
    int32_t* d_site = (int32_t*)ws.out(site_out, out_on_device, sizeof(int32_t) * (size_t)n);
    int8_t* d_off = (int8_t*)ws.out(offset_out, out_on_device, 3 * (size_t)n);
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace");
    hipLaunchKernelGGL(k_bas_proximity, dim3(blocks256(n)), dim3(256), sizeof(double) * 3 * (size_t)nsites, ws.st, G, d_sites, d_site, d_off);
    ws.back(site_out, out_on_device, d_site, sizeof(int32_t) * (size_t)n);
    ws.back(offset_out, out_on_device, d_off, 3 * (size_t)n);
    if (hipGetLastError() != hipSuccess || ws.failed || hipStreamSynchronize(ws.st) != hipSuccess)      // `sites` was read from the host
        return berr(CEG_ERR_HIP, "the proximity map failed");
    return CEG_OK;
}

extern "C" int ceg_grid_site_density(int32_t device, const int64_t* bins, int32_t bins_on_device, const int32_t* site, const int8_t* offset,
                                     int32_t map_on_device, const int32_t dims[3], int32_t nsites, int64_t* rho_out, int64_t* moment_out,
                                     int32_t out_on_device, void* stream)
{
    int64_t n = 0;
    if (!bins || !site || !offset || nsites < 0 || !rho_out || !moment_out) return berr(CEG_ERR_INVALID, "bad argument");
    if (int rc = check_grid(device, dims, &n)) return rc;
    DevGuard guard(device);
    if (!guard.ok) return berr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    const size_t ne = (size_t)nsites + 1;
    const int64_t* d_bins = (const int64_t*)ws.in(bins, bins_on_device, sizeof(int64_t) * (size_t)n);
    const int32_t* d_site = (const int32_t*)ws.in(site, map_on_device, sizeof(int32_t) * (size_t)n);
    const int8_t* d_off = (const int8_t*)ws.in(offset, map_on_device, 3 * (size_t)n);
    int64_t* d_rho = (int64_t*)ws.out(rho_out, out_on_device, sizeof(int64_t) * ne);
    int64_t* d_mom = (int64_t*)ws.out(moment_out, out_on_device, sizeof(int64_t) * 3 * ne);
    if (ws.failed) return berr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    if (hipMemsetAsync(d_rho, 0, sizeof(int64_t) * ne, ws.st) != hipSuccess || hipMemsetAsync(d_mom, 0, sizeof(int64_t) * 3 * ne, ws.st) != hipSuccess)
        return berr(CEG_ERR_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_bas_site_density, dim3(blocks256(n)), dim3(256), 0, ws.st, d_bins, d_site, d_off, dims[0], dims[1], dims[2], nsites, d_rho,
                       d_mom);
    ws.back(rho_out, out_on_device, d_rho, sizeof(int64_t) * ne);
    ws.back(moment_out, out_on_device, d_mom, sizeof(int64_t) * 3 * ne);
    if (hipGetLastError() != hipSuccess || ws.failed || ((!out_on_device || ws.staged) && hipStreamSynchronize(ws.st) != hipSuccess))
        return berr(CEG_ERR_HIP, "the site sums failed");
    return CEG_OK;
}
