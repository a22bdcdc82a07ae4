// ceg_basin_flow.hip -- attraction basins on the device (src/basins.jl of the reference):
//   local_basins      basins.jl:195-252   ceg_grid_basins: ONE levelled pass for all the starts.  u -> v is an edge when v is one of the
//   decompose_basins  basins.jl:765-792   six periodic GridNeighbors of u, lt(grid[u], grid[v]) and !skip(grid[v]); the edges do not
//                                         depend on the start.  The reference keeps x in basin i iff no other basin's breadth-first
// search reached x at an earlier level (keep_shortest_distance!, :140-172), i.e. iff d_i(x) = D(x) = min_i d_i(x): D is the level of one
// multi-source search, and owners(x) = the union of owners(u) over the predecessors u -> x with D(u) = D(x) - 1.
//   levels   k_flow_level, one launch per level, one thread per point of the frontier: the six neighbours are claimed with a
//            compare-and-swap on D and appended to the next frontier.  The claimer and the order inside a frontier show in no output.
//            The frontier's bounds live on the device (a ring of counts), so BATCH levels are launched between two synchronisations.
//   owners   k_flow_owners, one launch per level with its exact size, one thread per point: a pull from the predecessors.  A point
//            with one owner is one int32; a point with 2 .. CEG_BASINS_MAX_OWNERS owners takes that many entries of a pool and keeps
//            -(offset + 2) in place of the owner.  The merge is an insertion network over 16 registers: no indexed array, no scratch.
//   emit     k_flow_finish (owner map, sizes by integer atomics, runs of one owner inside a wave combined first), then the pairs of
//            the multi-owner points in linear-index order: counts per 2048 points, a hipcub exclusive scan, an emit.
// Every output is an integer that does not depend on the arrival order of the waves; no float atomics.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/ceg_hip.h"

extern "C" void ceg_set_last_error_(const char* msg);

namespace {

int ferr(int code, const char* msg)
{
    ceg_set_last_error_(msg);
    return code;
}

constexpr int MAXOWN = CEG_BASINS_MAX_OWNERS;
constexpr int CHUNK = 2048;                      // points of one workgroup of the compaction kernels (8 per thread)
constexpr int RING = 64;                         // level counts kept on the device
constexpr int BATCH = 16;                        // levels launched between two synchronisations (BATCH + 3 <= RING)
constexpr int LEVEL_BLOCKS = 1024;               // k_flow_level strides over its frontier: the size is not known to the host
constexpr int FINISH_BLOCKS = 512;                // workgroups of k_flow_finish when the sizes are counted in LDS first ...
constexpr int FINISH_LOCAL_MAX = 8192;           // ... which they are up to this many starts (32 KiB of LDS)
constexpr int32_t NONE = std::numeric_limits<int32_t>::max();
constexpr int32_t FILL = 0x7f7f7f7f;             // what a byte fill of 0x7f leaves: above every start index

struct FlowGeom {
    double skip_above;
    int32_t a, b, c, maxima;
};

struct LevelState {
    int32_t bad_range;                           // smallest start index out of range, FILL if none
    int32_t bad_dup;                             // smallest start index that repeats an earlier start, FILL if none
    int32_t cnt[RING];                           // points of level l at l % RING
    int32_t base[RING];                          // where level l begins in the frontier array
};

struct OwnerState {
    unsigned long long over;                     // (linear index << 8 | owners) of the smallest point above the cap, ~0 if none (first)
    unsigned long long pool_tail;
    int32_t over_level;                          // the level of that point, 0 if none: later levels do nothing
    int32_t pool_short;
};

__device__ __forceinline__ bool flow_lt(int maxima, double x, double y) { return maxima ? x > y : x < y; }

// GridNeighbors (:4-23): +1 then -1 along each axis in turn, wrapped
__device__ __forceinline__ int32_t flow_nbr(int q, int i, int j, int k, int a, int b, int c)
{
    switch (q) {
    case 0: i = i + 1 == a ? 0 : i + 1; break;
    case 1: i = i == 0 ? a - 1 : i - 1; break;
    case 2: j = j + 1 == b ? 0 : j + 1; break;
    case 3: j = j == 0 ? b - 1 : j - 1; break;
    case 4: k = k + 1 == c ? 0 : k + 1; break;
    default: k = k == 0 ? c - 1 : k - 1; break;
    }
    return i + a * (j + b * k);
}

// own[lin] = the smallest index among the starts at that point (own is filled with 0x7f7f7f7f before)
__global__ __launch_bounds__(256) void k_flow_seed_claim(const int32_t* __restrict__ starts, int32_t ns, FlowGeom G, int32_t* __restrict__ own,
                                                         LevelState* __restrict__ st)
{
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (t >= ns) return;
    const int32_t i = starts[3 * (int64_t)t], j = starts[3 * (int64_t)t + 1], k = starts[3 * (int64_t)t + 2];
    if (i < 0 || i >= G.a || j < 0 || j >= G.b || k < 0 || k >= G.c) {
        atomicMin(&st->bad_range, t);
        return;
    }
    atomicMin(own + (i + G.a * (j + G.b * k)), t);
}

// level 0: every start whose value is not skipped (:204-207); a start that lost its point to a smaller index is a duplicate
__global__ __launch_bounds__(256) void k_flow_seed(const int32_t* __restrict__ starts, int32_t ns, FlowGeom G, const double* __restrict__ g,
                                                   const int32_t* __restrict__ own, int32_t* __restrict__ D, uint8_t* __restrict__ nown,
                                                   int32_t* __restrict__ F, LevelState* __restrict__ st)
{
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (t >= ns) return;
    const int32_t i = starts[3 * (int64_t)t], j = starts[3 * (int64_t)t + 1], k = starts[3 * (int64_t)t + 2];
    if (i < 0 || i >= G.a || j < 0 || j >= G.b || k < 0 || k >= G.c) return;
    const int32_t x = i + G.a * (j + G.b * k);
    if (own[x] != t) {
        atomicMin(&st->bad_dup, t);
        return;
    }
    if (g[x] > G.skip_above) return;
    D[x] = 0;
    nown[x] = 1;
    F[atomicAdd(&st->cnt[0], 1)] = x;
}

// level l -> level l + 1.  cnt[l] and base[l] are final (written by the launches before); this launch counts level l + 1, sets
// base[l + 1] and clears the count that the next launch adds to.
__global__ __launch_bounds__(256) void k_flow_level(const double* __restrict__ g, FlowGeom G, int32_t* __restrict__ D, int32_t* __restrict__ F,
                                                    LevelState* __restrict__ st, int32_t l)
{
    const int32_t begin = st->base[l % RING], cnt = st->cnt[l % RING];
    const int32_t next = begin + cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->base[(l + 1) % RING] = next;
        st->cnt[(l + 2) % RING] = 0;
    }
    int32_t* nextcnt = &st->cnt[(l + 1) % RING];
    const int lane = (int)threadIdx.x & 63;
    // the trip count is the same for the 64 lanes of a wave: the claims of a wave are appended with one atomic per neighbour
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t - lane < cnt; t += (int64_t)gridDim.x * 256) {
        const bool active = t < cnt;
        const int32_t x = active ? F[begin + t] : 0;
        const double gx = g[x];
        const int i = x % G.a, j = (x / G.a) % G.b, k = x / (G.a * G.b);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int32_t v = flow_nbr(q, i, j, k, G.a, G.b, G.c);
            const double gv = g[v];
            bool won = active && flow_lt(G.maxima, gx, gv) && !(gv > G.skip_above);      // :225-226; a NaN fails lt
            won = won && __hip_atomic_load(D + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
            won = won && atomicCAS(D + v, -1, l + 1) == -1;
            const unsigned long long m = __ballot(won);
            if (m == 0) continue;
            const int leader = __ffsll((long long)m) - 1;
            int32_t at = 0;
            if (lane == leader) at = atomicAdd(nextcnt, __popcll(m));
            at = __shfl(at, leader);
            if (won) F[next + at + __popcll(m & ((1ull << lane) - 1))] = v;
        }
    }
}

// acc stays sorted, without duplicates, NONE-padded; what falls off its end is the 17th owner
__device__ __forceinline__ void own_insert(int32_t (&acc)[MAXOWN], int32_t o, bool& over)
{
    int32_t carry = o;
#pragma unroll
    for (int q = 0; q < MAXOWN; ++q) {
        const int32_t cur = acc[q];
        const bool dup = carry == cur;
        acc[q] = carry < cur ? carry : cur;
        carry = dup ? NONE : (carry < cur ? cur : carry);
    }
    over = over || carry != NONE;
}

// the number of distinct owners among the predecessors of x, however many: the smallest owner above `last`, repeated
__device__ int32_t count_owners(const double* __restrict__ g, FlowGeom G, const int32_t* __restrict__ D, const int32_t* __restrict__ own,
                                const uint8_t* __restrict__ nown, const int32_t* __restrict__ pool, int32_t x, int32_t l)
{
    const int i = x % G.a, j = (x / G.a) % G.b, k = x / (G.a * G.b);
    const double gx = g[x];
    int32_t n = 0;
    int64_t last = -1;
    for (;;) {
        int64_t best = NONE;
        for (int q = 0; q < 6; ++q) {
            const int32_t u = flow_nbr(q, i, j, k, G.a, G.b, G.c);
            if (D[u] != l - 1 || !flow_lt(G.maxima, g[u], gx)) continue;
            const int32_t ku = nown[u], o = own[u];
            for (int32_t e = 0; e < ku; ++e) {
                const int64_t w = ku == 1 ? o : pool[-(o + 2) + e];
                if (w > last && w < best) best = w;
            }
        }
        if (best == NONE) return n;
        last = best;
        ++n;
    }
}

// the owners of the points of level l >= 1 from those of level l - 1
__global__ __launch_bounds__(256) void k_flow_owners(const double* __restrict__ g, FlowGeom G, const int32_t* __restrict__ D,
                                                     const int32_t* __restrict__ F, int32_t begin, int32_t cnt, int32_t l, int32_t* own,
                                                     uint8_t* nown, int32_t* pool, int64_t poolcap, OwnerState* __restrict__ os)
{
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    const int32_t ol = os->over_level;
    if ((ol != 0 && ol < l) || os->pool_short) return;      // set by an earlier launch: what follows would merge lists that are not there
    const bool active = t < cnt;                            // every lane of a wave stays: the room in the pool is taken once per wave
    const int32_t x = active ? F[begin + t] : 0;
    const double gx = g[x];
    const int i = x % G.a, j = (x / G.a) % G.b, k = x / (G.a * G.b);
    int32_t acc[MAXOWN];
#pragma unroll
    for (int q = 0; q < MAXOWN; ++q) acc[q] = NONE;
    bool over = false;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int32_t u = flow_nbr(q, i, j, k, G.a, G.b, G.c);
        if (!active || D[u] != l - 1 || !flow_lt(G.maxima, g[u], gx)) continue;
        const int32_t ku = nown[u], o = own[u];
        if (ku == 1) {
            own_insert(acc, o, over);
        } else {
            const int32_t* list = pool + (-(o + 2));
            for (int32_t e = 0; e < ku; ++e) own_insert(acc, list[e], over);
        }
    }
    int32_t n = 0;
#pragma unroll
    for (int q = 0; q < MAXOWN; ++q) n += acc[q] != NONE;
    if (active) {
        own[x] = acc[0];
        nown[x] = 1;
    }
    if (over) {
        const int32_t all = count_owners(g, G, D, own, nown, pool, x, l);
        atomicCAS(&os->over_level, 0, l);
        atomicMin(&os->over, ((unsigned long long)x << 8) | (unsigned long long)(all < 255 ? all : 255));
    }
    // entries of this lane, their exclusive sum over the wave, one atomic for the wave
    const int lane = (int)threadIdx.x & 63;
    const int32_t need = (active && !over && n > 1) ? n : 0;
    int32_t incl = need;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const int32_t wave_total = __shfl(incl, 63);
    if (wave_total == 0) return;
    unsigned long long wave_off = 0;
    if (lane == 63) wave_off = atomicAdd(&os->pool_tail, (unsigned long long)wave_total);
    wave_off = __shfl(wave_off, 63);
    if (need == 0) return;
    const unsigned long long off = wave_off + (unsigned long long)(incl - need);
    if (off + (unsigned long long)n > (unsigned long long)poolcap) {
        os->pool_short = 1;
        return;
    }
#pragma unroll
    for (int q = 0; q < MAXOWN; ++q)
        if (q < n) pool[off + q] = acc[q];
    own[x] = -((int32_t)off + 2);
    nown[x] = (uint8_t)n;
}

// Inclusive count over the run of equal labels that ends at this lane, inside the wave; true on the last lane of a run.  Every lane
// of the wave takes part.
__device__ __forceinline__ bool wave_run_count(int label, int& v)
{
    const int lane = (int)threadIdx.x & 63;
    const int prev = __shfl_up(label, 1), next = __shfl_down(label, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != label);
    const int headlane = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane - d >= headlane) v += o;
    }
    return lane == 63 || next != label;
}

// owner map (the smallest owner, -1 for none) and sizes: a point counts once for each of its owners.  LOCAL: a workgroup takes
// `per_block` consecutive points and counts in an LDS table of ns entries, which it adds to `size` at the end (its non-zero entries);
// otherwise every run goes to `size` directly.
template <bool LOCAL>
__global__ __launch_bounds__(256) void k_flow_finish(const int32_t* __restrict__ own, const uint8_t* __restrict__ nown,
                                                     const int32_t* __restrict__ pool, int64_t n, int64_t per_block, int32_t ns,
                                                     int32_t* __restrict__ owner_out, int32_t* __restrict__ size)
{
    extern __shared__ int32_t s_hist[];
    int32_t* hist = LOCAL ? s_hist : size;
    if (LOCAL) {
        for (int32_t s = (int32_t)threadIdx.x; s < ns; s += 256) s_hist[s] = 0;
        __syncthreads();
    }
    const int64_t begin = (int64_t)blockIdx.x * per_block, end = begin + per_block < n ? begin + per_block : n;
    for (int64_t base = begin; base < end; base += 256) {
        const int64_t x = base + threadIdx.x;
        int lab = -1, v = 0;
        if (x < end) {
            const int32_t k = nown[x];
            int32_t o = -1;
            if (k == 1) {
                o = own[x];
                lab = o;
                v = 1;
            } else if (k > 1) {
                const int32_t* list = pool + (-(own[x] + 2));
                o = list[0];
                if (hist)
                    for (int32_t e = 0; e < k; ++e) atomicAdd(hist + list[e], 1);
            }
            if (owner_out) owner_out[x] = o;
        }
        const bool tail = wave_run_count(lab, v);
        if (hist && tail && lab >= 0) atomicAdd(hist + lab, v);
    }
    if (LOCAL) {
        __syncthreads();
        for (int32_t s = (int32_t)threadIdx.x; s < ns; s += 256)
            if (s_hist[s]) atomicAdd(size + s, s_hist[s]);
    }
}

// entries of the multi-owner points of each chunk; nown is padded with zeros to whole chunks
__global__ __launch_bounds__(256) void k_flow_shared_count(const uint8_t* __restrict__ nown, long long* __restrict__ chunkcnt)
{
    using Red = hipcub::BlockReduce<int, 256>;
    __shared__ typename Red::TempStorage tmp;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t w = reinterpret_cast<const uint64_t*>(nown)[t];
    int mine = 0;
    for (int q = 0; q < 8; ++q) {
        const int k = (int)((w >> (8 * q)) & 0xff);
        mine += k > 1 ? k : 0;
    }
    const int n = Red(tmp).Sum(mine);
    if (threadIdx.x == 0) chunkcnt[blockIdx.x] = n;
}

// (linear index, owner) of every owner of every multi-owner point, by index then owner
__global__ __launch_bounds__(256) void k_flow_shared_emit(const uint8_t* __restrict__ nown, const int32_t* __restrict__ own,
                                                          const int32_t* __restrict__ pool, const long long* __restrict__ chunkoff, int64_t cap,
                                                          int32_t* __restrict__ out)
{
    using Scan = hipcub::BlockScan<int, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t w = reinterpret_cast<const uint64_t*>(nown)[t];
    int mine = 0;
    for (int q = 0; q < 8; ++q) {
        const int k = (int)((w >> (8 * q)) & 0xff);
        mine += k > 1 ? k : 0;
    }
    int pre = 0;
    Scan(tmp).ExclusiveSum(mine, pre);
    int64_t pos = (int64_t)chunkoff[blockIdx.x] + pre;
    for (int q = 0; q < 8; ++q) {
        const int k = (int)((w >> (8 * q)) & 0xff);
        if (k <= 1) continue;
        const int64_t lin = t * 8 + q;
        const int32_t* list = pool + (-(own[lin] + 2));
        for (int e = 0; e < k; ++e, ++pos) {
            if (pos >= cap) continue;
            out[2 * pos] = (int32_t)lin;
            out[2 * pos + 1] = list[e];
        }
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
    const void* in(const void* src, int on_device, size_t bytes)
    {
        if (on_device) return src;
        void* p = get(bytes);
        if (p && bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) failed = true;
        return p;
    }
    // where the kernels write an array that the caller may want: the caller's device array, or a buffer of the call
    void* buf(void* dst, int on_device, size_t bytes) { return (dst && on_device) ? dst : get(bytes); }
    void back(void* dst, int on_device, const void* dev, size_t bytes)
    {
        if (dst && !on_device && bytes && hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) failed = true;
    }
    void fill(void* p, int byte, size_t bytes)
    {
        if (p && bytes && hipMemsetAsync(p, byte, bytes, st) != hipSuccess) failed = true;
    }
};

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int ceg_grid_basins(int32_t device, const double* grid, int32_t grid_on_device, const int32_t dims[3], const int32_t* starts,
                               int32_t starts_on_device, int64_t nstarts, int32_t maxima, double skip_above, int64_t maxdist,
                               int32_t* level_out, int32_t* owner_out, uint8_t* nowners_out, int32_t maps_on_device, int32_t* shared_out,
                               int64_t shared_capacity, int64_t* shared_count_out, int32_t* size_out, int32_t lists_on_device, void* stream)
{
    if (!grid || nstarts < 0 || nstarts > FILL || (nstarts > 0 && !starts) || (maxima != 0 && maxima != 1) || skip_above != skip_above ||
        maxdist < 0 || shared_capacity < 0 || (shared_capacity > 0 && !shared_out))
        return ferr(CEG_ERR_INVALID, "bad argument");
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return ferr(CEG_ERR_INVALID, "dims must be three positive numbers");
    const int64_t ab = (int64_t)dims[0] * dims[1];
    if (ab > std::numeric_limits<int32_t>::max() || ab * dims[2] > std::numeric_limits<int32_t>::max())
        return ferr(CEG_ERR_INVALID, "a*b*c does not fit int32");
    const int64_t n = ab * dims[2];
    if (ceg_device_count() <= 0) return ferr(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ceg_device_count()) return ferr(CEG_ERR_NO_DEVICE, "device not present");
    DevGuard guard(device);
    if (!guard.ok) return ferr(CEG_ERR_HIP, "hipSetDevice failed");
    Workspace ws((hipStream_t)stream);
    char msg[200];

    FlowGeom G{skip_above, dims[0], dims[1], dims[2], maxima};
    const int32_t ns = (int32_t)nstarts;
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK, npad = nchunk * CHUNK;
    const double* d_g = (const double*)ws.in(grid, grid_on_device, sizeof(double) * (size_t)n);
    const int32_t* d_starts = (const int32_t*)ws.in(starts, starts_on_device, sizeof(int32_t) * 3 * (size_t)ns);
    int32_t* d_D = (int32_t*)ws.buf(level_out, maps_on_device, sizeof(int32_t) * (size_t)n);
    int32_t* d_own = (int32_t*)ws.get(sizeof(int32_t) * (size_t)n);
    uint8_t* d_nown = (uint8_t*)ws.get((size_t)npad);                                    // padded: the compaction reads whole chunks
    int32_t* d_F = (int32_t*)ws.get(sizeof(int32_t) * (size_t)n);
    LevelState* d_ls = (LevelState*)ws.get(sizeof(LevelState));
    OwnerState* d_os = (OwnerState*)ws.get(sizeof(OwnerState));
    if (ws.failed) return ferr(CEG_ERR_HIP, "could not allocate the device workspace / upload the inputs");
    LevelState ls{};
    ws.fill(d_D, 0xff, sizeof(int32_t) * (size_t)n);
    ws.fill(d_own, 0x7f, sizeof(int32_t) * (size_t)n);
    ws.fill(d_nown, 0, (size_t)npad);
    ws.fill(d_ls, 0, sizeof(LevelState));
    ws.fill(d_ls, 0x7f, 2 * sizeof(int32_t));                                            // bad_range, bad_dup
    if (ws.failed) return ferr(CEG_ERR_HIP, "could not initialise the device workspace");
    if (ns > 0) {
        hipLaunchKernelGGL(k_flow_seed_claim, dim3(blocks256(ns)), dim3(256), 0, ws.st, d_starts, ns, G, d_own, d_ls);
        hipLaunchKernelGGL(k_flow_seed, dim3(blocks256(ns)), dim3(256), 0, ws.st, d_starts, ns, G, d_g, d_own, d_D, d_nown, d_F, d_ls);
    }

    // levels: BATCH launches, then the counts come back; level l + 1 <= maxdist - 1 (:226, current_dist is 1 at the start)
    std::vector<int32_t> cnts;
    const unsigned level_blocks = blocks256(n) < (unsigned)LEVEL_BLOCKS ? blocks256(n) : (unsigned)LEVEL_BLOCKS;
    for (int64_t l = 0;;) {
        int launched = 0;
        while (launched < BATCH && (maxdist == 0 || l + launched + 1 <= maxdist - 1)) {
            hipLaunchKernelGGL(k_flow_level, dim3(level_blocks), dim3(256), 0, ws.st, d_g, G, d_D, d_F, d_ls, (int32_t)(l + launched));
            ++launched;
        }
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&ls, d_ls, sizeof(ls), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
            hipStreamSynchronize(ws.st) != hipSuccess)
            return ferr(CEG_ERR_HIP, "the level pass failed");
        if (cnts.empty()) {
            if (ls.bad_range != FILL) {
                snprintf(msg, sizeof msg, "start %d is outside the grid", ls.bad_range);
                return ferr(CEG_ERR_INVALID, msg);
            }
            if (ls.bad_dup != FILL) {
                snprintf(msg, sizeof msg, "start %d repeats an earlier start", ls.bad_dup);
                return ferr(CEG_ERR_INVALID, msg);
            }
            cnts.push_back(ls.cnt[0]);
        }
        bool end = launched < BATCH;
        for (int q = 1; q <= launched; ++q) {
            const int32_t c = ls.cnt[(l + q) % RING];
            if (c == 0) {
                end = true;
                break;
            }
            cnts.push_back(c);
        }
        l += launched;
        if (end) break;
    }

    // owners, level by level; the pool holds one entry per owner of a multi-owner point: n entries first, the bound 16 n if that is short
    const int64_t poolmax = std::numeric_limits<int32_t>::max() - 2;
    int64_t poolcap = n < 4096 ? 4096 : n;
    if (const char* e = std::getenv("CEG_HIP_BASINS_POOL")) {                            // the first size, in entries (for tests of the second)
        const long long v = std::atoll(e);
        if (v > 0) poolcap = v < poolmax ? v : poolmax;
    }
    int32_t* d_pool = nullptr;
    long long* d_coff = nullptr;
    OwnerState os{};
    long long total = 0;
    for (int attempt = 0;; ++attempt) {
        d_pool = (int32_t*)ws.get(sizeof(int32_t) * (size_t)poolcap);
        long long* d_ccnt = (long long*)ws.get(sizeof(long long) * (size_t)(nchunk + 1));
        d_coff = (long long*)ws.get(sizeof(long long) * (size_t)(nchunk + 1));
        size_t tmp_bytes = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_ccnt, d_coff, (int)(nchunk + 1), ws.st);
        void* d_tmp = ws.get(tmp_bytes);
        if (ws.failed) return ferr(CEG_ERR_HIP, "could not allocate the device workspace");
        ws.fill(d_os, 0, sizeof(OwnerState));
        ws.fill(d_os, 0xff, sizeof(unsigned long long));                                 // over
        ws.fill(d_ccnt + nchunk, 0, sizeof(long long));
        if (ws.failed) return ferr(CEG_ERR_HIP, "could not initialise the device workspace");
        int32_t begin = cnts[0];
        for (size_t l = 1; l < cnts.size(); ++l) {
            hipLaunchKernelGGL(k_flow_owners, dim3(blocks256(cnts[l])), dim3(256), 0, ws.st, d_g, G, d_D, d_F, begin, cnts[l], (int32_t)l, d_own,
                               d_nown, d_pool, poolcap, d_os);
            begin += cnts[l];
        }
        hipLaunchKernelGGL(k_flow_shared_count, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_nown, d_ccnt);
        if (hipGetLastError() != hipSuccess ||
            hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_ccnt, d_coff, (int)(nchunk + 1), ws.st) != hipSuccess ||
            hipMemcpyAsync(&os, d_os, sizeof(os), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
            hipMemcpyAsync(&total, d_coff + nchunk, sizeof(long long), hipMemcpyDeviceToHost, ws.st) != hipSuccess ||
            hipStreamSynchronize(ws.st) != hipSuccess)
            return ferr(CEG_ERR_HIP, "the owner pass failed");
        if (os.over != ~0ull) {
            snprintf(msg, sizeof msg, "grid point %lld has %d owners, more than CEG_BASINS_MAX_OWNERS = %d", (long long)(os.over >> 8),
                     (int)(os.over & 0xff), MAXOWN);
            return ferr(CEG_ERR_UNSUPPORTED, msg);
        }
        if (!os.pool_short) break;
        if (attempt > 0 || poolcap >= poolmax) return ferr(CEG_ERR_UNSUPPORTED, "the owner lists of the multi-owner points do not fit 2^31 entries");
        poolcap = 16 * n < poolmax ? 16 * n : poolmax;
    }
    if (shared_count_out) *shared_count_out = total;

    // emit
    const int64_t nout = total < shared_capacity ? total : shared_capacity;
    int32_t* d_owner = owner_out ? (int32_t*)ws.buf(owner_out, maps_on_device, sizeof(int32_t) * (size_t)n) : nullptr;
    int32_t* d_size = (size_out && ns > 0) ? (int32_t*)ws.buf(size_out, lists_on_device, sizeof(int32_t) * (size_t)ns) : nullptr;
    int32_t* d_shared = nout > 0 ? (int32_t*)ws.buf(shared_out, lists_on_device, sizeof(int32_t) * 2 * (size_t)nout) : nullptr;
    if (d_size) ws.fill(d_size, 0, sizeof(int32_t) * (size_t)ns);
    if (ws.failed) return ferr(CEG_ERR_HIP, "could not allocate the device workspace");
    if (d_size && ns <= FINISH_LOCAL_MAX) {
        const unsigned nb = blocks256(n) < (unsigned)FINISH_BLOCKS ? blocks256(n) : (unsigned)FINISH_BLOCKS;
        const int64_t per_block = (n + nb - 1) / nb;
        hipLaunchKernelGGL(k_flow_finish<true>, dim3(nb), dim3(256), sizeof(int32_t) * (size_t)ns, ws.st, d_own, d_nown, d_pool, n, per_block, ns,
                           d_owner, d_size);
    } else if (d_owner || d_size) {
        hipLaunchKernelGGL(k_flow_finish<false>, dim3(blocks256(n)), dim3(256), 0, ws.st, d_own, d_nown, d_pool, n, (int64_t)256, ns, d_owner,
                           d_size);
    }
    if (d_shared)
        hipLaunchKernelGGL(k_flow_shared_emit, dim3((unsigned)nchunk), dim3(256), 0, ws.st, d_nown, d_own, d_pool, d_coff, nout, d_shared);
    ws.back(level_out, maps_on_device, d_D, sizeof(int32_t) * (size_t)n);
    ws.back(owner_out, maps_on_device, d_owner, sizeof(int32_t) * (size_t)n);
    ws.back(nowners_out, maps_on_device, d_nown, (size_t)n);
    if (d_size) ws.back(size_out, lists_on_device, d_size, sizeof(int32_t) * (size_t)ns);
    if (d_shared) ws.back(shared_out, lists_on_device, d_shared, sizeof(int32_t) * 2 * (size_t)nout);
    if (nowners_out && maps_on_device &&
        hipMemcpyAsync(nowners_out, d_nown, (size_t)n, hipMemcpyDeviceToDevice, ws.st) != hipSuccess)
        ws.failed = true;
    const bool host_out = ((level_out || owner_out || nowners_out) && !maps_on_device) || ((d_size || d_shared) && !lists_on_device);
    if (hipGetLastError() != hipSuccess || ws.failed || (host_out && hipStreamSynchronize(ws.st) != hipSuccess))
        return ferr(CEG_ERR_HIP, "the emit of the basins failed");
    return CEG_OK;
}
