// ceg_mc_sample.hip -- the sampler of a chain group (ceg_mc_group_set_sampler / _sample / _sampler_read / _sampler_reset): the counts
// of bin_trajectory (src/averageclusters.jl:154-202) and the per-cycle series of GCMCRecorder / run_montecarlo!
// (src/parameterinputs.jl:232-249, src/simulation.jl:784-799), taken from the resident state by one launch per frame (k_mcg_sample).
// The sweeps of ceg_mc_sweep.hip enqueue that launch behind the accept launch of a frame step; nothing here writes chain state.
#include "ceg_mc_state.h"

using namespace ceg_mcs;

namespace {

static_assert(sizeof(ceg_mc_sample_record_t) == 64 && sizeof(ceg_mc_sampler_t) == 152, "layouts the bindings restate");

// the map as the kernel sees it, by value (kernarg); bins == nullptr: series only
struct SampleMap {
    double I[9];                                 // inverse of the unit cell, column-major
    int32_t dims[3];
    int32_t nchannels, nkinds, nsym;
    const int32_t* chain_map;                    // [K]
    const int32_t* kind_channel;                 // [nkinds]
    const double* sym;                           // [nsym][3][4]
    unsigned long long* bins;                    // [nmaps][nchannels][nc][nb][na]
};

// averageclusters.jl:182-184 for one axis, 0-based; the clamp is for memory safety only
__device__ __forceinline__ int sample_index(double y, int n)
{
#pragma clang fp contract(off)
    const double u = y - floor(y);
    const int i = (int)ceil(u * (double)n) + (u == 0.0 ? 1 : 0) - 1;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

__device__ __forceinline__ void sample_count(const SampleMap& M, unsigned long long* block, double y0, double y1, double y2)
{
    const int i0 = sample_index(y0, M.dims[0]), i1 = sample_index(y1, M.dims[1]), i2 = sample_index(y2, M.dims[2]);
    atomicAdd(block + ((size_t)i2 * M.dims[1] + i1) * M.dims[0] + i0, 1ull);
}

// workgroup (c, t): lane l takes atom slot 256 t + l of chain c; thread 0 of tile 0 writes the chain's record of the frame, every wave
// adds its occupied slots to the record's natoms (the series is zero beyond the frames taken so far).  Integer atomics only.
__global__ __launch_bounds__(MC_THREADS) void k_mcg_sample(const McView* __restrict__ views, const SampleMap M, const SampleSource src,
                                                           ceg_mc_sample_record_t* __restrict__ rec, int64_t step)
{
    const int c = (int)blockIdx.x, tid = threadIdx.x;
    const McView& v = as_constant(views)[c];
    const int32_t* T = src.counts ? src.counts + (size_t)c * src.counts_stride : nullptr;
    const int nmol = T ? __atomic_load_n(T, __ATOMIC_RELAXED) : v.nmol;
    const int nslots = T ? __atomic_load_n(T + 1, __ATOMIC_RELAXED) : v.natoms;
    ceg_mc_sample_record_t& R = rec[c];
    if (blockIdx.y == 0 && tid == 0) {
        R.step = step;
        R.nmol = nmol;
        for (int i = 0; i < CEG_MC_GCMC_MAX_SPECIES; ++i) R.count[i] = (T && i < src.ncount) ? __atomic_load_n(T + 2 + i, __ATOMIC_RELAXED) : 0;
        R.delta_moves = src.delta_moves ? *reinterpret_cast<const double*>(reinterpret_cast<const char*>(src.delta_moves) + (size_t)c * src.stats_stride) : 0.0;
        R.delta_swaps = src.delta_swaps ? *reinterpret_cast<const double*>(reinterpret_cast<const char*>(src.delta_swaps) + (size_t)c * src.stats_stride) : 0.0;
    }
    const int slot = (int)blockIdx.y * MC_THREADS + tid;
    bool occupied = false;
    if (slot < nslots) {
        const double4 A = v.atoms[slot];
        int kind, mol;
        unpack(A.w, kind, mol);
        occupied = mol >= 0;
        // (a chain that had stopped by the frame's step -- ceg_mc_group_set_chain_plan -- is counted into its record and not binned)
        const bool frozen = src.stop && step >= src.stop[c];
        // (tempering: the map of the rung the chain holds, so that a map belongs to a temperature; a permutation of the chains)
        const int of = src.rung ? src.rung[c] : c;
        const int map = (M.bins && !frozen && (unsigned)of < gridDim.x) ? M.chain_map[of] : -1;
        const int channel = (M.bins && kind >= 0 && kind < M.nkinds) ? M.kind_channel[kind] : -1;
        if (occupied && map >= 0 && channel >= 0) {
#pragma clang fp contract(off)
            unsigned long long* block = M.bins + ((size_t)map * M.nchannels + channel) * ((size_t)M.dims[0] * M.dims[1] * M.dims[2]);
            const double* I = M.I;
            const double y0 = (I[0] * A.x + I[3] * A.y) + I[6] * A.z;
            const double y1 = (I[1] * A.x + I[4] * A.y) + I[7] * A.z;
            const double y2 = (I[2] * A.x + I[5] * A.y) + I[8] * A.z;
            sample_count(M, block, y0, y1, y2);
            for (int q = 0; q < M.nsym; ++q) {
                const double* S = M.sym + 12 * (size_t)q;
                sample_count(M, block, ((S[0] * y0 + S[1] * y1) + S[2] * y2) + S[3], ((S[4] * y0 + S[5] * y1) + S[6] * y2) + S[7],
                             ((S[8] * y0 + S[9] * y1) + S[10] * y2) + S[11]);
            }
        }
    }
    const unsigned long long live = __ballot(occupied);
    if ((tid & 63) == 0 && live) atomicAdd(&R.natoms, __popcll(live));
}

int bad_spec(const char* what)
{
    char msg[200];
    std::snprintf(msg, sizeof msg, "sampler: %s", what);
    return merr(CEG_ERR_INVALID, msg);
}

}  // namespace

struct ceg_mcs::GroupSampler {
    int64_t every = 1, from_step = 0, capacity = 0, frames = 0;
    int k = 0;
    SampleMap map{};                             // device pointers; bins == nullptr: no map
    size_t nbins = 0;
    int32_t *d_chain_map = nullptr, *d_kind_channel = nullptr;
    double* d_sym = nullptr;
    ceg_mc_sample_record_t* d_series = nullptr;  // [capacity][k], zero beyond `frames`
};

void ceg_mcs::sampler_free(GroupSampler* s)
{
    if (!s) return;
    for (void* p : {(void*)s->d_chain_map, (void*)s->d_kind_channel, (void*)s->d_sym, (void*)s->map.bins, (void*)s->d_series})
        if (p) (void)hipFree(p);
    delete s;
}

bool ceg_mcs::sampler_frame_after(const GroupSampler* s, uint64_t step)
{
    return step >= (uint64_t)s->from_step && (step + 1) % (uint64_t)s->every == 0;
}

// frames of the steps [first, first + nsteps): the multiples of `every` in (max(first, from_step), first + nsteps]
int ceg_mcs::sampler_admit(const GroupSampler* s, uint64_t first_step, int64_t nsteps)
{
    if (nsteps <= 0) return CEG_OK;
    if (first_step > (uint64_t)INT64_MAX || (uint64_t)nsteps > (uint64_t)INT64_MAX - first_step)
        return merr(CEG_ERR_INVALID, "a sampled sweep must end before step 2^63");
    const uint64_t end = first_step + (uint64_t)nsteps, lo = std::max(first_step, (uint64_t)s->from_step), e = (uint64_t)s->every;
    const uint64_t frames = lo < end ? end / e - lo / e : 0;
    if (frames > (uint64_t)(s->capacity - s->frames)) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "the sweep takes %llu frames and the sampler's series has room for %lld (series_capacity %lld, %lld taken)",
                      (unsigned long long)frames, (long long)(s->capacity - s->frames), (long long)s->capacity, (long long)s->frames);
        return merr(CEG_ERR_INVALID, msg);
    }
    return CEG_OK;
}

void ceg_mcs::sampler_enqueue(GroupSampler* s, hipStream_t stream, const McView* d_views, int k, int64_t step, const SampleSource& src)
{
    if (s->frames >= s->capacity || k != s->k) return;            // (admitted before the first launch: cannot happen)
    const unsigned tiles = (unsigned)std::max((src.max_slots + MC_THREADS - 1) / MC_THREADS, 1);
    hipLaunchKernelGGL(k_mcg_sample, dim3((unsigned)k, tiles), dim3(MC_THREADS), 0, stream, d_views, s->map, src, s->d_series + (size_t)s->frames * (size_t)k, step);
    if (hipPeekAtLastError() == hipSuccess) ++s->frames;          // (a frame that was not launched is not counted; the caller reads the error)
}

int64_t ceg_mcs::sampler_frames_taken(const GroupSampler* s) { return s->frames; }

// a sweep failed after it had enqueued frames: they are not counted, and their records are zeroed again where the device still answers
void ceg_mcs::sampler_rollback(GroupSampler* s, hipStream_t stream, int64_t frames)
{
    if (frames >= s->frames) return;
    (void)hipMemsetAsync(s->d_series + (size_t)frames * (size_t)s->k, 0, sizeof(ceg_mc_sample_record_t) * (size_t)(s->frames - frames) * (size_t)s->k, stream);
    s->frames = frames;
}

extern "C" int ceg_mc_group_set_sampler(ceg_mc_group_t* g, const ceg_mc_sampler_t* spec)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    size_t nbins = 0;
    bool with_map = false;
    if (spec) {
        if (spec->every < 1) return bad_spec("every must be >= 1");
        if (spec->from_step < 0 || spec->series_capacity < 0) return bad_spec("from_step and series_capacity must be >= 0");
        if ((uint64_t)spec->series_capacity > (uint64_t)1 << 40) return bad_spec("series_capacity is too large");
        if (spec->nsym < 0 || spec->nsym > CEG_MC_SAMPLER_MAX_SYM) return bad_spec("0 <= nsym <= CEG_MC_SAMPLER_MAX_SYM");
        const int32_t* d = spec->dims;
        with_map = d[0] != 0 || d[1] != 0 || d[2] != 0;
        if (with_map) {
            if (d[0] < 1 || d[1] < 1 || d[2] < 1) return bad_spec("dims must be all zero (no map) or all >= 1");
            if (spec->nmaps < 1 || spec->nchannels < 1) return bad_spec("a map needs nmaps >= 1 and nchannels >= 1");
            if (spec->nkinds < 0) return bad_spec("nkinds must be >= 0");
            if (!spec->chain_map || (spec->nkinds > 0 && !spec->kind_channel) || (spec->nsym > 0 && !spec->sym)) return bad_spec("a missing array");
            for (int c = 0; c < r.k; ++c)
                if (spec->chain_map[c] < -1 || spec->chain_map[c] >= spec->nmaps) return bad_spec("an entry of chain_map lies outside [-1, nmaps)");
            for (int q = 0; q < spec->nkinds; ++q)
                if (spec->kind_channel[q] < -1 || spec->kind_channel[q] >= spec->nchannels) return bad_spec("an entry of kind_channel lies outside [-1, nchannels)");
            for (int q = 0; q < 9; ++q)
                if (!std::isfinite(spec->unit_invmat[q])) return bad_spec("unit_invmat must be finite");
            for (int q = 0; q < 12 * spec->nsym; ++q)
                if (!std::isfinite(spec->sym[q])) return bad_spec("the symmetry operations must be finite");
            const double total = (double)d[0] * d[1] * d[2] * spec->nmaps * spec->nchannels;
            if (total > (double)CEG_MC_SAMPLER_MAX_BINS) return bad_spec("the map is too large (more than CEG_MC_SAMPLER_MAX_BINS bins over all maps and channels)");
            nbins = (size_t)d[0] * d[1] * d[2] * (size_t)spec->nmaps * (size_t)spec->nchannels;
        }
    }
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    if (!spec) {
        sampler_free(*r.sampler);
        *r.sampler = nullptr;
        return CEG_OK;
    }
    GroupSampler* s = new GroupSampler();
    s->every = spec->every; s->from_step = spec->from_step; s->capacity = spec->series_capacity;
    s->k = r.k;
    s->nbins = nbins;
    const size_t series_bytes = sizeof(ceg_mc_sample_record_t) * (size_t)s->capacity * (size_t)r.k;
    bool ok = series_bytes == 0 || (hipMalloc((void**)&s->d_series, series_bytes) == hipSuccess && hipMemsetAsync(s->d_series, 0, series_bytes, r.stream) == hipSuccess);
    if (ok && with_map) {
        SampleMap& M = s->map;
        for (int q = 0; q < 9; ++q) M.I[q] = spec->unit_invmat[q];
        for (int q = 0; q < 3; ++q) M.dims[q] = spec->dims[q];
        M.nchannels = spec->nchannels; M.nkinds = spec->nkinds; M.nsym = spec->nsym;
        auto upload = [&](void** dst, const void* src, size_t bytes) {
            return hipMalloc(dst, std::max(bytes, (size_t)16)) == hipSuccess && (bytes == 0 || hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
        };
        ok = upload((void**)&s->d_chain_map, spec->chain_map, sizeof(int32_t) * (size_t)r.k) &&
             upload((void**)&s->d_kind_channel, spec->kind_channel, sizeof(int32_t) * (size_t)spec->nkinds) &&
             upload((void**)&s->d_sym, spec->sym, sizeof(double) * 12 * (size_t)spec->nsym) &&
             hipMalloc((void**)&M.bins, sizeof(unsigned long long) * nbins) == hipSuccess &&
             hipMemsetAsync(M.bins, 0, sizeof(unsigned long long) * nbins, r.stream) == hipSuccess;
        M.chain_map = s->d_chain_map; M.kind_channel = s->d_kind_channel; M.sym = s->d_sym;
    }
    ok = ok && hipStreamSynchronize(r.stream) == hipSuccess;      // (the zeroing ran on the group's stream, which does not wait for the null stream)
    if (!ok) {
        sampler_free(s);
        return merr(CEG_ERR_HIP, "could not allocate the sampler's device buffers");
    }
    sampler_free(*r.sampler);
    *r.sampler = s;
    return CEG_OK;
}

extern "C" int ceg_mc_group_sample(ceg_mc_group_t* g)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    GroupSampler* s = *r.sampler;
    if (!s) return merr(CEG_ERR_INVALID, "the group has no sampler (ceg_mc_group_set_sampler)");
    int32_t max_slots = 0;
    for (int c = 0; c < r.k; ++c) {
        if (r.chains[c]->poisoned) return group_refuse_poisoned(c);
        max_slots = std::max(max_slots, r.chains[c]->v.natoms);
    }
    if (s->frames >= s->capacity) return merr(CEG_ERR_INVALID, "the sampler's series is full (series_capacity)");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (!group_views_current(g)) return merr(CEG_ERR_HIP, "view upload failed");
    sampler_enqueue(s, r.stream, r.d_views, r.k, -1, SampleSource{nullptr, 0, 0, nullptr, nullptr, 0, max_slots, nullptr,
                                                                    *r.tempering ? temper_device_rungs(*r.tempering) : nullptr});
    if (hipGetLastError() != hipSuccess) return merr(CEG_ERR_HIP, "sample kernel launch failed");
    return CEG_OK;                       // asynchronous: ordered on the group's stream
}

extern "C" int ceg_mc_group_sampler_read(ceg_mc_group_t* g, int64_t* bins_out, ceg_mc_sample_record_t* series_out, int64_t* frames_out)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const GroupSampler* s = *r.sampler;
    if (!s) return merr(CEG_ERR_INVALID, "the group has no sampler (ceg_mc_group_set_sampler)");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    if (bins_out && s->nbins > 0 && hipMemcpy(bins_out, s->map.bins, sizeof(int64_t) * s->nbins, hipMemcpyDeviceToHost) != hipSuccess)
        return merr(CEG_ERR_HIP, "D2H of the bins failed");
    if (series_out && s->frames > 0 &&
        hipMemcpy(series_out, s->d_series, sizeof(ceg_mc_sample_record_t) * (size_t)s->frames * (size_t)s->k, hipMemcpyDeviceToHost) != hipSuccess)
        return merr(CEG_ERR_HIP, "D2H of the series failed");
    if (frames_out) *frames_out = s->frames;
    return CEG_OK;
}

extern "C" int ceg_mc_group_sampler_reset(ceg_mc_group_t* g)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    GroupSampler* s = *r.sampler;
    if (!s) return merr(CEG_ERR_INVALID, "the group has no sampler (ceg_mc_group_set_sampler)");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    const size_t taken = sizeof(ceg_mc_sample_record_t) * (size_t)s->frames * (size_t)s->k;
    if ((s->nbins > 0 && hipMemsetAsync(s->map.bins, 0, sizeof(unsigned long long) * s->nbins, r.stream) != hipSuccess) ||
        (taken > 0 && hipMemsetAsync(s->d_series, 0, taken, r.stream) != hipSuccess))
        return merr(CEG_ERR_HIP, "hipMemsetAsync failed");
    s->frames = 0;
    return CEG_OK;
}
