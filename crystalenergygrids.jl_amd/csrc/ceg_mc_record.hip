// ceg_mc_record.hip -- the recorder of a chain group (ceg_mc_group_set_recorder / _snapshot / _recorder_rebase / _recorder_read /
// _recorder_min): the trajectory of run_montecarlo! (put!(output, o) every printevery cycles, src/simulation.jl:784-799) and
// RMinimumEnergy (src/parameterinputs.jl:86-108), taken from the resident state by one launch per cycle end (k_mcg_snapshot) on the
// group's stream.  The *_cycles sweeps of ceg_mc_sweep.hip enqueue it behind k_mcg_cycle_end / k_mcg_exchange; nothing here writes
// chain state.
#include "ceg_mc_state.h"

#include <climits>
#include <limits>

using namespace ceg_mcs;

namespace {

static_assert(sizeof(ceg_mc_recorder_t) == 48 && sizeof(ceg_mc_snapshot_record_t) == 40, "layouts the bindings restate");

// one slot of the store per chain: records [K], then the four arrays of the body, [K][...]; rec == nullptr: not written
struct RecordSlot {
    ceg_mc_snapshot_record_t* rec;
    double* xyz;                                 // [K][max_atoms][3]
    int32_t* kind;                               // [K][max_atoms]
    int32_t* mol_first;                          // [K][max_molecules + 1]
    int32_t* species;                            // [K][max_molecules]
};

struct Snapshot {                                // by value (kernarg)
    RecordSource src;
    RecordSlot frame, best;                      // frame.rec nullptr: no frame due; best.rec nullptr: no minimum kept
    double* mine;                                // [K]
    int64_t* mink;                               // [K]
    int64_t cc, step;
    int32_t max_atoms, max_molecules;
};

template <class T>
__device__ __forceinline__ T record_at(const T* base, int c, int stride)
{
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)c * (size_t)stride);
}

// exclusive prefix of `cnt` over the workgroup and the workgroup's sum; every thread calls it
__device__ __forceinline__ int record_scan(int cnt, int tid, int* s_wtot, int& total)
{
    const int wave = tid >> 6, lane = tid & 63;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();                             // (the sums of the previous chunk, and its s_first / s_slot, have been read)
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; ++w) {
        if (w < wave) before += s_wtot[w];
        total += s_wtot[w];
    }
    return before + incl - cnt;
}

// Workgroup c: chain c's configuration compacted into molecule order, into the frame's slot and -- where the chain's energy is
// strictly below its minimum -- into its best slot.  Two passes over the molecule table: the first checks every entry (1..16 atoms,
// inside the atom slots in use) and sums the atoms, so that a chain that does not fit gets its record and no body; the second, in
// chunks of MC_THREADS molecules, gives molecule j its first atom by a prefix sum over the chunk plus the chunks before, then copies
// MC_THREADS atoms at a time: one thread per ATOM reads the record (the molecule of an atom by a binary search of the chunk's
// prefixes in LDS; consecutive lanes read consecutive 32-byte records where the molecules sit side by side) and puts x, y, z into
// LDS, then one thread per DOUBLE writes them out, so that every store instruction of the payload covers consecutive addresses.
// Only this workgroup reads or writes mine[c] / mink[c], and it reads them before a barrier and writes them behind it.  Every
// index is checked before it is used.  (The energy is a sum of two or three terms: there is no product a contraction could fuse.)
__global__ __launch_bounds__(MC_THREADS) void k_mcg_snapshot(const McView* __restrict__ views, const Snapshot S)
{
    __shared__ int s_first[MC_THREADS], s_slot[MC_THREADS], s_wtot[MC_THREADS / 64], s_bad;
    __shared__ double s_xyz[3 * MC_THREADS];
    const int c = (int)blockIdx.x, tid = threadIdx.x;
    const McView& v = as_constant(views)[c];
    const RecordSource& R = S.src;
    const int32_t* T = R.counts ? R.counts + (size_t)c * R.counts_stride : nullptr;
    const int nmol = max(T ? __atomic_load_n(T, __ATOMIC_RELAXED) : v.nmol, 0);
    const int nslots = T ? __atomic_load_n(T + 1, __ATOMIC_RELAXED) : v.natoms;
    double E = R.energy[c];
    if (R.delta_moves) E = E + record_at(R.delta_moves, c, R.stats_stride);
    if (R.delta_swaps) E = E + record_at(R.delta_swaps, c, R.stats_stride);
    const bool stopped = R.stop && R.last_step >= (uint64_t)R.stop[c];
    const bool better = S.best.rec && !stopped && E < S.mine[c];
    const bool framed = S.frame.rec != nullptr;
    if (!framed && !better) return;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    // ---- pass 1: the entries checked, the atoms counted (a sum over the workgroup)
    int counted = 0;
    for (int j = tid; j < nmol; j += MC_THREADS) {
        const int2 mj = v.mol[j];
        if (mj.y >= 1 && mj.y <= MC_MAX_ATOMS && mj.x >= 0 && mj.x <= nslots - mj.y) counted += mj.y;
        else s_bad = 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) counted += __shfl_xor(counted, o);
    if ((tid & 63) == 0) s_wtot[tid >> 6] = counted;
    __syncthreads();
    int natoms = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; ++w) natoms += s_wtot[w];
    const bool fits = !s_bad && nmol <= S.max_molecules && natoms <= S.max_atoms;
    const size_t ma = (size_t)S.max_atoms, mm = (size_t)S.max_molecules;
    // the chain's part of either slot; nullptr where it takes no body
    double* fx = framed && fits ? S.frame.xyz + (size_t)c * ma * 3 : nullptr;
    int32_t* fk = fx ? S.frame.kind + (size_t)c * ma : nullptr;
    int32_t* ff = fx ? S.frame.mol_first + (size_t)c * (mm + 1) : nullptr;
    int32_t* fs = fx ? S.frame.species + (size_t)c * mm : nullptr;
    double* bx = better ? S.best.xyz + (size_t)c * ma * 3 : nullptr;
    int32_t* bk = better ? S.best.kind + (size_t)c * ma : nullptr;
    int32_t* bf = better ? S.best.mol_first + (size_t)c * (mm + 1) : nullptr;
    int32_t* bs = better ? S.best.species + (size_t)c * mm : nullptr;
    if (tid == 0) {
        ceg_mc_snapshot_record_t rec;
        rec.cycle = S.cc; rec.step = S.step; rec.energy = E; rec.nmol = nmol; rec.natoms = natoms;
        rec.flags = (fits ? 0 : 1) | (stopped ? 2 : 0); rec._pad = 0;
        if (framed) S.frame.rec[c] = rec;
        if (better) { S.best.rec[c] = rec; S.mine[c] = E; S.mink[c] = S.cc; }
    }
    // ---- pass 2: the body (a frame's slot is zero where nothing is written; the best slot is overwritten, so its tail is zeroed)
    int carry = 0;
    if (fits) {
        const int32_t spec0 = R.molspec ? record_at(R.spec_off, c, R.spec_stride) : 0;
        for (int base = 0; base < nmol; base += MC_THREADS) {
            const int j = base + tid;
            const int2 mj = j < nmol ? v.mol[j] : make_int2(0, 0);
            const int cnt = j < nmol ? mj.y : 0;
            int chunk;
            const int excl = record_scan(cnt, tid, s_wtot, chunk);
            s_first[tid] = j < nmol ? excl : INT_MAX;
            s_slot[tid] = mj.x;
            if (j < nmol) {
                const int32_t sp = R.molspec ? R.molspec[(size_t)spec0 + (size_t)j] : -1;
                if (ff) { ff[j] = carry + excl; fs[j] = sp; }
                if (bf) { bf[j] = carry + excl; bs[j] = sp; }
            }
            __syncthreads();
            for (int t0 = 0; t0 < chunk; t0 += MC_THREADS) {           // (the same trips for every thread: barriers inside)
                const int l = t0 + tid;
                if (l < chunk) {
                    int q = 0;                                         // last molecule of the chunk whose first atom is <= l
#pragma unroll
                    for (int step = MC_THREADS / 2; step > 0; step >>= 1)
                        if (s_first[q + step] <= l) q += step;
                    const double4 A = v.atoms[s_slot[q] + (l - s_first[q])];
                    int kind, mol;
                    unpack(A.w, kind, mol);
                    s_xyz[3 * tid] = A.x; s_xyz[3 * tid + 1] = A.y; s_xyz[3 * tid + 2] = A.z;
                    const size_t a = (size_t)(carry + l);
                    if (fk) fk[a] = kind;
                    if (bk) bk[a] = kind;
                }
                __syncthreads();
                const int n = 3 * min(chunk - t0, MC_THREADS);
                const size_t e0 = 3 * (size_t)(carry + t0);
                for (int e = tid; e < n; e += MC_THREADS) {
                    const double x = s_xyz[e];
                    if (fx) fx[e0 + e] = x;
                    if (bx) bx[e0 + e] = x;
                }
                __syncthreads();
            }
            carry += chunk;
        }
        if (tid == 0) {
            if (ff) ff[nmol] = carry;
            if (bf) bf[nmol] = carry;
        }
    }
    if (better) {
        const int a0 = fits ? carry : 0, m0 = fits ? nmol : 0, f0 = fits ? nmol + 1 : 0;
        for (size_t e = 3 * (size_t)a0 + tid; e < 3 * (size_t)S.max_atoms; e += MC_THREADS) bx[e] = 0.0;
        for (int a = a0 + tid; a < S.max_atoms; a += MC_THREADS) bk[a] = 0;
        for (int j = m0 + tid; j < S.max_molecules; j += MC_THREADS) bs[j] = 0;
        for (int j = f0 + tid; j <= S.max_molecules; j += MC_THREADS) bf[j] = 0;
    }
}

int bad_recorder(const char* what)
{
    char msg[240];
    std::snprintf(msg, sizeof msg, "recorder: %s", what);
    return merr(CEG_ERR_INVALID, msg);
}

}  // namespace

struct ceg_mcs::GroupRecorder {
    int64_t every = 0, origin = 0, capacity = 0;
    int64_t frames = 0, committed = 0;           // frames enqueued, frames of calls that ended well
    int32_t max_atoms = 1, max_molecules = 1;
    int k = 0;
    bool track_min = false, stale = false;
    bool energy_uploaded = false;                // d_energy holds `energy`
    std::vector<double> energy;                  // [K] the running energies, current between calls
    double* d_energy = nullptr;                  // [K] for ceg_mc_group_snapshot and the installation (a sweep stages its own copy)
    unsigned char* d_store = nullptr;            // [capacity] frames, then (track_min) the best slot; each: records, xyz, kind, mol_first, species
    double* d_mine = nullptr;                    // [K]
    int64_t* d_mink = nullptr;                   // [K]
    // bytes of one frame's arrays over the K chains, and their offsets inside the store
    size_t rec_bytes() const { return sizeof(ceg_mc_snapshot_record_t) * (size_t)k; }
    size_t xyz_bytes() const { return sizeof(double) * 3 * (size_t)max_atoms * (size_t)k; }
    size_t kind_bytes() const { return sizeof(int32_t) * (size_t)max_atoms * (size_t)k; }
    size_t first_bytes() const { return sizeof(int32_t) * ((size_t)max_molecules + 1) * (size_t)k; }
    size_t spec_bytes() const { return sizeof(int32_t) * (size_t)max_molecules * (size_t)k; }
    size_t slots() const { return (size_t)capacity + (track_min ? 1 : 0); }
    // the store holds each array for all slots in one piece ([slot][K][...]), so that a window of frames is one copy per array
    size_t o_rec() const { return 0; }
    size_t o_xyz() const { return o_rec() + slots() * rec_bytes(); }
    size_t o_kind() const { return o_xyz() + slots() * xyz_bytes(); }
    size_t o_first() const { return o_kind() + slots() * kind_bytes(); }
    size_t o_spec() const { return o_first() + slots() * first_bytes(); }
    size_t total() const { return o_spec() + slots() * spec_bytes(); }
    RecordSlot slot(size_t f) const
    {
        return RecordSlot{reinterpret_cast<ceg_mc_snapshot_record_t*>(d_store + o_rec() + f * rec_bytes()), reinterpret_cast<double*>(d_store + o_xyz() + f * xyz_bytes()),
                          reinterpret_cast<int32_t*>(d_store + o_kind() + f * kind_bytes()), reinterpret_cast<int32_t*>(d_store + o_first() + f * first_bytes()),
                          reinterpret_cast<int32_t*>(d_store + o_spec() + f * spec_bytes())};
    }
    bool due(int64_t cc) const { return every > 0 && cc >= origin && (cc - origin) % every == 0; }
};

void ceg_mcs::recorder_free(GroupRecorder* r)
{
    if (!r) return;
    for (void* p : {(void*)r->d_energy, (void*)r->d_store, (void*)r->d_mine, (void*)r->d_mink})
        if (p) (void)hipFree(p);
    delete r;
}

namespace {

// frames due at the ends of the cycles [cycle0, cycle0 + ncycles)
int64_t frames_due(const GroupRecorder* r, int64_t cycle0, int64_t ncycles)
{
    if (r->every <= 0 || ncycles <= 0) return 0;
    const int64_t end = cycle0 + ncycles, lo = std::max(cycle0, r->origin);
    if (lo >= end) return 0;
    const int64_t first = r->origin + (lo - r->origin + r->every - 1) / r->every * r->every;
    return first < end ? (end - 1 - first) / r->every + 1 : 0;
}

// zero the slots of the frames [from, to) again
void zero_frames(GroupRecorder* r, hipStream_t stream, int64_t from, int64_t to)
{
    if (to <= from) return;
    const size_t f = (size_t)from, n = (size_t)(to - from);
    (void)hipMemsetAsync(r->d_store + r->o_rec() + f * r->rec_bytes(), 0, n * r->rec_bytes(), stream);
    (void)hipMemsetAsync(r->d_store + r->o_xyz() + f * r->xyz_bytes(), 0, n * r->xyz_bytes(), stream);
    (void)hipMemsetAsync(r->d_store + r->o_kind() + f * r->kind_bytes(), 0, n * r->kind_bytes(), stream);
    (void)hipMemsetAsync(r->d_store + r->o_first() + f * r->first_bytes(), 0, n * r->first_bytes(), stream);
    (void)hipMemsetAsync(r->d_store + r->o_spec() + f * r->spec_bytes(), 0, n * r->spec_bytes(), stream);
}

void launch_snapshot(GroupRecorder* r, hipStream_t stream, const McView* d_views, int64_t cc, int64_t step, const RecordSource& src, bool framed, bool best)
{
    const RecordSlot none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const Snapshot S{src, framed ? r->slot((size_t)r->frames) : none, best ? r->slot((size_t)r->capacity) : none, r->d_mine, r->d_mink, cc, step,
                     r->max_atoms, r->max_molecules};
    hipLaunchKernelGGL(k_mcg_snapshot, dim3((unsigned)r->k), dim3(MC_THREADS), 0, stream, d_views, S);
}

}  // namespace

int ceg_mcs::recorder_admit(const GroupRecorder* r, const ceg_mc_cycles_t* cy, int k, bool swaps)
{
    if (r->stale) return bad_recorder("the recorder is stale after a failed sweep: call ceg_mc_group_set_recorder again");
    if (k != r->k) return bad_recorder("the group has another number of chains than the recorder");
    if (swaps && r->track_min)
        return bad_recorder("track_min with a species whose swap probability is > 0: delta_swaps is the acceptance rule's diff, not the state's energy change");
    const int64_t due = frames_due(r, cy->cycle0, cy->ncycles);
    if (due > r->capacity - r->frames) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "the call takes %lld frames and the store has room for %lld (frame_capacity %lld, %lld taken)", (long long)due,
                      (long long)(r->capacity - r->frames), (long long)r->capacity, (long long)r->frames);
        return bad_recorder(msg);
    }
    return CEG_OK;
}

bool ceg_mcs::recorder_wants(const GroupRecorder* r, int64_t cc) { return r->track_min || r->due(cc); }

void ceg_mcs::recorder_energies(const GroupRecorder* r, double* out) { memcpy(out, r->energy.data(), sizeof(double) * (size_t)r->k); }

void ceg_mcs::recorder_enqueue(GroupRecorder* r, hipStream_t stream, const McView* d_views, int k, int64_t cc, const RecordSource& src)
{
    const bool framed = r->due(cc);
    if (k != r->k || (framed && r->frames >= r->capacity)) return;    // (admitted before the first launch: cannot happen)
    launch_snapshot(r, stream, d_views, cc, (int64_t)src.last_step, src, framed, r->track_min);
    if (framed && hipPeekAtLastError() == hipSuccess) ++r->frames;    // (a frame that was not launched is not counted; the caller reads the error)
}

void ceg_mcs::recorder_commit(GroupRecorder* r, const double* energy)
{
    r->energy.assign(energy, energy + r->k);
    r->energy_uploaded = false;
    r->committed = r->frames;
}

void ceg_mcs::recorder_fail(GroupRecorder* r, hipStream_t stream)
{
    zero_frames(r, stream, r->committed, r->frames);
    r->frames = r->committed;
    r->stale = true;
}

extern "C" int ceg_mc_group_set_recorder(ceg_mc_group_t* g, const ceg_mc_recorder_t* spec)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const size_t k = (size_t)r.k;
    GroupRecorder* n = nullptr;
    if (spec) {
        if (spec->every < 0 || spec->origin < 0 || spec->frame_capacity < 0) return bad_recorder("every, origin and frame_capacity must be >= 0");
        if (spec->max_atoms < 1 || spec->max_molecules < 1) return bad_recorder("max_atoms and max_molecules must be >= 1");
        if (!spec->energy) return bad_recorder("the energies are missing");
        for (size_t c = 0; c < k; ++c)
            if (!std::isfinite(spec->energy[c])) return bad_recorder("every energy must be finite");
        n = new GroupRecorder();
        n->every = spec->every; n->origin = spec->origin; n->capacity = spec->frame_capacity;
        n->max_atoms = spec->max_atoms; n->max_molecules = spec->max_molecules;
        n->k = r.k;
        n->track_min = spec->track_min != 0;
        n->energy.assign(spec->energy, spec->energy + k);
        const double per_slot = (double)(n->rec_bytes() + n->xyz_bytes() + n->kind_bytes() + n->first_bytes() + n->spec_bytes());
        if (((double)spec->frame_capacity + 1.0) * per_slot > (double)CEG_MC_RECORDER_MAX_BYTES) {
            delete n;
            return bad_recorder("the store is too large (more than CEG_MC_RECORDER_MAX_BYTES over all frames and chains)");
        }
        for (int c = 0; n->track_min && c < r.k; ++c)
            if (r.chains[c]->poisoned) {
                delete n;
                return group_refuse_poisoned(c);
            }
    }
    Guard guard(r.device);
    if (!guard.ok || hipStreamSynchronize(r.stream) != hipSuccess) {
        delete n;
        return merr(CEG_ERR_HIP, guard.ok ? "stream synchronisation failed" : "hipSetDevice failed");
    }
    group_stream_idle(g);
    if (!spec) {
        recorder_free(*r.recorder);
        *r.recorder = nullptr;
        return CEG_OK;
    }
    std::vector<double> inf(k, std::numeric_limits<double>::infinity());
    std::vector<int64_t> never(k, -1);
    bool ok = hipMalloc((void**)&n->d_energy, sizeof(double) * k) == hipSuccess && hipMalloc((void**)&n->d_mine, sizeof(double) * k) == hipSuccess &&
              hipMalloc((void**)&n->d_mink, sizeof(int64_t) * k) == hipSuccess && hipMalloc((void**)&n->d_store, std::max(n->total(), (size_t)16)) == hipSuccess &&
              hipMemcpy(n->d_energy, n->energy.data(), sizeof(double) * k, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(n->d_mine, inf.data(), sizeof(double) * k, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(n->d_mink, never.data(), sizeof(int64_t) * k, hipMemcpyHostToDevice) == hipSuccess &&
              (n->total() == 0 || hipMemsetAsync(n->d_store, 0, n->total(), r.stream) == hipSuccess);
    n->energy_uploaded = ok;
    if (ok && n->track_min) {                    // the state now into every chain's best slot: mine = +inf loses to any finite energy
        ok = group_views_current(g);
        if (ok) {
            const RecordSource src{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, n->d_energy};
            launch_snapshot(n, r.stream, r.d_views, -1, -1, src, false, true);
            ok = hipGetLastError() == hipSuccess;
        }
    }
    ok = ok && hipStreamSynchronize(r.stream) == hipSuccess;      // (the zeroing ran on the group's stream, as the sampler's does)
    group_stream_idle(g);
    if (!ok) {
        recorder_free(n);
        return merr(CEG_ERR_HIP, "could not set up the recorder's device buffers");
    }
    recorder_free(*r.recorder);
    *r.recorder = n;
    return CEG_OK;
}

extern "C" int ceg_mc_group_snapshot(ceg_mc_group_t* g)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    GroupRecorder* n = *r.recorder;
    if (!n) return bad_recorder("the group has no recorder (ceg_mc_group_set_recorder)");
    if (n->stale) return bad_recorder("the recorder is stale after a failed sweep: call ceg_mc_group_set_recorder again");
    for (int c = 0; c < r.k; ++c)
        if (r.chains[c]->poisoned) return group_refuse_poisoned(c);
    if (n->frames >= n->capacity) return bad_recorder("the store is full (frame_capacity)");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (!n->energy_uploaded) {                   // (the copy waits for nothing on the group's stream: no launch that reads d_energy is in flight --
                                                 //  every sweep ends with a synchronisation, and an earlier snapshot left energy_uploaded set)
        if (hipMemcpy(n->d_energy, n->energy.data(), sizeof(double) * (size_t)r.k, hipMemcpyHostToDevice) != hipSuccess) return merr(CEG_ERR_HIP, "H2D of the energies failed");
        n->energy_uploaded = true;
    }
    if (!group_views_current(g)) return merr(CEG_ERR_HIP, "view upload failed");
    const RecordSource src{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, n->d_energy};
    launch_snapshot(n, r.stream, r.d_views, -1, -1, src, true, false);
    if (hipGetLastError() != hipSuccess) return merr(CEG_ERR_HIP, "snapshot kernel launch failed");
    ++n->frames;
    n->committed = n->frames;
    return CEG_OK;                               // asynchronous: ordered on the group's stream
}

extern "C" int ceg_mc_group_recorder_rebase(ceg_mc_group_t* g, const double* energy)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    GroupRecorder* n = *r.recorder;
    if (!n) return bad_recorder("the group has no recorder (ceg_mc_group_set_recorder)");
    if (!energy) return bad_recorder("the energies are missing");
    for (int c = 0; c < r.k; ++c)
        if (!std::isfinite(energy[c])) return bad_recorder("every energy must be finite");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");     // (a snapshot may still read d_energy)
    group_stream_idle(g);
    n->energy.assign(energy, energy + r.k);
    n->energy_uploaded = false;
    return CEG_OK;
}

namespace {

// slots [first, first + count) of the store's five arrays to the host, each where its pointer is not NULL
int read_slots(const GroupRecorder* n, size_t first, size_t count, ceg_mc_snapshot_record_t* rec, double* xyz, int32_t* kind, int32_t* mol_first, int32_t* species)
{
    if (count == 0) return CEG_OK;
    auto get = [&](void* dst, size_t at, size_t bytes) {
        return !dst || bytes == 0 || hipMemcpy(dst, n->d_store + at + first * bytes, count * bytes, hipMemcpyDeviceToHost) == hipSuccess;
    };
    if (!get(rec, n->o_rec(), n->rec_bytes()) || !get(xyz, n->o_xyz(), n->xyz_bytes()) || !get(kind, n->o_kind(), n->kind_bytes()) ||
        !get(mol_first, n->o_first(), n->first_bytes()) || !get(species, n->o_spec(), n->spec_bytes()))
        return merr(CEG_ERR_HIP, "D2H of the recorder's store failed");
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_mc_group_recorder_read(ceg_mc_group_t* g, int64_t first_frame, int64_t nframes, ceg_mc_snapshot_record_t* records_out, double* xyz_out,
                                          int32_t* kind_out, int32_t* mol_first_out, int32_t* species_out, int64_t* frames_out)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const GroupRecorder* n = *r.recorder;
    if (!n) return bad_recorder("the group has no recorder (ceg_mc_group_set_recorder)");
    if (first_frame < 0 || nframes < 0 || first_frame > n->frames || nframes > n->frames - first_frame)
        return bad_recorder("the window [first_frame, first_frame + nframes) lies outside the frames taken");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    if (int rc = read_slots(n, (size_t)first_frame, (size_t)nframes, records_out, xyz_out, kind_out, mol_first_out, species_out)) return rc;
    if (frames_out) *frames_out = n->frames;
    return CEG_OK;
}

extern "C" int ceg_mc_group_recorder_min(ceg_mc_group_t* g, int64_t* mink_out, double* mine_out, ceg_mc_snapshot_record_t* record_out, double* xyz_out,
                                         int32_t* kind_out, int32_t* mol_first_out, int32_t* species_out)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const GroupRecorder* n = *r.recorder;
    if (!n) return bad_recorder("the group has no recorder (ceg_mc_group_set_recorder)");
    if (!n->track_min) return bad_recorder("the recorder keeps no minimum (track_min)");
    if (n->stale) return bad_recorder("the recorder is stale after a failed sweep, whose launches may have written the minimum: call ceg_mc_group_set_recorder again");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    const size_t k = (size_t)n->k;
    if ((mink_out && hipMemcpy(mink_out, n->d_mink, sizeof(int64_t) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (mine_out && hipMemcpy(mine_out, n->d_mine, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess))
        return merr(CEG_ERR_HIP, "D2H of the minimum failed");
    return read_slots(n, (size_t)n->capacity, 1, record_out, xyz_out, kind_out, mol_first_out, species_out);
}
