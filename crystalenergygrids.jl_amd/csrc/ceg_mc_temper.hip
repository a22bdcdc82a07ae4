// ceg_mc_temper.hip -- tempering of a chain group (ceg_mc_group_set_tempering / _tempering_read): replica exchange between the chains
// on neighbouring rungs of a temperature ladder at the end of a cycle (run_parallel_tempering, src/simulation.jl:461-622; the rule is
// :533, compute_accept_move(E_i, E_{i+1}, inv(inv(T_i) - inv(T_{i+1})))) as one small launch per cycle (k_mcg_exchange) on the group's
// stream.  The *_cycles sweeps of ceg_mc_sweep.hip enqueue it behind k_mcg_cycle_end; it exchanges temperatures, not configurations:
// it writes the chains' rungs, energies and records and the next cycle's temperature into the chain's parameter slot.
#include "ceg_mc_state.h"

using namespace ceg_mcs;

namespace {

static_assert(sizeof(ceg_mc_tempering_t) == 32 && sizeof(ceg_mc_exchange_record_t) == 48, "layouts the bindings restate");

struct Exchange {                                // by value (kernarg)
    CycleSource src;
    TemperSource ts;
    int32_t* rung;                               // [K]
    double* energy;                              // [K] at the call's start; the last cycle of the call stores the end's
    int64_t* pairs;                              // [K][2] attempted, accepted of the rung pair (r, r + 1)
    ceg_mc_exchange_record_t* rec;               // [K] of this cycle
    const ceg_mc_cycle_record_t* cycle;          // [K] of this cycle, as k_mcg_cycle_end has just written them
    int64_t cc, every;
    int32_t k, last;                             // last: the call's last cycle
};

template <class T>
__device__ __forceinline__ T exchange_at(const T* base, int c, int stride)
{
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)c * (size_t)stride);
}

// lane r of a due pair: a on rung r, b on rung r + 1
__device__ __forceinline__ int exchange_decision(double Ea, double Eb, double Ta, double Tb, double u, double& e)
{
#pragma clang fp contract(off)
    const double ia = 1.0 / Ta;
    const double ib = 1.0 / Tb;
    const double d = ia - ib;
    const double Tp = 1.0 / d;
    const double x = (Ea - Eb) / Tp;
    e = exp(x);
    return (Eb < Ea || u < e) ? 1 : 0;
}

// one workgroup, lane c on chain c, then lane r on the rung pair (r, r + 1), then lane c again.  Ordinary loads and stores: the
// launches before and after it on the stream are whole kernels.  Every index into the LDS arrays and into next_row is a rung that
// was range-checked here.
__global__ __launch_bounds__(CEG_MC_GROUP_MAX) void k_mcg_exchange(const Exchange X)
{
#pragma clang fp contract(off)
    __shared__ int32_t s_chain[CEG_MC_GROUP_MAX], s_stopped[CEG_MC_GROUP_MAX], s_accepted[CEG_MC_GROUP_MAX];
    __shared__ double s_energy[CEG_MC_GROUP_MAX], s_temperature[CEG_MC_GROUP_MAX], s_u[CEG_MC_GROUP_MAX], s_threshold[CEG_MC_GROUP_MAX];
    const int c = (int)threadIdx.x, k = X.k;
    const CycleSource& S = X.src;
    const bool live = c < k;
    int r = -1;
    double E = 0.0;
    s_chain[c] = -1;
    s_accepted[c] = -1;
    s_stopped[c] = 1;
    __syncthreads();
    if (live) {
        r = X.rung[c];
        E = X.energy[c] + exchange_at(S.delta_moves, c, S.stats_stride);
        if (S.delta_swaps) E = E + exchange_at(S.delta_swaps, c, S.stats_stride);
        if (r < 0 || r >= k) r = -1;             // (a permutation by construction: memory safety only)
    }
    if (r >= 0) {                                // the inverse permutation, and what the pair's lane reads, by rung
        s_chain[r] = c;
        s_energy[r] = E;
        s_temperature[r] = X.cycle[c].temperature;
        s_stopped[r] = (S.stop && S.last_step >= (uint64_t)S.stop[c]) ? 1 : 0;
    }
    __syncthreads();
    const bool round = X.cc % X.every == 0;
    const int parity = (int)((X.cc / X.every) & 1);
    if (round && c >= parity && ((c - parity) & 1) == 0 && c + 1 < k && !s_stopped[c] && !s_stopped[c + 1]) {
        const int a = s_chain[c];
        const ceg_philox::Block w = ceg_philox::draw(X.ts.seed, S.last_step, exchange_at(X.ts.stream_id, a, X.ts.param_stride), ceg_philox::EXCHANGE);
        const double u = ceg_philox::uniform(w.w[0], w.w[1]);
        double e;
        const int acc = exchange_decision(s_energy[c], s_energy[c + 1], s_temperature[c], s_temperature[c + 1], u, e);
        s_accepted[c] = acc;
        s_u[c] = u;
        s_threshold[c] = e;
        X.pairs[2 * c] += 1;
        X.pairs[2 * c + 1] += acc;
    }
    __syncthreads();
    if (!live) return;
    // the pair of this chain's rung, named by its lower rung: -1 where the rung is in no pair of this round
    int lower = -1;
    if (round && r >= 0) {
        if (r >= parity && ((r - parity) & 1) == 0) lower = r + 1 < k ? r : -1;
        else if (r - 1 >= parity) lower = r - 1;
    }
    const int acc = lower >= 0 ? s_accepted[lower] : -1;
    const int other = lower == r ? r + 1 : lower;         // the pair's other rung
    ceg_mc_exchange_record_t rec;
    rec.rung = r;
    rec.rung_next = acc == 1 ? other : r;
    rec.partner = acc >= 0 ? s_chain[other] : -1;
    rec.accepted = acc;
    rec.energy = E;
    rec.u = acc >= 0 ? s_u[lower] : 0.0;
    rec.threshold = acc >= 0 ? s_threshold[lower] : 0.0;
    double* triple = reinterpret_cast<double*>(reinterpret_cast<char*>(S.triple) + (size_t)c * (size_t)S.triple_stride);
    rec.temperature_next = rec.rung_next >= 0 ? X.ts.next_row[rec.rung_next] : triple[0];
    X.rec[c] = rec;
    X.rung[c] = rec.rung_next;
    triple[0] = rec.temperature_next;
    if (X.last) X.energy[c] = E;
}

int bad_tempering(const char* what)
{
    char msg[240];
    std::snprintf(msg, sizeof msg, "tempering: %s", what);
    return merr(CEG_ERR_INVALID, msg);
}

}  // namespace

struct ceg_mcs::GroupTempering {
    int64_t every = 1, capacity = 0, cycles = 0;
    int k = 0;
    bool stale = false;
    int32_t* d_rung = nullptr;                   // [K]
    double* d_energy = nullptr;                  // [K]
    int64_t* d_pairs = nullptr;                  // [K][2]
    ceg_mc_exchange_record_t* d_records = nullptr;       // [capacity][K]
    std::vector<int32_t> rung;                   // the host's copy, current between calls
};

void ceg_mcs::temper_free(GroupTempering* t)
{
    if (!t) return;
    for (void* p : {(void*)t->d_rung, (void*)t->d_energy, (void*)t->d_pairs, (void*)t->d_records})
        if (p) (void)hipFree(p);
    delete t;
}

const int32_t* ceg_mcs::temper_rungs(const GroupTempering* t) { return t->rung.data(); }
const int32_t* ceg_mcs::temper_device_rungs(const GroupTempering* t) { return t->d_rung; }

int ceg_mcs::temper_admit(const GroupTempering* t, const ceg_mc_cycles_t* cy, const double* ladder, int k, bool swaps)
{
    if (t->stale) return bad_tempering("the state is stale after a failed sweep: call ceg_mc_group_set_tempering again");
    if (k != t->k) return bad_tempering("the group has another number of chains than the state");
    if (swaps) return bad_tempering("a species has a swap probability > 0: exchanges under GCMC swaps are not covered (phiPV_div_k belongs to one temperature)");
    if (cy->ncycles > t->capacity - t->cycles) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "the call runs %lld cycles and the records have room for %lld (record_capacity %lld, %lld taken)",
                      (long long)cy->ncycles, (long long)(t->capacity - t->cycles), (long long)t->capacity, (long long)t->cycles);
        return bad_tempering(msg);
    }
    const int64_t rows = cy->temperatures ? cy->ncycles : 1;
    for (int64_t j = 0; j < rows; ++j) {
        const double* row = cy->temperatures ? cy->temperatures + (size_t)j * (size_t)k : ladder;
        for (int r = 0; row && r + 1 < k; ++r)
            if (!(row[r] <= row[r + 1])) return bad_tempering("the temperatures are indexed by rung: every row must be non-decreasing");
    }
    return CEG_OK;
}

void ceg_mcs::temper_enqueue(GroupTempering* t, hipStream_t stream, int k, const CycleRun& run, int64_t j, const CycleSource& src, const TemperSource& ts)
{
    if (k != t->k || t->cycles + j >= t->capacity) return;        // (admitted before the first launch: cannot happen)
    const Exchange X{src, ts, t->d_rung, t->d_energy, t->d_pairs, t->d_records + (size_t)(t->cycles + j) * (size_t)k,
                     run.d_records + (size_t)j * (size_t)k, run.cycle0 + j, t->every, k, j + 1 == run.ncycles ? 1 : 0};
    hipLaunchKernelGGL(k_mcg_exchange, dim3(1u), dim3((unsigned)CEG_MC_GROUP_MAX), 0, stream, X);
}

bool ceg_mcs::temper_commit(GroupTempering* t, int64_t ncycles)
{
    if (hipMemcpy(t->rung.data(), t->d_rung, sizeof(int32_t) * (size_t)t->k, hipMemcpyDeviceToHost) != hipSuccess) {
        t->stale = true;
        return false;
    }
    t->cycles += ncycles;
    return true;
}

void ceg_mcs::temper_fail(GroupTempering* t) { t->stale = true; }

extern "C" int ceg_mc_group_set_tempering(ceg_mc_group_t* g, const ceg_mc_tempering_t* spec)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const size_t k = (size_t)r.k;
    std::vector<int32_t> rung(k);
    if (spec) {
        if (spec->every < 1) return bad_tempering("every must be >= 1");
        if (spec->record_capacity < 0 || (uint64_t)spec->record_capacity > (uint64_t)1 << 32) return bad_tempering("record_capacity must lie in [0, 2^32]");
        std::vector<char> seen(k, 0);
        for (size_t c = 0; c < k; ++c) {
            const int32_t q = spec->rung ? spec->rung[c] : (int32_t)c;
            if (q < 0 || (size_t)q >= k || seen[(size_t)q]) return bad_tempering("rung must be a permutation of 0..K-1");
            seen[(size_t)q] = 1;
            rung[c] = q;
        }
        if (!spec->energy) return bad_tempering("the energies are missing");
        for (size_t c = 0; c < k; ++c)
            if (!std::isfinite(spec->energy[c])) return bad_tempering("every energy must be finite");
    }
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    if (!spec) {
        temper_free(*r.tempering);
        *r.tempering = nullptr;
        return CEG_OK;
    }
    GroupTempering* t = new GroupTempering();
    t->every = spec->every; t->capacity = spec->record_capacity;
    t->k = r.k;
    t->rung = rung;
    const size_t rec_bytes = sizeof(ceg_mc_exchange_record_t) * (size_t)t->capacity * k;
    const bool ok = hipMalloc((void**)&t->d_rung, sizeof(int32_t) * k) == hipSuccess && hipMalloc((void**)&t->d_energy, sizeof(double) * k) == hipSuccess &&
                    hipMalloc((void**)&t->d_pairs, sizeof(int64_t) * 2 * k) == hipSuccess &&
                    (rec_bytes == 0 || hipMalloc((void**)&t->d_records, rec_bytes) == hipSuccess) &&
                    hipMemcpy(t->d_rung, rung.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(t->d_energy, spec->energy, sizeof(double) * k, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemsetAsync(t->d_pairs, 0, sizeof(int64_t) * 2 * k, r.stream) == hipSuccess &&
                    (rec_bytes == 0 || hipMemsetAsync(t->d_records, 0, rec_bytes, r.stream) == hipSuccess) &&
                    hipStreamSynchronize(r.stream) == hipSuccess;      // (the zeroing ran on the group's stream, as the sampler's does)
    if (!ok) {
        temper_free(t);
        return merr(CEG_ERR_HIP, "could not allocate the tempering state's device buffers");
    }
    temper_free(*r.tempering);
    *r.tempering = t;
    return CEG_OK;
}

extern "C" int ceg_mc_group_tempering_read(ceg_mc_group_t* g, int32_t* rung_out, double* energy_out, int64_t* pair_counts_out,
                                           ceg_mc_exchange_record_t* records_out, int64_t* cycles_out)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const GroupRef r = group_ref(g);
    const GroupTempering* t = *r.tempering;
    if (!t) return bad_tempering("the group has no tempering state (ceg_mc_group_set_tempering)");
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(r.stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    const size_t k = (size_t)t->k;
    if ((rung_out && hipMemcpy(rung_out, t->d_rung, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (energy_out && hipMemcpy(energy_out, t->d_energy, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (pair_counts_out && hipMemcpy(pair_counts_out, t->d_pairs, sizeof(int64_t) * 2 * k, hipMemcpyDeviceToHost) != hipSuccess) ||
        (records_out && t->cycles > 0 &&
         hipMemcpy(records_out, t->d_records, sizeof(ceg_mc_exchange_record_t) * (size_t)t->cycles * k, hipMemcpyDeviceToHost) != hipSuccess))
        return merr(CEG_ERR_HIP, "D2H of the tempering state failed");
    if (cycles_out) *cycles_out = t->cycles;
    return CEG_OK;
}
