// ceg_mc_group.hip -- chain groups (ceg_mc_group_*): K Markov chains, each a ceg_mc handle of ceg_mc.hip, driven together.
//   ceg_mc_group_trial / _accept   one step of K chains in one launch per class: the bodies of k_mc_trial / k_mc_accept (ceg_mc_state.h)
//   ceg_mc_group_sweep             S steps of translations and rotations: proposal, Metropolis rule and update on the device
//   ceg_mc_group_sweep_gcmc        the same with all six move kinds, swaps included, and the molecule table owned by the device
//   ceg_mc_group_set_blocks        block pockets: inblockpocket and the retry loop of choose_step!, resolved inside the GCMC trial launch
//   ceg_mc_group_sweep_cycles      either sweep over whole cycles: the same body (sweep_plain / sweep_gcmc) with a ceg_mc_cycles_t, one
//   ceg_mc_group_sweep_gcmc_cycles   launch of ceg_mc_cycles.hip behind the last step of every cycle (temperature table, dmax / thetamax)
//   ceg_mc_group_set_chain_plan      per chain: the phiPV_div_k of the swap rules and the absolute step at which the chain stops (isotherms)
//   ceg_mc_group_set_tempering       (ceg_mc_temper.hip) the *_cycles sweeps enqueue one exchange launch behind every cycle end
//   ceg_mc_group_set_recorder        (ceg_mc_record.hip) the *_cycles sweeps enqueue one snapshot launch behind the cycle ends it wants
// The two sweeps have their own kernels, per-chain parameters and read-back, and share one host driver (run_sweep).
#include "ceg_mc_gcmc.h"

using namespace ceg_mcs;

namespace {

// ---- a chain group (ceg_mc_group_*): one step of K chains in one launch per (FAST, INSERT, CELLS) class.  What a chain of the
// launch needs travels in mapped host memory like a small batch of k_mc_trial; the views stay in device memory.
struct McGroupRow {
    int32_t view, molecule, stride, _pad;    // view: index of the chain in the group (views[view]); molecule -1 for an insertion
    int64_t trial, out;                      // offsets of the chain's placements (doubles) and of its first row (rows)
    McLocal L;
};

// workgroup x of the launch: row x - ends[c - 1] of the chain c with ends[c - 1] <= x < ends[c] (ends: row prefix of the launch)
template <bool FAST, bool INSERT, bool CELLS>
__global__ __launch_bounds__(MC_THREADS, MC_TRIAL_WAVES) void k_mcg_trial(const McView* __restrict__ views, const McGroupRow* __restrict__ chains,
                                                           const int32_t* __restrict__ ends, int nchains, int table_ok,
                                                           const double* __restrict__ trial, double* __restrict__ out, unsigned* done,
                                                           unsigned long long* flag, unsigned long long seq, unsigned nblocks)
{
    __shared__ int s_chain, s_row0;
    const int x = (int)blockIdx.x;
    for (int t = threadIdx.x; t < nchains; t += MC_THREADS) {          // one round trip for the whole table
        const int lo = t > 0 ? ends[t - 1] : 0;
        if (lo <= x && x < ends[t]) { s_chain = t; s_row0 = lo; }
    }
    __syncthreads();
    const McGroupRow& C = as_constant(chains)[__builtin_amdgcn_readfirstlane(s_chain)];
    const int r = x - __builtin_amdgcn_readfirstlane(s_row0);
    const McAtChainRow at{C.out + r, r, nblocks, table_ok};
    mc_trial_row<FAST, INSERT, CELLS>(as_constant(views)[C.view], C.molecule, C.L, trial + C.trial, out, C.stride, done, flag, seq, at);
}

// one workgroup per accepted chain of a group (what the chain's update needs in pinned, device-mapped host memory)
struct McGroupAccept {
    int32_t view, molecule, stride, _pad;
    McPositions np;
    McCellOps ops;
};

__global__ __launch_bounds__(MC_THREADS) void k_mcg_accept(const McView* __restrict__ views, const McGroupAccept* __restrict__ items)
{
    const McGroupAccept& A = items[blockIdx.x];
    mc_accept_body(as_constant(views)[A.view], A.molecule, A.np, A.ops, A.stride);
}

// ---- sweeps (ceg_mc_group_sweep): the proposal and the decision of every step on the device.  Per step k_mcg_sweep_trial (rows
// before / after of every chain, the body of k_mcg_trial) and k_mcg_sweep_accept (Metropolis rule, statistics, log, the body of
// k_mcg_accept), back to back on the group's stream.  Every workgroup of a chain's step regenerates the chain's random numbers from
// (seed, step, stream id, purpose) (ceg_philox.h); what a step hands from the first kernel to the second -- the proposed positions
// and the two rows -- stays in device memory.
__device__ McCellOps d_mc_no_cell_ops;           // (sweeps refuse chains with neighbour cells: the accept body never reads it)

// workgroup (x, y): chain list[x / 2], row x % 2 (0 where the molecule is, 1 the proposal), term y of the row.  prop[3 chain + y]: the
// proposal as this workgroup's trial placement (written and read by the same threads); y = 0 is the copy k_mcg_sweep_accept reads.
template <bool FAST>
__global__ __launch_bounds__(MC_THREADS, MC_TRIAL_WAVES) void k_mcg_sweep_trial(const McView* __restrict__ views, const McSweepChain* __restrict__ params,
                                                                 const int32_t* __restrict__ bead, const int32_t* __restrict__ list, int table_ok,
                                                                 uint64_t seed, uint64_t step, McPositions* prop, double* __restrict__ rows)
{
    __shared__ McLocal s_L;
    const int c = list[blockIdx.x >> 1], r = (int)(blockIdx.x & 1u);
    const McView& v = as_constant(views)[c];
    const McSweepChain& P = as_constant(params)[c];
    const McMove mv = sweep_select(v, P, seed, step);
    if (mv.molecule < 0) return;
    const int2 mj = v.mol[mv.molecule];
    const int tid = threadIdx.x;
    if (tid < mj.y) {
        int kind, mol;
        unpack(v.atoms[mj.x + tid].w, kind, mol);
        s_L.kinds[tid] = kind;
        s_L.q[tid] = v.kind_charge[kind];
    }
    if (tid == 0) { s_L.first = mj.x; s_L.m = mj.y; }
    McPositions* mine = prop + 3 * (size_t)c + blockIdx.y;
    if (r == 1 && tid < 3 * mj.y) mine->xyz[tid] = sweep_coordinate(v, P, bead, mv, mj, seed, step, tid / 3, tid % 3);
    __syncthreads();
    const McAtChainRow at{2 * (int64_t)c + r, r, 0u, table_ok};
    mc_trial_row<FAST, false, false>(v, mv.molecule, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
}

// one workgroup per chain: compute_accept_move (src/montecarlo.jl:702-712) on the two rows, statistics, the log record, update_mc!
__global__ __launch_bounds__(MC_THREADS) void k_mcg_sweep_accept(const McView* __restrict__ views, const McSweepChain* __restrict__ params, uint64_t seed,
                                                                 uint64_t step, const McPositions* __restrict__ prop, const double* __restrict__ rows,
                                                                 ceg_mc_sweep_stats_t* __restrict__ stats, ceg_mc_sweep_record_t* __restrict__ log,
                                                                 const int64_t* __restrict__ stop)
{
    const int c = (int)blockIdx.x, tid = threadIdx.x;
    if (chain_stopped(stop, c, step)) {                            // (ceg_mc_group_set_chain_plan: the chain sat this step out)
        if (log && tid == 0) { log[c].molecule = -2; log[c].kind = -1; }
        return;
    }
    const McView& v = as_constant(views)[c];
    const McSweepChain& P = as_constant(params)[c];
    const McMove mv = sweep_select(v, P, seed, step);
    const ceg_philox::Block w = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::ACCEPT);
    const double u = ceg_philox::uniform(w.w[0], w.w[1]);
    ceg_mc_sweep_record_t* rec = log ? log + c : nullptr;          // (the record's other entries were zeroed before the first step)
    if (mv.molecule < 0) {
        if (rec && tid == 0) { rec->molecule = -1; rec->kind = -1; rec->u = u; }
        return;
    }
    const double* r = rows + 8 * (size_t)c;
    bool blocked;
    double delta;
    const int accepted = __builtin_amdgcn_readfirstlane(displacement_decision(r, u, P.temperature, blocked, delta));
    const McPositions& np = prop[3 * (size_t)c];
    if (tid == 0) {
        ceg_mc_sweep_stats_t& S = stats[c];
        if (mv.kind == 0) { S.translation_trials += 1; S.translation_accepted += accepted; }
        else { S.rotation_trials += 1; S.rotation_accepted += accepted; }
        if (blocked) S.blocked += 1;
        if (accepted) S.delta += delta;
        if (rec) {
            rec->molecule = mv.molecule; rec->kind = mv.kind; rec->accepted = accepted; rec->u = u;
            for (int t = 0; t < 8; ++t) rec->rows[t >> 2][t & 3] = r[t];
        }
    }
    if (rec && tid < 3 * v.mol[mv.molecule].y) rec->positions[tid / 3][tid % 3] = np.xyz[tid];
    if (accepted) mc_accept_body(v, mv.molecule, np, d_mc_no_cell_ops, P.stride);
}

// ---- GCMC sweeps (ceg_mc_group_sweep_gcmc): the six move kinds of src/mcmoves.jl:1-8 with the molecule table owned by the device.
// Per step k_mcg_gcmc_trial (the rows of mc_trial_row: before / after of a displacement, the current row of a deletion, the insertion
// row) and k_mcg_gcmc_accept (compute_accept_move / compute_accept_move_swap, statistics, log, and the bodies of k_mcg_accept /
// k_mc_insert / k_mc_remove).  What changes between steps -- molecule and atom counts, the species of every molecule, the counts per
// species, the stacks of freed atom slots -- sits in ordinary device memory (McGcmcTable and the arrays behind it), is written with
// ordinary stores by the accept kernel and read with ordinary loads by the next launch; the nmol / natoms entries of the chains' views
// (read through the constant address space) are not used here.

// workgroup (x, y): chain list[x / 2], row x % 2, term y of the row, as k_mcg_sweep_trial; a deletion has no row 1, an insertion no row 0
template <bool FAST>
__global__ __launch_bounds__(MC_THREADS, MC_TRIAL_WAVES) void k_mcg_gcmc_trial(const McView* __restrict__ views, const McGcmcChain* __restrict__ params,
                                                                const ceg_mc_gcmc_species_t* __restrict__ spec, int nspecies, const McGcmcTable* tables,
                                                                const int32_t* molspec, const int32_t* __restrict__ list, int table_ok, uint64_t seed,
                                                                uint64_t step, const McBlock* __restrict__ blocks, int nblock_kinds, int32_t* resolved,
                                                                McPositions* prop, double* __restrict__ rows)
{
    __shared__ McLocal s_L;
    const int c = list[blockIdx.x >> 1], r = (int)(blockIdx.x & 1u);
    const McView& v = as_constant(views)[c];
    const McGcmcChain& P = as_constant(params)[c];
    const McGcmcMove mv = gcmc_select(P, spec, nspecies, tables + c, molspec, seed, step);
    if (mv.flags) return;
    if ((mv.kind == 6 && r == 1) || (mv.kind == 5 && r == 0)) return;
    const ceg_mc_gcmc_species_t& S = spec[mv.species];
    const int2 mj = mv.kind == 5 ? make_int2(0, S.m) : v.mol[mv.molecule];
    const int tid = threadIdx.x;
    uint32_t attempt = 0;
    if (blocks && mv.kind != 6) {                // (masks installed: the same for every workgroup of the launch)
        const int w = gcmc_resolve(v, P, S, mv, mj, blocks, nspecies, nblock_kinds, seed, step);
        attempt = (uint32_t)(w >> 2);
        const bool reports = r == 1 && blockIdx.y == 0;
        if (reports && tid == 0) resolved[c] = w;
        if (w & MC_POCKET) {                     // no row is evaluated; the accept kernel logs the proposal that was tested
            if (reports && !(w & MC_EXHAUSTED) && tid < 3 * mj.y)
                prop[3 * (size_t)c].xyz[tid] = gcmc_coordinate(v, P, S, mv, mj, seed, step, attempt, tid / 3, tid % 3);
            return;
        }
    }
    if (tid < mj.y) {
        const int kind = S.kinds[tid];
        s_L.kinds[tid] = kind;
        s_L.q[tid] = v.kind_charge[kind];
    }
    if (tid == 0) { s_L.first = mj.x; s_L.m = mj.y; }
    McPositions* mine = prop + 3 * (size_t)c + blockIdx.y;
    if (r == 1 && tid < 3 * mj.y) mine->xyz[tid] = gcmc_coordinate(v, P, S, mv, mj, seed, step, attempt, tid / 3, tid % 3);
    __syncthreads();
    const McAtGcmcRow at{2 * (int64_t)c + r, mv.kind == 5 ? 0 : r, table_ok, mv.natoms};
    if (mv.kind == 5) mc_trial_row<FAST, true, false>(v, -1, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
    else mc_trial_row<FAST, false, false>(v, mv.molecule, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
}

// one workgroup per chain: the decision, statistics, the log record, the update of the state and of the chain's table
__global__ __launch_bounds__(MC_THREADS) void k_mcg_gcmc_accept(const McView* __restrict__ views, const McGcmcChain* __restrict__ params,
                                                                const ceg_mc_gcmc_species_t* __restrict__ spec, int nspecies, McGcmcTable* tables,
                                                                int32_t* molspec, int32_t* freeslots, uint64_t seed, uint64_t step,
                                                                const int32_t* resolved, int64_t* __restrict__ pockets,
                                                                const McPositions* __restrict__ prop, const double* __restrict__ rows,
                                                                ceg_mc_gcmc_stats_t* __restrict__ stats, ceg_mc_gcmc_record_t* __restrict__ log,
                                                                const double* __restrict__ chain_phi, const int64_t* __restrict__ stop)
{
    __shared__ McMolecule s_nm;
    const int c = (int)blockIdx.x, tid = threadIdx.x;
    if (chain_stopped(stop, c, step)) {                            // (ceg_mc_group_set_chain_plan: the chain sat this step out)
        if (log && tid == 0) { log[c].species = -1; log[c].molecule = -2; log[c].kind = -1; }
        return;
    }
    const McView& v = as_constant(views)[c];
    const McGcmcChain& P = as_constant(params)[c];
    McGcmcTable* T = tables + c;
    const McGcmcMove mv = gcmc_select(P, spec, nspecies, T, molspec, seed, step);
    const ceg_philox::Block w = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::ACCEPT);
    const double u = ceg_philox::uniform(w.w[0], w.w[1]);
    ceg_mc_gcmc_record_t* rec = log ? log + c : nullptr;          // (zeroed before the first step)
    ceg_mc_gcmc_stats_t& S = stats[c];
    const ceg_mc_gcmc_species_t& sp = spec[mv.species];
    const int i = mv.species, m = sp.m;
    int32_t* fstack = freeslots + P.free_off + (size_t)i * P.free_cap;
    const int nf = mv.kind == 5 ? gcmc_ld(&T->nfree[i]) : 0;
    // an insertion without a freed run takes fresh slots at the high-water mark: they must lie inside the reserved arrays
    const bool fits = mv.kind != 5 || nf > 0 || mv.natoms + m <= P.atoms_cap;
    const int flags = mv.flags | (fits ? 0 : 4);
    if (flags) {
        if (tid == 0) {
            if (flags & 1) S.spent += 1;
            else { S.trials[5] += 1; S.capacity += 1; }
            if (rec) {
                rec->species = i; rec->molecule = (flags & 1) ? -1 : mv.molecule; rec->kind = mv.kind; rec->accepted = 0;
                rec->n_species = mv.n_i; rec->flags = flags; rec->u = u;
            }
        }
        return;
    }
    const McPositions& np = prop[3 * (size_t)c];
    // what the trial launch resolved (masks installed): pockets[2c] counts the pocket-blocked steps, pockets[2c + 1] sums the attempts
    const int res = resolved && mv.kind != 6 ? gcmc_ld(resolved + c) : 0;
    const int attempt = res >> 2;
    if (res & MC_POCKET) {
        if (tid == 0) {
            S.trials[mv.kind] += 1;
            S.blocked += 1;
            pockets[2 * c] += 1;
            pockets[2 * c + 1] += attempt;
            if (rec) {
                rec->species = i; rec->molecule = mv.molecule; rec->kind = mv.kind; rec->accepted = 0;
                rec->n_species = mv.n_i; rec->flags = 8 | attempt << 16; rec->u = u;
            }
        }
        if (rec && !(res & MC_EXHAUSTED) && tid < 3 * m) rec->positions[tid / 3][tid % 3] = np.xyz[tid];
        return;
    }
    const double* r = rows + 8 * (size_t)c;
    double row[8];
    for (int t = 0; t < 8; ++t) row[t] = ((mv.kind == 6 && t >= 4) || (mv.kind == 5 && t < 4)) ? 0.0 : r[t];
    bool blocked = false;
    int acc;
    double tc = 0.0, delta;
    {
#pragma clang fp contract(off)
        if (mv.kind <= 4) {
            acc = displacement_decision(row, u, P.temperature, blocked, delta);
        } else {
            const double n = mv.kind == 5 ? 1.0 : -1.0;
            double d = sp.tail_framework;                         // modify_species_dryrun, tailcorrection.jl:86-96
            for (int j = 0; j < nspecies; ++j) {
                const int nj = gcmc_ld(&T->count[j]);
                d += (j == i ? n + 2.0 * (double)nj : 2.0 * (double)nj) * sp.tail_cross[j];
            }
            tc = d * n;
            const double temp = P.temperature;
            // the chain's own phiPV_div_k where the chain plan carries one ([K][nspecies]), else the species table's
            const double phi = chain_phi ? chain_phi[(size_t)c * (size_t)nspecies + (size_t)i] : sp.phiPV_div_k;
            if (mv.kind == 5) {
                const double E = ((row[4] + row[5]) + row[6]) + row[7];
                blocked = row[4] >= 1e90;
                delta = (E - sp.self_reciprocal) + tc;
                acc = (!blocked && u < ((phi / temp) / (double)(mv.n_i + 1)) * exp(-delta / temp)) ? 1 : 0;
            } else {
                const double E = ((row[0] + row[1]) + row[2]) + row[3];
                delta = -(E - sp.self_reciprocal) + tc;
                acc = (u < (((double)mv.n_i * temp) / phi) * exp(-delta / temp)) ? 1 : 0;
            }
        }
    }
    const int accepted = __builtin_amdgcn_readfirstlane(acc);
    if (tid == 0) {
        S.trials[mv.kind] += 1;
        S.accepted[mv.kind] += accepted;
        if (attempt) pockets[2 * c + 1] += attempt;
        if (blocked) S.blocked += 1;
        if (accepted) {
            if (mv.kind <= 4) S.delta_moves += delta;
            else S.delta_swaps += delta;
        }
        if (rec) {
            rec->species = i; rec->molecule = mv.molecule; rec->kind = mv.kind; rec->accepted = accepted;
            rec->n_species = mv.n_i; rec->flags = (blocked ? 2 : 0) | attempt << 16; rec->u = u; rec->tc = tc;
            for (int t = 0; t < 8; ++t) rec->rows[t >> 2][t & 3] = row[t];
        }
    }
    if (rec && mv.kind != 6 && tid < 3 * m) rec->positions[tid / 3][tid % 3] = np.xyz[tid];
    if (!accepted) return;
    if (mv.kind <= 4) {
        mc_accept_body(v, mv.molecule, np, d_mc_no_cell_ops, P.stride);
    } else if (mv.kind == 5) {
        const int first = nf > 0 ? gcmc_ld(fstack + nf - 1) : mv.natoms;
        if (tid < m) s_nm.kinds[tid] = sp.kinds[tid];
        if (tid == 0) s_nm.m = m;
        __syncthreads();
        mc_insert_body(v, mv.nmol, first, s_nm, np, d_mc_no_cell_ops, P.stride);
        if (tid == 0) {
            molspec[P.spec_off + mv.nmol] = i;
            T->nmol = mv.nmol + 1;
            T->count[i] = mv.n_i + 1;
            if (nf > 0) T->nfree[i] = nf - 1;
            else T->natoms = mv.natoms + m;
        }
    } else {
        const int last = mv.nmol - 1;
        const int first_gone = v.mol[mv.molecule].x;
        const int spec_last = gcmc_ld(molspec + P.spec_off + last);
        const int nfd = gcmc_ld(&T->nfree[i]);
        __syncthreads();                             // (every thread has read the table before thread 0 of the body rewrites it)
        mc_remove_body(v, mv.molecule, last, d_mc_no_cell_ops);
        if (tid == 0) {
            if (last != mv.molecule) molspec[P.spec_off + mv.molecule] = spec_last;
            if (nfd < P.free_cap) { fstack[nfd] = first_gone; T->nfree[i] = nfd + 1; }      // (a full stack cannot happen: the run would be lost, not reused)
            T->nmol = last;
            T->count[i] = mv.n_i - 1;
        }
    }
}

}  // namespace

// ---- chain groups: one step of K Markov chains (handles on one device) per trial launch and per accept launch.  The members' own
// asynchronous work runs on the group's stream while they are grouped, so per-handle calls and group calls stay in order.
struct ceg_mc_group {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<ceg_mc*> chains;
    std::vector<uint64_t> uploaded;              // v_version of each member's view in d_views (0: never uploaded)
    McView* d_views = nullptr;                   // [K] device memory, read by k_mcg_trial / k_mcg_accept
    McView* h_views = nullptr;                   // [K] pinned staging of the view uploads
    bool uploads_pending = false;                // an upload out of h_views may not have run yet
    // per-call staging, pinned and device-mapped: trial entries + row prefixes + placements in, rows out; accept entries
    unsigned char *h_in = nullptr, *dm_in = nullptr;
    double *h_out = nullptr, *dm_out = nullptr;
    McGroupAccept *h_acc = nullptr, *dm_acc = nullptr;
    bool accept_pending = false;                 // the last accept launch may still read h_acc
    unsigned long long *h_flag = nullptr, *dm_flag = nullptr;
    unsigned* d_done = nullptr;
    unsigned long long seq = 0;
    // the device memory of a sweep of either kind (SweepLayout): one block that only grows, written whole before the first step
    unsigned char* d_scratch = nullptr;
    size_t scratch_cap = 0;
    // block pockets (ceg_mc_group_set_blocks): [blk_species] species blocks then [blk_kinds] atom blocks, their masks in d_masks
    ceg_mc_block_t* d_blocks = nullptr;
    std::vector<uint8_t*> d_masks;
    int blk_species = 0, blk_kinds = 0;
    std::vector<int64_t> pockets;                // [2K] of the last GCMC sweep: pocket-blocked steps, sum of the attempt indices
    unsigned char* d_baseline = nullptr;         // partial sums and results of ceg_mc_group_baseline (ceg_mc_baseline.hip); only grows
    size_t baseline_cap = 0;
    GroupSampler* sampler = nullptr;             // density maps and series taken during sweeps (ceg_mc_sample.hip); nullptr: none
    GroupTempering* tempering = nullptr;         // rungs, energies and exchange records of the *_cycles sweeps (ceg_mc_temper.hip); nullptr: none
    GroupRecorder* recorder = nullptr;           // frames and minimum taken at the cycle ends of the *_cycles sweeps (ceg_mc_record.hip); nullptr: none
    // chain plan (ceg_mc_group_set_chain_plan): the host's copy for the checks and the launch lists, the device's for the kernels
    std::vector<double> plan_phi;                // [K][plan_species], empty: the species table's value for every chain
    std::vector<int64_t> plan_stop;              // [K], empty: no chain stops
    int plan_species = 0;
    double* d_plan_phi = nullptr;
    int64_t* d_plan_stop = nullptr;
    // device cells (ceg_mc_group_set_device_cells): ceg_mc_group_sweep / _cycles take the chains with neighbour cells
    bool device_cells = false;
    bool sweep_enqueued = false;                 // the last run_sweep got as far as its steps (a failure before that has launched and changed nothing)
    std::vector<int64_t> halted;                 // [K] of the last sweep call: the step at which a full cell halted the chain, -1: none
};

namespace {

constexpr size_t MCG_IN_BYTES = 1 << 20;         // entries, row prefixes and placements of one group trial call
constexpr size_t MCG_OUT_BYTES = 1 << 20;        // rows of one group trial call (32 768)

void group_free_blocks(ceg_mc_group* g)
{
    for (uint8_t* m : g->d_masks) (void)hipFree(m);
    g->d_masks.clear();
    if (g->d_blocks) (void)hipFree(g->d_blocks);
    g->d_blocks = nullptr;
    g->blk_species = g->blk_kinds = 0;
}

void group_free(ceg_mc_group* g)
{
    if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
    group_free_blocks(g);
    sampler_free(g->sampler);
    temper_free(g->tempering);
    recorder_free(g->recorder);
    if (g->d_views) (void)hipFree(g->d_views);
    if (g->d_done) (void)hipFree(g->d_done);
    if (g->d_scratch) (void)hipFree(g->d_scratch);
    if (g->d_baseline) (void)hipFree(g->d_baseline);
    if (g->d_plan_phi) (void)hipFree(g->d_plan_phi);
    if (g->d_plan_stop) (void)hipFree(g->d_plan_stop);
    for (void* p : {(void*)g->h_views, (void*)g->h_in, (void*)g->h_out, (void*)g->h_acc, (void*)g->h_flag})
        if (p) (void)hipHostFree(p);
    delete g;
}

int chain_err(int code, int c, const char* sep, const char* what)        // "chain <c><sep><what>"
{
    char msg[160];
    std::snprintf(msg, sizeof msg, "chain %d%s%s", c, sep, what);
    return merr(code, msg);
}

int group_bad(int c, const char* what) { return chain_err(CEG_ERR_INVALID, c, ": ", what); }

// the views of chains `used` (used[c] != 0) into d_views where they changed since their last upload, in stream order
bool group_upload_views(ceg_mc_group* g, const std::vector<char>& used)
{
    bool any = false;
    for (size_t c = 0; c < g->chains.size(); ++c)
        any = any || (used[c] && g->uploaded[c] != g->chains[c]->v_version);
    if (!any) return true;
    if (g->uploads_pending && hipStreamSynchronize(g->stream) != hipSuccess) return false;     // h_views is about to be rewritten
    for (size_t c = 0; c < g->chains.size(); ++c) {
        if (!used[c] || g->uploaded[c] == g->chains[c]->v_version) continue;
        g->h_views[c] = g->chains[c]->v;
        if (hipMemcpyAsync(g->d_views + c, g->h_views + c, sizeof(McView), hipMemcpyHostToDevice, g->stream) != hipSuccess) return false;
        g->uploaded[c] = g->chains[c]->v_version;
    }
    g->uploads_pending = true;
    return true;
}

}  // namespace

int ceg_mcs::group_refuse_poisoned(int c)
{
    return chain_err(CEG_ERR_HIP, c, " of the group is inconsistent after an earlier failure of accept / insert / remove: call ceg_mc_set_guests on it", "");
}

ceg_mcs::GroupRef ceg_mcs::group_ref(ceg_mc_group* g)
{
    return GroupRef{g->device, g->stream, g->chains.data(), (int)g->chains.size(), g->d_views, &g->d_baseline, &g->baseline_cap, &g->sampler, &g->tempering, &g->recorder};
}

bool ceg_mcs::group_views_current(ceg_mc_group* g) { return group_upload_views(g, std::vector<char>(g->chains.size(), 1)); }

void ceg_mcs::group_stream_idle(ceg_mc_group* g)
{
    g->accept_pending = false;
    g->uploads_pending = false;
}

extern "C" int ceg_mc_group_create(ceg_mc_group_t** group, ceg_mc_t* const* chains, int32_t k)
{
    if (!group || !chains || k < 1 || k > CEG_MC_GROUP_MAX) return merr(CEG_ERR_INVALID, "bad argument (1 <= k <= CEG_MC_GROUP_MAX chains)");
    *group = nullptr;
    for (int32_t c = 0; c < k; ++c) {
        ceg_mc* h = chains[c];
        if (!h) return group_bad(c, "no handle");
        if (h->device != chains[0]->device) return group_bad(c, "the handles of a group must live on one device");
        for (int32_t d = 0; d < c; ++d)
            if (chains[d] == h) return group_bad(c, "the handle appears twice");
        if (h->group) return group_bad(c, "the handle is already in a group");
        if (!h->guests_set) return group_bad(c, "ceg_mc_set_guests has never been called on the handle");
    }
    Guard guard(chains[0]->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    ceg_mc_group* g = new ceg_mc_group();
    g->device = chains[0]->device;
    g->chains.assign(chains, chains + k);
    g->uploaded.assign((size_t)k, 0);
    bool ok = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc((void**)&g->d_views, sizeof(McView) * (size_t)k) == hipSuccess &&
              hipHostMalloc((void**)&g->h_views, sizeof(McView) * (size_t)k, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&g->h_in, MCG_IN_BYTES, hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer((void**)&g->dm_in, g->h_in, 0) == hipSuccess &&
              hipHostMalloc((void**)&g->h_out, MCG_OUT_BYTES, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void**)&g->dm_out, g->h_out, 0) == hipSuccess &&
              hipHostMalloc((void**)&g->h_acc, sizeof(McGroupAccept) * (size_t)k, hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer((void**)&g->dm_acc, g->h_acc, 0) == hipSuccess &&
              hipHostMalloc((void**)&g->h_flag, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void**)&g->dm_flag, g->h_flag, 0) == hipSuccess &&
              hipMalloc((void**)&g->d_done, sizeof(unsigned)) == hipSuccess && hipMemset(g->d_done, 0, sizeof(unsigned)) == hipSuccess;
    if (ok) *g->h_flag = 0ull;
    for (int32_t c = 0; ok && c < k; ++c) ok = hipStreamSynchronize(chains[c]->stream) == hipSuccess;
    if (!ok) {
        group_free(g);
        return merr(CEG_ERR_HIP, "could not set up the chain group");
    }
    for (ceg_mc* h : g->chains) {                // from here on every member's asynchronous work goes to the group's stream
        h->group = g;
        h->own_stream = h->stream;
        h->stream = g->stream;
    }
    *group = g;
    return CEG_OK;
}

extern "C" int ceg_mc_group_destroy(ceg_mc_group_t* g)
{
    if (!g) return CEG_OK;
    Guard guard(g->device);
    const bool ok = guard.ok && hipStreamSynchronize(g->stream) == hipSuccess;
    for (ceg_mc* h : g->chains) {
        h->stream = h->own_stream;
        h->own_stream = nullptr;
        h->group = nullptr;
    }
    group_free(g);
    return ok ? CEG_OK : merr(CEG_ERR_HIP, "stream synchronisation failed");
}

extern "C" int ceg_mc_group_trial(ceg_mc_group_t* g, const int32_t* molecule, const int32_t* n, const int32_t* insert_kinds, int32_t insert_m,
                                  const double* trial, double* out)
{
    if (!g || !molecule || !n) return merr(CEG_ERR_INVALID, "bad argument");
    const int k = (int)g->chains.size();
    // chain c: its class (fast, insert, cells), rows, atoms per placement, offsets of its placements and rows
    std::vector<int> cls((size_t)k, -1), mm((size_t)k, 0);
    std::vector<int64_t> rows((size_t)k, 0), toff((size_t)k, 0), roff((size_t)k, 0);
    std::vector<char> used((size_t)k, 0);
    McMolecule nm{};
    int64_t total_rows = 0, total_in = 0;
    size_t lds = 0, pair_table = 0;
    for (int c = 0; c < k; ++c) {
        ceg_mc* h = g->chains[c];
        const int32_t mol = molecule[c];
        if (mol == -2) continue;
        if (h->poisoned) return group_refuse_poisoned(c);
        if (n[c] < 0) return group_bad(c, "negative number of placements");
        int m;
        if (mol == -1) {
            if (int rc = check_molecule(h, insert_kinds, insert_m, &nm)) return rc;
            m = insert_m;
            rows[c] = n[c];
        } else {
            if (mol < 0 || mol >= h->v.nmol) return group_bad(c, "no such molecule");
            m = h->h_mol[mol].y;
            rows[c] = (int64_t)n[c] + 1;
        }
        if (tables_bytes(h, m) > 64 * 1024) return merr(CEG_ERR_UNSUPPORTED, "k-space tables of the molecule do not fit in LDS");
        if (n[c] > 0 && !trial) return merr(CEG_ERR_INVALID, "bad argument");
        used[c] = 1;
        mm[c] = m;
        cls[c] = (h->v.fast ? 4 : 0) | (mol == -1 ? 2 : 0) | (h->v.use_cells ? 1 : 0);
        toff[c] = total_in;
        roff[c] = total_rows;
        total_in += (int64_t)n[c] * m * 3;
        total_rows += rows[c];
        lds = std::max(lds, tables_bytes(h, m));
        if (h->v.table_in_lds)
            pair_table = std::max(pair_table, pair_table_bytes(h->v));
    }
    if (total_rows > 0 && !out) return merr(CEG_ERR_INVALID, "bad argument");
    // the mapped input area: [K] entries, [K] row prefixes, the placements (8-byte aligned)
    const size_t entries_bytes = sizeof(McGroupRow) * (size_t)k, ends_bytes = (sizeof(int32_t) * (size_t)k + 15) & ~(size_t)15;
    if ((size_t)total_rows * 4 * sizeof(double) > MCG_OUT_BYTES || entries_bytes + ends_bytes + (size_t)total_in * sizeof(double) > MCG_IN_BYTES)
        return merr(CEG_ERR_UNSUPPORTED, "the call's placements or rows exceed the group's mapped staging (1 MiB each): ceg_mc_trial_device takes large batches");
    if (total_rows == 0) return CEG_OK;
    // the pair table in LDS only if the largest tables of the call leave room for it (run_trial's rule)
    const int table_ok = lds + pair_table <= 64 * 1024 ? 1 : 0;
    if (table_ok) lds += pair_table;
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (!group_upload_views(g, used)) return merr(CEG_ERR_HIP, "view upload failed");
    McGroupRow* entries = reinterpret_cast<McGroupRow*>(g->h_in);
    int32_t* ends = reinterpret_cast<int32_t*>(g->h_in + entries_bytes);
    double* tin = reinterpret_cast<double*>(g->h_in + entries_bytes + ends_bytes);
    if (total_in > 0) memcpy(tin, trial, sizeof(double) * (size_t)total_in);
    // entries grouped by class, in chain order within a class; one launch per class present
    struct Launch { int cls, first, count; int32_t rows; };
    std::vector<Launch> launches;
    int e = 0;
    for (int cl = 0; cl < 8; ++cl) {
        Launch L{cl, e, 0, 0};
        for (int c = 0; c < k; ++c) {
            if (cls[c] != cl) continue;
            ceg_mc* h = g->chains[c];
            McGroupRow& R = entries[e];
            R = McGroupRow{};
            R.view = c;
            R.molecule = molecule[c];
            R.stride = h->stride;
            R.trial = toff[c];
            R.out = roff[c];
            const bool ins = molecule[c] == -1;
            R.L.first = ins ? 0 : h->h_mol[molecule[c]].x;
            R.L.m = mm[c];
            for (int a = 0; a < mm[c]; ++a) {
                R.L.kinds[a] = ins ? nm.kinds[a] : h->h_kind[(size_t)R.L.first + a];
                R.L.q[a] = h->h_charge[(size_t)R.L.kinds[a]];
            }
            L.rows += (int32_t)rows[c];
            ends[e] = L.rows;
            ++e;
            ++L.count;
        }
        if (L.count > 0 && L.rows > 0) launches.push_back(L);
    }
    const unsigned nblocks = (unsigned)(3 * total_rows);
    ++g->seq;
    const McView* views = g->d_views;
    const double* d_in = reinterpret_cast<const double*>(g->dm_in + entries_bytes + ends_bytes);
    for (const Launch& L : launches) {
        const McGroupRow* d_entries = reinterpret_cast<const McGroupRow*>(g->dm_in) + L.first;
        const int32_t* d_ends = reinterpret_cast<const int32_t*>(g->dm_in + entries_bytes) + L.first;
        const dim3 grid((unsigned)L.rows, 3u), block(MC_THREADS);
#define CEG_MCG_LAUNCH(F, I, CL) hipLaunchKernelGGL((k_mcg_trial<F, I, CL>), grid, block, lds, g->stream, views, d_entries, d_ends, L.count, table_ok, d_in, \
                                                    g->dm_out, g->d_done, g->dm_flag, g->seq, nblocks)
        switch (L.cls) {
            case 0: CEG_MCG_LAUNCH(false, false, false); break;
            case 1: CEG_MCG_LAUNCH(false, false, true); break;
            case 2: CEG_MCG_LAUNCH(false, true, false); break;
            case 3: CEG_MCG_LAUNCH(false, true, true); break;
            case 4: CEG_MCG_LAUNCH(true, false, false); break;
            case 5: CEG_MCG_LAUNCH(true, false, true); break;
            case 6: CEG_MCG_LAUNCH(true, true, false); break;
            default: CEG_MCG_LAUNCH(true, true, true); break;
        }
#undef CEG_MCG_LAUNCH
        // (a launch that failed never raises the flag: nothing of this call is polled then, the stream is synchronised)
        if (hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(g->stream);
            return merr(CEG_ERR_HIP, "group trial kernel launch failed");
        }
    }
    if (!poll_flag(g->h_flag, g->seq) && hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "group trial kernel failed");
    g->accept_pending = false;                   // everything enqueued before this call has run
    g->uploads_pending = false;
    memcpy(out, g->h_out, sizeof(double) * 4 * (size_t)total_rows);
    return CEG_OK;
}

extern "C" int ceg_mc_group_accept(ceg_mc_group_t* g, const int32_t* molecule, const double* positions)
{
    if (!g || !molecule) return merr(CEG_ERR_INVALID, "bad argument");
    const int k = (int)g->chains.size();
    std::vector<char> used((size_t)k, 0);
    std::vector<const double*> at((size_t)k, nullptr);
    size_t off = 0, lds = 0;
    int count = 0;
    for (int c = 0; c < k; ++c) {
        if (molecule[c] < 0) continue;
        ceg_mc* h = g->chains[c];
        if (h->poisoned) return group_refuse_poisoned(c);
        if (molecule[c] >= h->v.nmol) return group_bad(c, "no such molecule");
        if (!positions) return merr(CEG_ERR_INVALID, "bad argument");
        const int m = h->h_mol[molecule[c]].y;
        used[c] = 1;
        at[c] = positions + off;
        off += 3 * (size_t)m;
        lds = std::max(lds, tables_bytes(h, m));
        ++count;
    }
    if (count == 0) return CEG_OK;
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (g->accept_pending && hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    g->accept_pending = false;
    if (!group_upload_views(g, used)) return merr(CEG_ERR_HIP, "view upload failed");
    // the cell operations of every chain on its host mirror (from here on a failure leaves the touched chains out of step)
    std::vector<char> rebuild((size_t)k, 0);
    int e = 0;
    for (int c = 0; c < k; ++c) {
        if (!used[c]) continue;
        ceg_mc* h = g->chains[c];
        McGroupAccept& A = g->h_acc[e++];
        A.view = c;
        A.molecule = molecule[c];
        A.stride = h->stride;
        A._pad = 0;
        const int m = h->h_mol[molecule[c]].y;
        for (int t = 0; t < 3 * m; ++t) A.np.xyz[t] = at[c][t];
        A.ops = McCellOps{};
        rebuild[c] = accept_cell_ops(h, molecule[c], at[c], A.ops) ? 1 : 0;
    }
    auto poison_all = [&](int rc) {
        for (int c = 0; c < k; ++c)
            if (used[c]) g->chains[c]->poisoned = true;
        return rc;
    };
    hipLaunchKernelGGL(k_mcg_accept, dim3((unsigned)count), dim3(MC_THREADS), lds, g->stream, g->d_views, g->dm_acc);
    if (hipGetLastError() != hipSuccess) return poison_all(merr(CEG_ERR_HIP, "group accept kernel launch failed"));
    g->accept_pending = true;
    for (int c = 0; c < k; ++c)          // a cell that outgrew its capacity: the whole structure again, on the group's stream
        if (rebuild[c]) {
            if (int rc = rebuild_cells(g->chains[c])) return poison_all(rc);
            g->accept_pending = false;   // (rebuild_cells leaves the stream idle)
        }
    return CEG_OK;                       // asynchronous: later calls on the group and on its members are ordered behind it
}

// ---- block pockets of a group: the masks go to the device once and stay there
extern "C" int ceg_mc_group_set_blocks(ceg_mc_group_t* g, const ceg_mc_block_t* species_blocks, int32_t nspecies, const ceg_mc_block_t* atom_blocks,
                                       int32_t nkinds)
{
    static_assert(sizeof(ceg_mc_block_t) == 240, "layout the bindings restate");
    if (!g || nspecies < 0 || nspecies > CEG_MC_GCMC_MAX_SPECIES || nkinds < 0 || (nspecies > 0 && !species_blocks) || (nkinds > 0 && !atom_blocks))
        return merr(CEG_ERR_INVALID, "bad argument (0 <= nspecies <= CEG_MC_GCMC_MAX_SPECIES, nkinds >= 0)");
    if (nspecies == 0 && nkinds > 0) return merr(CEG_ERR_INVALID, "atom blocks need the species blocks (NULL masks where a species has none)");
    std::vector<ceg_mc_block_t> all;
    all.insert(all.end(), species_blocks, species_blocks + nspecies);
    all.insert(all.end(), atom_blocks, atom_blocks + nkinds);
    for (size_t b = 0; b < all.size(); ++b) {
        const ceg_mc_block_t& B = all[b];
        bool ok = true;
        for (int d = 0; d < 3; ++d)
            ok = ok && B.dims[d] > 0 && std::isfinite(B.size[d]) && B.size[d] > 0.0 && std::isfinite(B.shift[d]) && std::isfinite(B.offset[d]);
        for (int d = 0; d < 9; ++d) ok = ok && std::isfinite(B.mat[d]) && std::isfinite(B.invmat[d]);
        if (!ok) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "%s block %d: dims must be > 0, size > 0 and the geometry finite", b < (size_t)nspecies ? "species" : "atom",
                          (int)(b < (size_t)nspecies ? b : b - (size_t)nspecies));
            return merr(CEG_ERR_INVALID, msg);
        }
    }
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    g->accept_pending = false;
    g->uploads_pending = false;
    group_free_blocks(g);
    if (all.empty()) return CEG_OK;
    bool ok = true;
    for (ceg_mc_block_t& B : all) {
        if (!B.mask) continue;
        const size_t bytes = ((size_t)B.dims[0] + 1) * ((size_t)B.dims[1] + 1) * ((size_t)B.dims[2] + 1);
        uint8_t* d = nullptr;
        ok = ok && hipMalloc((void**)&d, bytes) == hipSuccess;
        if (!ok) break;
        g->d_masks.push_back(d);
        ok = hipMemcpy(d, B.mask, bytes, hipMemcpyHostToDevice) == hipSuccess;
        B.mask = d;
    }
    ok = ok && hipMalloc((void**)&g->d_blocks, sizeof(ceg_mc_block_t) * all.size()) == hipSuccess &&
         hipMemcpy(g->d_blocks, all.data(), sizeof(ceg_mc_block_t) * all.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        group_free_blocks(g);
        return merr(CEG_ERR_HIP, "could not copy the block masks to the device");
    }
    g->blk_species = nspecies;
    g->blk_kinds = nkinds;
    return CEG_OK;
}

extern "C" int ceg_mc_group_block_counts(ceg_mc_group_t* g, int64_t* pocket_out, int64_t* attempts_out)
{
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    for (size_t c = 0; c < g->chains.size(); ++c) {
        if (pocket_out) pocket_out[c] = g->pockets.empty() ? 0 : g->pockets[2 * c];
        if (attempts_out) attempts_out[c] = g->pockets.empty() ? 0 : g->pockets[2 * c + 1];
    }
    return CEG_OK;
}

// ---- chain plan of a group: both arrays go to the device once and stay there
extern "C" int ceg_mc_group_set_chain_plan(ceg_mc_group_t* g, const ceg_mc_chain_plan_t* plan)
{
    static_assert(sizeof(ceg_mc_chain_plan_t) == 24, "layout the bindings restate");
    if (!g) return merr(CEG_ERR_INVALID, "bad argument");
    const size_t k = g->chains.size();
    const bool phi = plan && plan->phiPV_div_k, stop = plan && plan->stop_step;
    if (plan) {
        if (plan->nspecies < 0 || plan->nspecies > CEG_MC_GCMC_MAX_SPECIES) return merr(CEG_ERR_INVALID, "chain plan: 0 <= nspecies <= CEG_MC_GCMC_MAX_SPECIES");
        if (phi && plan->nspecies < 1) return merr(CEG_ERR_INVALID, "chain plan: phiPV_div_k needs nspecies >= 1");
        for (size_t c = 0; stop && c < k; ++c)
            if (plan->stop_step[c] < 0) return group_bad((int)c, "chain plan: stop_step must be >= 0");
    }
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    g->accept_pending = false;
    g->uploads_pending = false;
    // the new arrays first: a failure leaves the earlier plan installed
    double* d_phi = nullptr;
    int64_t* d_stop = nullptr;
    const size_t phi_bytes = phi ? sizeof(double) * k * (size_t)plan->nspecies : 0, stop_bytes = stop ? sizeof(int64_t) * k : 0;
    const bool ok = (!phi || (hipMalloc((void**)&d_phi, phi_bytes) == hipSuccess && hipMemcpy(d_phi, plan->phiPV_div_k, phi_bytes, hipMemcpyHostToDevice) == hipSuccess)) &&
                    (!stop || (hipMalloc((void**)&d_stop, stop_bytes) == hipSuccess && hipMemcpy(d_stop, plan->stop_step, stop_bytes, hipMemcpyHostToDevice) == hipSuccess));
    if (!ok) {
        if (d_phi) (void)hipFree(d_phi);
        if (d_stop) (void)hipFree(d_stop);
        return merr(CEG_ERR_HIP, "could not copy the chain plan to the device");
    }
    if (g->d_plan_phi) (void)hipFree(g->d_plan_phi);
    if (g->d_plan_stop) (void)hipFree(g->d_plan_stop);
    g->d_plan_phi = d_phi;
    g->d_plan_stop = d_stop;
    g->plan_species = phi ? plan->nspecies : 0;
    if (phi) g->plan_phi.assign(plan->phiPV_div_k, plan->phiPV_div_k + k * (size_t)plan->nspecies); else g->plan_phi.clear();
    if (stop) g->plan_stop.assign(plan->stop_step, plan->stop_step + k); else g->plan_stop.clear();
    return CEG_OK;
}

// ---- device cells of a group: the plain sweeps take the chains with neighbour cells
extern "C" int ceg_mc_group_set_device_cells(ceg_mc_group_t* g, int32_t on, int32_t min_capacity)
{
    if (!g || min_capacity < 0 || min_capacity > (1 << 20)) return merr(CEG_ERR_INVALID, "bad argument (0 <= min_capacity <= 2^20)");
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    for (size_t c = 0; on && min_capacity > 0 && c < g->chains.size(); ++c) {
        ceg_mc* h = g->chains[c];
        if (!h->cm.on || h->cm.cap >= min_capacity) continue;
        if (h->poisoned) return group_refuse_poisoned((int)c);
        h->cm.min_cap = min_capacity;
        if (int rc = rebuild_cells(h)) { h->poisoned = true; return rc; }
    }
    g->device_cells = on != 0;
    return CEG_OK;
}

extern "C" int ceg_mc_group_halted(ceg_mc_group_t* g, int64_t* halted_step_out)
{
    if (!g || !halted_step_out) return merr(CEG_ERR_INVALID, "bad argument");
    for (size_t c = 0; c < g->chains.size(); ++c) halted_step_out[c] = c < g->halted.size() ? g->halted[c] : -1;
    return CEG_OK;
}

// ---- what the two sweeps share on the host: the refusals, the launch plan, the layout of the group's device block and the driver
namespace {

// a chain no sweep takes: inconsistent after a failure, or with its guests in neighbour cells
int sweep_refuse_chain(const ceg_mc* h, int c, bool cells_ok = false)
{
    if (h->poisoned) return group_refuse_poisoned(c);
    if ((h->v.use_cells || h->cm.on) && !cells_ok)
        return chain_err(CEG_ERR_UNSUPPORTED, c, " keeps its guests in neighbour cells: sweeps take chains with the exhaustive pair loop only", "");
    return CEG_OK;
}

// temperature and step sizes of chain c (Params: either sweep's parameters)
// (temperature: the call's [K] values, or those of the first cycle of a table; nullptr: a table without rows, nothing to check)
template <class Params>
int sweep_check_steps(const Params* p, const double* temperature, int c)
{
    if (temperature && (!std::isfinite(temperature[c]) || !(temperature[c] > 0.0))) return group_bad(c, "the temperature must be finite and > 0");
    if (!std::isfinite(p->dmax[c]) || p->dmax[c] < 0.0) return group_bad(c, "dmax must be finite and >= 0");
    if (!std::isfinite(p->thetamax[c]) || p->thetamax[c] < 0.0) return group_bad(c, "thetamax must be finite and >= 0");
    return CEG_OK;
}

int sweep_check_stream_id(const uint32_t* stream_id, int c)
{
    for (int d = 0; d < c; ++d)
        if (stream_id[d] == stream_id[c]) return group_bad(c, "its stream id is already used by an earlier chain");
    return CEG_OK;
}

// the launches of a step: the chains by class (bit 0: fast rule energies, bit 1: neighbour cells), the LDS of their trial and
// accept kernels; add(): chain c takes part, with molecules of at most mmax atoms
constexpr int SWEEP_CLASSES = 4;
struct SweepPlan {
    std::vector<int32_t> list[SWEEP_CLASSES];
    size_t lds_trial[SWEEP_CLASSES] = {0, 0, 0, 0}, pair_table[SWEEP_CLASSES] = {0, 0, 0, 0}, lds_accept = 0;
    int add(int c, const ceg_mc* h, int mmax)
    {
        if (tables_bytes(h, mmax) > 64 * 1024) return merr(CEG_ERR_UNSUPPORTED, "k-space tables of the molecule do not fit in LDS");
        const int cl = (h->v.fast ? 1 : 0) | (h->v.use_cells ? 2 : 0);
        list[cl].push_back(c);
        lds_trial[cl] = std::max(lds_trial[cl], tables_bytes(h, mmax));
        lds_accept = std::max(lds_accept, tables_bytes(h, mmax));
        if (h->v.table_in_lds) pair_table[cl] = std::max(pair_table[cl], pair_table_bytes(h->v));
        return CEG_OK;
    }
};

// the group's device block during a sweep, in segments at 16-byte boundaries:
// [K] per-chain parameters | [K] launch lists | [3K] proposals | [8K] rows | what the sweep adds with segment(), read-back last
struct SweepLayout {
    size_t total = 0, par, list, prop, rows;
    SweepLayout(size_t k, size_t param_bytes)
        : par(segment(param_bytes * k)), list(segment(sizeof(int32_t) * k)), prop(segment(sizeof(McPositions) * 3 * k)), rows(segment(sizeof(double) * 8 * k)) {}
    size_t segment(size_t bytes) { const size_t at = total; total = (total + bytes + 15) & ~(size_t)15; return at; }
};

template <class T>
T* sweep_at(const ceg_mc_group* g, size_t offset) { return reinterpret_cast<T*>(g->d_scratch + offset); }     // (once run_sweep has sized the block)

int sweep_failed(ceg_mc_group* g)                        // some steps may have run: the chains' states are unknown
{
    for (ceg_mc* h : g->chains) h->poisoned = true;
    return merr(CEG_ERR_HIP, "a sweep kernel failed: every chain of the group is marked inconsistent");
}

// `stage` (lay.total bytes, all but the launch lists filled in) into the group's block, then nsteps steps of trial(class, grid, lds, list,
// table_ok, step) per class present and accept(grid, lds, step, record), back to back on the group's stream; afterwards the block from
// `o_back` on is back in `stage` and the records are in log_out.  A failure once the steps have started marks every chain inconsistent.
// With a sampler installed, frame(step) follows the accept launch of every step the sampler takes a frame after.  With cycle_len > 0,
// cycle_end(j) follows the last step of cycle j of the call (step s of the call with (s + 1) % cycle_len == 0), behind its frame.
template <class Record, class Trial, class Accept, class Frame, class CycleEnd>
int run_sweep(ceg_mc_group* g, const SweepPlan& plan, const SweepLayout& lay, std::vector<unsigned char>& stage, size_t o_back, uint64_t first_step,
              int64_t nsteps, Record* log_out, Trial&& trial, Accept&& accept, Frame&& frame, int64_t cycle_len, CycleEnd&& cycle_end)
{
    const size_t k = g->chains.size();
    g->sweep_enqueued = false;
    size_t lds_trial[SWEEP_CLASSES];
    int table_ok[SWEEP_CLASSES];
    for (int cl = 0; cl < SWEEP_CLASSES; ++cl) {                     // the pair table in LDS only where the largest tables leave room (run_trial's rule)
        table_ok[cl] = plan.lds_trial[cl] + plan.pair_table[cl] <= 64 * 1024 ? 1 : 0;
        lds_trial[cl] = plan.lds_trial[cl] + (table_ok[cl] ? plan.pair_table[cl] : 0);
    }
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (lay.total > g->scratch_cap) {                    // (nothing of an earlier sweep is in flight: every sweep ends with a synchronisation)
        if (g->d_scratch) (void)hipFree(g->d_scratch);
        g->d_scratch = nullptr; g->scratch_cap = 0;
        if (hipMalloc((void**)&g->d_scratch, lay.total) != hipSuccess) return merr(CEG_ERR_HIP, "hipMalloc failed");
        g->scratch_cap = lay.total;
    }
    Record* d_log = nullptr;
    const size_t log_bytes = log_out ? sizeof(Record) * k * (size_t)nsteps : 0;
    if (log_out && hipMalloc((void**)&d_log, log_bytes) != hipSuccess) return merr(CEG_ERR_HIP, "hipMalloc of the log failed");
    auto fail = [&](const char* what) {
        if (d_log) (void)hipFree(d_log);
        return merr(CEG_ERR_HIP, what);
    };
    // the launch lists; with stops in the chain plan each class in the order of its chains' stops, the latest first (chain order among
    // equals), so that the chains still running at a step are the head of their list and the trial grid shrinks with them
    const std::vector<int64_t>& stop = g->plan_stop;
    std::vector<int32_t> order[SWEEP_CLASSES] = {plan.list[0], plan.list[1], plan.list[2], plan.list[3]};
    if (!stop.empty())
        for (int cl = 0; cl < SWEEP_CLASSES; ++cl)
            std::stable_sort(order[cl].begin(), order[cl].end(), [&](int32_t a, int32_t b) { return stop[(size_t)a] > stop[(size_t)b]; });
    int32_t* l = reinterpret_cast<int32_t*>(stage.data() + lay.list);
    for (int cl = 0, e = 0; cl < SWEEP_CLASSES; ++cl)
        for (int32_t c : order[cl]) l[e++] = c;
    if (hipMemcpy(g->d_scratch, stage.data(), lay.total, hipMemcpyHostToDevice) != hipSuccess) return fail("H2D failed");
    if (!group_upload_views(g, std::vector<char>(k, 1))) return fail("view upload failed");
    if (d_log && hipMemsetAsync(d_log, 0, log_bytes, g->stream) != hipSuccess) return fail("hipMemsetAsync failed");
    g->sweep_enqueued = true;
    // ---- the steps: nothing between them but the stream's own order (no chain with a molecule and no log: nothing to do)
    const int32_t* d_list = sweep_at<const int32_t>(g, lay.list);
    unsigned first[SWEEP_CLASSES], live[SWEEP_CLASSES], listed = 0;       // live: chains of a class that have not stopped (the steps only go up)
    for (int cl = 0; cl < SWEEP_CLASSES; ++cl) {
        first[cl] = listed;
        live[cl] = (unsigned)plan.list[cl].size();
        listed += live[cl];
    }
    // (with every chain empty and no log the steps launch nothing; a sampler still takes its frames, and only those are launched)
    bool launched = true;
    const bool work = listed > 0 || d_log;
    const int64_t frames_before = g->sampler ? sampler_frames_taken(g->sampler) : 0;
    for (int64_t s = 0; s < nsteps && launched && (work || g->sampler || cycle_len > 0); ++s) {
        const uint64_t step = first_step + (uint64_t)s;
        const bool framed = g->sampler && sampler_frame_after(g->sampler, step);
        const bool ends = cycle_len > 0 && (s + 1) % cycle_len == 0;
        if (!work && !framed && !ends) continue;
        unsigned running = 0;
        for (int cl = 0; cl < SWEEP_CLASSES; ++cl) {
            if (!stop.empty())
                while (live[cl] > 0 && step >= (uint64_t)stop[(size_t)order[cl][live[cl] - 1]]) --live[cl];
            if (live[cl]) trial(cl, dim3(2u * live[cl], 3u), lds_trial[cl], d_list + first[cl], table_ok[cl], step);
            running += live[cl];
        }
        // (the accept launch keeps one workgroup per chain: a stopped chain's writes its record and returns; no chain left and no log: none)
        if (running > 0 || d_log) accept(dim3((unsigned)k), plan.lds_accept, step, d_log ? d_log + (size_t)s * k : nullptr);
        if (framed) frame(step);
        if (ends) cycle_end(s / cycle_len);
        launched = hipGetLastError() == hipSuccess;
    }
    const bool ok = hipStreamSynchronize(g->stream) == hipSuccess && launched &&
                    hipMemcpy(stage.data() + o_back, g->d_scratch + o_back, lay.total - o_back, hipMemcpyDeviceToHost) == hipSuccess &&
                    (!d_log || hipMemcpy(log_out, d_log, log_bytes, hipMemcpyDeviceToHost) == hipSuccess);
    g->accept_pending = false;
    g->uploads_pending = false;
    if (d_log) (void)hipFree(d_log);
    if (!ok && g->sampler) sampler_rollback(g->sampler, g->stream, frames_before);
    return ok ? CEG_OK : sweep_failed(g);
}

// the cycles of a call (ceg_mc_cycles.hip) on the host: `cycled` -- the call came through a *_cycles entry point, cy as it was given
struct SweepCycles {
    bool cycled;
    const ceg_mc_cycles_t* cy;
    ceg_mc_cycle_record_t* out;
    bool table() const { return cycled && cy->temperatures; }
    uint64_t last_step(uint64_t first_step, int64_t j) const { return first_step + (uint64_t)(j + 1) * (uint64_t)cy->steps_per_cycle - 1; }   // of cycle j of the call
    // the temperatures the first step runs at: the table's first row, nullptr for a table without rows, else the parameters' own
    const double* first_row(const double* temperature) const { return table() ? (cy->ncycles > 0 ? cy->temperatures : nullptr) : temperature; }
    // the three segments of the group's block the cycle ends use, behind the statistics (read back with them); none without cycles
    size_t o_rec = 0, o_table = 0, o_prior = 0;
    // tempering (ceg_mc_temper.hip), only for a call through a *_cycles entry point: the state, and without a table the segment of
    // the ladder (params->temperature, [K] by rung) that the exchange launch reads the next cycle's temperatures from
    GroupTempering* temper = nullptr;
    size_t o_ladder = 0;
    void ladder_layout(SweepLayout& lay, size_t k) { o_ladder = lay.segment(temper && !table() ? sizeof(double) * k : 0); }
    // recorder (ceg_mc_record.hip), likewise only for a *_cycles call: the recorder and the segment of the chains' energies at the call's start
    GroupRecorder* recorder = nullptr;
    size_t o_energy = 0;
    void recorder_layout(SweepLayout& lay, std::vector<unsigned char>& stage, size_t k)
    {
        o_energy = lay.segment(recorder ? sizeof(double) * k : 0);
        stage.assign(lay.total, 0);
        if (recorder) recorder_energies(recorder, reinterpret_cast<double*>(stage.data() + o_energy));
    }
    // the chain's first temperature: the caller's values are indexed by rung while a tempering state is installed
    double first_temperature(const double* temperature, int c) const { return !temperature ? 0.0 : temperature[temper ? temper_rungs(temper)[c] : c]; }
    // [K] by rung in device memory: what cycle j + 1 runs at (the call's last cycle: what it ran at)
    const double* next_row(const ceg_mc_group* g, int64_t j, size_t k) const
    {
        return table() ? sweep_at<const double>(g, o_table) + (size_t)std::min(j + 1, cy->ncycles - 1) * k : sweep_at<const double>(g, o_ladder);
    }
    void layout(SweepLayout& lay, size_t k)
    {
        if (!cycled) return;
        o_rec = lay.segment(sizeof(ceg_mc_cycle_record_t) * (size_t)cy->ncycles * k);
        o_table = lay.segment(table() ? sizeof(double) * (size_t)cy->ncycles * k : 0);
        o_prior = lay.segment(sizeof(int64_t) * 4 * k);
    }
    void fill(std::vector<unsigned char>& stage, size_t k, const double* ladder) const
    {
        if (!cycled) return;
        if (temper && !table()) memcpy(stage.data() + o_ladder, ladder, sizeof(double) * k);
        if (table()) memcpy(stage.data() + o_table, cy->temperatures, sizeof(double) * (size_t)cy->ncycles * k);
        if (cy->prior) memcpy(stage.data() + o_prior, cy->prior, sizeof(int64_t) * 4 * k);
    }
    CycleRun run(const ceg_mc_group* g) const
    {
        return CycleRun{cy->ncycles, cy->steps_per_cycle, cy->cycle0, cy->adapt, sweep_at<const int64_t>(g, o_prior),
                        table() ? sweep_at<const double>(g, o_table) : nullptr, sweep_at<ceg_mc_cycle_record_t>(g, o_rec)};
    }
    void read_back(const std::vector<unsigned char>& stage, size_t k) const
    {
        if (cycled && cy->ncycles > 0) memcpy(out, stage.data() + o_rec, sizeof(ceg_mc_cycle_record_t) * (size_t)cy->ncycles * k);
    }
};

// the device's book of chain h's cell lists from its CellMirror, where the mirror changed since the device's copy was current:
// cell_of / idx_of uploaded (8 bytes per atom slot), owner[] rebuilt from them by one launch on the group's stream.
// nslots: the atom slots the sweep can reach (slots beyond the host's lists are in no cell).
// (No sweep is in flight: every sweep ends with a synchronisation.)
int book_upload(ceg_mc_group* g, ceg_mc* h, McCellBook& B, size_t nslots)
{
    const CellMirror& cm = h->cm;
    const size_t entries = (size_t)cm.ncells() * (size_t)cm.cap;
    B = McCellBook{h->d_cell_of, h->d_idx_of, h->d_owner, (int32_t)cm.ncells(), (int32_t)nslots};
    if (h->book_version == cm.version && h->d_cell_of && h->d_owner && nslots <= h->book_slots && entries <= h->book_entries) return CEG_OK;
    h->book_version = 0;
    if (nslots > h->book_slots || !h->d_cell_of) {
        if (h->d_cell_of) (void)hipFree(h->d_cell_of);
        if (h->d_idx_of) (void)hipFree(h->d_idx_of);
        h->d_cell_of = h->d_idx_of = nullptr;
        h->book_slots = 0;
        const size_t n = std::max<size_t>(nslots, 1);
        if (hipMalloc((void**)&h->d_cell_of, sizeof(int32_t) * n) != hipSuccess || hipMalloc((void**)&h->d_idx_of, sizeof(int32_t) * n) != hipSuccess)
            return merr(CEG_ERR_HIP, "could not allocate the device's cell lists");
        h->book_slots = n;
    }
    if (entries > h->book_entries || !h->d_owner) {
        if (h->d_owner) (void)hipFree(h->d_owner);
        h->d_owner = nullptr;
        h->book_entries = 0;
        const size_t n = std::max<size_t>(entries, 1);
        if (hipMalloc((void**)&h->d_owner, sizeof(int32_t) * n) != hipSuccess) return merr(CEG_ERR_HIP, "could not allocate the device's cell lists");
        h->book_entries = n;
    }
    std::vector<int32_t> cof(std::max<size_t>(nslots, 1), -1), iof(std::max<size_t>(nslots, 1), -1);
    for (size_t s = 0; s < nslots && s < cm.cell_of.size(); ++s) { cof[s] = cm.cell_of[s]; iof[s] = cm.idx_of[s]; }
    B = McCellBook{h->d_cell_of, h->d_idx_of, h->d_owner, (int32_t)cm.ncells(), (int32_t)nslots};
    if (hipMemcpy(h->d_cell_of, cof.data(), sizeof(int32_t) * nslots, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_idx_of, iof.data(), sizeof(int32_t) * nslots, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(h->d_owner, 0xff, sizeof(int32_t) * entries, g->stream) != hipSuccess)
        return merr(CEG_ERR_HIP, "could not copy the cell lists to the device");
    cells_book_fill(g->stream, h->v, B);
    if (hipGetLastError() != hipSuccess) return merr(CEG_ERR_HIP, "could not fill the device's cell lists");
    h->book_version = cm.version;
    return CEG_OK;
}

// the CellMirror of chain h from the device's book after a sweep (the stream is idle); peak: the longest list the sweep's steps saw;
// false: the book is not a set of cell lists
bool book_read_back(ceg_mc* h, int peak)
{
    CellMirror& cm = h->cm;
    const size_t nslots = (size_t)std::max(h->v.natoms, 0), ncells = (size_t)cm.ncells();
    std::vector<int32_t> cof(std::max<size_t>(nslots, 1)), iof(std::max<size_t>(nslots, 1)), cnt(ncells);
    if (hipMemcpy(cof.data(), h->d_cell_of, sizeof(int32_t) * nslots, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(iof.data(), h->d_idx_of, sizeof(int32_t) * nslots, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cnt.data(), h->d_cell_count, sizeof(int32_t) * ncells, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    // checked on a flat copy first (every entry of every list named by exactly one atom slot), then written into the mirror's lists
    std::vector<size_t> at(ncells + 1, 0);
    int fill = 0;
    for (size_t c = 0; c < ncells; ++c) {
        if (cnt[c] < 0 || cnt[c] > cm.cap) return false;
        at[c + 1] = at[c] + (size_t)cnt[c];
        fill = std::max(fill, (int)cnt[c]);
    }
    std::vector<int32_t> flat(at[ncells], -1);
    size_t named = 0;
    for (size_t s = 0; s < nslots; ++s) {
        const int32_t c = cof[s], i = iof[s];
        if (c < 0) { cof[s] = iof[s] = -1; continue; }
        if ((size_t)c >= ncells || i < 0 || i >= cnt[(size_t)c] || flat[at[(size_t)c] + (size_t)i] != -1) return false;
        flat[at[(size_t)c] + (size_t)i] = (int32_t)s;
        ++named;
    }
    if (named != flat.size() || cm.members.size() != ncells) return false;
    for (size_t c = 0; c < ncells; ++c) cm.members[c].assign(flat.begin() + (std::ptrdiff_t)at[c], flat.begin() + (std::ptrdiff_t)at[c + 1]);
    if (cm.cell_of.size() < nslots) { cm.cell_of.resize(nslots, -1); cm.idx_of.resize(nslots, -1); }
    std::copy(cof.begin(), cof.begin() + (std::ptrdiff_t)nslots, cm.cell_of.begin());
    std::copy(iof.begin(), iof.begin() + (std::ptrdiff_t)nslots, cm.idx_of.begin());
    cm.max_fill = std::max(cm.max_fill, std::max(fill, peak));      // peak: the longest list within a step, as the host's put_in counts it
    return true;
}

// ceg_mc_group_sweep (C.cycled false: nsteps as given) and ceg_mc_group_sweep_cycles (nsteps from the cycles)
int sweep_plain(ceg_mc_group_t* g, const ceg_mc_sweep_params_t* p, int64_t nsteps, SweepCycles C, ceg_mc_sweep_stats_t* stats_out,
                ceg_mc_sweep_record_t* log_out)
{
    static_assert(sizeof(ceg_mc_sweep_record_t) == 472 && sizeof(ceg_mc_sweep_stats_t) == 48, "layouts the bindings restate");
    static_assert(sizeof(((ceg_mc_sweep_record_t*)nullptr)->positions) == sizeof(McPositions), "a record holds one placement");
    static_assert(offsetof(McSweepChain, dmax) == offsetof(McSweepChain, temperature) + 8 && offsetof(McSweepChain, thetamax) == offsetof(McSweepChain, temperature) + 16,
                  "temperature, dmax, thetamax adjacent, as CycleSource describes them");
    if (!g || !p || !stats_out || !p->stream_id || (!p->temperature && !(C.cycled && C.cy && C.cy->temperatures)) || !p->dmax || !p->thetamax || !p->p_rotation)
        return merr(CEG_ERR_INVALID, "bad argument");
    if (nsteps < 0) return merr(CEG_ERR_INVALID, "negative number of steps");
    if (g->d_blocks) return merr(CEG_ERR_UNSUPPORTED, "the group has block masks installed: only ceg_mc_group_sweep_gcmc tests block pockets");
    const int k = (int)g->chains.size();
    if (C.cycled)
        if (int rc = cycles_check(C.cy, k, p->first_step, false, C.out, &nsteps)) return rc;
    C.temper = C.cycled ? g->tempering : nullptr;        // (the plain sweep ignores a tempering state)
    C.recorder = C.cycled ? g->recorder : nullptr;       // (and a recorder)
    const double* temperature = C.first_row(p->temperature);
    // ---- every refusal before anything is launched or changed, chain by chain
    std::vector<McSweepChain> pc((size_t)k);
    std::vector<int32_t> beads;
    SweepPlan plan;
    for (int c = 0; c < k; ++c) {
        ceg_mc* h = g->chains[c];
        if (int rc = sweep_refuse_chain(h, c, g->device_cells)) return rc;
        if (int rc = sweep_check_steps(p, temperature, c)) return rc;
        if (!(p->p_rotation[c] >= 0.0 && p->p_rotation[c] <= 1.0)) return group_bad(c, "p_rotation must lie in [0, 1]");
        if (int rc = sweep_check_stream_id(p->stream_id, c)) return rc;
        McSweepChain& P = pc[(size_t)c];
        P.stream_id = p->stream_id[c];
        P.bead_off = (int32_t)beads.size();
        P.stride = h->stride;
        P.temperature = C.first_temperature(temperature, c); P.dmax = p->dmax[c]; P.thetamax = p->thetamax[c]; P.p_rotation = p->p_rotation[c];
        if (h->v.nmol > 0 && !p->bead) return merr(CEG_ERR_INVALID, "bad argument");
        int mmax = 0;
        for (int j = 0; j < h->v.nmol; ++j) {
            const int32_t b = p->bead[beads.size()];
            if (b < 0 || b >= h->h_mol[(size_t)j].y) return group_bad(c, "a bead lies outside its molecule");
            beads.push_back(b);
            mmax = std::max(mmax, h->h_mol[(size_t)j].y);
        }
        if (h->v.nmol == 0) continue;                    // (an empty chain is in no launch list: its steps are idle)
        if (int rc = plan.add(c, h, mmax)) return rc;
    }
    if (C.temper)
        if (int rc = temper_admit(C.temper, C.cy, p->temperature, k, false)) return rc;
    if (C.recorder)
        if (int rc = recorder_admit(C.recorder, C.cy, k, false)) return rc;
    if (g->sampler)
        if (int rc = sampler_admit(g->sampler, p->first_step, nsteps)) return rc;
    for (int c = 0; c < k; ++c) stats_out[c] = ceg_mc_sweep_stats_t{};
    g->halted.assign((size_t)k, -1);
    if (nsteps == 0) return CEG_OK;
    // chains with cells (device cells switched on): the book of each in the block, and the stops as a device array the accept launch
    // lowers to the halting step -- what the trial launches, the sampler and the cycle ends then read as the chain's stop
    bool with_cells = false;
    for (const ceg_mc* h : g->chains) with_cells = with_cells || h->v.use_cells;
    SweepLayout lay((size_t)k, sizeof(McSweepChain));
    const size_t o_bead = lay.segment(sizeof(int32_t) * beads.size()), o_book = lay.segment(with_cells ? sizeof(McCellBook) * (size_t)k : 0);
    C.ladder_layout(lay, (size_t)k);
    const size_t o_stats = lay.segment(sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    C.layout(lay, (size_t)k);
    const size_t o_stop = lay.segment(with_cells ? sizeof(int64_t) * (size_t)k : 0), o_halt = lay.segment(with_cells ? sizeof(int64_t) * (size_t)k : 0),
                 o_flags = lay.segment(with_cells ? sizeof(int32_t) * 2 * (size_t)k : 0);
    std::vector<unsigned char> stage;
    C.recorder_layout(lay, stage, (size_t)k);
    C.fill(stage, (size_t)k, p->temperature);
    memcpy(stage.data() + lay.par, pc.data(), sizeof(McSweepChain) * (size_t)k);
    if (!beads.empty()) memcpy(stage.data() + o_bead, beads.data(), sizeof(int32_t) * beads.size());
    if (with_cells) {
        Guard guard(g->device);
        if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
        McCellBook* books = reinterpret_cast<McCellBook*>(stage.data() + o_book);
        int64_t* st = reinterpret_cast<int64_t*>(stage.data() + o_stop);
        int64_t* ht = reinterpret_cast<int64_t*>(stage.data() + o_halt);
        for (int c = 0; c < k; ++c) {
            st[c] = g->plan_stop.empty() ? INT64_MAX : g->plan_stop[(size_t)c];
            ht[c] = -1;
            if (g->chains[c]->v.use_cells)
                if (int rc = book_upload(g, g->chains[c], books[c], (size_t)std::max(g->chains[c]->v.natoms, 0))) return rc;
        }
    }
    auto trial = [&](int cl, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        if (cl & 2)
            cells_sweep_trial(cl & 1, grid, lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), sweep_at<const int32_t>(g, o_bead), list, table_ok,
                              p->seed, step, sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows), sweep_at<const int64_t>(g, o_stop));
        else
            hipLaunchKernelGGL((cl & 1 ? k_mcg_sweep_trial<true> : k_mcg_sweep_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par),
                               sweep_at<const int32_t>(g, o_bead), list, table_ok, p->seed, step, sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_sweep_record_t* rec) {
        if (with_cells) {
            const CellSweep cs{sweep_at<const McCellBook>(g, o_book), sweep_at<int64_t>(g, o_stop), sweep_at<int64_t>(g, o_halt), sweep_at<int32_t>(g, o_flags)};
            cells_sweep_accept(grid, lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), cs, p->seed, step, sweep_at<const McPositions>(g, lay.prop),
                               sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_sweep_stats_t>(g, o_stats), rec);
            return;
        }
        hipLaunchKernelGGL(k_mcg_sweep_accept, grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), p->seed, step,
                           sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_sweep_stats_t>(g, o_stats), rec,
                           g->d_plan_stop);
    };
    int32_t max_slots = 0;
    for (const ceg_mc* h : g->chains) max_slots = std::max(max_slots, h->v.natoms);
    auto stop_of = [&]() -> const int64_t* { return with_cells ? sweep_at<const int64_t>(g, o_stop) : g->d_plan_stop; };
    auto frame = [&](uint64_t step) {                     // (the molecule table does not change: counts from the views)
        const SampleSource src{nullptr, 0, 0, &sweep_at<const ceg_mc_sweep_stats_t>(g, o_stats)->delta, nullptr, (int32_t)sizeof(ceg_mc_sweep_stats_t), max_slots,
                               stop_of(), C.temper ? temper_device_rungs(C.temper) : nullptr};
        sampler_enqueue(g->sampler, g->stream, g->d_views, k, (int64_t)step, src);
    };
    auto cycle_end = [&](int64_t j) {                     // (the molecule table does not change: counts from the views)
        const ceg_mc_sweep_stats_t* st = sweep_at<const ceg_mc_sweep_stats_t>(g, o_stats);
        const CycleSource src{&st->translation_trials, &st->translation_accepted, &st->rotation_trials, &st->rotation_accepted, &st->delta, nullptr, nullptr,
                              &sweep_at<McSweepChain>(g, lay.par)->temperature, (int32_t)sizeof(ceg_mc_sweep_stats_t), 0, (int32_t)sizeof(McSweepChain), 0,
                              stop_of(), C.last_step(p->first_step, j)};
        cycles_enqueue(g->stream, g->d_views, k, C.run(g), j, src);
        if (C.temper)
            temper_enqueue(C.temper, g->stream, k, C.run(g), j, src,
                           TemperSource{&sweep_at<const McSweepChain>(g, lay.par)->stream_id, (int32_t)sizeof(McSweepChain), 0, p->seed, C.next_row(g, j, (size_t)k)});
        if (C.recorder && recorder_wants(C.recorder, C.cy->cycle0 + j))
            recorder_enqueue(C.recorder, g->stream, g->d_views, k, C.cy->cycle0 + j,
                             RecordSource{nullptr, 0, (int32_t)sizeof(ceg_mc_sweep_stats_t), &st->delta, nullptr, nullptr, nullptr, 0, 0, stop_of(), src.last_step,
                                          sweep_at<const double>(g, C.o_energy)});
    };
    if (int rc = run_sweep(g, plan, lay, stage, o_stats, p->first_step, nsteps, log_out, trial, accept, frame, C.cycled ? C.cy->steps_per_cycle : 0, cycle_end)) {
        if (C.temper && g->sweep_enqueued) temper_fail(C.temper);       // (a failure before the steps has changed nothing: the state stays)
        if (C.recorder && g->sweep_enqueued) recorder_fail(C.recorder, g->stream);
        return rc;
    }
    if (C.recorder) {                                    // the energies after the call's last cycle, formed as the launch forms them
        const double* e0 = reinterpret_cast<const double*>(stage.data() + C.o_energy);
        std::vector<double> e((size_t)k);
        for (int c = 0; c < k; ++c) e[(size_t)c] = e0[c] + reinterpret_cast<const ceg_mc_sweep_stats_t*>(stage.data() + o_stats)[c].delta;
        recorder_commit(C.recorder, e.data());
    }
    if (C.temper && !temper_commit(C.temper, C.cy->ncycles)) return merr(CEG_ERR_HIP, "D2H of the rungs failed: the tempering state is stale");
    memcpy(stats_out, stage.data() + o_stats, sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    C.read_back(stage, (size_t)k);
    if (with_cells) {
        // ---- the host's cell lists from the device's book, for every chain with cells that accepted a move; a chain whose book
        //      failed a range check is marked inconsistent
        memcpy(g->halted.data(), stage.data() + o_halt, sizeof(int64_t) * (size_t)k);
        const int32_t* flags = reinterpret_cast<const int32_t*>(stage.data() + o_flags);
        int bad = -1;
        for (int c = 0; c < k; ++c) {
            ceg_mc* h = g->chains[c];
            if (!h->v.use_cells) continue;
            const bool moved = stats_out[c].translation_accepted + stats_out[c].rotation_accepted > 0;
            if (flags[2 * c] || (moved && !book_read_back(h, flags[2 * c + 1]))) { h->poisoned = true; bad = bad < 0 ? c : bad; }
        }
        if (bad >= 0) return chain_err(CEG_ERR_HIP, bad, ": the cell lists kept on the device failed a range check: the chain is marked inconsistent", "");
    }
    return CEG_OK;
}

// (energy + delta_moves) + delta_swaps in FP64, in this order: the energy of a chain after a GCMC call as k_mcg_snapshot forms it
double recorder_sum(double energy, const ceg_mc_gcmc_stats_t& st)
{
    const double moved = energy + st.delta_moves;
    return moved + st.delta_swaps;
}

// ceg_mc_group_sweep_gcmc and ceg_mc_group_sweep_gcmc_cycles, as sweep_plain
int sweep_gcmc(ceg_mc_group_t* g, const ceg_mc_gcmc_params_t* p, int64_t nsteps, SweepCycles C, ceg_mc_gcmc_stats_t* stats_out,
               ceg_mc_gcmc_record_t* log_out)
{
    static_assert(sizeof(ceg_mc_gcmc_species_t) == 584 && sizeof(ceg_mc_gcmc_params_t) == 88 && sizeof(ceg_mc_gcmc_stats_t) == 192 &&
                      sizeof(ceg_mc_gcmc_record_t) == 488,
                  "layouts the bindings restate");
    static_assert(sizeof(((ceg_mc_gcmc_record_t*)nullptr)->positions) == sizeof(McPositions), "a record holds one placement");
    static_assert(CEG_MC_GCMC_MAX_SPECIES >= 4, "the documented minimum");
    static_assert(offsetof(McGcmcChain, dmax) == offsetof(McGcmcChain, temperature) + 8 && offsetof(McGcmcChain, thetamax) == offsetof(McGcmcChain, temperature) + 16,
                  "temperature, dmax, thetamax adjacent, as CycleSource describes them");
    if (!g || !p || !stats_out || !p->stream_id || (!p->temperature && !(C.cycled && C.cy && C.cy->temperatures)) || !p->dmax || !p->thetamax || !p->species ||
        !p->max_molecules)
        return merr(CEG_ERR_INVALID, "bad argument");
    if (nsteps < 0) return merr(CEG_ERR_INVALID, "negative number of steps");
    const int k = (int)g->chains.size();
    const int ns = p->nspecies;
    // ---- every refusal before anything is launched or changed: the chains, the species table, then the parameters chain by chain
    for (int c = 0; c < k; ++c)
        if (int rc = sweep_refuse_chain(g->chains[c], c, g->device_cells)) return rc;
    if (ns < 1 || ns > CEG_MC_GCMC_MAX_SPECIES) return merr(CEG_ERR_INVALID, "1 <= nspecies <= CEG_MC_GCMC_MAX_SPECIES");
    const std::vector<double>& chain_phi = g->plan_phi;
    if (!chain_phi.empty() && g->plan_species != ns) return merr(CEG_ERR_INVALID, "nspecies differs from the nspecies of ceg_mc_group_set_chain_plan");
    int mmax = 1;
    int64_t swap_atoms = 0;                              // atoms of one molecule of every species that can be inserted
    for (int i = 0; i < ns; ++i) {
        const ceg_mc_gcmc_species_t& S = p->species[i];
        char msg[160];
        auto bad = [&](const char* what) {
            std::snprintf(msg, sizeof msg, "species %d: %s", i, what);
            return merr(CEG_ERR_INVALID, msg);
        };
        if (S.m < 1 || S.m > MC_MAX_ATOMS) return bad("1 <= m <= 16 atoms");
        if (S.bead < 0 || S.bead >= S.m) return bad("the bead lies outside the molecule");
        for (int a = 0; a < S.m; ++a) {
            if (S.kinds[a] < 0 || S.kinds[a] >= g->chains[0]->v.nkinds) return bad("atom kind outside the pair table");
            for (int d = 0; d < 3; ++d)
                if (!std::isfinite(S.model[a][d])) return bad("the model positions must be finite");
        }
        double prev = 0.0;
        for (int q = 0; q < 5; ++q) {
            if (!(S.cumulative[q] >= prev && S.cumulative[q] <= 1.0)) return bad("the cumulative probabilities must be non-decreasing in [0, 1]");
            prev = S.cumulative[q];
        }
        const bool swaps = S.cumulative[4] < 1.0;
        // (with per-chain values in the chain plan the table's own is not read: the plan's entries get the same check instead)
        if (swaps && chain_phi.empty() && !(std::isfinite(S.phiPV_div_k) && S.phiPV_div_k > 0.0))
            return bad("phiPV_div_k must be finite and > 0 where the swap probability is > 0");
        for (int c = 0; swaps && !chain_phi.empty() && c < k; ++c) {
            const double phi = chain_phi[(size_t)c * (size_t)ns + (size_t)i];
            if (!(std::isfinite(phi) && phi > 0.0)) return group_bad(c, "chain plan: phiPV_div_k must be finite and > 0 for a species whose swap probability is > 0");
        }
        if (!std::isfinite(S.self_reciprocal) || !std::isfinite(S.tail_framework)) return bad("self_reciprocal and the tail correction must be finite");
        for (int j = 0; j < ns; ++j)
            if (!std::isfinite(S.tail_cross[j])) return bad("self_reciprocal and the tail correction must be finite");
        mmax = std::max(mmax, (int)S.m);
        if (swaps) swap_atoms += S.m;
    }
    if (C.cycled)                                        // (a varying temperature only where no species swaps, simulation.jl:688)
        if (int rc = cycles_check(C.cy, k, p->first_step, swap_atoms > 0, C.out, &nsteps)) return rc;
    C.temper = C.cycled ? g->tempering : nullptr;        // (the plain sweep ignores a tempering state)
    C.recorder = C.cycled ? g->recorder : nullptr;       // (and a recorder)
    const double* temperature = C.first_row(p->temperature);
    if (g->d_blocks) {                                   // block pockets: the masks must be those of this species table
        if (ns != g->blk_species) return merr(CEG_ERR_INVALID, "nspecies differs from the nspecies of ceg_mc_group_set_blocks");
        for (int i = 0; i < ns && g->blk_kinds > 0; ++i)
            for (int a = 0; a < p->species[i].m; ++a)
                if (p->species[i].kinds[a] >= g->blk_kinds) return merr(CEG_ERR_INVALID, "a species' atom kind has no atom block (kind >= nkinds of ceg_mc_group_set_blocks)");
    }
    std::vector<McGcmcChain> pc((size_t)k);
    std::vector<McGcmcTable> tab((size_t)k);
    SweepPlan plan;
    size_t nspec_total = 0, nfree_total = 0, given = 0, nout_total = 0;
    std::vector<size_t> out_off((size_t)k, 0);           // chain c of molecule_species_out: the sum of max_molecules[0..c), as documented
    for (int c = 0; c < k; ++c) {
        ceg_mc* h = g->chains[c];
        if (int rc = sweep_check_steps(p, temperature, c)) return rc;
        if (int rc = sweep_check_stream_id(p->stream_id, c)) return rc;
        for (int i = 0; i < ns; ++i)
            for (int a = 0; a < p->species[i].m; ++a)
                if (p->species[i].kinds[a] >= h->v.nkinds) return group_bad(c, "a species' atom kind lies outside the chain's pair table");
        const int nmol = h->v.nmol;
        const int maxmol = p->max_molecules[c];
        if (maxmol < nmol || maxmol < 0) return group_bad(c, "max_molecules is below the chain's molecule count");
        if (nmol > 0 && !p->molecule_species) return merr(CEG_ERR_INVALID, "bad argument");
        McGcmcTable& D = tab[(size_t)c];
        D.nmol = nmol;
        D.natoms = h->v.natoms;
        for (int j = 0; j < nmol; ++j) {
            const int32_t s = p->molecule_species[given + (size_t)j];
            if (s < 0 || s >= ns) return group_bad(c, "a molecule's species lies outside the species table");
            const ceg_mc_gcmc_species_t& S = p->species[s];
            const int2 mj = h->h_mol[(size_t)j];
            if (mj.y != S.m) return group_bad(c, "a molecule's species has another atom count than the molecule");
            for (int a = 0; a < S.m; ++a)
                if (h->h_kind[(size_t)mj.x + a] != S.kinds[a]) return group_bad(c, "a molecule's species has other atom kinds than the molecule");
            D.count[s] += 1;
        }
        given += (size_t)nmol;
        if (int rc = plan.add(c, h, mmax)) return rc;    // (every chain is in a launch list: an empty one can take an insertion)
        McGcmcChain& P = pc[(size_t)c];
        P.stream_id = p->stream_id[c];
        P.stride = h->stride;
        P.max_molecules = maxmol;
        P.temperature = C.first_temperature(temperature, c); P.dmax = p->dmax[c]; P.thetamax = p->thetamax[c];
        // freed runs of the host mirror: the runs of m atoms go to the first species with m atoms
        int most = 0;
        for (int i = 0; i < ns; ++i) {
            bool firstof = true;
            for (int j = 0; j < i; ++j) firstof = firstof && p->species[j].m != p->species[i].m;
            D.nfree[i] = firstof && !h->free_runs.empty() ? (int32_t)h->free_runs[(size_t)p->species[i].m].size() : 0;
            most = std::max(most, (int)D.nfree[i]);
        }
        P.free_cap = most + std::max(maxmol, 1);
        P.spec_off = (int32_t)nspec_total;
        P.free_off = (int32_t)nfree_total;
        nspec_total += (size_t)std::max(maxmol, 1);       // (device storage: at least one entry per chain)
        out_off[(size_t)c] = nout_total;
        nout_total += (size_t)maxmol;
        nfree_total += (size_t)ns * (size_t)P.free_cap;
        // atom slots: an insertion takes a freed run of its species or fresh slots; the worst case is every insertable species filled
        // to max_molecules from fresh slots, one after the other
        const int64_t need = (int64_t)h->v.natoms + (int64_t)maxmol * swap_atoms;
        if (need > 0x3fffffff) return group_bad(c, "max_molecules is too large");
        P.atoms_cap = (int32_t)std::max<int64_t>(need, 1);
    }
    auto fill_counts = [&](int c, const McGcmcTable& D, const int32_t* ms) {
        for (int i = 0; i < CEG_MC_GCMC_MAX_SPECIES; ++i) stats_out[c].count[i] = i < ns ? D.count[i] : 0;
        stats_out[c].nmol = D.nmol;
        if (p->molecule_species_out && D.nmol > 0) memcpy(p->molecule_species_out + out_off[(size_t)c], ms, sizeof(int32_t) * (size_t)D.nmol);
    };
    if (C.temper)
        if (int rc = temper_admit(C.temper, C.cy, p->temperature, k, swap_atoms > 0)) return rc;
    if (C.recorder)
        if (int rc = recorder_admit(C.recorder, C.cy, k, swap_atoms > 0)) return rc;
    if (g->sampler)
        if (int rc = sampler_admit(g->sampler, p->first_step, nsteps)) return rc;
    for (int c = 0; c < k; ++c) stats_out[c] = ceg_mc_gcmc_stats_t{};
    g->halted.assign((size_t)k, -1);
    g->pockets.assign(2 * (size_t)k, 0);
    if (nsteps == 0) {
        size_t o = 0;
        for (int c = 0; c < k; ++c) {
            fill_counts(c, tab[(size_t)c], p->molecule_species ? p->molecule_species + o : nullptr);
            o += (size_t)tab[(size_t)c].nmol;
        }
        return CEG_OK;
    }
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    // ---- reserve atoms, mol and sf_mol of every chain for max_molecules (contents kept; a failure here has changed no state)
    for (int c = 0; c < k; ++c)
        if (int rc = ensure_capacity(g->chains[c], pc[(size_t)c].atoms_cap, std::max(pc[(size_t)c].max_molecules, 1))) return rc;
    for (int c = 0; c < k; ++c) pc[(size_t)c].atoms_cap = (int32_t)std::min<int64_t>(g->chains[c]->atoms_cap, 0x3fffffff);
    // ---- added to the common segments: [ns] species | [K] resolved attempts | [K] statistics | [K] tables | species of the molecules |
    //      stacks of freed slots | [2K] pocket counters (from the statistics on: read back after the sweep)
    SweepLayout lay((size_t)k, sizeof(McGcmcChain));
    const size_t o_spec = lay.segment(sizeof(ceg_mc_gcmc_species_t) * (size_t)ns), o_res = lay.segment(sizeof(int32_t) * (size_t)k);
    C.ladder_layout(lay, (size_t)k);
    const size_t o_stats = lay.segment(sizeof(ceg_mc_gcmc_stats_t) * (size_t)k), o_tab = lay.segment(sizeof(McGcmcTable) * (size_t)k),
                 o_ms = lay.segment(sizeof(int32_t) * nspec_total), o_free = lay.segment(sizeof(int32_t) * nfree_total),
                 o_pock = lay.segment(sizeof(int64_t) * 2 * (size_t)k);
    C.layout(lay, (size_t)k);
    // chains with cells (device cells switched on), as in sweep_plain: the books, the stops the accept launch lowers, halt and flags
    bool with_cells = false;
    for (const ceg_mc* h : g->chains) with_cells = with_cells || h->v.use_cells;
    const size_t o_stop = lay.segment(with_cells ? sizeof(int64_t) * (size_t)k : 0), o_halt = lay.segment(with_cells ? sizeof(int64_t) * (size_t)k : 0),
                 o_flags = lay.segment(with_cells ? sizeof(int32_t) * 2 * (size_t)k : 0), o_book = lay.segment(with_cells ? sizeof(McCellBook) * (size_t)k : 0);
    const ceg_mc_block_t* blocks = g->d_blocks;          // NULL: no masks, the kernels take the path without the resolve stage
    const int block_kinds = g->blk_kinds;
    std::vector<unsigned char> stage;
    C.recorder_layout(lay, stage, (size_t)k);
    C.fill(stage, (size_t)k, p->temperature);
    memcpy(stage.data() + lay.par, pc.data(), sizeof(McGcmcChain) * (size_t)k);
    memcpy(stage.data() + o_spec, p->species, sizeof(ceg_mc_gcmc_species_t) * (size_t)ns);
    memcpy(stage.data() + o_tab, tab.data(), sizeof(McGcmcTable) * (size_t)k);
    int32_t* ms = reinterpret_cast<int32_t*>(stage.data() + o_ms);
    int32_t* fr = reinterpret_cast<int32_t*>(stage.data() + o_free);
    for (int c = 0, o = 0; c < k; ++c) {
        const McGcmcChain& P = pc[(size_t)c];
        for (int j = 0; j < tab[(size_t)c].nmol; ++j) ms[P.spec_off + j] = p->molecule_species[o++];
        for (int i = 0; i < ns; ++i)
            for (int q = 0; q < tab[(size_t)c].nfree[i]; ++q)
                fr[(size_t)P.free_off + (size_t)i * P.free_cap + q] = g->chains[c]->free_runs[(size_t)p->species[i].m][(size_t)q];
    }
    if (with_cells) {
        McCellBook* books = reinterpret_cast<McCellBook*>(stage.data() + o_book);
        int64_t* sp = reinterpret_cast<int64_t*>(stage.data() + o_stop);
        int64_t* ht = reinterpret_cast<int64_t*>(stage.data() + o_halt);
        for (int c = 0; c < k; ++c) {
            sp[c] = g->plan_stop.empty() ? INT64_MAX : g->plan_stop[(size_t)c];
            ht[c] = -1;
            if (g->chains[c]->v.use_cells)               // (the lists cover every atom slot an insertion can take)
                if (int rc = book_upload(g, g->chains[c], books[c], (size_t)pc[(size_t)c].atoms_cap)) return rc;
        }
    }
    auto stop_of = [&]() -> const int64_t* { return with_cells ? sweep_at<const int64_t>(g, o_stop) : g->d_plan_stop; };
    auto trial = [&](int cl, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        if (cl & 2) {
            cells_gcmc_trial(cl & 1, grid, lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par), sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns,
                             sweep_at<const McGcmcTable>(g, o_tab), sweep_at<const int32_t>(g, o_ms), list, table_ok, p->seed, step, blocks, block_kinds,
                             sweep_at<int32_t>(g, o_res), sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows), stop_of());
            return;
        }
        hipLaunchKernelGGL((cl & 1 ? k_mcg_gcmc_trial<true> : k_mcg_gcmc_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par),
                               sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns, sweep_at<const McGcmcTable>(g, o_tab), sweep_at<const int32_t>(g, o_ms), list,
                               table_ok, p->seed, step, blocks, block_kinds, sweep_at<int32_t>(g, o_res), sweep_at<McPositions>(g, lay.prop),
                               sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_gcmc_record_t* rec) {
        if (with_cells) {
            const CellSweep cs{sweep_at<const McCellBook>(g, o_book), sweep_at<int64_t>(g, o_stop), sweep_at<int64_t>(g, o_halt), sweep_at<int32_t>(g, o_flags)};
            cells_gcmc_accept(grid, lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par), sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns,
                              sweep_at<McGcmcTable>(g, o_tab), sweep_at<int32_t>(g, o_ms), sweep_at<int32_t>(g, o_free), p->seed, step,
                              blocks ? sweep_at<const int32_t>(g, o_res) : nullptr, sweep_at<int64_t>(g, o_pock), sweep_at<const McPositions>(g, lay.prop),
                              sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_gcmc_stats_t>(g, o_stats), rec, g->d_plan_phi, cs);
            return;
        }
        hipLaunchKernelGGL(k_mcg_gcmc_accept, grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par),
                           sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns, sweep_at<McGcmcTable>(g, o_tab), sweep_at<int32_t>(g, o_ms),
                           sweep_at<int32_t>(g, o_free), p->seed, step, blocks ? sweep_at<const int32_t>(g, o_res) : nullptr, sweep_at<int64_t>(g, o_pock),
                           sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_gcmc_stats_t>(g, o_stats), rec,
                           g->d_plan_phi, g->d_plan_stop);
    };
    static_assert(offsetof(McGcmcTable, nmol) == 0 && offsetof(McGcmcTable, natoms) == 4 && offsetof(McGcmcTable, count) == 8 && sizeof(McGcmcTable) % 4 == 0,
                  "the head of a chain's table as SampleSource describes it");
    int32_t max_slots = 0;
    for (const McGcmcChain& P : pc) max_slots = std::max(max_slots, P.atoms_cap);
    auto frame = [&](uint64_t step) {                     // (counts from the device's table: the views' nmol / natoms are stale during the sweep)
        const ceg_mc_gcmc_stats_t* st = sweep_at<const ceg_mc_gcmc_stats_t>(g, o_stats);
        const SampleSource src{&sweep_at<const McGcmcTable>(g, o_tab)->nmol, (int32_t)(sizeof(McGcmcTable) / 4), ns, &st->delta_moves, &st->delta_swaps,
                               (int32_t)sizeof(ceg_mc_gcmc_stats_t), max_slots, stop_of(), C.temper ? temper_device_rungs(C.temper) : nullptr};
        sampler_enqueue(g->sampler, g->stream, g->d_views, k, (int64_t)step, src);
    };
    auto cycle_end = [&](int64_t j) {                     // (the molecule count from the device's table, as the frames)
        const ceg_mc_gcmc_stats_t* st = sweep_at<const ceg_mc_gcmc_stats_t>(g, o_stats);
        const CycleSource src{&st->trials[0], &st->accepted[0], &st->trials[1], &st->accepted[1], &st->delta_moves, &st->delta_swaps,
                              &sweep_at<const McGcmcTable>(g, o_tab)->nmol, &sweep_at<McGcmcChain>(g, lay.par)->temperature,
                              (int32_t)sizeof(ceg_mc_gcmc_stats_t), (int32_t)sizeof(McGcmcTable), (int32_t)sizeof(McGcmcChain), 0,
                              stop_of(), C.last_step(p->first_step, j)};
        cycles_enqueue(g->stream, g->d_views, k, C.run(g), j, src);
        if (C.temper)
            temper_enqueue(C.temper, g->stream, k, C.run(g), j, src,
                           TemperSource{&sweep_at<const McGcmcChain>(g, lay.par)->stream_id, (int32_t)sizeof(McGcmcChain), 0, p->seed, C.next_row(g, j, (size_t)k)});
        if (C.recorder && recorder_wants(C.recorder, C.cy->cycle0 + j))      // (counts and species from the device's table, as the frames)
            recorder_enqueue(C.recorder, g->stream, g->d_views, k, C.cy->cycle0 + j,
                             RecordSource{&sweep_at<const McGcmcTable>(g, o_tab)->nmol, (int32_t)(sizeof(McGcmcTable) / 4), (int32_t)sizeof(ceg_mc_gcmc_stats_t),
                                          &st->delta_moves, &st->delta_swaps, sweep_at<const int32_t>(g, o_ms), &sweep_at<const McGcmcChain>(g, lay.par)->spec_off,
                                          (int32_t)sizeof(McGcmcChain), 0, stop_of(), src.last_step, sweep_at<const double>(g, C.o_energy)});
    };
    if (int rc = run_sweep(g, plan, lay, stage, o_stats, p->first_step, nsteps, log_out, trial, accept, frame, C.cycled ? C.cy->steps_per_cycle : 0, cycle_end)) {
        if (C.temper && g->sweep_enqueued) temper_fail(C.temper);       // (a failure before the steps has changed nothing: the state stays)
        if (C.recorder && g->sweep_enqueued) recorder_fail(C.recorder, g->stream);
        return rc;
    }
    if (C.recorder) {                                    // the energies after the call's last cycle, formed as the launch forms them
        const double* e0 = reinterpret_cast<const double*>(stage.data() + C.o_energy);
        std::vector<double> e((size_t)k);
        for (int c = 0; c < k; ++c) e[(size_t)c] = recorder_sum(e0[c], reinterpret_cast<const ceg_mc_gcmc_stats_t*>(stage.data() + o_stats)[c]);
        recorder_commit(C.recorder, e.data());
    }
    if (C.temper && !temper_commit(C.temper, C.cy->ncycles)) return merr(CEG_ERR_HIP, "D2H of the rungs failed: the tempering state is stale");
    C.read_back(stage, (size_t)k);
    memcpy(g->pockets.data(), stage.data() + o_pock, sizeof(int64_t) * 2 * (size_t)k);
    // ---- the host mirrors from the device: molecule table, kinds, freed runs, counts and high-water mark of every chain that swapped
    const ceg_mc_gcmc_stats_t* st = reinterpret_cast<const ceg_mc_gcmc_stats_t*>(stage.data() + o_stats);
    const McGcmcTable* nt = reinterpret_cast<const McGcmcTable*>(stage.data() + o_tab);
    for (int c = 0; c < k; ++c) {
        ceg_mc* h = g->chains[c];
        const McGcmcChain& P = pc[(size_t)c];
        const McGcmcTable& D = nt[c];
        if (st[c].accepted[5] + st[c].accepted[6] == 0) continue;
        if (D.nmol < 0 || D.nmol > P.max_molecules || D.natoms < 0 || D.natoms > h->atoms_cap) return sweep_failed(g);
        std::vector<int2> mol((size_t)D.nmol);
        if (D.nmol > 0 && hipMemcpy(mol.data(), h->d_molidx, sizeof(int2) * (size_t)D.nmol, hipMemcpyDeviceToHost) != hipSuccess) return sweep_failed(g);
        h->h_mol = mol;
        h->h_kind.resize((size_t)D.natoms, 0);
        for (int j = 0; j < D.nmol; ++j) {
            const ceg_mc_gcmc_species_t& S = p->species[ms[P.spec_off + j]];
            for (int a = 0; a < S.m; ++a) h->h_kind[(size_t)mol[(size_t)j].x + a] = S.kinds[a];
        }
        if (h->free_runs.empty()) h->free_runs.assign(MC_MAX_ATOMS + 1, {});
        for (int i = 0; i < ns; ++i) h->free_runs[(size_t)p->species[i].m].clear();
        for (int i = 0; i < ns; ++i)
            for (int q = 0; q < D.nfree[i]; ++q) h->free_runs[(size_t)p->species[i].m].push_back(fr[(size_t)P.free_off + (size_t)i * P.free_cap + q]);
        h->v.nmol = D.nmol;
        h->v.natoms = D.natoms;
        ++h->v_version;
    }
    for (int c = 0; c < k; ++c) {
        stats_out[c] = st[c];
        fill_counts(c, nt[c], ms + pc[(size_t)c].spec_off);
    }
    if (with_cells) {                                    // the host's cell lists of every chain with cells that accepted a step, as in sweep_plain
        memcpy(g->halted.data(), stage.data() + o_halt, sizeof(int64_t) * (size_t)k);
        const int32_t* flags = reinterpret_cast<const int32_t*>(stage.data() + o_flags);
        int bad = -1;
        for (int c = 0; c < k; ++c) {
            ceg_mc* h = g->chains[c];
            if (!h->v.use_cells) continue;
            int64_t moved = 0;
            for (int q = 0; q < 7; ++q) moved += st[c].accepted[q];
            if (flags[2 * c] || (moved > 0 && !book_read_back(h, flags[2 * c + 1]))) { h->poisoned = true; bad = bad < 0 ? c : bad; }
        }
        if (bad >= 0) return chain_err(CEG_ERR_HIP, bad, ": the cell lists kept on the device failed a range check: the chain is marked inconsistent", "");
    }
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_mc_group_sweep(ceg_mc_group_t* g, const ceg_mc_sweep_params_t* p, int64_t nsteps, ceg_mc_sweep_stats_t* stats_out,
                                  ceg_mc_sweep_record_t* log_out)
{
    return sweep_plain(g, p, nsteps, SweepCycles{false, nullptr, nullptr}, stats_out, log_out);
}

extern "C" int ceg_mc_group_sweep_gcmc(ceg_mc_group_t* g, const ceg_mc_gcmc_params_t* p, int64_t nsteps, ceg_mc_gcmc_stats_t* stats_out,
                                       ceg_mc_gcmc_record_t* log_out)
{
    return sweep_gcmc(g, p, nsteps, SweepCycles{false, nullptr, nullptr}, stats_out, log_out);
}

extern "C" int ceg_mc_group_sweep_cycles(ceg_mc_group_t* g, const ceg_mc_sweep_params_t* p, const ceg_mc_cycles_t* cy, ceg_mc_sweep_stats_t* stats_out,
                                         ceg_mc_cycle_record_t* cycles_out, ceg_mc_sweep_record_t* log_out)
{
    return sweep_plain(g, p, 0, SweepCycles{true, cy, cycles_out}, stats_out, log_out);
}

extern "C" int ceg_mc_group_sweep_gcmc_cycles(ceg_mc_group_t* g, const ceg_mc_gcmc_params_t* p, const ceg_mc_cycles_t* cy, ceg_mc_gcmc_stats_t* stats_out,
                                              ceg_mc_cycle_record_t* cycles_out, ceg_mc_gcmc_record_t* log_out)
{
    return sweep_gcmc(g, p, 0, SweepCycles{true, cy, cycles_out}, stats_out, log_out);
}
