// ceg_mc_sweep.hip -- the sweeps of a chain group (struct ceg_mc_group, ceg_mc_group.h): whole runs of steps of K chains on the device.
//   ceg_mc_group_sweep             S steps of translations and rotations: proposal, Metropolis rule and update on the device
//   ceg_mc_group_sweep_gcmc        the same with all six move kinds, swaps included, and the molecule table owned by the device
//   ceg_mc_group_sweep_cycles, _sweep_gcmc_cycles   either sweep over whole cycles: behind the last step of every cycle one launch of
//       ceg_mc_cycles.hip, the exchange of ceg_mc_temper.hip and the snapshot of ceg_mc_record.hip where the group has them installed
// A sweep has its own kernels (here those of the chains with the exhaustive pair loop; ceg_mc_cells.hip: with neighbour cells),
// per-chain parameters, checks and read-back; the host driver (run_sweep) owns the group's block, the launch lists, the steps, the
// sampler's frames and the cycle ends, which it finds through the sweep's SweepWhere.  SweepCells: the segments of the chains with
// cells; SweepCycles: what a *_cycles call adds before, during and after the run.
#include "ceg_mc_gcmc.h"
#include "ceg_mc_group.h"

using namespace ceg_mcs;

namespace {

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
// [K] per-chain parameters | [K] launch lists | [3K] proposals | [8K] rows | what the sweep adds with segment(), read-back last;
// stage: the host's copy of the block (SweepCycles::stage, the last to add a segment, sizes it), staged<T>(offset) into it
struct SweepLayout {
    size_t total = 0, par, list, prop, rows;
    std::vector<unsigned char> stage;
    SweepLayout(size_t k, size_t param_bytes)
        : par(segment(param_bytes * k)), list(segment(sizeof(int32_t) * k)), prop(segment(sizeof(McPositions) * 3 * k)), rows(segment(sizeof(double) * 8 * k)) {}
    size_t segment(size_t bytes) { const size_t at = total; total = (total + bytes + 15) & ~(size_t)15; return at; }
    template <class T>
    T* staged(size_t offset) { return reinterpret_cast<T*>(stage.data() + offset); }
};

template <class T>
T* sweep_at(const ceg_mc_group* g, size_t offset) { return reinterpret_cast<T*>(g->d_scratch + offset); }     // (once run_sweep has sized the block)

int sweep_failed(ceg_mc_group* g)                        // some steps may have run: the chains' states are unknown
{
    for (ceg_mc* h : g->chains) h->poisoned = true;
    return merr(CEG_ERR_HIP, "a sweep kernel failed: every chain of the group is marked inconsistent");
}

// the cycles of a call (ceg_mc_cycles.hip) on the host: `cycled` -- the call came through a *_cycles entry point, cy as it was given.
// Around the run a sweep calls begin() where its checks reach the cycles, admit() behind its last check, finish() behind run_sweep.
struct SweepCycles {
    bool cycled;
    const ceg_mc_cycles_t* cy;
    ceg_mc_cycle_record_t* out;
    bool table() const { return cycled && cy->temperatures; }
    int64_t cycle_len() const { return cycled ? cy->steps_per_cycle : 0; }
    uint64_t last_step(uint64_t first_step, int64_t j) const { return first_step + (uint64_t)(j + 1) * (uint64_t)cy->steps_per_cycle - 1; }   // of cycle j of the call
    // the three segments of the group's block the cycle ends use, behind the statistics (read back with them); none without cycles
    size_t o_rec = 0, o_table = 0, o_prior = 0;
    // tempering (ceg_mc_temper.hip), only for a call through a *_cycles entry point: the state, and without a table the segment of
    // the ladder (params->temperature, [K] by rung) that the exchange launch reads the next cycle's temperatures from
    GroupTempering* temper = nullptr;
    size_t o_ladder = 0;
    // recorder (ceg_mc_record.hip), likewise only for a *_cycles call: the recorder and the segment of the chains' energies at the call's start
    GroupRecorder* recorder = nullptr;
    size_t o_energy = 0;
    // the cycles checked (*nsteps from them) and the group's tempering state and recorder taken (a call without cycles ignores both);
    // *first_row: the temperatures the first step runs at -- the table's first row, nullptr for a table without rows, else the parameters' own
    // (swaps: a varying temperature only where no species swaps, simulation.jl:688)
    int begin(const ceg_mc_group* g, uint64_t first_step, bool swaps, const double* temperature, int64_t* nsteps, const double** first_row)
    {
        if (int rc = cycled ? cycles_check(cy, (int)g->chains.size(), first_step, swaps, out, nsteps) : CEG_OK) return rc;
        temper = cycled ? g->tempering : nullptr;
        recorder = cycled ? g->recorder : nullptr;
        *first_row = table() ? (cy->ncycles > 0 ? cy->temperatures : nullptr) : temperature;
        return CEG_OK;
    }
    // the chain's first temperature: the caller's values are indexed by rung while a tempering state is installed
    double first_temperature(const double* temperature, int c) const { return !temperature ? 0.0 : temperature[temper ? temper_rungs(temper)[c] : c]; }
    // the last refusals of a call, then the first thing it changes: no chain has halted
    int admit(ceg_mc_group* g, const double* ladder, uint64_t first_step, int64_t nsteps, bool swaps) const
    {
        const int k = (int)g->chains.size();
        if (int rc = temper ? temper_admit(temper, cy, ladder, k, swaps) : CEG_OK) return rc;
        if (int rc = recorder ? recorder_admit(recorder, cy, k, swaps) : CEG_OK) return rc;
        if (int rc = g->sampler ? sampler_admit(g->sampler, first_step, nsteps) : CEG_OK) return rc;
        g->halted.assign((size_t)k, -1);
        return CEG_OK;
    }
    void ladder_layout(SweepLayout& lay, size_t k) { o_ladder = lay.segment(temper && !table() ? sizeof(double) * k : 0); }
    void layout(SweepLayout& lay, size_t k)
    {
        if (!cycled) return;
        o_rec = lay.segment(sizeof(ceg_mc_cycle_record_t) * (size_t)cy->ncycles * k);
        o_table = lay.segment(table() ? sizeof(double) * (size_t)cy->ncycles * k : 0);
        o_prior = lay.segment(sizeof(int64_t) * 4 * k);
    }
    // the last segment of a block, then lay.stage at its size with the recorder's energies and what the cycles stage
    void stage(SweepLayout& lay, size_t k, const double* ladder)
    {
        o_energy = lay.segment(recorder ? sizeof(double) * k : 0);
        lay.stage.assign(lay.total, 0);
        if (recorder) recorder_energies(recorder, lay.staged<double>(o_energy));
        if (!cycled) return;
        if (temper && !table()) memcpy(lay.staged<double>(o_ladder), ladder, sizeof(double) * k);
        if (table()) memcpy(lay.staged<double>(o_table), cy->temperatures, sizeof(double) * (size_t)cy->ncycles * k);
        if (cy->prior) memcpy(lay.staged<int64_t>(o_prior), cy->prior, sizeof(int64_t) * 4 * k);
    }
    CycleRun run(const ceg_mc_group* g) const
    {
        return CycleRun{cy->ncycles, cy->steps_per_cycle, cy->cycle0, cy->adapt, sweep_at<const int64_t>(g, o_prior),
                        table() ? sweep_at<const double>(g, o_table) : nullptr, sweep_at<ceg_mc_cycle_record_t>(g, o_rec)};
    }
    // [K] by rung in device memory: what cycle j + 1 runs at (the call's last cycle: what it ran at)
    const double* next_row(const ceg_mc_group* g, int64_t j, size_t k) const
    {
        return table() ? sweep_at<const double>(g, o_table) + (size_t)std::min(j + 1, cy->ncycles - 1) * k : sweep_at<const double>(g, o_ladder);
    }
    // behind run_sweep (rc: what it returned).  A failure once the steps were enqueued leaves tempering state and recorder stale (before
    // that it has changed nothing: both stay).  Else the recorder gets the energies after the call's last cycle, formed as the launch
    // forms them -- after(energy at the call's start, chain) is the sweep's own sum -- the tempering state its rungs, the caller the records.
    template <class After>
    int finish(ceg_mc_group* g, int rc, SweepLayout& lay, After&& after) const
    {
        const size_t k = g->chains.size();
        if (rc && temper && g->sweep_enqueued) temper_fail(temper);
        if (rc && recorder && g->sweep_enqueued) recorder_fail(recorder, g->stream);
        if (rc) return rc;
        std::vector<double> e(recorder ? k : 0);
        for (size_t c = 0; c < e.size(); ++c) e[c] = after(lay.staged<const double>(o_energy)[c], (int)c);
        if (recorder) recorder_commit(recorder, e.data());
        if (temper && !temper_commit(temper, cy->ncycles)) return merr(CEG_ERR_HIP, "D2H of the rungs failed: the tempering state is stale");
        if (cycled && cy->ncycles > 0) memcpy(out, lay.staged<const ceg_mc_cycle_record_t>(o_rec), sizeof(ceg_mc_cycle_record_t) * (size_t)cy->ncycles * k);
        return CEG_OK;
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

// chains with cells in a sweep (device cells switched on): the book of each in the group's block, and the stops as a device array the
// accept launch lowers to the halting step -- what the trial launches, the sampler and the cycle ends then read as the chain's stop.
// Four segments behind SweepCycles::layout (read back with the statistics); none where no chain of the group has cells.
struct SweepCells {
    bool with_cells = false;
    size_t o_stop = 0, o_halt = 0, o_flags = 0, o_book = 0;
    explicit SweepCells(const ceg_mc_group* g) { for (const ceg_mc* h : g->chains) with_cells = with_cells || h->v.use_cells; }
    void layout(SweepLayout& lay, size_t k)
    {
        o_stop = lay.segment(with_cells ? sizeof(int64_t) * k : 0), o_halt = lay.segment(with_cells ? sizeof(int64_t) * k : 0);
        o_flags = lay.segment(with_cells ? sizeof(int32_t) * 2 * k : 0), o_book = lay.segment(with_cells ? sizeof(McCellBook) * k : 0);
    }
    // the stops, no halt, and the book of every chain with cells; nslots(c): the atom slots the sweep can reach in chain c
    template <class Slots>
    int fill(ceg_mc_group* g, SweepLayout& lay, Slots&& nslots) const
    {
        if (!with_cells) return CEG_OK;
        for (size_t c = 0; c < g->chains.size(); ++c) {
            lay.staged<int64_t>(o_stop)[c] = g->plan_stop.empty() ? INT64_MAX : g->plan_stop[c];
            lay.staged<int64_t>(o_halt)[c] = -1;
            if (g->chains[c]->v.use_cells)
                if (int rc = book_upload(g, g->chains[c], lay.staged<McCellBook>(o_book)[c], nslots((int)c))) return rc;
        }
        return CEG_OK;
    }
    CellSweep cell_sweep(const ceg_mc_group* g) const
    {
        return CellSweep{sweep_at<const McCellBook>(g, o_book), sweep_at<int64_t>(g, o_stop), sweep_at<int64_t>(g, o_halt), sweep_at<int32_t>(g, o_flags)};
    }
    const int64_t* stop_of(const ceg_mc_group* g) const { return with_cells ? sweep_at<const int64_t>(g, o_stop) : g->d_plan_stop; }
    // after the sweep: the halting steps, and the host's cell lists from the device's book for every chain with cells that accepted a
    // step (accepted[c] > 0); a chain whose book failed a range check is marked inconsistent
    int read_back(ceg_mc_group* g, SweepLayout& lay, const std::vector<int64_t>& accepted) const
    {
        if (!with_cells) return CEG_OK;
        const size_t k = g->chains.size();
        memcpy(g->halted.data(), lay.staged<const int64_t>(o_halt), sizeof(int64_t) * k);
        const int32_t* flags = lay.staged<const int32_t>(o_flags);
        int bad = -1;
        for (size_t c = 0; c < k; ++c) {
            ceg_mc* h = g->chains[c];
            if (!h->v.use_cells) continue;
            if (flags[2 * c] || (accepted[c] > 0 && !book_read_back(h, flags[2 * c + 1]))) { h->poisoned = true; bad = bad < 0 ? (int)c : bad; }
        }
        return bad < 0 ? CEG_OK : chain_err(CEG_ERR_HIP, bad, ": the cell lists kept on the device failed a range check: the chain is marked inconsistent", "");
    }
};

// where a sweep keeps what the sampler's frames and the cycle ends read: byte offsets into the group's block (NOWHERE: the sweep
// has no such thing), entry of chain 0 with the stride to the next chain's.  A sweep fills it once, behind its layout; run_sweep forms
// SampleSource, CycleSource, TemperSource and RecordSource from it once the block has its address.
constexpr size_t NOWHERE = ~(size_t)0;
struct SweepWhere {
    size_t stats, stats_stride;                          // the statistics (the block is read back from here on), and in them:
    size_t translation_trials, translation_accepted, rotation_trials, rotation_accepted;     // the counters CycleSource names
    size_t delta_moves, delta_swaps;                     // the running sum(s) of the accepted changes
    size_t counts, counts_stride;                        // (molecules, high-water mark, molecules per species [ns]); NOWHERE: the views' nmol / natoms
    int32_t ns;
    size_t temperature, stream_id, param_stride;         // in the per-chain parameters (temperature, dmax, thetamax adjacent)
    size_t molspec, spec_off;                            // the species of the molecules, and each chain's first entry in the parameters
    int32_t max_slots;                                   // no chain's high-water mark exceeds this during the sweep
    size_t stop;                                         // SweepCells::o_stop; NOWHERE: the chain plan's own array
};

// lay.stage (all but the launch lists filled in) into the group's block, then nsteps steps of trial(class, grid, lds, list, table_ok,
// step) per class present and accept(grid, lds, step, record), back to back on the group's stream; afterwards the block from the
// statistics on is back in lay.stage and the records are in log_out.  A failure once the steps have started marks every chain inconsistent.
// With a sampler installed, a frame follows the accept launch of every step the sampler takes a frame after.  In a call with cycles
// the cycle end, then the exchange of a tempering state, then the snapshot a recorder wants follow the last step of every cycle (step s
// of the call with (s + 1) % cycle_len == 0), behind its frame.
template <class Record, class Trial, class Accept>
int run_sweep(ceg_mc_group* g, const SweepPlan& plan, SweepLayout& lay, const SweepWhere& W, const SweepCycles& C, uint64_t seed, uint64_t first_step,
              int64_t nsteps, Record* log_out, Trial&& trial, Accept&& accept)
{
    const size_t k = g->chains.size();
    const int64_t cycle_len = C.cycle_len();
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
    int32_t* l = lay.staged<int32_t>(lay.list);
    for (int cl = 0, e = 0; cl < SWEEP_CLASSES; ++cl)
        for (int32_t c : order[cl]) l[e++] = c;
    if (hipMemcpy(g->d_scratch, lay.stage.data(), lay.total, hipMemcpyHostToDevice) != hipSuccess) return fail("H2D failed");
    if (!group_upload_views(g, std::vector<char>(k, 1))) return fail("view upload failed");
    if (d_log && hipMemsetAsync(d_log, 0, log_bytes, g->stream) != hipSuccess) return fail("hipMemsetAsync failed");
    g->sweep_enqueued = true;
    // ---- what the frames and the cycle ends read, from the sweep's description (the block has its address now)
    auto i32 = [&](size_t offset) { return offset == NOWHERE ? nullptr : sweep_at<const int32_t>(g, offset); };
    auto i64 = [&](size_t offset) { return offset == NOWHERE ? nullptr : sweep_at<const int64_t>(g, offset); };
    auto f64 = [&](size_t offset) { return offset == NOWHERE ? nullptr : sweep_at<double>(g, offset); };
    const int64_t* d_stop = W.stop == NOWHERE ? g->d_plan_stop : i64(W.stop);
    const int32_t counts_stride = (int32_t)(W.counts_stride / 4);
    const SampleSource frame_src{i32(W.counts), counts_stride, W.ns, f64(W.delta_moves), f64(W.delta_swaps), (int32_t)W.stats_stride, W.max_slots,
                                 d_stop, C.temper ? temper_device_rungs(C.temper) : nullptr};
    CycleSource cycle_src{i64(W.translation_trials), i64(W.translation_accepted), i64(W.rotation_trials), i64(W.rotation_accepted), f64(W.delta_moves),
                          f64(W.delta_swaps), i32(W.counts), f64(W.temperature), (int32_t)W.stats_stride, (int32_t)W.counts_stride, (int32_t)W.param_stride,
                          0, d_stop, 0};
    auto cycle_end = [&](int64_t j) {                     // cycle j of the call has had its last step
        cycle_src.last_step = C.last_step(first_step, j);
        cycles_enqueue(g->stream, g->d_views, (int)k, C.run(g), j, cycle_src);
        if (C.temper)
            temper_enqueue(C.temper, g->stream, (int)k, C.run(g), j, cycle_src,
                           TemperSource{sweep_at<const uint32_t>(g, W.stream_id), (int32_t)W.param_stride, 0, seed, C.next_row(g, j, k)});
        if (C.recorder && recorder_wants(C.recorder, C.cy->cycle0 + j))
            recorder_enqueue(C.recorder, g->stream, g->d_views, (int)k, C.cy->cycle0 + j,
                             RecordSource{i32(W.counts), counts_stride, (int32_t)W.stats_stride, f64(W.delta_moves), f64(W.delta_swaps), i32(W.molspec),
                                          i32(W.spec_off), W.spec_off == NOWHERE ? 0 : (int32_t)W.param_stride, 0, d_stop, cycle_src.last_step,
                                          sweep_at<const double>(g, C.o_energy)});
    };
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
        if (framed) sampler_enqueue(g->sampler, g->stream, g->d_views, (int)k, (int64_t)step, frame_src);
        if (ends) cycle_end(s / cycle_len);
        launched = hipGetLastError() == hipSuccess;
    }
    const bool ok = hipStreamSynchronize(g->stream) == hipSuccess && launched &&
                    hipMemcpy(lay.stage.data() + W.stats, g->d_scratch + W.stats, lay.total - W.stats, hipMemcpyDeviceToHost) == hipSuccess &&
                    (!d_log || hipMemcpy(log_out, d_log, log_bytes, hipMemcpyDeviceToHost) == hipSuccess);
    g->accept_pending = false;
    g->uploads_pending = false;
    if (d_log) (void)hipFree(d_log);
    if (!ok && g->sampler) sampler_rollback(g->sampler, g->stream, frames_before);
    return ok ? CEG_OK : sweep_failed(g);
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
    const double* temperature;
    if (int rc = C.begin(g, p->first_step, false, p->temperature, &nsteps, &temperature)) return rc;
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
    if (int rc = C.admit(g, p->temperature, p->first_step, nsteps, false)) return rc;
    for (int c = 0; c < k; ++c) stats_out[c] = ceg_mc_sweep_stats_t{};
    if (nsteps == 0) return CEG_OK;
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    // ---- added to the common segments: the beads | [K] statistics (from here on: read back after the sweep)
    SweepCells cells(g);
    SweepLayout lay((size_t)k, sizeof(McSweepChain));
    const size_t o_bead = lay.segment(sizeof(int32_t) * beads.size());
    C.ladder_layout(lay, (size_t)k);
    const size_t o_stats = lay.segment(sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    C.layout(lay, (size_t)k);
    cells.layout(lay, (size_t)k);
    C.stage(lay, (size_t)k, p->temperature);
    memcpy(lay.staged<McSweepChain>(lay.par), pc.data(), sizeof(McSweepChain) * (size_t)k);
    if (!beads.empty()) memcpy(lay.staged<int32_t>(o_bead), beads.data(), sizeof(int32_t) * beads.size());
    if (int rc = cells.fill(g, lay, [&](int c) { return (size_t)std::max(g->chains[c]->v.natoms, 0); })) return rc;
    SweepWhere W{};                                      // (the molecule table does not change: counts from the views)
    W.stats = o_stats; W.stats_stride = sizeof(ceg_mc_sweep_stats_t);
    W.translation_trials = o_stats + offsetof(ceg_mc_sweep_stats_t, translation_trials); W.translation_accepted = o_stats + offsetof(ceg_mc_sweep_stats_t, translation_accepted);
    W.rotation_trials = o_stats + offsetof(ceg_mc_sweep_stats_t, rotation_trials); W.rotation_accepted = o_stats + offsetof(ceg_mc_sweep_stats_t, rotation_accepted);
    W.delta_moves = o_stats + offsetof(ceg_mc_sweep_stats_t, delta); W.delta_swaps = W.counts = W.molspec = W.spec_off = NOWHERE;
    W.temperature = lay.par + offsetof(McSweepChain, temperature); W.stream_id = lay.par + offsetof(McSweepChain, stream_id); W.param_stride = sizeof(McSweepChain);
    for (const ceg_mc* h : g->chains) W.max_slots = std::max(W.max_slots, h->v.natoms);
    W.stop = cells.with_cells ? cells.o_stop : NOWHERE;
    auto trial = [&](int cl, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        if (cl & 2)
            cells_sweep_trial(cl & 1, grid, lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), sweep_at<const int32_t>(g, o_bead), list, table_ok,
                              p->seed, step, sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows), cells.stop_of(g));
        else
            hipLaunchKernelGGL((cl & 1 ? k_mcg_sweep_trial<true> : k_mcg_sweep_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par),
                               sweep_at<const int32_t>(g, o_bead), list, table_ok, p->seed, step, sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_sweep_record_t* rec) {
        if (cells.with_cells) {
            cells_sweep_accept(grid, lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), cells.cell_sweep(g), p->seed, step,
                               sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_sweep_stats_t>(g, o_stats), rec);
            return;
        }
        hipLaunchKernelGGL(k_mcg_sweep_accept, grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), p->seed, step,
                           sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_sweep_stats_t>(g, o_stats), rec,
                           g->d_plan_stop);
    };
    const int ran = run_sweep(g, plan, lay, W, C, p->seed, p->first_step, nsteps, log_out, trial, accept);
    const ceg_mc_sweep_stats_t* st = lay.staged<const ceg_mc_sweep_stats_t>(o_stats);
    if (int rc = C.finish(g, ran, lay, [&](double e0, int c) { return e0 + st[c].delta; })) return rc;
    memcpy(stats_out, st, sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    std::vector<int64_t> moved((size_t)k);
    for (int c = 0; c < k; ++c) moved[(size_t)c] = st[c].translation_accepted + st[c].rotation_accepted;
    return cells.read_back(g, lay, moved);
}

// ---- the GCMC sweep's own steps on the host

// the species table of a call: CEG_ERR_INVALID for every refusal of the header that a species itself gives (with per-chain values in
// the chain plan, those in the table's place).  *mmax: the atoms of the largest species; *swap_atoms: the atoms of one molecule of
// every species that can be inserted
int gcmc_check_species(const ceg_mc_group* g, const ceg_mc_gcmc_params_t* p, int* mmax, int64_t* swap_atoms)
{
    const int k = (int)g->chains.size(), ns = p->nspecies;
    const std::vector<double>& chain_phi = g->plan_phi;
    *mmax = 1;
    *swap_atoms = 0;
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
        *mmax = std::max(*mmax, (int)S.m);
        if (swaps) *swap_atoms += S.m;
    }
    return CEG_OK;
}

// block pockets: the masks the group has installed must be those of this species table
int gcmc_check_blocks(const ceg_mc_group* g, const ceg_mc_gcmc_params_t* p)
{
    if (!g->d_blocks) return CEG_OK;
    if (p->nspecies != g->blk_species) return merr(CEG_ERR_INVALID, "nspecies differs from the nspecies of ceg_mc_group_set_blocks");
    for (int i = 0; i < p->nspecies && g->blk_kinds > 0; ++i)
        for (int a = 0; a < p->species[i].m; ++a)
            if (p->species[i].kinds[a] >= g->blk_kinds) return merr(CEG_ERR_INVALID, "a species' atom kind has no atom block (kind >= nkinds of ceg_mc_group_set_blocks)");
    return CEG_OK;
}

// the host mirrors from the device after a sweep: molecule table, kinds, freed runs, counts and high-water mark of every chain that
// swapped (st, tables, molspec, freeslots: the sweep's segments as read back; pc: the chains' parameters)
int gcmc_mirrors_from_device(ceg_mc_group* g, const ceg_mc_gcmc_params_t* p, const std::vector<McGcmcChain>& pc, const ceg_mc_gcmc_stats_t* st,
                             const McGcmcTable* tables, const int32_t* molspec, const int32_t* freeslots)
{
    const int ns = p->nspecies;
    for (size_t c = 0; c < g->chains.size(); ++c) {
        ceg_mc* h = g->chains[c];
        const McGcmcChain& P = pc[c];
        const McGcmcTable& D = tables[c];
        if (st[c].accepted[5] + st[c].accepted[6] == 0) continue;
        if (D.nmol < 0 || D.nmol > P.max_molecules || D.natoms < 0 || D.natoms > h->atoms_cap) return sweep_failed(g);
        std::vector<int2> mol((size_t)D.nmol);
        if (D.nmol > 0 && hipMemcpy(mol.data(), h->d_molidx, sizeof(int2) * (size_t)D.nmol, hipMemcpyDeviceToHost) != hipSuccess) return sweep_failed(g);
        h->h_mol = mol;
        h->h_kind.resize((size_t)D.natoms, 0);
        for (int j = 0; j < D.nmol; ++j) {
            const ceg_mc_gcmc_species_t& S = p->species[molspec[P.spec_off + j]];
            for (int a = 0; a < S.m; ++a) h->h_kind[(size_t)mol[(size_t)j].x + a] = S.kinds[a];
        }
        if (h->free_runs.empty()) h->free_runs.assign(MC_MAX_ATOMS + 1, {});
        for (int i = 0; i < ns; ++i) h->free_runs[(size_t)p->species[i].m].clear();
        for (int i = 0; i < ns; ++i)
            for (int q = 0; q < D.nfree[i]; ++q) h->free_runs[(size_t)p->species[i].m].push_back(freeslots[(size_t)P.free_off + (size_t)i * P.free_cap + q]);
        h->v.nmol = D.nmol;
        h->v.natoms = D.natoms;
        ++h->v_version;
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
    static_assert(offsetof(McGcmcTable, nmol) == 0 && offsetof(McGcmcTable, natoms) == 4 && offsetof(McGcmcTable, count) == 8 && sizeof(McGcmcTable) % 4 == 0,
                  "the head of a chain's table as SampleSource describes it");
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
    if (!g->plan_phi.empty() && g->plan_species != ns) return merr(CEG_ERR_INVALID, "nspecies differs from the nspecies of ceg_mc_group_set_chain_plan");
    int mmax;
    int64_t swap_atoms;
    if (int rc = gcmc_check_species(g, p, &mmax, &swap_atoms)) return rc;
    const double* temperature;
    if (int rc = C.begin(g, p->first_step, swap_atoms > 0, p->temperature, &nsteps, &temperature)) return rc;
    if (int rc = gcmc_check_blocks(g, p)) return rc;
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
    if (int rc = C.admit(g, p->temperature, p->first_step, nsteps, swap_atoms > 0)) return rc;
    for (int c = 0; c < k; ++c) stats_out[c] = ceg_mc_gcmc_stats_t{};
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
    SweepCells cells(g);
    SweepLayout lay((size_t)k, sizeof(McGcmcChain));
    const size_t o_spec = lay.segment(sizeof(ceg_mc_gcmc_species_t) * (size_t)ns), o_res = lay.segment(sizeof(int32_t) * (size_t)k);
    C.ladder_layout(lay, (size_t)k);
    const size_t o_stats = lay.segment(sizeof(ceg_mc_gcmc_stats_t) * (size_t)k), o_tab = lay.segment(sizeof(McGcmcTable) * (size_t)k),
                 o_ms = lay.segment(sizeof(int32_t) * nspec_total), o_free = lay.segment(sizeof(int32_t) * nfree_total),
                 o_pock = lay.segment(sizeof(int64_t) * 2 * (size_t)k);
    C.layout(lay, (size_t)k);
    cells.layout(lay, (size_t)k);
    C.stage(lay, (size_t)k, p->temperature);
    memcpy(lay.staged<McGcmcChain>(lay.par), pc.data(), sizeof(McGcmcChain) * (size_t)k);
    memcpy(lay.staged<ceg_mc_gcmc_species_t>(o_spec), p->species, sizeof(ceg_mc_gcmc_species_t) * (size_t)ns);
    memcpy(lay.staged<McGcmcTable>(o_tab), tab.data(), sizeof(McGcmcTable) * (size_t)k);
    int32_t* ms = lay.staged<int32_t>(o_ms);
    int32_t* fr = lay.staged<int32_t>(o_free);
    for (int c = 0, o = 0; c < k; ++c) {
        const McGcmcChain& P = pc[(size_t)c];
        for (int j = 0; j < tab[(size_t)c].nmol; ++j) ms[P.spec_off + j] = p->molecule_species[o++];
        for (int i = 0; i < ns; ++i)
            for (int q = 0; q < tab[(size_t)c].nfree[i]; ++q)
                fr[(size_t)P.free_off + (size_t)i * P.free_cap + q] = g->chains[c]->free_runs[(size_t)p->species[i].m][(size_t)q];
    }
    // (the cell lists cover every atom slot an insertion can take)
    if (int rc = cells.fill(g, lay, [&](int c) { return (size_t)pc[(size_t)c].atoms_cap; })) return rc;
    SweepWhere W{};                                      // (counts and species from the device's table: the views' nmol / natoms are stale during the sweep)
    W.stats = o_stats; W.stats_stride = sizeof(ceg_mc_gcmc_stats_t);
    W.translation_trials = o_stats + offsetof(ceg_mc_gcmc_stats_t, trials); W.translation_accepted = o_stats + offsetof(ceg_mc_gcmc_stats_t, accepted);
    W.rotation_trials = W.translation_trials + sizeof(int64_t); W.rotation_accepted = W.translation_accepted + sizeof(int64_t);
    W.delta_moves = o_stats + offsetof(ceg_mc_gcmc_stats_t, delta_moves); W.delta_swaps = o_stats + offsetof(ceg_mc_gcmc_stats_t, delta_swaps);
    W.counts = o_tab; W.counts_stride = sizeof(McGcmcTable); W.ns = ns;
    W.temperature = lay.par + offsetof(McGcmcChain, temperature); W.stream_id = lay.par + offsetof(McGcmcChain, stream_id); W.param_stride = sizeof(McGcmcChain);
    W.molspec = o_ms; W.spec_off = lay.par + offsetof(McGcmcChain, spec_off);
    for (const McGcmcChain& P : pc) W.max_slots = std::max(W.max_slots, P.atoms_cap);
    W.stop = cells.with_cells ? cells.o_stop : NOWHERE;
    const ceg_mc_block_t* blocks = g->d_blocks;          // NULL: no masks, the kernels take the path without the resolve stage
    const int block_kinds = g->blk_kinds;
    auto trial = [&](int cl, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        if (cl & 2) {
            cells_gcmc_trial(cl & 1, grid, lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par), sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns,
                             sweep_at<const McGcmcTable>(g, o_tab), sweep_at<const int32_t>(g, o_ms), list, table_ok, p->seed, step, blocks, block_kinds,
                             sweep_at<int32_t>(g, o_res), sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows), cells.stop_of(g));
            return;
        }
        hipLaunchKernelGGL((cl & 1 ? k_mcg_gcmc_trial<true> : k_mcg_gcmc_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par),
                               sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns, sweep_at<const McGcmcTable>(g, o_tab), sweep_at<const int32_t>(g, o_ms), list,
                               table_ok, p->seed, step, blocks, block_kinds, sweep_at<int32_t>(g, o_res), sweep_at<McPositions>(g, lay.prop),
                               sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_gcmc_record_t* rec) {
        if (cells.with_cells) {
            cells_gcmc_accept(grid, lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par), sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns,
                              sweep_at<McGcmcTable>(g, o_tab), sweep_at<int32_t>(g, o_ms), sweep_at<int32_t>(g, o_free), p->seed, step,
                              blocks ? sweep_at<const int32_t>(g, o_res) : nullptr, sweep_at<int64_t>(g, o_pock), sweep_at<const McPositions>(g, lay.prop),
                              sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_gcmc_stats_t>(g, o_stats), rec, g->d_plan_phi, cells.cell_sweep(g));
            return;
        }
        hipLaunchKernelGGL(k_mcg_gcmc_accept, grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par),
                           sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns, sweep_at<McGcmcTable>(g, o_tab), sweep_at<int32_t>(g, o_ms),
                           sweep_at<int32_t>(g, o_free), p->seed, step, blocks ? sweep_at<const int32_t>(g, o_res) : nullptr, sweep_at<int64_t>(g, o_pock),
                           sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_gcmc_stats_t>(g, o_stats), rec,
                           g->d_plan_phi, g->d_plan_stop);
    };
    const int ran = run_sweep(g, plan, lay, W, C, p->seed, p->first_step, nsteps, log_out, trial, accept);
    const ceg_mc_gcmc_stats_t* st = lay.staged<const ceg_mc_gcmc_stats_t>(o_stats);
    const McGcmcTable* nt = lay.staged<const McGcmcTable>(o_tab);
    if (int rc = C.finish(g, ran, lay, [&](double e0, int c) { return recorder_sum(e0, st[c]); })) return rc;
    memcpy(g->pockets.data(), lay.staged<const int64_t>(o_pock), sizeof(int64_t) * 2 * (size_t)k);
    if (int rc = gcmc_mirrors_from_device(g, p, pc, st, nt, ms, fr)) return rc;
    std::vector<int64_t> moved((size_t)k, 0);
    for (int c = 0; c < k; ++c) {
        stats_out[c] = st[c];
        fill_counts(c, nt[c], ms + pc[(size_t)c].spec_off);
        for (int q = 0; q < 7; ++q) moved[(size_t)c] += st[c].accepted[q];
    }
    return cells.read_back(g, lay, moved);
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
