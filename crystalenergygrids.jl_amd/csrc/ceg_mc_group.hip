// ceg_mc_group.hip -- chain groups (ceg_mc_group_*): K Markov chains, each a ceg_mc handle of ceg_mc.hip, driven together.
//   ceg_mc_group_trial / _accept   one step of K chains in one launch per class: the bodies of k_mc_trial / k_mc_accept (ceg_mc_state.h)
//   ceg_mc_group_sweep             S steps of translations and rotations: proposal, Metropolis rule and update on the device
//   ceg_mc_group_sweep_gcmc        the same with all six move kinds, swaps included, and the molecule table owned by the device
//   ceg_mc_group_set_blocks        block pockets: inblockpocket and the retry loop of choose_step!, resolved inside the GCMC trial launch
//   ceg_mc_group_sweep_cycles      either sweep over whole cycles: the same body (sweep_plain / sweep_gcmc) with a ceg_mc_cycles_t, one
//   ceg_mc_group_sweep_gcmc_cycles   launch of ceg_mc_cycles.hip behind the last step of every cycle (temperature table, dmax / thetamax)
//   ceg_mc_group_set_chain_plan      per chain: the phiPV_div_k of the swap rules and the absolute step at which the chain stops (isotherms)
// The two sweeps have their own kernels, per-chain parameters and read-back, and share one host driver (run_sweep).
#include "ceg_mc_state.h"

using namespace ceg_mcs;

namespace {

// ---- a chain group (ceg_mc_group_*): one step of K chains in one launch per (FAST, INSERT, CELLS) class.  What a chain of the
// launch needs travels in mapped host memory like a small batch of k_mc_trial; the views stay in device memory.
struct McGroupRow {
    int32_t view, molecule, stride, _pad;    // view: index of the chain in the group (views[view]); molecule -1 for an insertion
    int64_t trial, out;                      // offsets of the chain's placements (doubles) and of its first row (rows)
    McLocal L;
};

struct McAtChainRow {
    int64_t out;             // row of `out` (fetched in front of the body: at its end it would be a round trip to host memory)
    int r;                   // row of the chain
    unsigned n;              // workgroups of all the launches of the call
    int table_ok;            // the call's LDS leaves room for the pair tables
    template <bool INSERT> __device__ __forceinline__ int64_t b() const { return INSERT ? (int64_t)r + 1 : (int64_t)r; }
    __device__ __forceinline__ double* row(double* o) const { return o + 4 * (size_t)out; }
    __device__ __forceinline__ unsigned nblocks() const { return n; }
    __device__ __forceinline__ bool table_in_lds(const McView& v) const { return table_ok && v.table_in_lds; }
    __device__ __forceinline__ int natoms(const McView& v) const { return v.natoms; }
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
struct McSweepChain {            // per chain, device memory
    uint32_t stream_id;
    int32_t bead_off;            // the chain's first entry of the bead array
    int32_t stride, _pad;
    double temperature, dmax, thetamax, p_rotation;
};

struct McMove { int32_t molecule, kind; };       // kind 0 translation, 1 rotation; molecule -1: the chain is idle

__device__ McCellOps d_mc_no_cell_ops;           // (sweeps refuse chains with neighbour cells: the accept body never reads it)

// the chain plan's stop (ceg_mc_group_set_chain_plan): chain c takes no part in the absolute steps >= stop[c]; nullptr: no chain stops
__device__ __forceinline__ bool chain_stopped(const int64_t* __restrict__ stop, int c, uint64_t step) { return stop && step >= (uint64_t)stop[c]; }

__device__ __forceinline__ McMove sweep_select(const McView& v, const McSweepChain& P, uint64_t seed, uint64_t step)
{
    const int nmol = v.nmol;
    if (nmol <= 0) return McMove{-1, -1};
    const ceg_philox::Block w = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::SELECT);
    int j = (int)floor(ceg_philox::uniform(w.w[0], w.w[1]) * (double)nmol);
    j = j < nmol - 1 ? j : nmol - 1;
    const bool rotate = v.mol[j].y > 1 && ceg_philox::uniform(w.w[2], w.w[3]) < P.p_rotation;
    return McMove{j, rotate ? 1 : 0};
}

// (dx, dy, dz) turned by the angle with sine s and cosine c about `axis`: the matrices of src/mcmoves.jl:155-161 (SMatrix fills column by column)
__device__ __forceinline__ void rotate_about(int axis, double s, double c, double& dx, double& dy, double& dz)
{
#pragma clang fp contract(off)
    const double x = dx, y = dy, z = dz;
    if (axis == 0) { dy = c * y - s * z; dz = s * y + c * z; }
    else if (axis == 1) { dx = c * x + s * z; dz = c * z - s * x; }
    else { dx = c * x - s * y; dy = s * x + c * y; }
}

// coordinate `comp` of atom `a` of the proposed placement of molecule mv.molecule (atoms [mj.x, mj.x + mj.y)): random_translation /
// random_rotation of src/mcmoves.jl:139-164 on the resident positions
// (stream id, step sizes and the atom the molecule rotates about as plain arguments: ceg_mc_group_sweep takes them from its per-chain
// parameters and bead array, ceg_mc_group_sweep_gcmc from its own parameters and species table)
__device__ __forceinline__ double sweep_coordinate_of(const McView& v, uint32_t stream_id, double dmax, double thetamax, int bead_atom, int kind, const int2 mj,
                                                      uint64_t seed, uint64_t step, int a, int comp)
{
#pragma clang fp contract(off)
    const double4 A = v.atoms[mj.x + a];
    const ceg_philox::Block g = ceg_philox::draw(seed, step, stream_id, ceg_philox::GEOMETRY_A);
    if (kind == 0) {
        uint32_t wa = g.w[0], wb = g.w[1];
        if (comp == 1) { wa = g.w[2]; wb = g.w[3]; }
        if (comp == 2) {
            const ceg_philox::Block h = ceg_philox::draw(seed, step, stream_id, ceg_philox::GEOMETRY_B);
            wa = h.w[0]; wb = h.w[1];
        }
        const double r = (2.0 * ceg_philox::uniform(wa, wb) - 1.0) * dmax;
        return (comp == 0 ? A.x : (comp == 1 ? A.y : A.z)) + r;
    }
    const double theta = thetamax * (2.0 * ceg_philox::uniform(g.w[0], g.w[1]) - 1.0);
    int axis = (int)floor(3.0 * ceg_philox::uniform(g.w[2], g.w[3]));
    axis = axis < 2 ? axis : 2;
    double s, c;
    sincos(theta, &s, &c);
    const double4 R = v.atoms[mj.x + bead_atom];
    double dx = A.x - R.x, dy = A.y - R.y, dz = A.z - R.z;
    rotate_about(axis, s, c, dx, dy, dz);
    return comp == 0 ? R.x + dx : (comp == 1 ? R.y + dy : R.z + dz);
}

__device__ __forceinline__ double sweep_coordinate(const McView& v, const McSweepChain& P, const int32_t* __restrict__ bead, const McMove mv, const int2 mj,
                                                   uint64_t seed, uint64_t step, int a, int comp)
{
    return sweep_coordinate_of(v, P.stream_id, P.dmax, P.thetamax, mv.kind == 0 ? 0 : bead[P.bead_off + mv.molecule], mv.kind, mj, seed, step, a, comp);
}

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

// compute_accept_move (src/montecarlo.jl:702-712) on the rows before (row[0..3]) and after (row[4..7]) a displacement: the sums in the
// reference's order; a proposal inside the framework's hard core is blocked; delta = after - before
__device__ __forceinline__ int displacement_decision(const double* row, double u, double temperature, bool& blocked, double& delta)
{
#pragma clang fp contract(off)
    const double b = ((row[0] + row[1]) + row[2]) + row[3], a = ((row[4] + row[5]) + row[6]) + row[7];
    blocked = row[4] >= 1e90;
    delta = a - b;
    return (!blocked && (a < b || u < exp((b - a) / temperature))) ? 1 : 0;
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
constexpr int MC_GCMC_SPECIES = CEG_MC_GCMC_MAX_SPECIES;

struct McGcmcChain {             // per chain, fixed during a sweep
    uint32_t stream_id;
    int32_t stride;
    int32_t max_molecules, atoms_cap;
    int32_t spec_off;            // the chain's first entry of the species-of-molecule array
    int32_t free_off, free_cap;  // stack of species i: freeslots[free_off + i * free_cap ...]
    int32_t _pad;
    double temperature, dmax, thetamax;
};

struct McGcmcTable {             // per chain, written by k_mcg_gcmc_accept
    int32_t nmol, natoms;        // natoms: high-water mark of the atom slots
    int32_t count[MC_GCMC_SPECIES], nfree[MC_GCMC_SPECIES];
};

struct McGcmcMove {
    int32_t species, kind;       // kind 0..6 (include/ceg_hip.h)
    int32_t molecule;            // device index; an insertion: the index it takes; -1 spent
    int32_t n_i, nmol, natoms;
    int32_t flags;               // 1 spent, 4 capacity
};

__device__ __forceinline__ int32_t gcmc_ld(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// the move of chain `P` at `step`, by the whole workgroup (the j-th molecule of the species is found by a scan of the table)
__device__ __forceinline__ McGcmcMove gcmc_select(const McGcmcChain& P, const ceg_mc_gcmc_species_t* __restrict__ spec, int nspecies,
                                                  const McGcmcTable* T, const int32_t* molspec, uint64_t seed, uint64_t step)
{
    __shared__ int s_wcnt[MC_THREADS / 64], s_found;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    McGcmcMove mv;
    mv.nmol = gcmc_ld(&T->nmol);
    mv.natoms = gcmc_ld(&T->natoms);
    const ceg_philox::Block w = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::GCMC_SELECT);
    int i = (int)floor(ceg_philox::uniform(w.w[0], w.w[1]) * (double)nspecies);
    i = i < nspecies - 1 ? i : nspecies - 1;
    const double uk = ceg_philox::uniform(w.w[2], w.w[3]);
    int kind = 5;
    for (int k = 4; k >= 0; --k)
        if (uk < spec[i].cumulative[k]) kind = k;
    const ceg_philox::Block wm = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::GCMC_MOLECULE);
    if (kind == 5 && ceg_philox::uniform(wm.w[2], wm.w[3]) < 0.5) kind = 6;
    mv.species = i;
    mv.kind = kind;
    mv.n_i = gcmc_ld(&T->count[i]);
    mv.flags = 0;
    mv.molecule = -1;
    if (kind == 5) {
        mv.molecule = mv.nmol;
        if (mv.nmol >= P.max_molecules) mv.flags = 4;
        return mv;
    }
    if (mv.n_i <= 0) { mv.flags = 1; return mv; }
    int j = (int)floor(ceg_philox::uniform(wm.w[0], wm.w[1]) * (double)mv.n_i);
    j = j < mv.n_i - 1 ? j : mv.n_i - 1;
    const int32_t* ms = molspec + P.spec_off;
    const int chunk = (mv.nmol + MC_THREADS - 1) / MC_THREADS;
    const int lo = tid * chunk, hi = lo + chunk < mv.nmol ? lo + chunk : mv.nmol;
    int cnt = 0;
    for (int t = lo; t < hi; ++t) cnt += gcmc_ld(ms + t) == i ? 1 : 0;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (tid == 0) s_found = -1;
    if (lane == 63) s_wcnt[wave] = incl;
    __syncthreads();
    int before = incl - cnt;
    for (int q = 0; q < wave; ++q) before += s_wcnt[q];
    if (cnt > 0 && before <= j && j < before + cnt) {
        int seen = before;
        for (int t = lo; t < hi; ++t)
            if (gcmc_ld(ms + t) == i && seen++ == j) s_found = t;
    }
    __syncthreads();
    mv.molecule = __builtin_amdgcn_readfirstlane(s_found);
    if (mv.molecule < 0) mv.flags = 1;          // (the counts and the table disagree: cannot happen; the step is spent)
    return mv;
}

// the placement of one atom by the random_* kinds and the insertion (src/mcmoves.jl:139-164 with the MC cell / 180 degrees,
// simulation.jl:294-305) from the blocks g, h, k of purposes 6, 7, 8 of its attempt: (px, py, pz) the atom, (bx, by, bz) the bead atom
__device__ __forceinline__ void gcmc_random_point(const double* M, int kind, int m, const ceg_philox::Block& g, const ceg_philox::Block& h,
                                                  const ceg_philox::Block& k, double& px, double& py, double& pz, double bx, double by, double bz)
{
#pragma clang fp contract(off)
    if (kind != 3) {                             // random_translation: r = mat (U3 - 0.5)
        const double ua = ceg_philox::uniform(g.w[0], g.w[1]) - 0.5, ub = ceg_philox::uniform(g.w[2], g.w[3]) - 0.5,
                     uc = ceg_philox::uniform(h.w[0], h.w[1]) - 0.5;
        const double rx = (M[0] * ua + M[3] * ub) + M[6] * uc, ry = (M[1] * ua + M[4] * ub) + M[7] * uc, rz = (M[2] * ua + M[5] * ub) + M[8] * uc;
        px += rx; py += ry; pz += rz;
        bx += rx; by += ry; bz += rz;
    }
    if (kind == 2 || m == 1) return;
    const double theta = 3.141592653589793 * (2.0 * ceg_philox::uniform(h.w[2], h.w[3]) - 1.0);
    int axis = (int)floor(3.0 * ceg_philox::uniform(k.w[0], k.w[1]));
    axis = axis < 2 ? axis : 2;
    double s, c;
    sincos(theta, &s, &c);
    double dx = px - bx, dy = py - by, dz = pz - bz;
    rotate_about(axis, s, c, dx, dy, dz);
    px = bx + dx; py = by + dy; pz = bz + dz;
}

// atom `a` and the bead atom of what a random_* kind or the insertion displaces: the species' model for an insertion, else the molecule
__device__ __forceinline__ void gcmc_random_source(const McView& v, const ceg_mc_gcmc_species_t& S, int kind, const int2 mj, int a, double& px, double& py,
                                                   double& pz, double& bx, double& by, double& bz)
{
    if (kind == 5) {
        px = S.model[a][0]; py = S.model[a][1]; pz = S.model[a][2];
        bx = S.model[S.bead][0]; by = S.model[S.bead][1]; bz = S.model[S.bead][2];
    } else {
        const double4 A = v.atoms[mj.x + a], B = v.atoms[mj.x + S.bead];
        px = A.x; py = A.y; pz = A.z;
        bx = B.x; by = B.y; bz = B.z;
    }
}

// coordinate `comp` of atom `a` of the proposal: kinds 0 / 1 from sweep_coordinate, the random_* kinds and the insertion from attempt
// `attempt` of purposes 6-8 (0 wherever choose_step! does not retry)
__device__ __forceinline__ double gcmc_coordinate(const McView& v, const McGcmcChain& P, const ceg_mc_gcmc_species_t& S, const McGcmcMove& mv, const int2 mj,
                                                  uint64_t seed, uint64_t step, uint32_t attempt, int a, int comp)
{
    if (mv.kind <= 1) {
        if (mv.kind == 1 && mj.y == 1) return comp == 0 ? v.atoms[mj.x].x : (comp == 1 ? v.atoms[mj.x].y : v.atoms[mj.x].z);
        return sweep_coordinate_of(v, P.stream_id, P.dmax, P.thetamax, S.bead, mv.kind, mj, seed, step, a, comp);
    }
    double px, py, pz, bx, by, bz;
    gcmc_random_source(v, S, mv.kind, mj, a, px, py, pz, bx, by, bz);
    ceg_philox::Block g{}, k{};
    const ceg_philox::Block h = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::attempt_purpose(ceg_philox::GCMC_RANDOM_B, attempt));
    if (mv.kind != 3) g = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::attempt_purpose(ceg_philox::GCMC_RANDOM_A, attempt));
    if (mv.kind != 2 && mj.y != 1) k = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::attempt_purpose(ceg_philox::GCMC_RANDOM_C, attempt));
    gcmc_random_point(v.mat, mv.kind, mj.y, g, h, k, px, py, pz, bx, by, bz);
    return comp == 0 ? px : (comp == 1 ? py : pz);
}

// ---- block pockets (ceg_mc_group_set_blocks): inblockpocket and the retry loop of choose_step! (src/simulation.jl:271-326,
// src/montecarlo.jl:631-640), resolved by every workgroup of a chain's step in front of its row.
// blocks[0 .. nspecies): the species blocks; blocks[nspecies + kind]: the atom blocks (nkinds == 0: none); masks in device memory.
using McBlock = ceg_mc_block_t;

// BlockFile getindex at p + offset (src/coordinates.jl:58-66,97-101; blocked_at of ceg_egrid.hip): a NULL mask is empty
__device__ __forceinline__ bool block_holds(const McBlock& B, double px, double py, double pz)
{
#pragma clang fp contract(off)
    if (!B.mask) return false;
    px = px + B.offset[0]; py = py + B.offset[1]; pz = pz + B.offset[2];
    const double* I = B.invmat;
    const double* M = B.mat;
    double a0 = (I[0] * px + I[3] * py) + I[6] * pz;
    double a1 = (I[1] * px + I[4] * py) + I[7] * pz;
    double a2 = (I[2] * px + I[5] * py) + I[8] * pz;
    a0 -= floor(a0); a1 -= floor(a1); a2 -= floor(a2);
    const double q[3] = {(M[0] * a0 + M[3] * a1) + M[6] * a2, (M[1] * a0 + M[4] * a1) + M[7] * a2, (M[2] * a0 + M[5] * a1) + M[8] * a2};
    int idx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double sh = (q[c] - B.shift[c]) * (double)B.dims[c] / B.size[c] + 1.0;
        const int i = (int)rint(sh) - 1;
        idx[c] = i < 0 ? 0 : (i > B.dims[c] ? B.dims[c] : i);                          // memory safety only
    }
    const size_t ny = (size_t)B.dims[1] + 1, nz = (size_t)B.dims[2] + 1;
    return B.mask[((size_t)idx[0] * ny + idx[1]) * nz + idx[2]] != 0;
}

// what a step's trial launch hands to its accept launch, one word per chain: attempt << 2 | exhausted << 1 | pocket-blocked
constexpr int MC_POCKET = 1, MC_EXHAUSTED = 2;
constexpr int MC_RESOLVE_PASSES = (ceg_philox::GCMC_ATTEMPTS + 15) / 16;

// The attempt of the step's proposal and whether the step is pocket-blocked, by the whole workgroup.  16 attempts per pass, one per
// 16 lanes, lane a of an attempt on atom a: the three Philox blocks of the attempt are drawn by its lanes 0-2 and shared, every lane
// places its atom and looks it up; a ballot gives each attempt its verdict and the lowest passing attempt of the pass ends the loop.
// Kinds 0, 1, 3 have the one proposal (attempt 0) and pass with its verdict.
__device__ __forceinline__ int gcmc_resolve(const McView& v, const McGcmcChain& P, const ceg_mc_gcmc_species_t& S, const McGcmcMove& mv, const int2 mj,
                                            const McBlock* __restrict__ blocks, int nspecies, int nkinds, uint64_t seed, uint64_t step)
{
    static_assert(MC_THREADS == 256 && MC_MAX_ATOMS == 16, "16 attempts of 16 lanes");
    __shared__ unsigned s_verdict[2][MC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, a = tid & 15;
    const bool retried = mv.kind == 2 || mv.kind == 4 || mv.kind == 5;
    const int npass = retried ? MC_RESOLVE_PASSES : 1;
    const McBlock& SB = blocks[mv.species];
    const int akind = S.kinds[a < mj.y ? a : 0];
    for (int p = 0; p < npass; ++p) {
        const int t = 16 * p + (tid >> 4);
        const bool live = a < mj.y && (retried ? t < (int)ceg_philox::GCMC_ATTEMPTS : t == 0);
        double x = 0.0, y = 0.0, z = 0.0;
        if (mv.kind <= 1) {
            if (live) {
                x = gcmc_coordinate(v, P, S, mv, mj, seed, step, 0u, a, 0);
                y = gcmc_coordinate(v, P, S, mv, mj, seed, step, 0u, a, 1);
                z = gcmc_coordinate(v, P, S, mv, mj, seed, step, 0u, a, 2);
            }
        } else {
            const ceg_philox::Block mine = ceg_philox::draw(seed, step, P.stream_id, ceg_philox::attempt_purpose(ceg_philox::GCMC_RANDOM_A + (uint32_t)(a % 3), (uint32_t)t));
            ceg_philox::Block g, h, k;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                g.w[w] = (uint32_t)__shfl((int)mine.w[w], 0, 16);
                h.w[w] = (uint32_t)__shfl((int)mine.w[w], 1, 16);
                k.w[w] = (uint32_t)__shfl((int)mine.w[w], 2, 16);
            }
            if (live) {
                double bx, by, bz;
                gcmc_random_source(v, S, mv.kind, mj, a, x, y, z, bx, by, bz);
                gcmc_random_point(v.mat, mv.kind, mj.y, g, h, k, x, y, z, bx, by, bz);
            }
        }
        bool in_species = false, in_any = false;
        if (live) {
            in_species = block_holds(SB, x, y, z);
            in_any = in_species || (nkinds > 0 && block_holds(blocks[nspecies + akind], x, y, z));
        }
        const unsigned long long bs = __ballot(in_species), ba = __ballot(in_any);
        unsigned verdict = 0;                    // bits 0-3: the wave's four attempts pass; bits 4-7: their placements lie in a pocket
        for (int q = 0; q < 4; ++q) {
            const unsigned s16 = (unsigned)(bs >> (16 * q)) & 0xffffu, a16 = (unsigned)(ba >> (16 * q)) & 0xffffu;
            const int tq = 16 * p + 4 * wave + q;
            const bool pass = retried ? tq < (int)ceg_philox::GCMC_ATTEMPTS && (mv.kind == 5 ? ((s16 >> S.bead) & 1u) == 0u : a16 == 0u) : tq == 0;
            verdict |= (pass ? 1u : 0u) << q | (a16 != 0u ? 16u : 0u) << q;
        }
        if ((tid & 63) == 0) s_verdict[p & 1][wave] = verdict;
        __syncthreads();                         // (one per pass: the buffer of pass p is next written in pass p + 2, behind the barrier of p + 1)
        unsigned pass = 0, pocket = 0;
        for (int w = 0; w < MC_THREADS / 64; ++w) {
            const unsigned r = s_verdict[p & 1][w];
            pass |= (r & 15u) << (4 * w);
            pocket |= (r >> 4) << (4 * w);
        }
        pass = (unsigned)__builtin_amdgcn_readfirstlane((int)pass);
        if (pass) {
            const int q = __ffs((int)pass) - 1;
            return (16 * p + q) << 2 | (((pocket >> q) & 1u) ? MC_POCKET : 0);
        }
    }
    return ((int)ceg_philox::GCMC_ATTEMPTS - 1) << 2 | MC_EXHAUSTED | MC_POCKET;
}

struct McAtGcmcRow {
    int64_t out;
    int r;                   // 0: where the molecule is; 1: the proposal (an insertion passes 0: its only row is the proposal)
    int table_ok, n;         // n: high-water mark of the atom slots, from the device's table
    template <bool INSERT> __device__ __forceinline__ int64_t b() const { return INSERT ? (int64_t)r + 1 : (int64_t)r; }
    __device__ __forceinline__ double* row(double* o) const { return o + 4 * (size_t)out; }
    __device__ __forceinline__ unsigned nblocks() const { return 0u; }
    __device__ __forceinline__ bool table_in_lds(const McView& v) const { return table_ok && v.table_in_lds; }
    __device__ __forceinline__ int natoms(const McView&) const { return n; }
};

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
    // chain plan (ceg_mc_group_set_chain_plan): the host's copy for the checks and the launch lists, the device's for the kernels
    std::vector<double> plan_phi;                // [K][plan_species], empty: the species table's value for every chain
    std::vector<int64_t> plan_stop;              // [K], empty: no chain stops
    int plan_species = 0;
    double* d_plan_phi = nullptr;
    int64_t* d_plan_stop = nullptr;
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
    return GroupRef{g->device, g->stream, g->chains.data(), (int)g->chains.size(), g->d_views, &g->d_baseline, &g->baseline_cap, &g->sampler};
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

// ---- what the two sweeps share on the host: the refusals, the launch plan, the layout of the group's device block and the driver
namespace {

// a chain no sweep takes: inconsistent after a failure, or with its guests in neighbour cells
int sweep_refuse_chain(const ceg_mc* h, int c)
{
    if (h->poisoned) return group_refuse_poisoned(c);
    if (h->v.use_cells || h->cm.on)
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

// the launches of a step: the chains by class (0: exact rule energies, 1: fast), the LDS of their trial and accept kernels;
// add(): chain c takes part, with molecules of at most mmax atoms
struct SweepPlan {
    std::vector<int32_t> list[2];
    size_t lds_trial[2] = {0, 0}, pair_table[2] = {0, 0}, lds_accept = 0;
    int add(int c, const ceg_mc* h, int mmax)
    {
        if (tables_bytes(h, mmax) > 64 * 1024) return merr(CEG_ERR_UNSUPPORTED, "k-space tables of the molecule do not fit in LDS");
        const int cl = h->v.fast ? 1 : 0;
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

// `stage` (lay.total bytes, all but the launch lists filled in) into the group's block, then nsteps steps of trial(fast, grid, lds, list,
// table_ok, step) per class present and accept(grid, lds, step, record), back to back on the group's stream; afterwards the block from
// `o_back` on is back in `stage` and the records are in log_out.  A failure once the steps have started marks every chain inconsistent.
// With a sampler installed, frame(step) follows the accept launch of every step the sampler takes a frame after.  With cycle_len > 0,
// cycle_end(j) follows the last step of cycle j of the call (step s of the call with (s + 1) % cycle_len == 0), behind its frame.
template <class Record, class Trial, class Accept, class Frame, class CycleEnd>
int run_sweep(ceg_mc_group* g, const SweepPlan& plan, const SweepLayout& lay, std::vector<unsigned char>& stage, size_t o_back, uint64_t first_step,
              int64_t nsteps, Record* log_out, Trial&& trial, Accept&& accept, Frame&& frame, int64_t cycle_len, CycleEnd&& cycle_end)
{
    const size_t k = g->chains.size();
    size_t lds_trial[2];
    int table_ok[2];
    for (int cl = 0; cl < 2; ++cl) {                     // the pair table in LDS only where the largest tables leave room (run_trial's rule)
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
    std::vector<int32_t> order[2] = {plan.list[0], plan.list[1]};
    if (!stop.empty())
        for (int cl = 0; cl < 2; ++cl)
            std::stable_sort(order[cl].begin(), order[cl].end(), [&](int32_t a, int32_t b) { return stop[(size_t)a] > stop[(size_t)b]; });
    int32_t* l = reinterpret_cast<int32_t*>(stage.data() + lay.list);
    for (int cl = 0, e = 0; cl < 2; ++cl)
        for (int32_t c : order[cl]) l[e++] = c;
    if (hipMemcpy(g->d_scratch, stage.data(), lay.total, hipMemcpyHostToDevice) != hipSuccess) return fail("H2D failed");
    if (!group_upload_views(g, std::vector<char>(k, 1))) return fail("view upload failed");
    if (d_log && hipMemsetAsync(d_log, 0, log_bytes, g->stream) != hipSuccess) return fail("hipMemsetAsync failed");
    // ---- the steps: nothing between them but the stream's own order (no chain with a molecule and no log: nothing to do)
    const int32_t* d_list = sweep_at<const int32_t>(g, lay.list);
    const unsigned n0 = (unsigned)plan.list[0].size(), n1 = (unsigned)plan.list[1].size();
    unsigned live0 = n0, live1 = n1;                     // chains of either class that have not stopped (the steps only go up)
    // (with every chain empty and no log the steps launch nothing; a sampler still takes its frames, and only those are launched)
    bool launched = true;
    const bool work = n0 + n1 > 0 || d_log;
    const int64_t frames_before = g->sampler ? sampler_frames_taken(g->sampler) : 0;
    for (int64_t s = 0; s < nsteps && launched && (work || g->sampler || cycle_len > 0); ++s) {
        const uint64_t step = first_step + (uint64_t)s;
        const bool framed = g->sampler && sampler_frame_after(g->sampler, step);
        const bool ends = cycle_len > 0 && (s + 1) % cycle_len == 0;
        if (!work && !framed && !ends) continue;
        if (!stop.empty()) {
            while (live0 > 0 && step >= (uint64_t)stop[(size_t)order[0][live0 - 1]]) --live0;
            while (live1 > 0 && step >= (uint64_t)stop[(size_t)order[1][live1 - 1]]) --live1;
        }
        if (live0) trial(false, dim3(2u * live0, 3u), lds_trial[0], d_list, table_ok[0], step);
        if (live1) trial(true, dim3(2u * live1, 3u), lds_trial[1], d_list + n0, table_ok[1], step);
        // (the accept launch keeps one workgroup per chain: a stopped chain's writes its record and returns; no chain left and no log: none)
        if (live0 + live1 > 0 || d_log) accept(dim3((unsigned)k), plan.lds_accept, step, d_log ? d_log + (size_t)s * k : nullptr);
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
    void layout(SweepLayout& lay, size_t k)
    {
        if (!cycled) return;
        o_rec = lay.segment(sizeof(ceg_mc_cycle_record_t) * (size_t)cy->ncycles * k);
        o_table = lay.segment(table() ? sizeof(double) * (size_t)cy->ncycles * k : 0);
        o_prior = lay.segment(sizeof(int64_t) * 4 * k);
    }
    void fill(std::vector<unsigned char>& stage, size_t k) const
    {
        if (!cycled) return;
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
    const double* temperature = C.first_row(p->temperature);
    // ---- every refusal before anything is launched or changed, chain by chain
    std::vector<McSweepChain> pc((size_t)k);
    std::vector<int32_t> beads;
    SweepPlan plan;
    for (int c = 0; c < k; ++c) {
        ceg_mc* h = g->chains[c];
        if (int rc = sweep_refuse_chain(h, c)) return rc;
        if (int rc = sweep_check_steps(p, temperature, c)) return rc;
        if (!(p->p_rotation[c] >= 0.0 && p->p_rotation[c] <= 1.0)) return group_bad(c, "p_rotation must lie in [0, 1]");
        if (int rc = sweep_check_stream_id(p->stream_id, c)) return rc;
        McSweepChain& P = pc[(size_t)c];
        P.stream_id = p->stream_id[c];
        P.bead_off = (int32_t)beads.size();
        P.stride = h->stride;
        P.temperature = temperature ? temperature[c] : 0.0; P.dmax = p->dmax[c]; P.thetamax = p->thetamax[c]; P.p_rotation = p->p_rotation[c];
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
    if (g->sampler)
        if (int rc = sampler_admit(g->sampler, p->first_step, nsteps)) return rc;
    for (int c = 0; c < k; ++c) stats_out[c] = ceg_mc_sweep_stats_t{};
    if (nsteps == 0) return CEG_OK;
    SweepLayout lay((size_t)k, sizeof(McSweepChain));
    const size_t o_bead = lay.segment(sizeof(int32_t) * beads.size()), o_stats = lay.segment(sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    C.layout(lay, (size_t)k);
    std::vector<unsigned char> stage(lay.total, 0);
    C.fill(stage, (size_t)k);
    memcpy(stage.data() + lay.par, pc.data(), sizeof(McSweepChain) * (size_t)k);
    if (!beads.empty()) memcpy(stage.data() + o_bead, beads.data(), sizeof(int32_t) * beads.size());
    auto trial = [&](bool fast, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        hipLaunchKernelGGL((fast ? k_mcg_sweep_trial<true> : k_mcg_sweep_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par),
                               sweep_at<const int32_t>(g, o_bead), list, table_ok, p->seed, step, sweep_at<McPositions>(g, lay.prop), sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_sweep_record_t* rec) {
        hipLaunchKernelGGL(k_mcg_sweep_accept, grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McSweepChain>(g, lay.par), p->seed, step,
                           sweep_at<const McPositions>(g, lay.prop), sweep_at<const double>(g, lay.rows), sweep_at<ceg_mc_sweep_stats_t>(g, o_stats), rec,
                           g->d_plan_stop);
    };
    int32_t max_slots = 0;
    for (const ceg_mc* h : g->chains) max_slots = std::max(max_slots, h->v.natoms);
    auto frame = [&](uint64_t step) {                     // (the molecule table does not change: counts from the views)
        const SampleSource src{nullptr, 0, 0, &sweep_at<const ceg_mc_sweep_stats_t>(g, o_stats)->delta, nullptr, (int32_t)sizeof(ceg_mc_sweep_stats_t), max_slots,
                               g->d_plan_stop};
        sampler_enqueue(g->sampler, g->stream, g->d_views, k, (int64_t)step, src);
    };
    auto cycle_end = [&](int64_t j) {                     // (the molecule table does not change: counts from the views)
        const ceg_mc_sweep_stats_t* st = sweep_at<const ceg_mc_sweep_stats_t>(g, o_stats);
        const CycleSource src{&st->translation_trials, &st->translation_accepted, &st->rotation_trials, &st->rotation_accepted, &st->delta, nullptr, nullptr,
                              &sweep_at<McSweepChain>(g, lay.par)->temperature, (int32_t)sizeof(ceg_mc_sweep_stats_t), 0, (int32_t)sizeof(McSweepChain), 0,
                              g->d_plan_stop, C.last_step(p->first_step, j)};
        cycles_enqueue(g->stream, g->d_views, k, C.run(g), j, src);
    };
    if (int rc = run_sweep(g, plan, lay, stage, o_stats, p->first_step, nsteps, log_out, trial, accept, frame, C.cycled ? C.cy->steps_per_cycle : 0, cycle_end))
        return rc;
    memcpy(stats_out, stage.data() + o_stats, sizeof(ceg_mc_sweep_stats_t) * (size_t)k);
    C.read_back(stage, (size_t)k);
    return CEG_OK;
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
        if (int rc = sweep_refuse_chain(g->chains[c], c)) return rc;
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
        P.temperature = temperature ? temperature[c] : 0.0; P.dmax = p->dmax[c]; P.thetamax = p->thetamax[c];
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
    if (g->sampler)
        if (int rc = sampler_admit(g->sampler, p->first_step, nsteps)) return rc;
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
    SweepLayout lay((size_t)k, sizeof(McGcmcChain));
    const size_t o_spec = lay.segment(sizeof(ceg_mc_gcmc_species_t) * (size_t)ns), o_res = lay.segment(sizeof(int32_t) * (size_t)k),
                 o_stats = lay.segment(sizeof(ceg_mc_gcmc_stats_t) * (size_t)k), o_tab = lay.segment(sizeof(McGcmcTable) * (size_t)k),
                 o_ms = lay.segment(sizeof(int32_t) * nspec_total), o_free = lay.segment(sizeof(int32_t) * nfree_total),
                 o_pock = lay.segment(sizeof(int64_t) * 2 * (size_t)k);
    C.layout(lay, (size_t)k);
    const ceg_mc_block_t* blocks = g->d_blocks;          // NULL: no masks, the kernels take the path without the resolve stage
    const int block_kinds = g->blk_kinds;
    std::vector<unsigned char> stage(lay.total, 0);
    C.fill(stage, (size_t)k);
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
    auto trial = [&](bool fast, dim3 grid, size_t lds, const int32_t* list, int table_ok, uint64_t step) {
        hipLaunchKernelGGL((fast ? k_mcg_gcmc_trial<true> : k_mcg_gcmc_trial<false>), grid, dim3(MC_THREADS), lds, g->stream, g->d_views, sweep_at<const McGcmcChain>(g, lay.par),
                               sweep_at<const ceg_mc_gcmc_species_t>(g, o_spec), ns, sweep_at<const McGcmcTable>(g, o_tab), sweep_at<const int32_t>(g, o_ms), list,
                               table_ok, p->seed, step, blocks, block_kinds, sweep_at<int32_t>(g, o_res), sweep_at<McPositions>(g, lay.prop),
                               sweep_at<double>(g, lay.rows));
    };
    auto accept = [&](dim3 grid, size_t lds, uint64_t step, ceg_mc_gcmc_record_t* rec) {
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
                               (int32_t)sizeof(ceg_mc_gcmc_stats_t), max_slots, g->d_plan_stop};
        sampler_enqueue(g->sampler, g->stream, g->d_views, k, (int64_t)step, src);
    };
    auto cycle_end = [&](int64_t j) {                     // (the molecule count from the device's table, as the frames)
        const ceg_mc_gcmc_stats_t* st = sweep_at<const ceg_mc_gcmc_stats_t>(g, o_stats);
        const CycleSource src{&st->trials[0], &st->accepted[0], &st->trials[1], &st->accepted[1], &st->delta_moves, &st->delta_swaps,
                              &sweep_at<const McGcmcTable>(g, o_tab)->nmol, &sweep_at<McGcmcChain>(g, lay.par)->temperature,
                              (int32_t)sizeof(ceg_mc_gcmc_stats_t), (int32_t)sizeof(McGcmcTable), (int32_t)sizeof(McGcmcChain), 0,
                              g->d_plan_stop, C.last_step(p->first_step, j)};
        cycles_enqueue(g->stream, g->d_views, k, C.run(g), j, src);
    };
    if (int rc = run_sweep(g, plan, lay, stage, o_stats, p->first_step, nsteps, log_out, trial, accept, frame, C.cycled ? C.cy->steps_per_cycle : 0, cycle_end))
        return rc;
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
