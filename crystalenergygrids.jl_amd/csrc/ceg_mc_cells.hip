// ceg_mc_cells.hip -- sweeps of chains that keep their guests in neighbour cells (ceg_mc_group_set_device_cells): the kernels of the
// four sweep entry points with the cell walk in the trial rows (mc_trial_row<FAST, INSERT, true>) and the cell operations of an
// accepted step -- displacement, insertion, deletion -- worked out in the accept launch, on the device's book of the cell lists
// (McCellBook).
//   k_mcc_book_fill      owner[] of a chain's book from cell_of[] / idx_of[] (before a sweep)
//   k_mcc_sweep_trial    k_mcg_sweep_trial with the cell walk; a halted or stopped chain's workgroups return at once
//   k_mcc_sweep_accept   k_mcg_sweep_accept for every chain of a group that has a chain with cells: the replay of
//                        CellMirror's take_out / put_in / refresh on staged copies in LDS, a full cell halts the chain
//   k_mcc_gcmc_trial     k_mcg_gcmc_trial with the cell walk, likewise
//   k_mcc_gcmc_accept    k_mcg_gcmc_accept with the replay of a displacement, an insertion or a deletion
#include "ceg_mc_gcmc.h"

using namespace ceg_mcs;

namespace {

__device__ McCellOps d_mcc_no_cell_ops;          // (a chain without cells: the accept body never reads it)

// cell_of_position (ceg_consumers.h) in device code: the same operations in the same order, nothing contracted
__device__ __forceinline__ int mcc_bin_of(const McView& v, double x, double y, double z)
{
#pragma clang fp contract(off)
    int b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double f = v.invmat[i] * x + v.invmat[3 + i] * y + v.invmat[6 + i] * z;
        f -= floor(f);
        const int q = (int)(f * v.nb[i]);
        b[i] = q < 0 ? 0 : (q >= v.nb[i] ? v.nb[i] - 1 : q);
    }
    return (b[0] * v.nb[1] + b[1]) * v.nb[2] + b[2];
}

__global__ void k_mcc_book_fill(McCellBook B, int32_t cap)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= B.nslots) return;
    const int c = B.cell_of[s], i = B.idx_of[s];
    if (c >= 0 && c < B.ncells && i >= 0 && i < cap) B.owner[(size_t)c * cap + i] = s;
}

// as k_mcg_sweep_trial (ceg_mc_sweep.hip), for the chains with cells
template <bool FAST>
__global__ __launch_bounds__(MC_THREADS, MC_TRIAL_WAVES) void k_mcc_sweep_trial(const McView* __restrict__ views, const McSweepChain* __restrict__ params,
                                                                 const int32_t* __restrict__ bead, const int32_t* __restrict__ list, int table_ok,
                                                                 uint64_t seed, uint64_t step, McPositions* prop, double* __restrict__ rows,
                                                                 const int64_t* stop)
{
    __shared__ McLocal s_L;
    const int c = list[blockIdx.x >> 1], r = (int)(blockIdx.x & 1u);
    if (chain_stopped(stop, c, step)) return;                      // (halted on a full cell, or stopped by the chain plan)
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
    mc_trial_row<FAST, false, true>(v, mv.molecule, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
}

// ---- the replay of CellMirror's sequential semantics for an accepted displacement (accept_cell_ops of ceg_mc.hip).
// Cell reference j: j = a the cell atom a sits in, j = MC_MAX_ATOMS + a the cell of its new position; references of one cell share
// the copy of the lowest j (canon).  A staged cell is its count and a window of its entries from `base` on: the last
// MC_MAX_ATOMS entries it has now (a take-out reads the tail, at most MC_MAX_ATOMS times) and the MC_MAX_ATOMS it can gain.
constexpr int MCC_REFS = 2 * MC_MAX_ATOMS, MCC_WIN = 2 * MC_MAX_ATOMS;
static_assert(MCC_REFS <= 64, "the candidates and the cell references of a step are compacted by one wave's ballot");
static_assert(2 * MC_MAX_ATOMS <= MC_MAX_CELL_OPS, "an atom gives at most two cell operations: one McCellOps holds a displacement");
static_assert(MC_THREADS >= 129 && MC_MAX_ATOMS <= 64, "mcc_commit: lanes 0.., 64.., 128 write the three parts of the book");
struct MccStage {
    int32_t cell[MCC_REFS], canon[MCC_REFS], cnt[MCC_REFS], base[MCC_REFS], touched[MCC_REFS];
    int32_t win[MCC_REFS][MCC_WIN];
    int32_t cof[MC_MAX_ATOMS], iof[MC_MAX_ATOMS];                 // cell and entry of the molecule's atoms as the replay goes
    int32_t cj[MCC_REFS], cc[MCC_REFS], ci[MCC_REFS], cslot[MCC_REFS], ncand;   // entries whose content changed, in the order of the replay:
                                                                 // staged cell (-1: a cell that is not staged), cell, entry, atom slot
    int32_t lcell[MC_MAX_ATOMS], lidx[MC_MAX_ATOMS];              // a deletion: cell and entry of the atoms of the molecule that takes over the index
    int32_t fslot[MC_MAX_ATOMS], fidx[MC_MAX_ATOMS], nforeign;    // idx_of of other molecules' atoms that moved into a hole, in order
    int32_t result;                                              // 0 applied, 1 a cell is full, 2 a range check failed
    int32_t peak;                                                // the longest list there was during the replay (CellMirror::max_fill)
};

// 0: `ops` holds the cell operations of the step and commit() may run; 1: a touched cell would exceed cell_cap; 2: the book is
// out of range somewhere.  Nothing is written to global memory.  All threads of the workgroup call it and get the same answer.
// mode MCC_MOVE: a displacement of the molecule in atom slots [first, first + m) to np (accept_cell_ops); MCC_INSERT: a new molecule in
// those slots at np (put-in of its atoms in order); MCC_REMOVE: the molecule in those slots goes (take-out of its atoms in order), then
// the atoms [lfirst, lfirst + lm) of the last molecule, which takes over the index, are refreshed (lm = 0: it was the last itself).
constexpr int MCC_MOVE = 0, MCC_INSERT = 1, MCC_REMOVE = 2;
__device__ __forceinline__ int mcc_replay(const McView& v, const McCellBook& B, MccStage& S, McCellOps& ops, int mode, int first, int m, const McPositions* np,
                                          int lfirst, int lm)
{
    const int tid = threadIdx.x, cap = v.cell_cap;
    const bool has_old = mode != MCC_INSERT, has_new = mode != MCC_REMOVE;
    int bad = 0;
    // 1. the lanes fetch cell, entry and new bin per atom
    if (tid < MCC_REFS) { S.cell[tid] = -1; S.touched[tid] = 0; }
    if (first < 0 || m < 1 || m > MC_MAX_ATOMS || first + m > B.nslots || cap < 1) return 2;          // (uniform)
    if (lm < 0 || lm > MC_MAX_ATOMS || (lm > 0 && (lfirst < 0 || lfirst + lm > B.nslots))) return 2;
    __syncthreads();
    if (tid < m) {
        int c = -1, i = -1, n = -1;
        if (has_old) {
            c = B.cell_of[first + tid]; i = B.idx_of[first + tid];
            if (c < 0 || c >= B.ncells || i < 0 || i >= cap) bad = 1;
        }
        if (has_new) {
            n = mcc_bin_of(v, np->xyz[3 * tid], np->xyz[3 * tid + 1], np->xyz[3 * tid + 2]);
            if (n < 0 || n >= B.ncells) bad = 1;
        }
        if (!bad) { S.cell[tid] = c; S.cell[MC_MAX_ATOMS + tid] = n; S.cof[tid] = c; S.iof[tid] = i; }
    }
    if (tid >= 64 && tid < 64 + lm) {
        const int c = B.cell_of[lfirst + tid - 64], i = B.idx_of[lfirst + tid - 64];
        if (c < 0 || c >= B.ncells || i < 0 || i >= cap) bad = 1;
        S.lcell[tid - 64] = c; S.lidx[tid - 64] = i;
    }
    if (__syncthreads_or(bad)) return 2;
    // 2. the counts of the distinct cells
    if (tid < MCC_REFS && S.cell[tid] >= 0) {
        int j = tid;
        for (int q = tid - 1; q >= 0; --q)
            if (S.cell[q] == S.cell[tid]) j = q;
        S.canon[tid] = j;
        if (j == tid) {
            const int n = v.cell_count[S.cell[tid]];
            if (n < 0 || n > cap) bad = 1;
            S.cnt[tid] = n;
            S.base[tid] = n > MC_MAX_ATOMS ? n - MC_MAX_ATOMS : 0;
        }
    }
    if (__syncthreads_or(bad)) return 2;
    // 3. their tail entries
    for (int e = tid; e < MCC_REFS * MC_MAX_ATOMS; e += MC_THREADS) {
        const int j = e / MC_MAX_ATOMS, t = e % MC_MAX_ATOMS;
        if (S.cell[j] < 0 || S.canon[j] != j) continue;
        const int idx = S.base[j] + t;
        if (idx >= S.cnt[j]) continue;
        const int s = B.owner[(size_t)S.cell[j] * cap + idx];
        if (s < 0 || s >= B.nslots) bad = 1;
        S.win[j][t] = s;
    }
    if (__syncthreads_or(bad)) return 2;
    // 4. the replay, atom by atom, on the staged copies
    if (tid == 0) {
        int res = 0, nc = 0, nf = 0, peak = 0;
        for (int a = 0; a < m && res == 0; ++a) {
            const int slot = first + a, cn = S.cell[MC_MAX_ATOMS + a];
            if (has_old && has_new && S.cof[a] == cn) {            // refresh: new coordinates in place
                S.cj[nc] = S.canon[a]; S.cc[nc] = cn; S.ci[nc] = S.iof[a]; S.cslot[nc] = slot; ++nc;
                continue;
            }
            if (has_old) {                                         // take_out: the last entry into the hole
                const int jo = S.canon[a], i = S.iof[a], no = S.cnt[jo];
                const int tail = no - 1 - S.base[jo];
                if (i >= no || tail < 0 || tail >= MCC_WIN) { res = 2; break; }
                const int moved = S.win[jo][tail];
                if (i >= S.base[jo]) S.win[jo][i - S.base[jo]] = moved;
                S.cj[nc] = jo; S.cc[nc] = S.cell[jo]; S.ci[nc] = i; S.cslot[nc] = moved; ++nc;
                if (moved >= first && moved < first + m) S.iof[moved - first] = i;
                else { S.fslot[nf] = moved; S.fidx[nf] = i; ++nf; }
                S.cnt[jo] = no - 1;
                S.touched[jo] = 1;
                S.cof[a] = -1; S.iof[a] = -1;
            }
            if (has_new) {                                         // put_in: append
                const int jn = S.canon[MC_MAX_ATOMS + a], nn = S.cnt[jn];
                if (nn >= cap) { res = 1; break; }
                if (nn - S.base[jn] >= MCC_WIN) { res = 2; break; }
                S.win[jn][nn - S.base[jn]] = slot;
                S.cj[nc] = jn; S.cc[nc] = cn; S.ci[nc] = nn; S.cslot[nc] = slot; ++nc;
                S.cof[a] = cn; S.iof[a] = nn;
                S.cnt[jn] = nn + 1;
                peak = peak > nn + 1 ? peak : nn + 1;
                S.touched[jn] = 1;
            }
        }
        // a deletion: the records of the molecule that takes over the index carry the new index -- refreshed where they sit now (an
        // atom of it that moved into a hole above has its new entry in the list of moved atoms; the last one counts)
        for (int a = 0; a < lm && res == 0; ++a) {
            int i = S.lidx[a];
            for (int q = 0; q < nf; ++q)
                if (S.fslot[q] == lfirst + a) i = S.fidx[q];
            S.cj[nc] = -1; S.cc[nc] = S.lcell[a]; S.ci[nc] = i; S.cslot[nc] = lfirst + a; ++nc;
        }
        S.ncand = nc; S.nforeign = nf; S.result = res; S.peak = peak;
    }
    __syncthreads();
    const int res = S.result;
    if (res) return res;
    // 5. McCellOps: of the entries that changed the last state of each, where it still lies inside its list; the counts of the
    //    cells that lost or gained an entry
    if (tid < 64) {
        const int nc = S.ncand;
        bool alive = tid < nc && (S.cj[tid] < 0 || S.ci[tid] < S.cnt[S.cj[tid]]);
        for (int q = tid + 1; alive && q < nc; ++q)
            if (S.cc[q] == S.cc[tid] && S.ci[q] == S.ci[tid]) alive = false;
        const unsigned long long mask = __ballot(alive);
        if (alive) {
            const int at = __popcll(mask & ((1ull << tid) - 1ull));
            ops.dst[at] = S.cc[tid] * cap + S.ci[tid];
            ops.src[at] = S.cslot[tid];
        }
        const bool counted = tid < MCC_REFS && S.touched[tid];
        const unsigned long long cmask = __ballot(counted);
        if (counted) {
            const int at = __popcll(cmask & ((1ull << tid) - 1ull));
            ops.cell[at] = S.cell[tid];
            ops.count[at] = S.cnt[tid];
        }
        if (tid == 0) { ops.nops = __popcll(mask); ops.ncnt = __popcll(cmask); }
    }
    __syncthreads();
    return 0;
}

__device__ __forceinline__ int mcc_replay_move(const McView& v, const McCellBook& B, MccStage& S, McCellOps& ops, int first, int m, const McPositions& np)
{
    return mcc_replay(v, B, S, ops, MCC_MOVE, first, m, &np, 0, 0);
}

// the book after a replay that returned 0: owner[] at the entries of `ops`, cell_of / idx_of of the molecule's atoms and of the atoms
// of other molecules that moved into a hole (one thread, in order: an atom can move twice)
__device__ __forceinline__ void mcc_commit(const McCellBook& B, const MccStage& S, const McCellOps& ops, int first, int m)
{
    const int tid = threadIdx.x;
    if (tid < ops.nops) B.owner[ops.dst[tid]] = ops.src[tid];
    if (tid >= 64 && tid < 64 + m) { B.cell_of[first + tid - 64] = S.cof[tid - 64]; B.idx_of[first + tid - 64] = S.iof[tid - 64]; }
    if (tid == 128)
        for (int q = 0; q < S.nforeign; ++q) B.idx_of[S.fslot[q]] = S.fidx[q];
}

// as k_mcg_sweep_accept (ceg_mc_sweep.hip); a chain with cells replays its cell operations before anything of the step is written
__global__ __launch_bounds__(MC_THREADS) void k_mcc_sweep_accept(const McView* __restrict__ views, const McSweepChain* __restrict__ params,
                                                                 const McCellBook* __restrict__ books, uint64_t seed, uint64_t step,
                                                                 const McPositions* __restrict__ prop, const double* __restrict__ rows,
                                                                 ceg_mc_sweep_stats_t* __restrict__ stats, ceg_mc_sweep_record_t* __restrict__ log,
                                                                 int64_t* stop, int64_t* halt, int32_t* flags)
{
    __shared__ MccStage s_stage;
    __shared__ McCellOps s_ops;
    const int c = (int)blockIdx.x, tid = threadIdx.x;
    if (chain_stopped(stop, c, step)) {                            // (stopped by the chain plan, or halted at an earlier step)
        if (log && tid == 0) { log[c].molecule = -2; log[c].kind = -1; }
        return;
    }
    const McView& v = as_constant(views)[c];
    const McSweepChain& P = as_constant(params)[c];
    const McCellBook B = books[c];
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
    const int2 mj = v.mol[mv.molecule];
    const bool cells = v.use_cells && B.cell_of;
    if (accepted && cells) {
        const int res = mcc_replay_move(v, B, s_stage, s_ops, mj.x, mj.y, np);
        if (res) {                                                 // nothing of the step is applied: the chain halts here
            if (tid == 0) {
                stop[c] = (int64_t)step;
                halt[c] = (int64_t)step;
                if (res == 2) flags[2 * c] = 1;
                if (rec) { rec->molecule = -2; rec->kind = -1; }
            }
            return;
        }
    }
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
    if (rec && tid < 3 * mj.y) rec->positions[tid / 3][tid % 3] = np.xyz[tid];
    if (!accepted) return;
    if (cells) {
        if (tid == 0 && s_stage.peak > flags[2 * c + 1]) flags[2 * c + 1] = s_stage.peak;       // (one workgroup per chain: no race)
        mcc_commit(B, s_stage, s_ops, mj.x, mj.y);
        mc_accept_body(v, mv.molecule, np, s_ops, P.stride);
    } else {
        mc_accept_body(v, mv.molecule, np, d_mcc_no_cell_ops, P.stride);
    }
}

// ---- GCMC sweeps on chains with cells.  As k_mcg_gcmc_trial (ceg_mc_sweep.hip) with the cell walk; a halted or stopped chain's workgroups
// return at once
template <bool FAST>
__global__ __launch_bounds__(MC_THREADS, MC_TRIAL_WAVES) void k_mcc_gcmc_trial(const McView* __restrict__ views, const McGcmcChain* __restrict__ params,
                                                                const ceg_mc_gcmc_species_t* __restrict__ spec, int nspecies, const McGcmcTable* tables,
                                                                const int32_t* molspec, const int32_t* __restrict__ list, int table_ok, uint64_t seed,
                                                                uint64_t step, const McBlock* __restrict__ blocks, int nblock_kinds, int32_t* resolved,
                                                                McPositions* prop, double* __restrict__ rows, const int64_t* stop)
{
    __shared__ McLocal s_L;
    const int c = list[blockIdx.x >> 1], r = (int)(blockIdx.x & 1u);
    if (chain_stopped(stop, c, step)) return;                      // (halted on a full cell, or stopped by the chain plan)
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
    if (mv.kind == 5) mc_trial_row<FAST, true, true>(v, -1, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
    else mc_trial_row<FAST, false, true>(v, mv.molecule, s_L, mine->xyz, rows, P.stride, nullptr, nullptr, 0ull, at);
}

// as k_mcg_gcmc_accept (ceg_mc_sweep.hip); a chain with cells replays the cell operations of an accepted step -- displacement, insertion
// or deletion -- before anything of the step is written
__global__ __launch_bounds__(MC_THREADS) void k_mcc_gcmc_accept(const McView* __restrict__ views, const McGcmcChain* __restrict__ params,
                                                                const ceg_mc_gcmc_species_t* __restrict__ spec, int nspecies, McGcmcTable* tables,
                                                                int32_t* molspec, int32_t* freeslots, uint64_t seed, uint64_t step,
                                                                const int32_t* resolved, int64_t* __restrict__ pockets,
                                                                const McPositions* __restrict__ prop, const double* __restrict__ rows,
                                                                ceg_mc_gcmc_stats_t* __restrict__ stats, ceg_mc_gcmc_record_t* __restrict__ log,
                                                                const double* __restrict__ chain_phi, const McCellBook* __restrict__ books, int64_t* stop, int64_t* halt,
                                                                int32_t* cflags)
{
    __shared__ McMolecule s_nm;
    __shared__ MccStage s_stage;
    __shared__ McCellOps s_ops;
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
    // ---- the cell operations of an accepted step, before anything is written
    const McCellBook B = books[c];
    const bool cells = v.use_cells && B.cell_of;
    const int first_new = mv.kind == 5 ? (nf > 0 ? gcmc_ld(fstack + nf - 1) : mv.natoms) : 0;
    if (accepted && cells) {
        int res;
        if (mv.kind <= 4) {
            const int2 mj = v.mol[mv.molecule];
            res = mcc_replay(v, B, s_stage, s_ops, MCC_MOVE, mj.x, mj.y, &np, 0, 0);
        } else if (mv.kind == 5) {
            res = mcc_replay(v, B, s_stage, s_ops, MCC_INSERT, first_new, m, &np, 0, 0);
        } else {
            const int2 gone = v.mol[mv.molecule], lastm = v.mol[mv.nmol - 1];
            res = mcc_replay(v, B, s_stage, s_ops, MCC_REMOVE, gone.x, gone.y, nullptr, lastm.x, mv.nmol - 1 != mv.molecule ? lastm.y : 0);
        }
        if (res) {                                                 // nothing of the step is applied: the chain halts here
            if (tid == 0) {
                stop[c] = (int64_t)step;
                halt[c] = (int64_t)step;
                if (res == 2) cflags[2 * c] = 1;
                if (rec) { rec->species = -1; rec->molecule = -2; rec->kind = -1; }
            }
            return;
        }
    }
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
    const McCellOps& ops = cells ? s_ops : d_mcc_no_cell_ops;
    if (cells) {
        if (tid == 0 && s_stage.peak > cflags[2 * c + 1]) cflags[2 * c + 1] = s_stage.peak;       // (one workgroup per chain: no race)
        const int2 at = mv.kind == 5 ? make_int2(first_new, m) : v.mol[mv.molecule];
        mcc_commit(B, s_stage, s_ops, at.x, at.y);
        __syncthreads();                             // (v.mol is read above and rewritten by the bodies of an insertion or a deletion)
    }
    if (mv.kind <= 4) {
        mc_accept_body(v, mv.molecule, np, ops, P.stride);
    } else if (mv.kind == 5) {
        const int first = first_new;
        if (tid < m) s_nm.kinds[tid] = sp.kinds[tid];
        if (tid == 0) s_nm.m = m;
        __syncthreads();
        mc_insert_body(v, mv.nmol, first, s_nm, np, ops, P.stride);
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
        mc_remove_body(v, mv.molecule, last, ops);
        if (tid == 0) {
            if (last != mv.molecule) molspec[P.spec_off + mv.molecule] = spec_last;
            if (nfd < P.free_cap) { fstack[nfd] = first_gone; T->nfree[i] = nfd + 1; }      // (a full stack cannot happen: the run would be lost, not reused)
            T->nmol = last;
            T->count[i] = mv.n_i - 1;
        }
    }
}

}  // namespace

void ceg_mcs::cells_book_fill(hipStream_t stream, const McView& v, const McCellBook& book)
{
    if (book.nslots > 0)
        hipLaunchKernelGGL(k_mcc_book_fill, dim3((unsigned)((book.nslots + 255) / 256)), dim3(256), 0, stream, book, v.cell_cap);
}

void ceg_mcs::cells_sweep_trial(bool fast, dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McSweepChain* params, const int32_t* bead,
                                const int32_t* list, int table_ok, uint64_t seed, uint64_t step, McPositions* prop, double* rows, const int64_t* stop)
{
    hipLaunchKernelGGL((fast ? k_mcc_sweep_trial<true> : k_mcc_sweep_trial<false>), grid, dim3(MC_THREADS), lds, stream, views, params, bead, list, table_ok, seed,
                       step, prop, rows, stop);
}

void ceg_mcs::cells_sweep_accept(dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McSweepChain* params, const CellSweep& cs, uint64_t seed,
                                 uint64_t step, const McPositions* prop, const double* rows, ceg_mc_sweep_stats_t* stats, ceg_mc_sweep_record_t* log)
{
    hipLaunchKernelGGL(k_mcc_sweep_accept, grid, dim3(MC_THREADS), lds, stream, views, params, cs.books, seed, step, prop, rows, stats, log, cs.stop, cs.halt,
                       cs.flags);
}

void ceg_mcs::cells_gcmc_trial(bool fast, dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McGcmcChain* params,
                               const ceg_mc_gcmc_species_t* spec, int nspecies, const McGcmcTable* tables, const int32_t* molspec, const int32_t* list,
                               int table_ok, uint64_t seed, uint64_t step, const ceg_mc_block_t* blocks, int nblock_kinds, int32_t* resolved,
                               McPositions* prop, double* rows, const int64_t* stop)
{
    hipLaunchKernelGGL((fast ? k_mcc_gcmc_trial<true> : k_mcc_gcmc_trial<false>), grid, dim3(MC_THREADS), lds, stream, views, params, spec, nspecies, tables,
                       molspec, list, table_ok, seed, step, blocks, nblock_kinds, resolved, prop, rows, stop);
}

void ceg_mcs::cells_gcmc_accept(dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McGcmcChain* params,
                                const ceg_mc_gcmc_species_t* spec, int nspecies, McGcmcTable* tables, int32_t* molspec, int32_t* freeslots,
                                uint64_t seed, uint64_t step, const int32_t* resolved, int64_t* pockets, const McPositions* prop, const double* rows,
                                ceg_mc_gcmc_stats_t* stats, ceg_mc_gcmc_record_t* log, const double* chain_phi, const CellSweep& cs)
{
    hipLaunchKernelGGL(k_mcc_gcmc_accept, grid, dim3(MC_THREADS), lds, stream, views, params, spec, nspecies, tables, molspec, freeslots, seed, step,
                       resolved, pockets, prop, rows, stats, log, chain_phi, cs.books, cs.stop, cs.halt, cs.flags);
}
