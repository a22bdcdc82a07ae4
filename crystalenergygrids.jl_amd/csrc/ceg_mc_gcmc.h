// ceg_mc_gcmc.h -- what the GCMC sweep kernels of ceg_mc_sweep.hip (chains with the exhaustive pair loop) and of ceg_mc_cells.hip
// (chains with neighbour cells) share: the per-chain parameters and the device's molecule table of ceg_mc_group_sweep_gcmc, the
// selection of a step's move, its proposal, and the block pockets with the retry loop of choose_step!.
#pragma once
#include "ceg_mc_sweep.h"

namespace ceg_mcs {

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

// defined in ceg_mc_cells.hip: the GCMC sweep launches of the chains with cells (trial) and of a group that has one (accept)
void cells_gcmc_trial(bool fast, dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McGcmcChain* params,
                      const ceg_mc_gcmc_species_t* spec, int nspecies, const McGcmcTable* tables, const int32_t* molspec, const int32_t* list,
                      int table_ok, uint64_t seed, uint64_t step, const ceg_mc_block_t* blocks, int nblock_kinds, int32_t* resolved,
                      McPositions* prop, double* rows, const int64_t* stop);
void cells_gcmc_accept(dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McGcmcChain* params,
                       const ceg_mc_gcmc_species_t* spec, int nspecies, McGcmcTable* tables, int32_t* molspec, int32_t* freeslots,
                       uint64_t seed, uint64_t step, const int32_t* resolved, int64_t* pockets, const McPositions* prop, const double* rows,
                       ceg_mc_gcmc_stats_t* stats, ceg_mc_gcmc_record_t* log, const double* chain_phi, const CellSweep& cs);

}  // namespace ceg_mcs
