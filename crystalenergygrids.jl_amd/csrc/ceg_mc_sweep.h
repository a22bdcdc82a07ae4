// ceg_mc_sweep.h -- what the sweep kernels of ceg_mc_sweep.hip (chains with the exhaustive pair loop) and of ceg_mc_cells.hip (chains
// with neighbour cells) share: the per-chain parameters of ceg_mc_group_sweep, the selection and the proposal of a step, the
// Metropolis rule of a displacement, and the device's book of the cell lists (McCellBook) with its launchers.
#pragma once
#include "ceg_mc_state.h"

namespace ceg_mcs {

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

struct McSweepChain {            // per chain, device memory
    uint32_t stream_id;
    int32_t bead_off;            // the chain's first entry of the bead array
    int32_t stride, _pad;
    double temperature, dmax, thetamax, p_rotation;
};

struct McMove { int32_t molecule, kind; };       // kind 0 translation, 1 rotation; molecule -1: the chain is idle

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

// ---- the cell lists of a chain on the device (ceg_mc_group_set_device_cells), the device form of CellMirror::cell_of / idx_of /
// members: authoritative only while a sweep runs.  One entry per chain in the group's block; cell_of == nullptr: the chain keeps no
// neighbour cells (or the group has not switched device cells on).
struct McCellBook {
    int32_t* cell_of;            // [nslots] cell of the atom slot, -1: in no cell
    int32_t* idx_of;             // [nslots] its entry in that cell
    int32_t* owner;              // [ncells * cell_cap] the atom slot whose record sits at that entry
    int32_t ncells, nslots;
};

// what a sweep with cells chains hands to its launches beside the arguments of the plain kernels
struct CellSweep {
    const McCellBook* books;     // [K]
    int64_t* stop;               // [K] the chain plan's stops (INT64_MAX: none), lowered to the halting step by the accept launch
    int64_t* halt;               // [K] -1, or the step at which a full cell (or a failed range check) halted the chain
    int32_t* flags;              // [K][2]: 1 where a range check of the book failed (the host marks the chain inconsistent); the longest
                                 // cell list there was within an applied step (CellMirror::max_fill counts the fill between take-out and put-in)
};

// defined in ceg_mc_cells.hip
void cells_book_fill(hipStream_t stream, const McView& v, const McCellBook& book);       // owner[] from cell_of[] / idx_of[]
void cells_sweep_trial(bool fast, dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McSweepChain* params, const int32_t* bead,
                       const int32_t* list, int table_ok, uint64_t seed, uint64_t step, McPositions* prop, double* rows, const int64_t* stop);
void cells_sweep_accept(dim3 grid, size_t lds, hipStream_t stream, const McView* views, const McSweepChain* params, const CellSweep& cs, uint64_t seed,
                        uint64_t step, const McPositions* prop, const double* rows, ceg_mc_sweep_stats_t* stats, ceg_mc_sweep_record_t* log);

}  // namespace ceg_mcs
