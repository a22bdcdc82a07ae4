// ceg_mc_state.h -- what ceg_mc.hip (ceg_mc_*), ceg_mc_group.hip and ceg_mc_sweep.hip (ceg_mc_group_*) and ceg_mc_baseline.hip (ceg_mc_baseline,
// ceg_mc_group_baseline) share: the kernel-side view of a handle, the bodies of the trial row, of the three updates and of the
// structure-factor rebuild, and the host-side handle with its cell mirror.  Several translation units include this, so the names live
// in namespace ceg_mcs; the kernels stay in the anonymous namespaces of the files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/ceg_hip.h"
#include "ceg_consumers.h"
#include "ceg_rows.h"
#include "ceg_pairfrac.h"
#include "ceg_philox.h"

extern "C" void ceg_set_last_error_(const char* msg);

namespace ceg_mcs {

using ceg::DevRule;
using ceg_consumers::InterpGeom;
using ceg_consumers::interp_point;
using ceg_consumers::rule_energy;
using ceg_consumers::rule_energy_fast;

constexpr int MC_MAX_ATOMS = 16;
constexpr int MC_THREADS = 256;
#ifndef MC_TRIAL_WAVES
#define MC_TRIAL_WAVES 3          // waves per SIMD asked of the trial kernel (the neighbour-cell code had pushed it to 169 VGPRs = 2 waves)
#endif

struct McGrid {
    InterpGeom g;
    const float* grid;        // node-major [x][y][z][8] in K; nullptr: zero grid (interpolate_grid returns 0, grids.jl:213)
};

// everything a kernel needs, by value (kernarg)
struct McView {
    double mat[9], invmat[9];                  // MC cell (pair distances, src/utils.jl:294-302)
    double ew_invmat[9];                       // inverse of the Ewald supercell matrix
    double cutoff2, coulombic;
    int32_t nkinds, nrules, fast, table_in_lds;
    int32_t ks[3], nk;
    int32_t natoms, nmol;                      // natoms: high-water mark of the atom slots
    const McGrid* vdw;                         // [nkinds]
    McGrid coulomb;
    const double* kind_charge;                 // [nkinds]
    const DevRule* rules;
    const int32_t* rule_offset;                // [nkinds*nkinds + 1]
    const int32_t* ijk;                        // [3 nk]
    const double* kf;                          // [nk]
    const double2* sf_fw;                      // [nk] StoreRigidChargeFramework
    double2* sf_tot;                           // [nk] sums[:, 1]
    double2* sf_mol;                           // [nmol][nk] sums[:, ij+1]
    double4* atoms;                            // x, y, z, (molecule << 32 | kind); molecule < 0: free slot
    double4* fatoms;                           // the same slots with invmat * position (the pair tests of ceg_pairfrac.h)
    int2* mol;                                 // [nmol] atoms of molecule j: slots [mol[j].x, mol[j].x + mol[j].y)
    // neighbour cells of the guest atoms (what the reference gets from CellListMap, src/energy.jl:341-349,399-404):
    // fractional bins of the MC cell, fixed capacity, each holding COPIES of its atoms' records
    int32_t use_cells, cell_cap;
    int32_t nb[3];
    double hfrac[3];                           // cutoff / perpendicular width: fractional half-extent of the cutoff sphere
    double4* cells;                            // [nb0*nb1*nb2][cell_cap]
    double4* fcells;                           // the same entries, fractional
    int32_t* cell_count;                       // [nb0*nb1*nb2]
    // the k-vectors as rows cut into segments and dealt to 64 lanes in rounds (ceg_rows.h)
    int32_t nrounds, ns;
    int32_t fastwrap, _pad1;                   // ceg_consumers::wrap_mode: 0 literal pair distances, 1 fast wrap, 2 fast wrap in an upper-triangular cell
    const double* geom;                        // mat[9], invmat[9] in device memory (literal fall-back of the fast pair distance)
    const int32_t* desc;                       // [nrounds * 64]
    const int32_t* qof;                        // [ns * 64] k-vector of (slot, lane), -1 in the padding slots
};

// what an update does to the cells, worked out on the host mirror of the cell lists: cells[dst[i]] = atoms[src[i]] once the
// atom records are current, then cell_count[cell[i]] = count[i]
constexpr int MC_MAX_CELL_OPS = 2 * 16;
struct McCellOps {
    int32_t nops, ncnt;
    int32_t dst[MC_MAX_CELL_OPS], src[MC_MAX_CELL_OPS], cell[MC_MAX_CELL_OPS], count[MC_MAX_CELL_OPS];
};

// an atom record into its slot, Cartesian and fractional
__device__ __forceinline__ void put_atom(const McView& v, int slot, const double4 A)
{
    const double* I = v.invmat;
    v.atoms[slot] = A;
    v.fatoms[slot] = make_double4(__builtin_fma(I[6], A.z, __builtin_fma(I[3], A.y, I[0] * A.x)), __builtin_fma(I[7], A.z, __builtin_fma(I[4], A.y, I[1] * A.x)),
                                  __builtin_fma(I[8], A.z, __builtin_fma(I[5], A.y, I[2] * A.x)), A.w);
}

__device__ __forceinline__ void apply_cell_ops(const McView& v, const McCellOps& ops, int tid)
{
    if (tid < ops.nops) {
        v.cells[ops.dst[tid]] = v.atoms[ops.src[tid]];
        v.fcells[ops.dst[tid]] = v.fatoms[ops.src[tid]];
    }
    if (tid < ops.ncnt) v.cell_count[ops.cell[tid]] = ops.count[tid];
}

// a molecule that is not (yet) in the system: kinds of its atoms (single_contribution_ewald with ij < 0, ewald.jl:704-728)
struct McMolecule { int32_t m; int32_t kinds[MC_MAX_ATOMS]; };

struct McPositions { double xyz[MC_MAX_ATOMS * 3]; };

// the molecule on trial as the host knows it (k_mc_trial: no dependent loads of slot, kinds and charges in front of a batch-1 call)
struct McLocal { int32_t first, m; int32_t kinds[MC_MAX_ATOMS]; double q[MC_MAX_ATOMS]; };

__device__ __forceinline__ void unpack(double w, int& kind, int& mol)
{
    const long long bits = __double_as_longlong(w);
    kind = (int)(bits & 0xffffffffll);
    mol = (int)(bits >> 32);
}

// e^{2 pi i m f} tables of `m_atoms` atoms at s_pos (setup_Eik / move_one_system!, src/ewald.jl:109-146,352-366),
// by sine / cosine of the exact angle (ceg_math.h sincos_2pi); entry t of atom a at tab[a * stride + t]: t in [0, kx] -> x, then y (m = -ky..ky), then z
// s_q != nullptr: the z entries carry the atom's charge as a factor (what the row-wise walk of ceg_rows.h expects)
__device__ __forceinline__ void fill_tables(const McView& v, const double* s_pos, int m_atoms, double2* tab, int stride, int tid, int nthreads,
                                            const double* s_q = nullptr)
{
    const int kx = v.ks[0], ky = v.ks[1], kz = v.ks[2];
    const int nxp = kx + 1, nyp = 2 * ky + 1;
    const double* I = v.ew_invmat;
    for (int e = tid; e < m_atoms * stride; e += nthreads) {
        const int a = e / stride, t = e - a * stride;
        const double x = s_pos[3 * a], y = s_pos[3 * a + 1], z = s_pos[3 * a + 2];
        double f;
        int mm;
        if (t < nxp) { f = I[0] * x + I[3] * y + I[6] * z; mm = t; }
        else if (t < nxp + nyp) { f = I[1] * x + I[4] * y + I[7] * z; mm = t - nxp - ky; }
        else { f = I[2] * x + I[5] * y + I[8] * z; mm = t - nxp - nyp - kz; }
        const double ff = f - rint(f);
        double s, c;
        ceg::sincos_2pi((double)mm * ff, s, c);
        const double w = (s_q && t >= nxp + nyp) ? s_q[a] : 1.0;
        tab[e] = make_double2(w * c, w * s);
    }
}

// the same tables filled by ONE wave (k_mcw_ewald): entry t per lane, the atoms in an inner loop -- no division by the stride, the axis
// decoded once per entry
__device__ __forceinline__ void fill_tables_wave(const McView& v, const double* s_pos, int m_atoms, double2* tab, int stride, int lane, const double* s_q)
{
    const int kx = v.ks[0], ky = v.ks[1], kz = v.ks[2];
    const int nxp = kx + 1, nyp = 2 * ky + 1;
    const double* I = v.ew_invmat;
    for (int t = lane; t < stride; t += 64) {
        const int ax = t < nxp ? 0 : (t < nxp + nyp ? 1 : 2);
        const int mm = ax == 0 ? t : (ax == 1 ? t - nxp - ky : t - nxp - nyp - kz);
        const double i0 = I[ax], i1 = I[ax + 3], i2 = I[ax + 6];
        for (int a = 0; a < m_atoms; ++a) {
            const double f = i0 * s_pos[3 * a] + i1 * s_pos[3 * a + 1] + i2 * s_pos[3 * a + 2];
            const double ff = f - rint(f);
            double s, c;
            ceg::sincos_2pi((double)mm * ff, s, c);
            const double w = ax == 2 ? s_q[a] : 1.0;
            tab[a * stride + t] = make_double2(w * c, w * s);
        }
    }
}

// The structure factor of the molecule whose tables (charge on z) are `tab`, k-vector by k-vector in the row-wise order of ceg_rows.h:
// wave `wave` of `nwaves` takes the rounds wave, wave + nwaves, ...; sink(q, re, im) for every real k-vector.
template <class Sink>
__device__ __forceinline__ void rows_structure_factor(const McView& v, const double2* tab, int stride, int m_atoms, int wave, int nwaves, int lane, Sink&& sink)
{
    const int nxp = v.ks[0] + 1, nyp = 2 * v.ks[1] + 1;
    int slot = 0;
    for (int r = 0; r < v.nrounds; ++r) {
        const int d = v.desc[r * 64 + lane];
        const int L = __builtin_amdgcn_readfirstlane(d >> 27);
        if (r % nwaves == wave) {
            const int at = slot * 64 + lane;
            ceg_rows::round_dispatch(L, m_atoms, tab, stride, nxp, nyp, d & 0x1ff, (d >> 9) & 0x1ff, (d >> 18) & 0x1ff, [&](int sidx, double sr, double si) {
                const int q = v.qof[at + sidx * 64];
                if (q >= 0) sink(q, sr, si);
            });
        }
        slot += L;
    }
}

// structure factor of the molecule at k-vector q from the tables: sum_a q_a Ex[i] Ey[j] Ez[k]   (src/ewald.jl:148-185)
__device__ __forceinline__ double2 molecule_sf(const McView& v, const double2* tab, int stride, const double* s_q, int m_atoms, int64_t q)
{
    const int ky = v.ks[1], kz = v.ks[2];
    const int nxp = v.ks[0] + 1, nyp = 2 * ky + 1;
    const int i = v.ijk[3 * q], j = v.ijk[3 * q + 1], k = v.ijk[3 * q + 2];
    double sr = 0.0, si = 0.0;
    for (int a = 0; a < m_atoms; ++a) {
        const double2 ex = tab[a * stride + i];
        const double2 ey = tab[a * stride + nxp + ky + j];
        const double2 ez = tab[a * stride + nxp + nyp + kz + k];
        const double yr = ey.x * ez.x - ey.y * ez.y, yi = ey.x * ez.y + ey.y * ez.x;
        const double cr = s_q[a] * yr, ci = s_q[a] * yi;
        sr += ex.x * cr - ex.y * ci;
        si += ex.x * ci + ex.y * cr;
    }
    return make_double2(sr, si);
}

// INSERT: the molecule is described by `nm` and is not in the system -- no current-position row, nothing excluded from the
// pair sum, rest = framework + sums[:, 1]
// The row of one workgroup.  `at` says which: at.b() = 0 the molecule where it is now, b >= 1 trial placement b - 1 (at
// trial[(b - 1) m 3]); the row goes to at.row(out)[0..3]; at.nblocks() workgroups share `done` (the last one to finish raises `flag`).
// k_mc_trial passes its kernarg view and McAtBlock, k_mcg_trial a chain's view from device memory and McAtChainRow.  (The row index,
// the output pointer and the workgroup count are worked out where they are used: computed in front of the body, they stayed live
// through it and cost the batch-1 kernel a spill.)
struct McAtBlock {
    template <bool INSERT> __device__ __forceinline__ int64_t b() const { return INSERT ? (int64_t)blockIdx.x + 1 : (int64_t)blockIdx.x; }
    __device__ __forceinline__ double* row(double* out) const { return out + 4 * (size_t)blockIdx.x; }
    __device__ __forceinline__ unsigned nblocks() const { return gridDim.x * gridDim.y; }
    __device__ __forceinline__ bool table_in_lds(const McView& v) const { return v.table_in_lds; }
    __device__ __forceinline__ int natoms(const McView& v) const { return v.natoms; }
};

template <bool FAST, bool INSERT, bool CELLS, class At>
__device__ __forceinline__ void mc_trial_row(const McView& v, int32_t molecule, const McLocal& L, const double* __restrict__ trial,
                                             double* __restrict__ out, int stride, unsigned* done, unsigned long long* flag,
                                             unsigned long long seq, const At& at)
{
    const int64_t b = at.template b<INSERT>();        // 0: where the molecule is now; b >= 1: trial b - 1
    const bool table_in_lds = at.table_in_lds(v);
    // dynamic LDS: [m][stride] double2 tables, then (table_in_lds) the pair table
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_pos[MC_MAX_ATOMS * 3];
    __shared__ double s_q[MC_MAX_ATOMS];
    __shared__ int32_t s_kind[MC_MAX_ATOMS];
    __shared__ double s_red[MC_THREADS / 64][5];
    __shared__ int s_bin0[3], s_nbin[3], s_wtot[MC_THREADS / 64], s_first[MC_THREADS], s_cell[MC_THREADS];
    const int tid = threadIdx.x;
    // gridDim.y == 3: the three terms of a row on three workgroups (blockIdx.y = 0 framework grids, 1 reciprocal sum, 2 guest-guest pairs) --
    // the latency of a small batch is the longest term, not their sum; gridDim.y == 1: one workgroup does all three
    const int term = gridDim.y == 1 ? -1 : (int)blockIdx.y;
    const bool do_frame = term < 0 || term == 0, do_ewald = term < 0 || term == 1, do_pairs = term < 0 || term == 2;
    const int first = L.first, m = L.m;
    double2* tab = reinterpret_cast<double2*>(s_raw);
    const DevRule* rules = v.rules;
    const int32_t* offset = v.rule_offset;
    if (table_in_lds && do_pairs) {
        DevRule* lr = reinterpret_cast<DevRule*>(s_raw + sizeof(double2) * (size_t)m * stride);
        int32_t* lo = reinterpret_cast<int32_t*>(lr + (v.nrules > 0 ? v.nrules : 1));
        for (int t = tid; t < v.nrules; t += MC_THREADS) lr[t] = v.rules[t];
        for (int t = tid; t < v.nkinds * v.nkinds + 1; t += MC_THREADS) lo[t] = v.rule_offset[t];
        rules = lr;
        offset = lo;
    }
    if (tid < 3 * m) {
        if (b == 0) {
            const double4 A = v.atoms[first + tid / 3];
            s_pos[tid] = (tid % 3 == 0) ? A.x : ((tid % 3 == 1) ? A.y : A.z);
        } else {
            s_pos[tid] = trial[(size_t)(b - 1) * m * 3 + tid];
        }
    }
    if (tid < m) {
        s_kind[tid] = L.kinds[tid];
        s_q[tid] = L.q[tid];
    }
    // the k-space constants of the first k-vectors of this thread do not depend on the positions: fetched before anything else
    constexpr int R = 3;
    const double2* mine = v.sf_mol + (size_t)(INSERT ? 0 : molecule) * v.nk;
    struct KChunk { double2 old[R], f[R], t[R]; double kf[R]; };
    auto load_chunk = [&](const int64_t q0, KChunk& c) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t q = q0 + (int64_t)r * MC_THREADS;
            const bool in = q < v.nk;
            const int64_t qq = in ? q : 0;
            c.old[r] = (INSERT || !in) ? make_double2(0.0, 0.0) : mine[qq];
            c.f[r] = in ? v.sf_fw[qq] : make_double2(0.0, 0.0);
            c.t[r] = in ? v.sf_tot[qq] : make_double2(0.0, 0.0);
            c.kf[r] = in ? v.kf[qq] : 0.0;
        }
    };
    KChunk cur;
    if (v.nk > 0 && do_ewald) load_chunk(tid, cur);
    double4 A_first = make_double4(0.0, 0.0, 0.0, 0.0);             // likewise the first guest atom of this thread
    // (with no guest this reads slot 0 of the minimum array ceg_mc_create allocates and zeroes: in bounds, and used by no pair.  A test
    //  of natoms here moves the register allocation of the batch-1 kernels, which tests/test_mc_chains_static.py pins.)
    if (do_pairs && !CELLS) A_first = v.atoms[tid < at.natoms(v) ? tid : 0];
    __syncthreads();

    double fv = 0.0, fd = 0.0, inter = 0.0, rs = 0.0, ss = 0.0;
    // ---- framework_interactions (montecarlo.jl:490-504): thread 16a + 8g + corner, g = 0 the VdW grid of atom a, g = 1 the Coulomb grid --
    // one grid CORNER per thread, three shuffles per sum (the 64-term polynomial on one thread was the longest chain of a batch-1 call)
    if (do_frame) {
        static_assert(16 * MC_MAX_ATOMS <= MC_THREADS, "one thread per corner");
        const int a = tid >> 4, gsel = (tid >> 3) & 1, corner = tid & 7;
        double part = 0.0;
        bool blocked = false, have = false, isvdw = false;
        if (tid < 16 * m) {
            const double px = s_pos[3 * a], py = s_pos[3 * a + 1], pz = s_pos[3 * a + 2];
            if (gsel == 0) {
                const McGrid* G = v.vdw + s_kind[a];
                if (G->grid) { part = ceg_consumers::interp_corner(G->g, G->grid, px, py, pz, corner, blocked); have = true; isvdw = G->g.is_vdw != 0; }
            } else if (v.coulomb.grid) {
                part = ceg_consumers::interp_corner(v.coulomb.g, v.coulomb.grid, px, py, pz, corner, blocked);
                have = true;
                isvdw = v.coulomb.g.is_vdw != 0;
            }
        }
        int blk = blocked ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            part += __shfl_xor(part, o);
            blk |= __shfl_xor(blk, o);
        }
        if (have && corner == 0) {
            const double val = (isvdw && blk) ? 1e100 : part;         // grids.jl:245-248
            if (gsel == 0) fv = val;
            else fd = (val == 1e100) ? val : s_q[a] * val;            // montecarlo.jl:500
        }
    }
    // ---- single_contribution_ewald (ewald.jl:704-738)
    if (v.nk > 0 && do_ewald) {
        if (b != 0) fill_tables(v, s_pos, m, tab, stride, tid, MC_THREADS);
        __syncthreads();
        // three k-vectors per thread at a time, the constants of the next three fetched while these are worked on: one L2 round trip for
        // the whole walk where a plain loop pays one per round (5-6 rounds of 256 k-vectors; the latency of a small batch was this loop)
        for (int64_t q0 = tid; q0 < v.nk; q0 += (int64_t)R * MC_THREADS) {
            KChunk nxt;
            load_chunk(q0 + (int64_t)R * MC_THREADS, nxt);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t q = q0 + (int64_t)r * MC_THREADS;
                const int64_t qq = q < v.nk ? q : q0;
                const double2 S = (b == 0) ? cur.old[r] : molecule_sf(v, tab, stride, s_q, m, qq);
                const double rr = cur.f[r].x + (cur.t[r].x - cur.old[r].x), ri = cur.f[r].y + (cur.t[r].y - cur.old[r].y);      // rest = framework + (sums[:,1] - sums[:,ij+1])
                rs += cur.kf[r] * (rr * S.x + ri * S.y);
                ss += cur.kf[r] * (S.x * S.x + S.y * S.y);
            }
            cur = nxt;
        }
    }
    // ---- single_contribution_vdw (energy.jl:407-427)
    if (table_in_lds) __syncthreads();
    if (do_pairs) {
        const double* M = v.mat;
        const double* I = v.invmat;
        auto pairs_with = [&](const double4 A) __attribute__((always_inline)) {
            int kind1, mol;
            unpack(A.w, kind1, mol);
            if (mol < 0 || (!INSERT && mol == molecule)) return;            // :419 (and free slots)
            for (int a = 0; a < m; ++a) {
                double r2;
                {
#pragma clang fp contract(off)
                    const double dx = s_pos[3 * a] - A.x, dy = s_pos[3 * a + 1] - A.y, dz = s_pos[3 * a + 2] - A.z;
                    double f0 = I[0] * dx + I[3] * dy + I[6] * dz;
                    double f1 = I[1] * dx + I[4] * dy + I[7] * dz;
                    double f2 = I[2] * dx + I[5] * dy + I[8] * dz;
                    f0 = ((f0 + 0.5) - floor(f0 + 0.5)) - 0.5;
                    f1 = ((f1 + 0.5) - floor(f1 + 0.5)) - 0.5;
                    f2 = ((f2 + 0.5) - floor(f2 + 0.5)) - 0.5;
                    const double vx = M[0] * f0 + M[3] * f1 + M[6] * f2;
                    const double vy = M[1] * f0 + M[4] * f1 + M[7] * f2;
                    const double vz = M[2] * f0 + M[5] * f1 + M[8] * f2;
                    r2 = vx * vx + vy * vy + vz * vz;
                }
                if (!(r2 < v.cutoff2)) continue;                            // :422
                const int t = kind1 * v.nkinds + s_kind[a];
                if (FAST && r2 >= 0.25) {
                    double r, rinv;
                    ceg::fast_sqrt_rsqrt(r2, r, rinv);
                    for (int q = offset[t]; q < offset[t + 1]; ++q) inter += rule_energy_fast(rules[q], r2, r, rinv, v.coulombic);
                } else {
                    for (int q = offset[t]; q < offset[t + 1]; ++q) inter += rule_energy(rules[q], r2, v.coulombic);
                }
            }
        };
        if (!CELLS) {
            for (int l = tid; l < at.natoms(v); l += MC_THREADS) pairs_with(l == tid ? A_first : v.atoms[l]);
        } else {
            // only the cells the cutoff spheres of the molecule's atoms can reach (ceg_consumers.h)
            if (tid < 3) ceg_consumers::cell_range(I, s_pos, m, tid, v.nb[tid], v.hfrac[tid], s_bin0[tid], s_nbin[tid]);
            __syncthreads();
            const int n0 = s_nbin[0], n1 = s_nbin[1], n2 = s_nbin[2];
            const int ncell = n0 * n1 * n2;
            const int wave = tid >> 6, lane = tid & 63;
            for (int base = 0; base < ncell; base += MC_THREADS) {
                const int e = base + tid;
                int cnt = 0, cell = 0;
                if (e < ncell) {
                    const int j2 = e % n2, j1 = (e / n2) % n1, j0 = e / (n2 * n1);
                    int c0 = s_bin0[0] + j0, c1 = s_bin0[1] + j1, c2 = s_bin0[2] + j2;
                    if (c0 >= v.nb[0]) c0 -= v.nb[0];
                    if (c1 >= v.nb[1]) c1 -= v.nb[1];
                    if (c2 >= v.nb[2]) c2 -= v.nb[2];
                    cell = (c0 * v.nb[1] + c1) * v.nb[2] + c2;
                    cnt = v.cell_count[cell];
                }
                int incl = cnt;                                            // inclusive scan over the workgroup
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(incl, o);
                    if (lane >= o) incl += up;
                }
                if (lane == 63) s_wtot[wave] = incl;
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < MC_THREADS / 64; ++w) {
                    if (w < wave) before += s_wtot[w];
                    total += s_wtot[w];
                }
                s_first[tid] = before + incl - cnt;
                s_cell[tid] = cell;
                __syncthreads();
                for (int l = tid; l < total; l += MC_THREADS) {
                    int j = 0;                                             // last cell whose first entry is <= l
#pragma unroll
                    for (int step = MC_THREADS / 2; step > 0; step >>= 1)
                        if (s_first[j + step] <= l) j += step;
                    pairs_with(v.cells[(size_t)s_cell[j] * v.cell_cap + (l - s_first[j])]);
                }
                __syncthreads();
            }
        }
    }
    // ---- block reduction
    double vals[5] = {fv, fd, inter, rs, ss};
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vals[c] += __shfl_xor(vals[c], o);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0)
        for (int c = 0; c < 5; ++c) s_red[wave][c] = vals[c];
    __syncthreads();
    if (tid == 0) {
        double tot[5] = {0, 0, 0, 0, 0};
        for (int w = 0; w < MC_THREADS / 64; ++w)
            for (int c = 0; c < 5; ++c) tot[c] += s_red[w][c];
        double* o = at.row(out);
        if (do_frame) { o[0] = tot[0]; o[1] = tot[1]; }
        if (do_pairs) o[2] = tot[2];
        if (do_ewald) o[3] = 2.0 * tot[3] + tot[4];
        // small batches: the rows sit in mapped host memory and the host polls `flag` instead of going through
        // hipStreamSynchronize (whose wake-up costs about as much as this kernel); the last workgroup to finish raises it
        if (flag) {
            __threadfence_system();
            if (atomicAdd(done, 1u) == at.nblocks() - 1) {
                *done = 0u;
                __threadfence_system();
                __atomic_store_n(flag, seq, __ATOMIC_RELEASE);
            }
        }
    }
}

// the chains' views through the constant address space: the pointers in them are then known to address global memory (read through a
// generic pointer they became flat accesses, +16 VGPRs in k_mcg_accept); the array does not change while a kernel runs
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> __device__ __forceinline__ const __attribute__((address_space(4))) T* as_constant(const T* p) { return (const __attribute__((address_space(4))) T*)p; }
#else
template <class T> __device__ __forceinline__ const T* as_constant(const T* p) { return p; }
#endif

// update_mc! for a displacement (montecarlo.jl:615-628): positions; sums[:,1] += new - sums[:,ij+1]; sums[:,ij+1] = new
__device__ __forceinline__ void mc_accept_body(const McView& v, int32_t molecule, const McPositions& np, const McCellOps& ops, int stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_pos[MC_MAX_ATOMS * 3];
    __shared__ double s_q[MC_MAX_ATOMS];
    const int tid = threadIdx.x;
    const int first = v.mol[molecule].x, m = v.mol[molecule].y;
    if (tid < 3 * m) s_pos[tid] = np.xyz[tid];
    if (tid < m) {
        double4 A = v.atoms[first + tid];
        int kind, mol;
        unpack(A.w, kind, mol);
        s_q[tid] = v.kind_charge[kind];
        A.x = np.xyz[3 * tid]; A.y = np.xyz[3 * tid + 1]; A.z = np.xyz[3 * tid + 2];
        put_atom(v, first + tid, A);
    }
    __syncthreads();
    if (v.use_cells) apply_cell_ops(v, ops, tid);
    if (v.nk == 0) return;
    double2* tab = reinterpret_cast<double2*>(s_raw);
    fill_tables(v, s_pos, m, tab, stride, tid, MC_THREADS, s_q);
    __syncthreads();
    double2* mine = v.sf_mol + (size_t)molecule * v.nk;
    rows_structure_factor(v, tab, stride, m, tid >> 6, MC_THREADS / 64, tid & 63, [&](int q, double sr, double si) {
        const double2 old = mine[q];
        double2 t = v.sf_tot[q];
        t.x += sr - old.x;
        t.y += si - old.y;
        v.sf_tot[q] = t;
        mine[q] = make_double2(sr, si);
    });
}

// add_one_system! (ewald.jl:775-792, montecarlo.jl:615-621): new molecule `molecule` (= old nmol) in atom slots [first, first + m)
__device__ __forceinline__ void mc_insert_body(const McView& v, int32_t molecule, int32_t first, const McMolecule& nm, const McPositions& np, const McCellOps& ops, int stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_pos[MC_MAX_ATOMS * 3];
    __shared__ double s_q[MC_MAX_ATOMS];
    const int tid = threadIdx.x, m = nm.m;
    if (tid < 3 * m) s_pos[tid] = np.xyz[tid];
    if (tid < m) {
        const long long bits = ((long long)molecule << 32) | (long long)(uint32_t)nm.kinds[tid];
        put_atom(v, first + tid, make_double4(np.xyz[3 * tid], np.xyz[3 * tid + 1], np.xyz[3 * tid + 2], __longlong_as_double(bits)));
        s_q[tid] = v.kind_charge[nm.kinds[tid]];
    }
    if (tid == 0) v.mol[molecule] = make_int2(first, m);
    __syncthreads();
    if (v.use_cells) apply_cell_ops(v, ops, tid);
    if (v.nk == 0) return;
    double2* tab = reinterpret_cast<double2*>(s_raw);
    fill_tables(v, s_pos, m, tab, stride, tid, MC_THREADS, s_q);
    __syncthreads();
    double2* mine = v.sf_mol + (size_t)molecule * v.nk;
    rows_structure_factor(v, tab, stride, m, tid >> 6, MC_THREADS / 64, tid & 63, [&](int q, double sr, double si) {
        double2 t = v.sf_tot[q];
        t.x += sr;
        t.y += si;
        v.sf_tot[q] = t;
        mine[q] = make_double2(sr, si);
    });
}

// remove_one_system! (ewald.jl:794-810, :404-413): sums[:,1] -= sums[:,ij+1]; the LAST molecule takes index `molecule`
// (its structure factor column and the molecule id of its atoms); the atom slots of the removed molecule become free
__device__ __forceinline__ void mc_remove_body(const McView& v, int32_t molecule, int32_t last, const McCellOps& ops)
{
    const int tid = threadIdx.x;
    const int2 gone = v.mol[molecule], moved = v.mol[last];
    double2* mine = v.sf_mol + (size_t)molecule * v.nk;
    const double2* lastsf = v.sf_mol + (size_t)last * v.nk;
    for (int64_t q = tid; q < v.nk; q += MC_THREADS) {
        const double2 old = mine[q];
        double2 t = v.sf_tot[q];
        t.x -= old.x;
        t.y -= old.y;
        v.sf_tot[q] = t;
        if (last != molecule) mine[q] = lastsf[q];
    }
    if (tid < gone.y) {
        double4 A = v.atoms[gone.x + tid];
        int kind, mol;
        unpack(A.w, kind, mol);
        const long long bits = (long long)(0xffffffff00000000ull | (unsigned long long)(uint32_t)kind);      // molecule id -1: free slot
        A.w = __longlong_as_double(bits);
        put_atom(v, gone.x + tid, A);
    }
    if (last != molecule && tid >= 64 && tid < 64 + moved.y) {
        double4 A = v.atoms[moved.x + tid - 64];
        int kind, mol;
        unpack(A.w, kind, mol);
        const long long bits = ((long long)molecule << 32) | (long long)(uint32_t)kind;
        A.w = __longlong_as_double(bits);
        put_atom(v, moved.x + tid - 64, A);
    }
    __syncthreads();
    if (v.use_cells) apply_cell_ops(v, ops, tid);
    if (tid == 0 && last != molecule) v.mol[molecule] = moved;
}

// compute_ewald(::IncrementalEwaldContext) (ewald.jl:630-652), first half: sums[:, ij+1] of molecule `molecule` from its current
// positions (one workgroup of MC_THREADS; dynamic LDS: the [m][stride] tables)
__device__ __forceinline__ void mc_sf_molecule_body(const McView& v, int molecule, int stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_pos[MC_MAX_ATOMS * 3];
    __shared__ double s_q[MC_MAX_ATOMS];
    const int tid = threadIdx.x;
    const int first = v.mol[molecule].x, m = v.mol[molecule].y;
    if (tid < m) {
        const double4 A = v.atoms[first + tid];
        int kind, mol;
        unpack(A.w, kind, mol);
        s_q[tid] = v.kind_charge[kind];
        s_pos[3 * tid] = A.x; s_pos[3 * tid + 1] = A.y; s_pos[3 * tid + 2] = A.z;
    }
    __syncthreads();
    double2* tab = reinterpret_cast<double2*>(s_raw);
    fill_tables(v, s_pos, m, tab, stride, tid, MC_THREADS, s_q);
    __syncthreads();
    double2* mine = v.sf_mol + (size_t)molecule * v.nk;
    rows_structure_factor(v, tab, stride, m, tid >> 6, MC_THREADS / 64, tid & 63,
                          [&](int q, double sr, double si) { mine[q] = make_double2(sr, si); });
}

// second half: sums[q, 1] = sum over the molecules, in molecule order
__device__ __forceinline__ void mc_sf_total_body(const McView& v, int64_t q)
{
    if (q >= v.nk) return;
    double sr = 0.0, si = 0.0;
    for (int j = 0; j < v.nmol; ++j) {
        const double2 s = v.sf_mol[(size_t)j * v.nk + q];
        sr += s.x;
        si += s.y;
    }
    v.sf_tot[q] = make_double2(sr, si);
}

inline int merr(int code, const char* msg)
{
    ceg_set_last_error_(msg);
    return code;
}

struct Guard {
    int prev = -1;
    bool ok;
    explicit Guard(int device)
    {
        (void)hipGetDevice(&prev);
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~Guard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Host mirror of the cell lists (which atom slot sits where); the device holds the records themselves.  Every update is
// worked out here first and shipped to the device as a handful of "copy atom record `src` to cell entry `dst`" operations
// inside the update kernel's arguments, so the bookkeeping costs no extra launch, no upload and no device-side search.
struct CellMirror {
    bool on = false;
    int nb[3] = {1, 1, 1};
    int cap = 0;
    double invmat[9];
    ceg_consumers::CellBins bins{};
    std::vector<std::vector<int32_t>> members;          // [ncells] atom slots
    std::vector<int32_t> cell_of, idx_of;               // per atom slot; cell_of < 0: not in any cell
    std::vector<std::pair<int32_t, int32_t>> touched;   // (cell, entry) whose content changed
    std::vector<int32_t> touched_cells;
    int max_fill = 0;
    int min_cap = 0;                                    // rebuild_cells gives every cell at least this many entries (ceg_mc_group_set_device_cells)
    uint64_t version = 1;                               // bumped by every change of the lists or of the capacity (a sweep uploads the lists to the device when it moved)

    int ncells() const { return nb[0] * nb[1] * nb[2]; }
    int bin_of(const double* p) const { return ceg_consumers::cell_of_position(bins, invmat, p); }
    void begin() { touched.clear(); touched_cells.clear(); ++version; }
    void touch(int32_t c, int32_t i)
    {
        for (const auto& t : touched)
            if (t.first == c && t.second == i) return;
        touched.emplace_back(c, i);
    }
    void touch_cell(int32_t c)
    {
        if (std::find(touched_cells.begin(), touched_cells.end(), c) == touched_cells.end()) touched_cells.push_back(c);
    }
    void ensure_slot(int64_t slot)
    {
        if ((int64_t)cell_of.size() <= slot) { cell_of.resize((size_t)slot + 1, -1); idx_of.resize((size_t)slot + 1, -1); }
    }
    void take_out(int32_t slot)
    {
        const int32_t c = cell_of[slot], i = idx_of[slot];
        if (c < 0) return;
        std::vector<int32_t>& mem = members[c];
        const int32_t moved = mem.back();
        mem[i] = moved;
        idx_of[moved] = i;
        mem.pop_back();
        cell_of[slot] = -1; idx_of[slot] = -1;
        touch(c, i);
        touch_cell(c);
    }
    void put_in(int32_t slot, int32_t c)
    {
        ensure_slot(slot);
        std::vector<int32_t>& mem = members[c];
        mem.push_back(slot);
        cell_of[slot] = c; idx_of[slot] = (int32_t)mem.size() - 1;
        max_fill = std::max(max_fill, (int)mem.size());
        touch(c, idx_of[slot]);
        touch_cell(c);
    }
    void refresh(int32_t slot)
    {
        if (cell_of[slot] >= 0) touch(cell_of[slot], idx_of[slot]);
    }
    // false: an entry beyond the capacity is in use (or too many operations): the caller rebuilds the device arrays
    bool finish(McCellOps& ops) const
    {
        ops.nops = 0; ops.ncnt = 0;
        if (max_fill > cap) return false;
        for (const auto& t : touched) {
            const std::vector<int32_t>& mem = members[t.first];
            if (t.second >= (int32_t)mem.size()) continue;           // the entry fell off the end of its list
            if (ops.nops == MC_MAX_CELL_OPS) return false;
            ops.dst[ops.nops] = t.first * cap + t.second;
            ops.src[ops.nops] = mem[t.second];
            ++ops.nops;
        }
        for (int32_t c : touched_cells) {
            if (ops.ncnt == MC_MAX_CELL_OPS) return false;
            ops.cell[ops.ncnt] = c;
            ops.count[ops.ncnt] = (int32_t)members[c].size();
            ++ops.ncnt;
        }
        return true;
    }
};

// LDS bytes of the pair table of a view (rules, then offsets) where a trial kernel keeps it beside the k-space tables
inline size_t pair_table_bytes(const McView& v) { return sizeof(DevRule) * (size_t)(v.nrules > 0 ? v.nrules : 1) + sizeof(int32_t) * ((size_t)v.nkinds * v.nkinds + 1); }

}  // namespace ceg_mcs

struct ceg_mc_group;

struct ceg_mc {
    int device = 0;
    ceg_mcs::McView v{};
    hipStream_t stream = nullptr;
    // owned device arrays
    ceg_mcs::McGrid* d_vdw = nullptr;
    double* d_charge = nullptr;
    ceg::DevRule* d_rules = nullptr;
    int32_t* d_offset = nullptr;
    int32_t* d_ijk = nullptr;
    double* d_kf = nullptr;
    double2 *d_fw = nullptr, *d_tot = nullptr, *d_mol = nullptr;
    double4* d_atoms = nullptr;
    int2* d_molidx = nullptr;
    int64_t atoms_cap = 0, mol_cap = 0;
    std::vector<int2> h_mol;                     // host copy of (start, count) per molecule
    std::vector<std::vector<int32_t>> free_runs; // free_runs[m]: starts of free runs of m atom slots
    ceg_mcs::CellMirror cm;                      // neighbour cells of the guest atoms (when the MC cell is large enough to gain)
    double4* d_cells = nullptr;
    int32_t* d_cell_count = nullptr;
    // the device's copy of the cell lists (McCellBook of ceg_mc_sweep.h), authoritative only while a sweep of the handle's group runs
    int32_t *d_cell_of = nullptr, *d_idx_of = nullptr, *d_owner = nullptr;
    size_t book_slots = 0, book_entries = 0;     // allocated sizes: atom slots of d_cell_of / d_idx_of, entries of d_owner
    uint64_t book_version = 0;                   // CellMirror::version the device's copy agrees with (0: never uploaded)
    int stride = 0;
    // row-wise k-vector layout (ceg_rows.h) and, per distinct molecule (tuple of atom kinds), the pair-table rows of its kinds
    int32_t *d_desc = nullptr, *d_qof = nullptr;
    double* d_geom = nullptr;
    std::vector<ceg::DevRule> h_rules;
    std::vector<int32_t> h_offset;
    std::vector<int32_t> h_kind;                 // kind per atom slot (host copy)
    std::vector<double> h_charge;                // charge per kind (host copy)
    double* d_etab = nullptr;                    // erfc(alpha r)/r records of ceg_pairfrac.h (CoulombEwaldDirect rules sharing one alpha)
    int32_t ebase = 0, eni = 0;
    struct Compact { ceg::DevRule* d_rules = nullptr; int32_t* d_off = nullptr; void* d_fast = nullptr; int32_t nrules = 0; };
    std::map<std::vector<int32_t>, Compact> compact;
    // pinned, device-mapped staging for small batches; device scratch for large ones
    double *h_in = nullptr, *h_out = nullptr, *dm_in = nullptr, *dm_out = nullptr;
    double *d_in = nullptr, *d_out = nullptr;
    size_t d_in_cap = 0, d_out_cap = 0;
    // completion flag of the mapped-buffer path (polled by the host) and the device-side count of finished workgroups
    unsigned long long *h_flag = nullptr, *dm_flag = nullptr;
    unsigned* d_done = nullptr;
    unsigned long long seq = 0;
    // set when a state-changing call failed after it had started to change the host mirror (counts, slot lists, cell lists) or the
    // device state: host and device may then disagree, so every later call fails until ceg_mc_set_guests rebuilds both
    bool poisoned = false;
    bool guests_set = false;                     // ceg_mc_set_guests has succeeded at least once (what a chain group asks of its members)
    uint64_t v_version = 1;                      // bumped wherever `v` is written (a group re-uploads its copy of `v` when this moved)
    ceg_mc_group* group = nullptr;               // the chain group this handle belongs to (its work then runs on the group's stream)
    hipStream_t own_stream = nullptr;            // the handle's own stream while it is in a group
    unsigned char* d_baseline = nullptr;         // partial sums and result of ceg_mc_baseline (ceg_mc_baseline.hip); only grows
    size_t baseline_cap = 0;
};

namespace ceg_mcs {

inline size_t tables_bytes(const ceg_mc* h, int m) { return sizeof(double2) * (size_t)m * (size_t)h->stride; }      // LDS of the e^{2 pi i m f} tables of m atoms

// wait for the completion flag of a polled launch to reach `seq`; false after ~20 ms without it (a failed launch never raises the flag:
// the caller then synchronises the stream, which is what reports the error)
inline bool poll_flag(const unsigned long long* h_flag, unsigned long long seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        if (__atomic_load_n(h_flag, __ATOMIC_ACQUIRE) == seq) return true;
        if ((spin & 1023u) == 1023u && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 20.0) return false;
        __builtin_ia32_pause();
    }
}

// defined in ceg_mc.hip
int ensure_capacity(ceg_mc* h, int64_t natoms, int64_t nmol);       // grow the device arrays (contents kept); the stream is idle when this returns
int rebuild_cells(ceg_mc* h);                                       // the device cell arrays from the host lists; leaves the stream idle
bool accept_cell_ops(ceg_mc* h, int32_t molecule, const double* positions, McCellOps& ops);
int check_molecule(const ceg_mc* h, const int32_t* kinds, int32_t m, McMolecule* nm);

// defined in ceg_mc_sample.hip: the sampler of a group (ceg_mc_group_set_sampler).  The group owns it and frees it; a sweep asks it
// before its first launch whether its frames fit, and after the accept launch of a frame step enqueues the frame.
struct GroupSampler;
// where a frame finds what the views do not hold during a sweep, per chain c: counts + c * counts_stride = (molecules, high-water
// mark of the atom slots, molecules per species [ncount]) in device memory (nullptr: nmol / natoms of the views, no species);
// delta_moves / delta_swaps + c * stats_stride bytes: the running sums of the sweep's statistics (nullptr: 0);
// stop: the chain plan's [K] stops (nullptr: none) -- a frame after a step >= stop[c] writes chain c's record and bins nothing of it
struct SampleSource {
    const int32_t* counts;
    int32_t counts_stride, ncount;
    const double *delta_moves, *delta_swaps;
    int32_t stats_stride;
    int32_t max_slots;                           // no chain's high-water mark exceeds this while the frame runs
    const int64_t* stop;
    const int32_t* rung;                         // [K] tempering: chain c is binned into the map of rung[c]; nullptr: of c
};
void sampler_free(GroupSampler* s);
int sampler_admit(const GroupSampler* s, uint64_t first_step, int64_t nsteps);      // CEG_ERR_INVALID: the sweep's frames do not fit
bool sampler_frame_after(const GroupSampler* s, uint64_t step);
void sampler_enqueue(GroupSampler* s, hipStream_t stream, const McView* d_views, int k, int64_t step, const SampleSource& src);
int64_t sampler_frames_taken(const GroupSampler* s);
void sampler_rollback(GroupSampler* s, hipStream_t stream, int64_t frames);        // back to `frames` frames after a failed sweep

// defined in ceg_mc_cycles.hip: the cycle end of ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles (k_mcg_cycle_end).
// Where the launch finds, per chain c, what it reads and writes (all device memory): the four counters and the one or two sums of
// the call's statistics at + c * stats_stride bytes (delta_swaps nullptr: 0); the molecule count at nmol + c * nmol_stride bytes
// (nullptr: nmol of the views); the chain's (temperature, dmax, thetamax), three adjacent doubles, at triple + c * triple_stride bytes.
// stop: the chain plan's [K] stops (nullptr: none) and last_step, the absolute last step of the cycle: a chain with last_step >=
// stop[c] gets its record with the counters as they stand and its step sizes carried over.
struct CycleSource {
    const int64_t *translation_trials, *translation_accepted, *rotation_trials, *rotation_accepted;
    const double *delta_moves, *delta_swaps;
    const int32_t* nmol;
    double* triple;
    int32_t stats_stride, nmol_stride, triple_stride, _pad;
    const int64_t* stop;
    uint64_t last_step;
};
// the cycles of one call: what cycles_check has admitted, and the three segments of the group's block the launches use
struct CycleRun {
    int64_t ncycles, steps_per_cycle, cycle0;
    int32_t adapt;
    const int64_t* d_prior;                      // [K][4]
    const double* d_table;                       // [ncycles][K], or nullptr: no table
    ceg_mc_cycle_record_t* d_records;            // [ncycles][K]
};
// CEG_ERR_INVALID for every refusal of the header that the cycles themselves give; *nsteps = ncycles * steps_per_cycle
int cycles_check(const ceg_mc_cycles_t* cy, int k, uint64_t first_step, bool constant_columns, const void* cycles_out, int64_t* nsteps);
void cycles_enqueue(hipStream_t stream, const McView* d_views, int k, const CycleRun& run, int64_t j, const CycleSource& src);

// defined in ceg_mc_temper.hip: the tempering state of a group (ceg_mc_group_set_tempering) and the exchange launch (k_mcg_exchange)
// that the *_cycles sweeps enqueue behind cycles_enqueue.  The group owns the state and frees it.
struct GroupTempering;
// what the exchange launch needs beside the cycle end's own arguments: the chains' stream ids (stream_id + c * param_stride bytes),
// the seed of the call, and the [K] temperatures by rung of the NEXT cycle in device memory (the call's last cycle: of the ended one)
struct TemperSource {
    const uint32_t* stream_id;
    int32_t param_stride, _pad;
    uint64_t seed;
    const double* next_row;
};
void temper_free(GroupTempering* t);
// CEG_ERR_INVALID where a *_cycles call cannot run with the state: stale, too few record slots left, a row (of the table, else the
// ladder) that decreases, swaps.  ladder: params->temperature, [K] by rung (read where the cycles have no table)
int temper_admit(const GroupTempering* t, const ceg_mc_cycles_t* cy, const double* ladder, int k, bool swaps);
const int32_t* temper_rungs(const GroupTempering* t);                // [K] the host's copy
const int32_t* temper_device_rungs(const GroupTempering* t);         // [K] device memory
void temper_enqueue(GroupTempering* t, hipStream_t stream, int k, const CycleRun& run, int64_t j, const CycleSource& src, const TemperSource& ts);
bool temper_commit(GroupTempering* t, int64_t ncycles);              // a call has ended well (stream idle): its records count, the host's rungs follow
void temper_fail(GroupTempering* t);                                 // a call failed once enqueued: the state is stale

// defined in ceg_mc_record.hip: the recorder of a group (ceg_mc_group_set_recorder) and the snapshot launch (k_mcg_snapshot) that the
// *_cycles sweeps enqueue behind cycles_enqueue / temper_enqueue at the cycle ends the recorder wants.  The group owns it and frees it.
struct GroupRecorder;
// where the launch finds, per chain c, what the views do not hold during a sweep (all device memory): counts + c * counts_stride =
// (molecules, high-water mark of the atom slots) as SampleSource describes them (nullptr: nmol / natoms of the views); the running
// sums of the call's statistics at delta_* + c * stats_stride bytes (nullptr: 0); the species of the chain's molecule j at
// molspec[*(spec_off + c * spec_stride bytes) + j] (molspec nullptr: -1); stop and last_step as in CycleSource; energy: [K] the
// chains' energies at the call's start
struct RecordSource {
    const int32_t* counts;
    int32_t counts_stride, stats_stride;
    const double *delta_moves, *delta_swaps;
    const int32_t *molspec, *spec_off;
    int32_t spec_stride, _pad;
    const int64_t* stop;
    uint64_t last_step;
    const double* energy;
};
void recorder_free(GroupRecorder* r);
// CEG_ERR_INVALID where a *_cycles call cannot run with the recorder: stale, its due frames exceed the room left, track_min under swaps
int recorder_admit(const GroupRecorder* r, const ceg_mc_cycles_t* cy, int k, bool swaps);
bool recorder_wants(const GroupRecorder* r, int64_t cc);            // a launch at the end of cycle cc (a frame is due, or track_min)
void recorder_energies(const GroupRecorder* r, double* out);        // [K] the running energies (what a call stages as RecordSource::energy)
void recorder_enqueue(GroupRecorder* r, hipStream_t stream, const McView* d_views, int k, int64_t cc, const RecordSource& src);
void recorder_commit(GroupRecorder* r, const double* energy);       // a call has ended well: its frames count, [K] the energies after its last cycle
void recorder_fail(GroupRecorder* r, hipStream_t stream);           // a call failed once enqueued: none of its frames, the recorder is stale

// defined in ceg_mc_group.hip: what ceg_mc_baseline.hip and ceg_mc_sample.hip need of a group
struct GroupRef {
    int device;
    hipStream_t stream;
    ceg_mc* const* chains;
    int k;
    const McView* d_views;                       // [k], current in stream order once group_views_current has returned true
    unsigned char** d_baseline;                  // the group's counterpart of ceg_mc::d_baseline / baseline_cap
    size_t* baseline_cap;
    GroupSampler** sampler;                      // nullptr behind it: no sampler installed
    GroupTempering** tempering;                  // nullptr behind it: no tempering installed
    GroupRecorder** recorder;                    // nullptr behind it: no recorder installed
};
GroupRef group_ref(ceg_mc_group* g);
bool group_views_current(ceg_mc_group* g);       // every member's view into d_views where it changed since its last upload
void group_stream_idle(ceg_mc_group* g);         // the caller has synchronised the group's stream
int group_refuse_poisoned(int c);                // CEG_ERR_HIP, "chain <c> of the group is inconsistent ..."

}  // namespace ceg_mcs
