// ceg_egrid.hip -- energy_grid (src/grids.jl:346-424) of a CrystalEnergySetup for a rigid molecule in many orientations:
// every (rotation, lattice point) element of `allvals` in one device pass, positions generated in the kernels.
//
// Reciprocal term.  Every atom of the molecule sits at o + R p_a (o = lattice offset, R = rotation), so the structure factor of the
// molecule factorises:  S(k; o, R) = P_o(k) T_R(k),  P_o(k) = exp(2 pi i k.(invmat o)),  T_R(k) = sum_a q_a exp(2 pi i k.(invmat R p_a)).
// With |P_o| = 1, compute_ewald (src/ewald.jl:555-577) becomes
//     E = 2 (sum_k Re(W_o(k) T_R(k)) + energy_net_charges) + (sum_k kf_k |T_R(k)|^2 + static_contribution),
//     W_o(k) = kf_k conj(S_f(k)) P_o(k),
// i.e. nrot self terms and one real contraction (points x 2 nk) . (2 nk x nrot).  P_o is separable along the lattice,
// P_o = PA[iA] PB[iB] PC[iC]; the three tables ((numA + numB + numC) x nk complex, kf conj(S_f) folded into PC) are built once per
// call from the exactly reduced angle of every entry.
//
//   k_egrid_tables   the three phase tables
//   k_egrid_T        T_R(k) for every rotation (stored as (Re, -Im), [k][rotation]) and the nrot self terms
//   k_egrid_cross    the contraction: one workgroup per lattice row (iB, iC), one wave per 16 points along iA, up to 64 rotations;
//                    v_mfma_f64_16x16x4: A = W (16 points x 4 k-vectors, formed in registers from PA and the row's PB PC), B = T
//                    (4 k-vectors x 16 rotations, staged in LDS per chunk of 16 k-vectors and shared by the waves).  MFMA runs at the
//                    v_fma_f64 rate on this part (profiles/r03_mfma_coissue.txt); it is used because one lane then forms ONE W
//                    entry per 2 x (number of rotation tiles) matrix instructions and keeps 4 accumulators per tile, where a
//                    v_fma_f64 tile of the same shape would need every W entry in every lane or an LDS read per two FMAs.
//   k_egrid_terms    per element: blocking mask, grid interpolations (ceg_consumers::interp_point, unchanged), the sum
//   k_egrid_reduce   ceg_energy_grid_reduced only: the rotation axis of a finished slab collapsed per lattice point -- minimum, first
//                    orientation that attains it, meanBoltzmann (src/utils.jl:415-443) at up to 8 temperatures
//
// Every element's arithmetic is independent of how the lattice is cut into launches, and so is the order in which k_egrid_reduce
// combines the elements of a point, so slabbed host output, single-slab output and device output are bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ceg_hip.h"
#include "ceg_consumers.h"
#include "ceg_math.h"

extern "C" void ceg_set_last_error_(const char* msg);

namespace {

using ceg_consumers::InterpGeom;
using ceg_consumers::interp_point;

constexpr int MAX_ATOMS = 16;
constexpr int KC = 16;              // k-vectors per LDS chunk of k_egrid_cross (4 MFMA steps)
constexpr int MAX_TILES = 4;        // rotation tiles (of 16) per launch of k_egrid_cross
constexpr int MAX_WAVES = 8;        // waves (tiles of 16 points along iA) per workgroup of k_egrid_cross

typedef double double4_t __attribute__((ext_vector_type(4)));

// what the kernels need of the call, in device memory (too large for kernel arguments: 17 grid geometries)
struct EgridParams {
    InterpGeom vdw_geom[MAX_ATOMS];
    const float* vdw_grid[MAX_ATOMS];      // nullptr: zero grid
    InterpGeom coulomb_geom;
    const float* coulomb_grid;             // nullptr: no Coulomb terms
    double base[MAX_ATOMS][3];
    double q[MAX_ATOMS];
    double steps[9];
    double recip_invmat[9];
    // BlockFile
    double block_mat[9], block_invmat[9], block_size[3], block_shift[3];
    int32_t block_dims[3];
    int32_t has_block;
    int32_t natoms, nrot, has_recip_sum, _pad;
    int32_t num[3];
    int32_t _pad2;
    double energy_net_charges, static_contribution;
};

// i * d mod 1 with the product formed exactly (i a small integer, d = k . g)
__device__ __forceinline__ double frac_of_product(double i, double d)
{
    const double hi = i * d;
    const double lo = __builtin_fma(i, d, -hi);
    return (hi - rint(hi)) + lo;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    return make_double2(__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x));
}

// tab [(numA + numB + numC)][nkp] complex: rows 0 .. numA-1 = PA, then PB, then PC * kf conj(S_f).  g [3][3]: invmat * step of each axis.
// k-vectors beyond nk (padding to a multiple of KC) keep the zeros the buffer was cleared to.
__global__ __launch_bounds__(256) void k_egrid_tables(const int32_t* __restrict__ ijk, const double* __restrict__ kf, const double* __restrict__ sf_re,
                                                       const double* __restrict__ sf_im, int nk, int nkp, int numA, int numB, int numC,
                                                       const double* __restrict__ g, double2* __restrict__ tab)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)(numA + numB + numC) * nk;
    if (t >= total) return;
    const int row = (int)(t / nk), k = (int)(t % nk);
    const int axis = row < numA ? 0 : (row < numA + numB ? 1 : 2);
    const int i = axis == 0 ? row : (axis == 1 ? row - numA : row - numA - numB);
    const double* ga = g + 3 * axis;
    const double d = __builtin_fma((double)ijk[3 * k + 2], ga[2], __builtin_fma((double)ijk[3 * k + 1], ga[1], (double)ijk[3 * k] * ga[0]));
    double sn, cs;
    ceg::sincos_2pi(frac_of_product((double)i, d), sn, cs);
    double2 p = make_double2(cs, sn);
    if (axis == 2) p = cmul(p, make_double2(kf[k] * sf_re[k], -(kf[k] * sf_im[k])));
    tab[(size_t)row * nkp + k] = p;
}

// One workgroup per rotation.  Tt [nkp][nrot_pad] = (Re T_R(k), -Im T_R(k)); self [nrot] = sum_k kf |T_R(k)|^2.
__global__ __launch_bounds__(256) void k_egrid_T(const EgridParams* __restrict__ P, const double* __restrict__ rot, const int32_t* __restrict__ ijk,
                                                  const double* __restrict__ kf, int nk, int nrot_pad, double2* __restrict__ Tt,
                                                  double* __restrict__ self)
{
    __shared__ double s_f[MAX_ATOMS][3];
    __shared__ double s_sum[256];
    const int r = blockIdx.x;
    const int natoms = P->natoms;
    if ((int)threadIdx.x < natoms) {
        const int a = threadIdx.x;
        const double* R = rot + 9 * (size_t)r;
        const double* I = P->recip_invmat;
        double x, y, z;
        {
#pragma clang fp contract(off)
            const double bx = P->base[a][0], by = P->base[a][1], bz = P->base[a][2];
            x = (R[0] * bx + R[3] * by) + R[6] * bz;
            y = (R[1] * bx + R[4] * by) + R[7] * bz;
            z = (R[2] * bx + R[5] * by) + R[8] * bz;
        }
        for (int c = 0; c < 3; ++c) {
            const double f = I[c] * x + I[c + 3] * y + I[c + 6] * z;
            s_f[a][c] = f - rint(f);
        }
    }
    __syncthreads();
    double part = 0.0;
    for (int k = threadIdx.x; k < nk; k += 256) {
        const double m0 = (double)ijk[3 * k], m1 = (double)ijk[3 * k + 1], m2 = (double)ijk[3 * k + 2];
        double tre = 0.0, tim = 0.0;
        for (int a = 0; a < natoms; ++a) {
            double s0, c0, s1, c1, s2, c2;
            ceg::sincos_2pi(frac_of_product(m0, s_f[a][0]), s0, c0);
            ceg::sincos_2pi(frac_of_product(m1, s_f[a][1]), s1, c1);
            ceg::sincos_2pi(frac_of_product(m2, s_f[a][2]), s2, c2);
            const double2 e = cmul(cmul(make_double2(c0, s0), make_double2(c1, s1)), make_double2(c2, s2));
            tre = __builtin_fma(P->q[a], e.x, tre);
            tim = __builtin_fma(P->q[a], e.y, tim);
        }
        Tt[(size_t)k * nrot_pad + r] = make_double2(tre, -tim);
        part += kf[k] * (tre * tre + tim * tim);
    }
    s_sum[threadIdx.x] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) self[r] = s_sum[0];
}

// out[rot + nrot (iA + numA row)] = sum_k Re(W T) for rot in [r0, r0 + 16 NT), row = blockIdx.x = iB + numB (iC - c0); wave w of the
// workgroup owns the points iA = 16 (blockIdx.y MAX_WAVES + w) .. + 15.
// MFMA operand maps (v_mfma_f64_16x16x4): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D register v: row i = (lane >> 4) + 4 v, column j = lane & 15.
template <int NT>
__global__ __launch_bounds__(64 * MAX_WAVES) void k_egrid_cross(const double2* __restrict__ tab, const double2* __restrict__ Tt, int nkp, int nrot, int nrot_pad,
                                                                 int r0, int numA, int numB, int numC, int c0, double* __restrict__ out)
{
    __shared__ double2 s_T[KC][NT * 16];
    __shared__ double2 s_Q[KC];
    const int nthreads = blockDim.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x;
    const int iB = row % numB, iC = c0 + row / numB;
    const int li = lane & 15, lk = lane >> 4;
    const int iA0 = 16 * (blockIdx.y * MAX_WAVES + wave);
    const int iA_load = min(iA0 + li, numA - 1);                 // lanes beyond the row compute a copy of its last point and store nothing
    const double2* PA = tab + (size_t)iA_load * nkp;
    const double2* PB = tab + (size_t)(numA + iB) * nkp;
    const double2* PC = tab + (size_t)(numA + numB + iC) * nkp;
    double4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < nkp; kc += KC) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < KC * NT * 16; idx += nthreads) {
            const int kk = idx / (NT * 16), j = idx % (NT * 16);
            s_T[kk][j] = Tt[(size_t)(kc + kk) * nrot_pad + r0 + j];
        }
        if (threadIdx.x < KC) s_Q[threadIdx.x] = cmul(PB[kc + threadIdx.x], PC[kc + threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KC / 4; ++s) {
            const int kl = 4 * s + lk;
            const double2 w = cmul(PA[kc + kl], s_Q[kl]);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double2 b = s_T[kl][16 * t + li];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.x, b.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.y, b.y, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int r = r0 + 16 * t + li;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int iA = iA0 + lk + 4 * v;
            if (iA < numA && r < nrot) out[(size_t)r + (size_t)nrot * ((size_t)iA + (size_t)numA * row)] = acc[t][v];
        }
    }
}

// BlockFile getindex (src/coordinates.jl:83-101): offsetpoint, round to nearest even, mask [nx][ny][nz]
__device__ __forceinline__ bool blocked_at(const EgridParams* __restrict__ P, const uint8_t* __restrict__ mask, double px, double py, double pz)
{
#pragma clang fp contract(off)
    const double* I = P->block_invmat;
    const double* M = P->block_mat;
    double a0 = (I[0] * px + I[3] * py) + I[6] * pz;
    double a1 = (I[1] * px + I[4] * py) + I[7] * pz;
    double a2 = (I[2] * px + I[5] * py) + I[8] * pz;
    a0 -= floor(a0); a1 -= floor(a1); a2 -= floor(a2);
    const double q[3] = {(M[0] * a0 + M[3] * a1) + M[6] * a2, (M[1] * a0 + M[4] * a1) + M[7] * a2, (M[2] * a0 + M[5] * a1) + M[8] * a2};
    int idx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double sh = (q[c] - P->block_shift[c]) * (double)P->block_dims[c] / P->block_size[c] + 1.0;
        const int i = (int)rint(sh) - 1;
        idx[c] = i < 0 ? 0 : (i > P->block_dims[c] ? P->block_dims[c] : i);           // memory safety only
    }
    const size_t ny = (size_t)P->block_dims[1] + 1, nz = (size_t)P->block_dims[2] + 1;
    return mask[((size_t)idx[0] * ny + idx[1]) * nz + idx[2]] != 0;
}

// one thread per element (rotation fastest, then iA, iB, iC: the order of `out`)
__global__ __launch_bounds__(256) void k_egrid_terms(const EgridParams* __restrict__ P, const double* __restrict__ rot, const double* __restrict__ self,
                                                      const uint8_t* __restrict__ mask, int c0, int64_t nelem, double* __restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nelem) return;
    const int nrot = P->nrot, natoms = P->natoms;
    const int r = (int)(e % nrot);
    int64_t p = e / nrot;
    const int iA = (int)(p % P->num[0]);
    p /= P->num[0];
    const int iB = (int)(p % P->num[1]);
    const int iC = c0 + (int)(p / P->num[1]);
    const double* R = rot + 9 * (size_t)r;
    const double* S = P->steps;
    double vdw = 0.0, direct = 0.0;
    bool blocked = false;
    for (int a = 0; a < natoms; ++a) {
        double x, y, z;
        {
#pragma clang fp contract(off)
            // rotpos = r * p (grids.jl:389); thisofs = (iA-1)*stepA + (iB-1)*stepB + (iC-1)*stepC (:396); ofs + pos (:409)
            const double bx = P->base[a][0], by = P->base[a][1], bz = P->base[a][2];
            const double rx = (R[0] * bx + R[3] * by) + R[6] * bz;
            const double ry = (R[1] * bx + R[4] * by) + R[7] * bz;
            const double rz = (R[2] * bx + R[5] * by) + R[8] * bz;
            const double ox = ((double)iA * S[0] + (double)iB * S[3]) + (double)iC * S[6];
            const double oy = ((double)iA * S[1] + (double)iB * S[4]) + (double)iC * S[7];
            const double oz = ((double)iA * S[2] + (double)iB * S[5]) + (double)iC * S[8];
            x = ox + rx; y = oy + ry; z = oz + rz;
        }
        if (P->has_block && blocked_at(P, mask, x, y, z)) { blocked = true; break; }
        const double v = P->vdw_grid[a] ? interp_point(P->vdw_geom[a], P->vdw_grid[a], x, y, z) : 0.0;
        vdw = a == 0 ? v : vdw + v;
        if (P->coulomb_grid) {
            const double c = P->q[a] * interp_point(P->coulomb_geom, P->coulomb_grid, x, y, z);
            direct = a == 0 ? c : direct + c;
        }
    }
    double val;
    if (blocked) val = 1e100;                                     // (1e100, 0) (grids.jl:313)
    else if (!P->coulomb_grid) val = vdw;                         // (vdw, 0)   (grids.jl:317)
    else {
        const double cross = P->has_recip_sum ? out[e] : 0.0;
        const double reciprocal = 2.0 * (cross + P->energy_net_charges) + (self[r] + P->static_contribution);
        val = vdw + (direct + reciprocal);
    }
    out[e] = val;
}

constexpr int RED_LANES = 16;       // lanes per lattice point of k_egrid_reduce (4 points per wave)

struct ReduceTemps {
    double T[CEG_EGRID_MAX_TEMPS];
};

// (value, index) of the smaller of two candidates with Julia's findmin order: a NaN beats every number, ties go to the lower index
__device__ __forceinline__ void min_step(double& v, int& i, double ov, int oi)
{
    const bool vn = v != v, on = ov != ov;
    const bool take = vn == on ? ((vn || ov == v) ? oi < i : ov < v) : on;
    if (take) { v = ov; i = oi; }
}

// The rotation axis of a slab [point][rotation] collapsed: RED_LANES consecutive lanes own one point and read its nrot consecutive
// doubles coalesced, lane l the rotations l, l + 16, ...  Pass 1: minimum and its first index.  Pass 2 (the point's elements come
// from cache): per temperature t  m = min - 30 T_t,  f_k = exp((m - x_k)/T_t) w_k  as meanBoltzmann forms them (utils.jl:433-436),
// and its mean sum(f_k x_k) / sum(f_k) taken about the minimum,  min + sum(f_k (x_k - min)) / sum(f_k):  the same number, but every
// term of the numerator is >= 0 (no cancellation between energies of either sign), one orientation or equal elements give the
// element itself, bit for bit, and the error scales with the spread of the energies, not their size.  Both sums are taken per
// lane in rising k and then across the 16 lanes by a butterfly whose every step adds the same two numbers in all lanes: the order
// depends on nrot alone.
// mean [NT][mean_stride], mn, amin: outputs of the launch's first point (mn / amin may be nullptr).
template <int NT>
__global__ __launch_bounds__(256) void k_egrid_reduce(const double* __restrict__ slab, int nrot, int64_t npoints, ReduceTemps temps,
                                                       const double* __restrict__ weights, double* __restrict__ mean, int64_t mean_stride,
                                                       double* __restrict__ mn, int32_t* __restrict__ amin)
{
#pragma clang fp contract(off)
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / RED_LANES;
    if (p >= npoints) return;                                     // all 16 lanes of a point leave together
    const int l = threadIdx.x % RED_LANES;
    const double* x = slab + (size_t)p * nrot;
    double vmin = 0.0;
    int imin = 0x7fffffff;                                        // a lane without elements (nrot < 16): loses every comparison
    bool have = false;
    for (int k = l; k < nrot; k += RED_LANES) {
        const double v = x[k];
        if (!have) { vmin = v; imin = k; have = true; }
        else min_step(vmin, imin, v, k);
    }
    if (!have) vmin = __builtin_huge_val();
#pragma unroll
    for (int o = RED_LANES / 2; o > 0; o >>= 1) {
        const double ov = __shfl_xor(vmin, o, RED_LANES);
        const int oi = __shfl_xor(imin, o, RED_LANES);
        min_step(vmin, imin, ov, oi);
    }
    if (l == 0) {
        if (mn) mn[p] = vmin;
        if (amin) amin[p] = imin;
    }
    if (NT == 0) return;
    double m[NT > 0 ? NT : 1], factors[NT > 0 ? NT : 1], total[NT > 0 ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        m[t] = vmin - 30.0 * temps.T[t];
        factors[t] = 0.0;
        total[t] = 0.0;
    }
    for (int k = l; k < nrot; k += RED_LANES) {
        const double v = x[k];
        const double w = weights ? weights[k] : 1.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double factor = exp((m[t] - v) / temps.T[t]) * w;
            factors[t] += factor;
            total[t] += factor * (v - vmin);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int o = RED_LANES / 2; o > 0; o >>= 1) {
            factors[t] += __shfl_xor(factors[t], o, RED_LANES);
            total[t] += __shfl_xor(total[t], o, RED_LANES);
        }
        if (l == 0) mean[(size_t)t * mean_stride + p] = vmin + total[t] / factors[t];
    }
}

int eerr(int code, const char* msg)
{
    ceg_set_last_error_(msg);
    return code;
}

struct Workspace {
    unsigned char* d = nullptr;
    hipStream_t stream = nullptr;
    bool async = false;
    ~Workspace()
    {
        if (!d) return;
        if (async) (void)hipFreeAsync(d, stream);
        else (void)hipFree(d);
    }
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// what ceg_energy_grid_reduced asks for on top of the elements (checked by the entry point)
struct Reduction {
    const double* temperatures;
    int32_t ntemps;
    const double* weights;
    double* out_mean;
    double* out_min;
    int32_t* out_argmin;
};

// Both entry points: the elements slab by slab into `out` (red == nullptr), or into a slab of the workspace that k_egrid_reduce
// collapses into the outputs of `red`.
int egrid_run(ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid, ceg_recip_t* recip, const double* base, const double* charges,
              int32_t natoms, const double* rotations, int32_t nrot, const double steps[9], const int32_t num[3], const uint8_t* block,
              const int32_t block_dims[3], const double block_size[3], const double block_shift[3], const double block_mat[9],
              const double block_invmat[9], double energy_net_charges, double static_contribution, double* out, const Reduction* red,
              int32_t out_on_device, void* stream)
{
    if (!vdw_grids || !base || !charges || !rotations || !steps || !num) return eerr(CEG_ERR_INVALID, "NULL argument");
    if (natoms < 1) return eerr(CEG_ERR_INVALID, "natoms < 1");
    if (natoms > MAX_ATOMS) return eerr(CEG_ERR_UNSUPPORTED, "molecule has more atoms than the kernels hold (16)");
    if (nrot < 1) return eerr(CEG_ERR_INVALID, "nrot < 1");
    for (int a = 0; a < 3; ++a)
        if (num[a] < 1) return eerr(CEG_ERR_INVALID, "num < 1");
    if ((recip == nullptr) != (coulomb_grid == nullptr))
        return eerr(CEG_ERR_INVALID, "recip and coulomb_grid must both be given or both be NULL");
    if (block) {
        if (!block_dims || !block_size || !block_shift || !block_mat || !block_invmat) return eerr(CEG_ERR_INVALID, "block mask without its csetup");
        for (int a = 0; a < 3; ++a)
            if (block_dims[a] < 1 || !(block_size[a] > 0.0)) return eerr(CEG_ERR_INVALID, "bad block csetup");
    }
    const int64_t points = (int64_t)num[0] * num[1] * num[2];
    if (points > (int64_t)1 << 40 || (int64_t)num[0] * num[1] > 0x7fffffffLL / 64) return eerr(CEG_ERR_INVALID, "lattice too large");
    if (ceg_device_count() <= 0) return eerr(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");

    // one device for every handle
    int device = -1;
    auto same_device = [&](int d) {
        if (device < 0) device = d;
        return device == d;
    };
    bool one = true;
    for (int a = 0; a < natoms; ++a)
        if (vdw_grids[a]) one = one && same_device(vdw_grids[a]->device);
    if (coulomb_grid) one = one && same_device(coulomb_grid->device) && same_device(recip->device);
    if (!one) return eerr(CEG_ERR_INVALID, "the grid and k-space handles live on different devices");
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (device < 0) device = prev < 0 ? 0 : prev;
    if (hipSetDevice(device) != hipSuccess) return eerr(CEG_ERR_HIP, "hipSetDevice failed");
    struct Restore {
        int prev;
        ~Restore() { if (prev >= 0) (void)hipSetDevice(prev); }
    } restore{prev};

    const int numA = num[0], numB = num[1], numC = num[2];
    const int64_t nk = recip ? recip->nk : 0;
    const int nkp = (int)((nk + KC - 1) / KC * KC);
    const int nrot_pad = (nrot + 15) / 16 * 16;
    const int ntab = numA + numB + numC;

    // ---- the call's constants, packed on the host and uploaded in one copy
    const size_t o_params = 0;
    const size_t o_rot = align256(o_params + sizeof(EgridParams));
    const size_t o_ijk = align256(o_rot + sizeof(double) * 9 * (size_t)nrot);
    const size_t o_kf = align256(o_ijk + sizeof(int32_t) * 3 * (size_t)nk);
    const size_t o_re = align256(o_kf + sizeof(double) * (size_t)nk);
    const size_t o_im = align256(o_re + sizeof(double) * (size_t)nk);
    const size_t o_g = align256(o_im + sizeof(double) * (size_t)nk);
    const size_t o_w = align256(o_g + sizeof(double) * 9);
    const size_t o_mask = align256(o_w + (red && red->weights ? sizeof(double) * (size_t)nrot : 0));
    const size_t mask_bytes = block ? (size_t)(block_dims[0] + 1) * (block_dims[1] + 1) * (block_dims[2] + 1) : 0;
    const size_t host_bytes = align256(o_mask + mask_bytes);
    // device-only part, cleared to zero (the padding of the tables must be zero)
    const size_t o_self = host_bytes;
    const size_t o_T = align256(o_self + sizeof(double) * (size_t)nrot);
    const size_t o_tab = align256(o_T + sizeof(double2) * (size_t)nkp * nrot_pad);
    const size_t total_bytes = align256(o_tab + sizeof(double2) * (size_t)ntab * nkp);

    std::vector<unsigned char> hbuf(o_mask, 0);
    EgridParams& P = *reinterpret_cast<EgridParams*>(hbuf.data() + o_params);
    for (int a = 0; a < natoms; ++a) {
        if (vdw_grids[a]) {
            P.vdw_geom[a] = vdw_grids[a]->g;
            P.vdw_grid[a] = vdw_grids[a]->d_grid;
        }
        for (int c = 0; c < 3; ++c) P.base[a][c] = base[3 * a + c];
        P.q[a] = charges[a];
    }
    if (coulomb_grid) {
        P.coulomb_geom = coulomb_grid->g;
        P.coulomb_grid = coulomb_grid->d_grid;
        for (int c = 0; c < 9; ++c) P.recip_invmat[c] = recip->invmat[c];
    }
    for (int c = 0; c < 9; ++c) P.steps[c] = steps[c];
    if (block) {
        for (int c = 0; c < 9; ++c) { P.block_mat[c] = block_mat[c]; P.block_invmat[c] = block_invmat[c]; }
        for (int c = 0; c < 3; ++c) { P.block_size[c] = block_size[c]; P.block_shift[c] = block_shift[c]; P.block_dims[c] = block_dims[c]; }
        P.has_block = 1;
    }
    P.natoms = natoms;
    P.nrot = nrot;
    P.has_recip_sum = nk > 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c) P.num[c] = num[c];
    P.energy_net_charges = energy_net_charges;
    P.static_contribution = static_contribution;
    std::memcpy(hbuf.data() + o_rot, rotations, sizeof(double) * 9 * (size_t)nrot);
    if (nk > 0) {
        std::memcpy(hbuf.data() + o_ijk, recip->h_ijk.data(), sizeof(int32_t) * 3 * (size_t)nk);
        std::memcpy(hbuf.data() + o_kf, recip->h_kf.data(), sizeof(double) * (size_t)nk);
        std::memcpy(hbuf.data() + o_re, recip->h_sf_re.data(), sizeof(double) * (size_t)nk);
        std::memcpy(hbuf.data() + o_im, recip->h_sf_im.data(), sizeof(double) * (size_t)nk);
        // g[axis] = invmat * step of the axis: the phase of lattice point (iA, iB, iC) is iA k.g[0] + iB k.g[1] + iC k.g[2]
        double* g = reinterpret_cast<double*>(hbuf.data() + o_g);
        const double* I = recip->invmat;
        for (int ax = 0; ax < 3; ++ax)
            for (int c = 0; c < 3; ++c) g[3 * ax + c] = I[c] * steps[3 * ax] + I[c + 3] * steps[3 * ax + 1] + I[c + 6] * steps[3 * ax + 2];
    }
    if (red && red->weights) std::memcpy(hbuf.data() + o_w, red->weights, sizeof(double) * (size_t)nrot);

    // ---- slabs of iC: host output travels in them, and a reduction never holds more elements than one of them
    const size_t per_c = sizeof(double) * (size_t)nrot * numA * numB;
    int slab_c = numC;
    if (!out_on_device || red) {
        size_t cap = (size_t)256 << 20;
        if (const char* e = getenv("CEG_HIP_EGRID_SLAB_BYTES")) { const long long v = atoll(e); if (v > 0) cap = (size_t)v; }
        slab_c = (int)std::max<size_t>(1, std::min<size_t>((size_t)numC, cap / per_c));
    }

    hipStream_t st = out_on_device ? (hipStream_t)stream : nullptr;
    Workspace ws;
    ws.stream = st;
    ws.async = out_on_device != 0;
    // behind the tables: the slab of elements (unless they go straight to a device `out`), then the slab's reduced outputs for the host
    const int ntemps = red ? red->ntemps : 0;
    const size_t slab_points = (size_t)numA * numB * slab_c;
    const size_t o_slab = total_bytes;
    const size_t o_rmean = o_slab + (out_on_device && !red ? 0 : align256(per_c * (size_t)slab_c));
    const size_t o_rmin = o_rmean + (red && !out_on_device ? align256(sizeof(double) * slab_points * ntemps) : 0);
    const size_t o_ramin = o_rmin + (red && !out_on_device && red->out_min ? align256(sizeof(double) * slab_points) : 0);
    const size_t out_bytes = o_ramin + (red && !out_on_device && red->out_argmin ? align256(sizeof(int32_t) * slab_points) : 0) - total_bytes;
    if ((ws.async ? hipMallocAsync((void**)&ws.d, total_bytes + out_bytes, st) : hipMalloc((void**)&ws.d, total_bytes + out_bytes)) != hipSuccess) {
        ws.d = nullptr;
        return eerr(CEG_ERR_HIP, "could not allocate the device workspace");
    }
    unsigned char* d = ws.d;
    // pageable source: the runtime has taken its copy of hbuf / block when these calls return
    if (hipMemcpyAsync(d, hbuf.data(), o_mask, hipMemcpyHostToDevice, st) != hipSuccess ||
        (block && hipMemcpyAsync(d + o_mask, block, mask_bytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemsetAsync(d + o_self, 0, total_bytes - o_self, st) != hipSuccess)
        return eerr(CEG_ERR_HIP, "could not upload the call's constants");
    const EgridParams* dP = reinterpret_cast<const EgridParams*>(d + o_params);
    const double* d_rot = reinterpret_cast<const double*>(d + o_rot);
    const int32_t* d_ijk = reinterpret_cast<const int32_t*>(d + o_ijk);
    const double* d_kf = reinterpret_cast<const double*>(d + o_kf);
    const double* d_re = reinterpret_cast<const double*>(d + o_re);
    const double* d_im = reinterpret_cast<const double*>(d + o_im);
    const double* d_g = reinterpret_cast<const double*>(d + o_g);
    const uint8_t* d_mask = d + o_mask;
    double* d_self = reinterpret_cast<double*>(d + o_self);
    double2* d_T = reinterpret_cast<double2*>(d + o_T);
    double2* d_tab = reinterpret_cast<double2*>(d + o_tab);
    const double* d_w = red && red->weights ? reinterpret_cast<const double*>(d + o_w) : nullptr;
    double* d_slab = out_on_device && !red ? out : reinterpret_cast<double*>(d + o_slab);
    ReduceTemps temps{};
    for (int t = 0; t < ntemps; ++t) temps.T[t] = red->temperatures[t];

    if (nk > 0) {
        const int64_t nt = (int64_t)ntab * nk;
        hipLaunchKernelGGL(k_egrid_tables, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, d_ijk, d_kf, d_re, d_im, (int)nk, nkp, numA, numB, numC,
                           d_g, d_tab);
        hipLaunchKernelGGL(k_egrid_T, dim3((unsigned)nrot), dim3(256), 0, st, dP, d_rot, d_ijk, d_kf, (int)nk, nrot_pad, d_T, d_self);
        if (hipGetLastError() != hipSuccess) return eerr(CEG_ERR_HIP, "table kernel launch failed");
    }
    const int tilesA = (numA + 15) / 16;
    const int waves = std::min(MAX_WAVES, tilesA);
    for (int c0 = 0; c0 < numC; c0 += slab_c) {
        const int nc = std::min(slab_c, numC - c0);
        const int64_t nelem = (int64_t)nrot * numA * numB * nc;
        if (nk > 0) {
            const dim3 grid((unsigned)(numB * nc), (unsigned)((tilesA + MAX_WAVES - 1) / MAX_WAVES));
            for (int r0 = 0; r0 < nrot; r0 += 16 * MAX_TILES) {
                const int nt = std::min(MAX_TILES, (nrot - r0 + 15) / 16);
                auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, grid, dim3(64 * waves), 0, st, d_tab, d_T, nkp, (int)nrot, nrot_pad, r0, numA, numB, numC, c0, d_slab);
                };
                if (nt == 4) launch(k_egrid_cross<4>);
                else if (nt == 3) launch(k_egrid_cross<3>);
                else if (nt == 2) launch(k_egrid_cross<2>);
                else launch(k_egrid_cross<1>);
            }
        }
        hipLaunchKernelGGL(k_egrid_terms, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, st, dP, d_rot, d_self, d_mask, c0, nelem, d_slab);
        if (hipGetLastError() != hipSuccess) return eerr(CEG_ERR_HIP, "energy-grid kernel launch failed");
        if (!red) {
            if (!out_on_device &&
                hipMemcpy(out + (size_t)nrot * numA * numB * c0, d_slab, sizeof(double) * (size_t)nelem, hipMemcpyDeviceToHost) != hipSuccess)
                return eerr(CEG_ERR_HIP, "kernel execution or D2H failed");
            continue;
        }
        // the slab's points p0 .. p0 + np of the lattice: straight into device outputs, or into the workspace and from there to the host
        const int64_t p0 = (int64_t)numA * numB * c0, np = (int64_t)numA * numB * nc, points = (int64_t)numA * numB * numC;
        double* r_mean = !ntemps ? nullptr : (out_on_device ? red->out_mean + p0 : reinterpret_cast<double*>(d + o_rmean));
        double* r_min = !red->out_min ? nullptr : (out_on_device ? red->out_min + p0 : reinterpret_cast<double*>(d + o_rmin));
        int32_t* r_amin = !red->out_argmin ? nullptr : (out_on_device ? red->out_argmin + p0 : reinterpret_cast<int32_t*>(d + o_ramin));
        const int64_t mean_stride = out_on_device ? points : (int64_t)slab_points;
        auto reduce = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((np * RED_LANES + 255) / 256)), dim3(256), 0, st, d_slab, (int)nrot, np, temps, d_w, r_mean,
                               mean_stride, r_min, r_amin);
        };
        switch (ntemps) {
        case 0: reduce(k_egrid_reduce<0>); break;
        case 1: reduce(k_egrid_reduce<1>); break;
        case 2: reduce(k_egrid_reduce<2>); break;
        case 3: reduce(k_egrid_reduce<3>); break;
        case 4: reduce(k_egrid_reduce<4>); break;
        case 5: reduce(k_egrid_reduce<5>); break;
        case 6: reduce(k_egrid_reduce<6>); break;
        case 7: reduce(k_egrid_reduce<7>); break;
        default: reduce(k_egrid_reduce<8>); break;
        }
        if (hipGetLastError() != hipSuccess) return eerr(CEG_ERR_HIP, "reduction kernel launch failed");
        if (out_on_device) continue;
        bool ok = true;
        for (int t = 0; t < ntemps; ++t)
            ok = ok && hipMemcpy(red->out_mean + (size_t)t * points + p0, r_mean + (size_t)t * mean_stride, sizeof(double) * (size_t)np,
                                 hipMemcpyDeviceToHost) == hipSuccess;
        if (r_min) ok = ok && hipMemcpy(red->out_min + p0, r_min, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost) == hipSuccess;
        if (r_amin) ok = ok && hipMemcpy(red->out_argmin + p0, r_amin, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) return eerr(CEG_ERR_HIP, "kernel execution or D2H failed");
    }
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_energy_grid(ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid, ceg_recip_t* recip, const double* base,
                               const double* charges, int32_t natoms, const double* rotations, int32_t nrot, const double steps[9],
                               const int32_t num[3], const uint8_t* block, const int32_t block_dims[3], const double block_size[3],
                               const double block_shift[3], const double block_mat[9], const double block_invmat[9],
                               double energy_net_charges, double static_contribution, double* out, int32_t out_on_device, void* stream)
{
    if (!out) return eerr(CEG_ERR_INVALID, "out is NULL");
    return egrid_run(vdw_grids, coulomb_grid, recip, base, charges, natoms, rotations, nrot, steps, num, block, block_dims, block_size,
                     block_shift, block_mat, block_invmat, energy_net_charges, static_contribution, out, nullptr, out_on_device, stream);
}

extern "C" int ceg_energy_grid_reduced(ceg_interp_t* const* vdw_grids, ceg_interp_t* coulomb_grid, ceg_recip_t* recip, const double* base,
                                       const double* charges, int32_t natoms, const double* rotations, int32_t nrot, const double steps[9],
                                       const int32_t num[3], const uint8_t* block, const int32_t block_dims[3], const double block_size[3],
                                       const double block_shift[3], const double block_mat[9], const double block_invmat[9],
                                       double energy_net_charges, double static_contribution, const double* temperatures, int32_t ntemps,
                                       const double* weights, double* out_mean, double* out_min, int32_t* out_argmin, int32_t out_on_device,
                                       void* stream)
{
    if (ntemps < 0 || ntemps > CEG_EGRID_MAX_TEMPS) return eerr(CEG_ERR_INVALID, "ntemps out of range (0 .. CEG_EGRID_MAX_TEMPS)");
    if (ntemps > 0 && !temperatures) return eerr(CEG_ERR_INVALID, "temperatures is NULL");
    for (int t = 0; t < ntemps; ++t)
        if (!(temperatures[t] > 0.0) || !(temperatures[t] < __builtin_huge_val()))
            return eerr(CEG_ERR_INVALID, "a temperature is not finite and positive");
    if ((ntemps > 0) != (out_mean != nullptr)) return eerr(CEG_ERR_INVALID, "out_mean must be given if and only if ntemps > 0");
    if (!out_mean && !out_min && !out_argmin) return eerr(CEG_ERR_INVALID, "no output requested");
    const Reduction red{temperatures, ntemps, weights, out_mean, out_min, out_argmin};
    return egrid_run(vdw_grids, coulomb_grid, recip, base, charges, natoms, rotations, nrot, steps, num, block, block_dims, block_size,
                     block_shift, block_mat, block_invmat, energy_net_charges, static_contribution, nullptr, &red, out_on_device, stream);
}
