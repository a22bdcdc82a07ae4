// ceg_mc_baseline.hip -- baseline_energy (src/montecarlo.jl:530-542) of one chain (ceg_mc_baseline) or of every chain of a group
// (ceg_mc_group_baseline) from the device-resident state, in a fixed number of launches whatever the number of chains and molecules:
//
//   framework_vdw, framework_direct   sum of framework_interactions (montecarlo.jl:490-504) over every atom in the system
//   inter                             compute_vdw (src/energy.jl:355-383): every unordered pair of atoms of different molecules, once
//   recip_framework, recip_guests     sum_k kf Re(conj(S_fw) S) and sum_k kf |S|^2, S = sums[:, 1] (src/ewald.jl:555-577)
//
// A chain's work is cut into ITEMS, one wave each, laid out by its atom slots alone (T = ceil(natoms / 64) tiles of 64 slots):
//   items [0, T)                  framework: the 64 slots of tile t, one grid CORNER per lane as in row 0 of ceg_mc_trial
//   items [T, T + T (T + 1) / 2)  pairs: row tile i (one slot per lane) against column tile j >= i (staged in LDS); the diagonal
//                                 tile keeps column slot > row slot, every tile drops pairs inside one molecule and free slots
//   then `kitems` items           k-space: item k takes k-vectors 64 k + lane, + 64 kitems, ...
// Every item writes one double4 of partial sums to partial[first + item]; k_mc_baseline_sum adds a chain's partials in item order on
// one thread per quantity.  No floating-point atomics: the bytes of the result depend on the chain's slot layout and nothing else, so a
// group member gets what the same handle gets alone (both go through these kernels; the view arrives by kernarg or from the group's
// array and is copied to LDS first).
// CEG_MC_BASELINE_REFRESH runs the structure-factor rebuild of ceg_mc_set_guests first (the bodies of k_mc_sf_molecules /
// k_mc_sf_total, ceg_mc_state.h), over (molecule, chain) and (k-vector, chain).
#include "ceg_mc_state.h"

using namespace ceg_mcs;

namespace {

constexpr int BL_TILE = 64;                    // atom slots per tile = lanes per wave
constexpr int BL_MAX_KITEMS = 16;              // k-space items of a chain at most

struct BlChain {                               // what the HOST fixed for a chain of this call (the kernels size nothing from the view alone)
    int32_t tiles, kitems, stride, nmol;
    int64_t first;                             // the chain's first partial
};

__host__ __device__ inline int bl_pair_items(int tiles) { return tiles * (tiles + 1) / 2; }

// the chain of this workgroup (blockIdx.y): its view and sizes into LDS, from the group's arrays or from the kernel arguments
__device__ __forceinline__ void bl_load(const McView& v1, const McView* views, const BlChain& d1, const BlChain* descs, McView& sv, BlChain& sd)
{
    if (threadIdx.x == 0) {
        if (views) {
            sv = views[blockIdx.y];
            sd = descs[blockIdx.y];
        } else {
            sv = v1;
            sd = d1;
        }
    }
    __syncthreads();
}

// the libm-grade rule energies behind a call (pairs closer than 0.5 A and the handles without fast rules)
__device__ __attribute__((noinline)) double bl_rule_energy_call(const DevRule* R, double r2, double coulombic) { return rule_energy(*R, r2, coulombic); }

__device__ __forceinline__ double bl_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ __launch_bounds__(BL_TILE) void k_mc_baseline_items(McView v1, const McView* __restrict__ views, BlChain d1, const BlChain* __restrict__ descs,
                                                              double4* __restrict__ partial)
{
    __shared__ McView s_v;
    __shared__ BlChain s_d;
    __shared__ double4 s_col[BL_TILE];
    __shared__ double s_val[BL_TILE][2];
    bl_load(v1, views, d1, descs, s_v, s_d);
    const McView& v = s_v;
    const int lane = threadIdx.x, item = blockIdx.x;
    const int T = s_d.tiles, nP = bl_pair_items(T);
    if (item >= T + nP + s_d.kitems) return;
    const int natoms = v.natoms < T * BL_TILE ? v.natoms : T * BL_TILE;        // the partials were sized for T tiles
    double4 res = make_double4(0.0, 0.0, 0.0, 0.0);
    if (item < T) {
        // ---- framework_interactions of the occupied slots of tile `item`: lane 16 a + 8 g + corner of a pass takes atom 4 pass + a,
        // g = 0 its VdW grid, g = 1 the Coulomb grid (the arithmetic of mc_trial_row)
        const int slot0 = item * BL_TILE;
        s_val[lane][0] = 0.0;
        s_val[lane][1] = 0.0;
        __syncthreads();
        for (int pass = 0; pass < BL_TILE / 4; ++pass) {
            const int a = 4 * pass + (lane >> 4), gsel = (lane >> 3) & 1, corner = lane & 7;
            const int slot = slot0 + a;
            if (slot0 + 4 * pass >= natoms) break;
            double part = 0.0, q = 0.0;
            bool blocked = false, have = false, isvdw = false;
            if (slot < natoms) {
                const double4 A = v.atoms[slot];
                int kind, mol;
                unpack(A.w, kind, mol);
                if (mol >= 0) {
                    if (gsel == 0) {
                        const McGrid* G = v.vdw + kind;
                        if (G->grid) { part = ceg_consumers::interp_corner(G->g, G->grid, A.x, A.y, A.z, corner, blocked); have = true; isvdw = G->g.is_vdw != 0; }
                    } else if (v.coulomb.grid) {
                        part = ceg_consumers::interp_corner(v.coulomb.g, v.coulomb.grid, A.x, A.y, A.z, corner, blocked);
                        have = true;
                        isvdw = v.coulomb.g.is_vdw != 0;
                        q = v.kind_charge[kind];
                    }
                }
            }
            int blk = blocked ? 1 : 0;
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                part += __shfl_xor(part, o);
                blk |= __shfl_xor(blk, o);
            }
            if (have && corner == 0) {
                const double val = (isvdw && blk) ? 1e100 : part;              // grids.jl:245-248
                s_val[a][gsel] = gsel == 0 ? val : ((val == 1e100) ? val : q * val);        // montecarlo.jl:500
            }
        }
        __syncthreads();
        // the atoms and molecules that were summed: a molecule is counted at its first slot
        double na = 0.0, nm = 0.0;
        const int slot = slot0 + lane;
        if (slot < natoms) {
            int kind, mol;
            unpack(v.atoms[slot].w, kind, mol);
            if (mol >= 0) {
                na = 1.0;
                if (mol < v.nmol && v.mol[mol].x == slot) nm = 1.0;
            }
        }
        res = make_double4(bl_wave_sum(s_val[lane][0]), bl_wave_sum(s_val[lane][1]), bl_wave_sum(na), bl_wave_sum(nm));
    } else if (item < T + nP) {
        // ---- compute_vdw: row tile i against column tile j >= i
        int p = item - T, i = 0;
        while (p >= T - i) { p -= T - i; ++i; }
        const int j = i + p;
        const double4 none = make_double4(0.0, 0.0, 0.0, __longlong_as_double(-1ll));
        const int rs = i * BL_TILE + lane, cs = j * BL_TILE + lane;
        const double4 R = rs < natoms ? v.atoms[rs] : none;
        s_col[lane] = cs < natoms ? v.atoms[cs] : none;
        __syncthreads();
        int kr, mr;
        unpack(R.w, kr, mr);
        const double* M = v.mat;
        const double* I = v.invmat;
        const double cutoff2 = v.cutoff2, band = 1e-9 * v.cutoff2, coulombic = v.coulombic;
        const int wrap = v.fastwrap, fast = v.fast, nkinds = v.nkinds;
        const DevRule* rules = v.rules;
        const int32_t* offset = v.rule_offset;
        double inter = 0.0;
        for (int c = 0; c < BL_TILE; ++c) {
            const double4 A = s_col[c];
            int kc, mc;
            unpack(A.w, kc, mc);
            if (mc < 0) continue;                                              // free slot (the same for every lane)
            if (mr < 0 || mc == mr || (i == j && c <= lane)) continue;         // energy.jl:419; each pair once
            const double dx = R.x - A.x, dy = R.y - A.y, dz = R.z - A.z;
            double r2;
            if (wrap == 0) r2 = ceg_consumers::pair_distance2_literal(M, I, dx, dy, dz);
            else if (wrap == 1) r2 = ceg_consumers::pair_distance2_fast<false>(M, I, v.geom, dx, dy, dz, cutoff2, band);
            else r2 = ceg_consumers::pair_distance2_fast<true>(M, I, v.geom, dx, dy, dz, cutoff2, band);
            if (!(r2 < cutoff2)) continue;                                     // :422
            const int t = kc * nkinds + kr;
            if (fast && r2 >= 0.25) {
                double r, rinv;
                ceg::fast_sqrt_rsqrt(r2, r, rinv);
                for (int q = offset[t]; q < offset[t + 1]; ++q) inter += rule_energy_fast(rules[q], r2, r, rinv, coulombic);
            } else {
                for (int q = offset[t]; q < offset[t + 1]; ++q) inter += bl_rule_energy_call(&rules[q], r2, coulombic);
            }
        }
        res.x = bl_wave_sum(inter);
    } else {
        // ---- the reciprocal pieces from the resident structure factors
        const int kk = item - T - nP;
        double rf = 0.0, rg = 0.0;
        for (int64_t q = (int64_t)kk * BL_TILE + lane; q < v.nk; q += (int64_t)s_d.kitems * BL_TILE) {
            const double2 f = v.sf_fw[q], s = v.sf_tot[q];
            const double kf = v.kf[q];
            rf += kf * (f.x * s.x + f.y * s.y);
            rg += kf * (s.x * s.x + s.y * s.y);
        }
        res.x = bl_wave_sum(rf);
        res.y = bl_wave_sum(rg);
    }
    if (lane == 0) partial[s_d.first + item] = res;
}

// a chain's partials added in item order, one thread per quantity
__global__ __launch_bounds__(BL_TILE) void k_mc_baseline_sum(BlChain d1, const BlChain* __restrict__ descs, const double4* __restrict__ partial,
                                                            ceg_mc_baseline_t* __restrict__ out)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const BlChain d = descs ? descs[c] : d1;
    const int T = d.tiles, nP = bl_pair_items(T);
    if (lane > 6) return;
    const int b = (lane == 2) ? T : ((lane == 3 || lane == 4) ? T + nP : 0);
    const int e = (lane == 2) ? T + nP : ((lane == 3 || lane == 4) ? T + nP + d.kitems : T);
    const int comp = (lane == 1 || lane == 4) ? 1 : (lane == 5 ? 2 : (lane == 6 ? 3 : 0));
    double s = 0.0;
    for (int it = b; it < e; ++it) {
        const double4 P = partial[d.first + it];
        s += comp == 0 ? P.x : (comp == 1 ? P.y : (comp == 2 ? P.z : P.w));
    }
    ceg_mc_baseline_t* o = out + c;
    switch (lane) {
    case 0: o->framework_vdw = s; break;
    case 1: o->framework_direct = s; break;
    case 2: o->inter = s; break;
    case 3: o->recip_framework = s; break;
    case 4: o->recip_guests = s; break;
    case 5: o->natoms = (int32_t)s; break;
    default: o->nmol = (int32_t)s; break;
    }
}

// CEG_MC_BASELINE_REFRESH: sums[:, ij+1] of molecule blockIdx.x of chain blockIdx.y, then sums[:, 1] of that chain
__global__ __launch_bounds__(MC_THREADS) void k_mc_baseline_sf_molecules(McView v1, const McView* __restrict__ views, BlChain d1, const BlChain* __restrict__ descs)
{
    __shared__ McView s_v;
    __shared__ BlChain s_d;
    bl_load(v1, views, d1, descs, s_v, s_d);
    const int nmol = s_v.nmol < s_d.nmol ? s_v.nmol : s_d.nmol;
    if ((int)blockIdx.x >= nmol) return;
    mc_sf_molecule_body(s_v, (int)blockIdx.x, s_d.stride);
}

__global__ __launch_bounds__(256) void k_mc_baseline_sf_total(McView v1, const McView* __restrict__ views, BlChain d1, const BlChain* __restrict__ descs)
{
    __shared__ McView s_v;
    __shared__ BlChain s_d;
    bl_load(v1, views, d1, descs, s_v, s_d);
    mc_sf_total_body(s_v, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

BlChain plan_chain(const ceg_mc* h, int64_t first)
{
    BlChain d{};
    d.tiles = (h->v.natoms + BL_TILE - 1) / BL_TILE;
    d.kitems = h->v.nk > 0 ? (int32_t)std::min<int64_t>(((int64_t)h->v.nk + BL_TILE - 1) / BL_TILE, BL_MAX_KITEMS) : 0;
    d.stride = h->stride;
    d.nmol = h->v.nmol;
    d.first = first;
    return d;
}

int chain_items(const BlChain& d) { return d.tiles + bl_pair_items(d.tiles) + d.kitems; }

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// The launches of one call for the `k` chains of `descs` (views == nullptr: the one chain of `v1`): [refresh: 2] + items + sum, the
// results copied to `out`, the stream synchronised.  `refreshed` is set once a refresh launch has been issued.
int run_baseline(hipStream_t stream, const McView& v1, const McView* d_views, const std::vector<BlChain>& descs, const std::vector<const ceg_mc*>& chains,
                 bool refresh, unsigned char** scratch, size_t* scratch_cap, ceg_mc_baseline_t* out, bool* refreshed)
{
    static_assert(sizeof(ceg_mc_baseline_t) == 48 && sizeof(BlChain) == 24, "layouts the bindings and the scratch area restate");
    const int k = (int)descs.size();
    int64_t total = 0;
    int max_items = 0, max_nmol = 0, max_m = 1;
    int64_t max_nk = 0;
    for (int c = 0; c < k; ++c) {
        total += chain_items(descs[c]);
        max_items = std::max(max_items, chain_items(descs[c]));
        max_nmol = std::max(max_nmol, (int)descs[c].nmol);
        max_nk = std::max<int64_t>(max_nk, chains[c]->v.nk);
    }
    size_t lds = 0;
    if (refresh)
        for (int c = 0; c < k; ++c) {
            if (chains[c]->v.nk == 0) continue;
            for (const int2& mj : chains[c]->h_mol) max_m = std::max(max_m, mj.y);
            lds = std::max(lds, tables_bytes(chains[c], max_m));
        }
    if (lds + 2048 > 64 * 1024) return merr(CEG_ERR_UNSUPPORTED, "k-space tables of a molecule do not fit in LDS beside the chain's view");
    // scratch: [k] BlChain | [k] results | the partials
    const size_t o_res = align64(sizeof(BlChain) * (size_t)k), o_part = o_res + align64(sizeof(ceg_mc_baseline_t) * (size_t)k);
    const size_t bytes = o_part + sizeof(double4) * (size_t)std::max<int64_t>(total, 1);
    if (bytes > *scratch_cap) {
        if (hipStreamSynchronize(stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
        if (*scratch) (void)hipFree(*scratch);
        *scratch = nullptr;
        *scratch_cap = 0;
        if (hipMalloc((void**)scratch, bytes + bytes / 2) != hipSuccess) return merr(CEG_ERR_HIP, "could not allocate the partial sums");
        *scratch_cap = bytes + bytes / 2;
    }
    BlChain* d_descs = reinterpret_cast<BlChain*>(*scratch);
    ceg_mc_baseline_t* d_res = reinterpret_cast<ceg_mc_baseline_t*>(*scratch + o_res);
    double4* d_part = reinterpret_cast<double4*>(*scratch + o_part);
    const BlChain* descs_arg = nullptr;
    if (d_views) {
        if (hipMemcpyAsync(d_descs, descs.data(), sizeof(BlChain) * (size_t)k, hipMemcpyHostToDevice, stream) != hipSuccess) return merr(CEG_ERR_HIP, "H2D failed");
        descs_arg = d_descs;
    }
    const BlChain d1 = descs[0];
    if (refresh && max_nk > 0) {
        *refreshed = true;
        if (max_nmol > 0)
            hipLaunchKernelGGL(k_mc_baseline_sf_molecules, dim3((unsigned)max_nmol, (unsigned)k), dim3(MC_THREADS), lds, stream, v1, d_views, d1, descs_arg);
        hipLaunchKernelGGL(k_mc_baseline_sf_total, dim3((unsigned)((max_nk + 255) / 256), (unsigned)k), dim3(256), 0, stream, v1, d_views, d1, descs_arg);
        if (hipGetLastError() != hipSuccess) return merr(CEG_ERR_HIP, "structure-factor kernels failed to launch");
    }
    if (max_items > 0)
        hipLaunchKernelGGL(k_mc_baseline_items, dim3((unsigned)max_items, (unsigned)k), dim3(BL_TILE), 0, stream, v1, d_views, d1, descs_arg, d_part);
    hipLaunchKernelGGL(k_mc_baseline_sum, dim3((unsigned)k), dim3(BL_TILE), 0, stream, d1, descs_arg, d_part, d_res);
    if (hipGetLastError() != hipSuccess) return merr(CEG_ERR_HIP, "baseline kernels failed to launch");
    if (hipMemcpyAsync(out, d_res, sizeof(ceg_mc_baseline_t) * (size_t)k, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return merr(CEG_ERR_HIP, "baseline kernels failed");
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_mc_baseline(ceg_mc_t* h, int32_t flags, ceg_mc_baseline_t* out)
{
    if (!h || !out) return merr(CEG_ERR_INVALID, "bad argument (NULL handle or out)");
    if (flags & ~CEG_MC_BASELINE_REFRESH) return merr(CEG_ERR_INVALID, "unknown flag bits (CEG_MC_BASELINE_REFRESH is the only flag)");
    if (h->poisoned) return merr(CEG_ERR_HIP, "the handle is inconsistent after an earlier failure of accept / insert / remove: call ceg_mc_set_guests");
    Guard guard(h->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    bool refreshed = false;
    const int rc = run_baseline(h->stream, h->v, nullptr, {plan_chain(h, 0)}, {h}, (flags & CEG_MC_BASELINE_REFRESH) != 0, &h->d_baseline, &h->baseline_cap, out,
                                &refreshed);
    if (rc != CEG_OK && refreshed) h->poisoned = true;
    return rc;
}

extern "C" int ceg_mc_group_baseline(ceg_mc_group_t* g, int32_t flags, ceg_mc_baseline_t* out)
{
    if (!g || !out) return merr(CEG_ERR_INVALID, "bad argument (NULL group or out)");
    if (flags & ~CEG_MC_BASELINE_REFRESH) return merr(CEG_ERR_INVALID, "unknown flag bits (CEG_MC_BASELINE_REFRESH is the only flag)");
    const GroupRef r = group_ref(g);
    std::vector<BlChain> descs((size_t)r.k);
    std::vector<const ceg_mc*> chains((size_t)r.k);
    int64_t first = 0;
    for (int c = 0; c < r.k; ++c) {
        if (r.chains[c]->poisoned) return group_refuse_poisoned(c);
        chains[c] = r.chains[c];
        descs[c] = plan_chain(r.chains[c], first);
        first += chain_items(descs[c]);
    }
    Guard guard(r.device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (!group_views_current(g)) return merr(CEG_ERR_HIP, "view upload failed");
    bool refreshed = false;
    const int rc = run_baseline(r.stream, r.chains[0]->v, r.d_views, descs, chains, (flags & CEG_MC_BASELINE_REFRESH) != 0, r.d_baseline, r.baseline_cap, out,
                                &refreshed);
    if (rc == CEG_OK) group_stream_idle(g);
    else if (refreshed)
        for (int c = 0; c < r.k; ++c) r.chains[c]->poisoned = true;
    return rc;
}
