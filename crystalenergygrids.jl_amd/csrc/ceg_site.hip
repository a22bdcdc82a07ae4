// ceg_site.hip -- site hopping (ceg_site_group_*): the reference's second Monte-Carlo model (src/sitehopping.jl), whole runs of K
// chains on two tables.  A step is two gathers over the population and one Metropolis decision (run_montecarlo!(::SiteHopping),
// src/simulation.jl:922-966), so it gets no launch of its own: one wave owns a chain and runs every step of every cycle of a launch
// (k_site_sweep), the population in LDS, the two table rows read from global memory where the population points.  The state that
// outlives a launch -- population, running energy, counters -- sits in device memory, so a call can be cut into launches anywhere.
// The step is specified word for word in include/ceg_hip.h and restated in ceg_hip/mcrng.py (site_step).  The group knows no
// ceg_mc_t: it is self-contained.  With tempering installed (ceg_site_group_set_tempering) the chains are ladders of R rungs and the
// same call launches k_site_sweep_pt instead: one workgroup per ladder, one wave per rung, the exchange of run_parallel_tempering
// (src/simulation.jl:461-634) drawn per step inside the kernel (mcrng.site_ladder_replay).  ceg_site_group_sweep_grouped is the
// groupcycles / restartgroupcycle mode of the same loop (src/simulation.jl:917-982): k_site_sweep_grouped, one wave per chain again,
// accepts or rejects the hops of a cycle as one move and can restart every cycle from a fresh random population, all inside the
// kernel (mcrng.site_grouped_replay).
// The second half of the file builds the two tables (ceg_site_tables / ceg_site_tables_device) from a guest-free ceg_mc_t of the
// mobile species in three launches for any number of sites: k_site_points (framework terms and structure factor per site),
// k_site_recip_pairs (the reciprocal pair term, v_mfma_f64_16x16x4 over 16 x 16 site tiles of the upper triangle) and
// k_site_real_pairs (the molecule-pair sums over the same tiles).  It reads the handle's view and writes nothing of the handle.
#include "ceg_host.h"
#include "ceg_mc_state.h"
#include "ceg_philox.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using ceg_host::fail;

namespace {

static_assert(sizeof(ceg_site_params_t) == 24 && sizeof(ceg_site_cycles_t) == 32 && sizeof(ceg_site_stats_t) == 32 &&
              sizeof(ceg_site_cycle_record_t) == 56 && sizeof(ceg_site_record_t) == 40 && sizeof(ceg_site_recorder_t) == 32 &&
              sizeof(ceg_site_frame_record_t) == 16 && sizeof(ceg_site_tempering_t) == 32, "layouts the bindings restate");

constexpr uint32_t SITE_SELECT = 10;             // the purpose of the (molecule, site) draw; 3 (ceg_philox::ACCEPT) gives u
constexpr uint32_t SITE_EXCHANGE = 12;           // the purpose of a ladder's exchange draw (11 is the host's SITE_POPULATE)
constexpr int BASE_THREADS = 256;
constexpr int PT_MAX_RUNGS = 16;                 // 16 waves: one workgroup of 1024 threads

struct SiteRecorderView {                        // every == 0 and track_min == 0: no recorder
    int64_t every, origin, capacity;
    int64_t frame0, first_due;                   // frames held when the call began; the first due cycle >= the call's cycle0
    uint16_t* frames;                            // [capacity][K][m]
    ceg_site_frame_record_t* frec;               // [capacity][K]
    uint16_t* best;                              // [K][m]
    double* mine;                                // [K]
    int64_t* mink;                               // [K]
    int32_t track_min;
};

struct SiteSweep {                               // by value (kernarg)
    const double* framework;                     // [n]
    const double* interactions;                  // [n][n]
    uint16_t* pop;                               // [K][m]
    double *energy, *delta;                      // [K]
    int64_t *attempted, *accepted;               // [K]
    const double* temperature;                   // [ncycles][K]
    const uint32_t* stream;                      // [K]
    ceg_site_cycle_record_t* cyc;                // [ncycles][K] or nullptr
    ceg_site_record_t* log;                      // [ncycles * spc][K] or nullptr
    uint64_t seed, first_step;
    int64_t cycle0, spc, t0, t1;                 // this launch runs the call's steps [t0, t1)
    int32_t n, m, k;
    SiteRecorderView rec;
};

// x of lane (l ^ O) for O = 1, 2, 4, 8 inside a row of 16 lanes, all lanes active: data-parallel moves, no LDS round trip.
// quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, [3,2,1,0] = 0x1B (l ^ 3); row_half_mirror 0x141 (l ^ 7), so l ^ 4 = (l ^ 7) ^ 3;
// row_ror:8 = 0x128 (l ^ 8).
template <int CTRL>
__device__ __forceinline__ double dpp_move(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
template <int O>
__device__ __forceinline__ double from_lane_xor(double x)
{
    static_assert(O == 1 || O == 2 || O == 4 || O == 8, "inside a row");
    if (O == 1) return dpp_move<0xB1>(x);
    if (O == 2) return dpp_move<0x4E>(x);
    if (O == 4) return dpp_move<0x1B>(dpp_move<0x141>(x));
    return dpp_move<0x128>(x);
}

// Workgroup = wave c = chain c.  Every value but the lane's share of the two row sums is wave-uniform.  The order of every
// floating-point operation is the one include/ceg_hip.h writes down.  s_pop is written by lane 0 and read by all lanes: a barrier
// (one wave: a wait) stands between.  Indices: i < m and new < n by the clamps, population entries < n as validated on the host
// and written only here, frame slots checked against the capacity, log and cycle records inside [ncycles * spc][K] / [ncycles][K].
__global__ __launch_bounds__(64) void k_site_sweep(const SiteSweep S)
{
    extern __shared__ uint16_t s_pop[];
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int m = S.m;
    const size_t n = (size_t)S.n, K = (size_t)S.k;
    uint16_t* gpop = S.pop + (size_t)c * (size_t)m;
    for (int j = lane; j < m; j += 64) s_pop[j] = gpop[j];
    double energy = S.energy[c], delta = S.delta[c];
    int64_t attempted = S.attempted[c], accepted = S.accepted[c];
    const uint32_t stream = S.stream[c];
    int64_t cyc = S.t0 / S.spc, in = S.t0 - cyc * S.spc;
    double T = S.temperature[(size_t)cyc * K + c];
    double mine = S.rec.track_min ? S.rec.mine[c] : 0.0;
    __syncthreads();
    for (int64_t t = S.t0; t < S.t1; ++t) {
        const uint64_t s = S.first_step + (uint64_t)t;
        const ceg_philox::Block a = ceg_philox::draw(S.seed, s, stream, SITE_SELECT);
        const ceg_philox::Block b = ceg_philox::draw(S.seed, s, stream, ceg_philox::ACCEPT);
        const int i = min((int)floor(ceg_philox::uniform(a.w[0], a.w[1]) * (double)m), m - 1);
        const int nw = min((int)floor(ceg_philox::uniform(a.w[2], a.w[3]) * (double)S.n), S.n - 1);
        const double u = ceg_philox::uniform(b.w[0], b.w[1]);
        const int old = (int)s_pop[i];
        const double* __restrict__ row_old = S.interactions + (size_t)old * n;
        const double* __restrict__ row_new = S.interactions + (size_t)nw * n;
        const double f_old = S.framework[old], f_new = S.framework[nw];
        double so = 0.0, sn = 0.0;
        for (int j = lane; j < m; j += 64) {
            const size_t p = (size_t)s_pop[j];
            double x = row_old[p], y = row_new[p];
            if (j == i) { x = 0.0; y = 0.0; }
            so += x;
            sn += y;
        }
        so += __shfl_xor(so, 32); sn += __shfl_xor(sn, 32);
        so += __shfl_xor(so, 16); sn += __shfl_xor(sn, 16);
        so += from_lane_xor<8>(so); sn += from_lane_xor<8>(sn);
        so += from_lane_xor<4>(so); sn += from_lane_xor<4>(sn);
        so += from_lane_xor<2>(so); sn += from_lane_xor<2>(sn);
        so += from_lane_xor<1>(so); sn += from_lane_xor<1>(sn);
        const double before = f_old + so, after = f_new + sn;
        bool ok = after < before;
        if (!ok) ok = u < exp((before - after) / T);        // (wave-uniform: a downhill step pays neither the division nor the exp)
        ++attempted;
        if (ok) {
            const double d = after - before;
            energy = energy + d;
            delta = delta + d;
            ++accepted;
            if (lane == 0) s_pop[i] = (uint16_t)nw;
        }
        if (S.log && lane == 0) {
            ceg_site_record_t r;
            r.molecule = i; r.old_site = old; r.new_site = nw; r.accepted = ok ? 1 : 0;
            r.before = before; r.after = after; r.u = u;
            S.log[(size_t)t * K + c] = r;
        }
        __syncthreads();
        if (++in == S.spc) {                     // ---- the end of cycle cc
            const int64_t cc = S.cycle0 + cyc;
            int32_t flags = 0;
            const SiteRecorderView& R = S.rec;
            if (R.every > 0 && cc >= R.origin && (cc - R.origin) % R.every == 0) {
                const int64_t slot = R.frame0 + (cc - R.first_due) / R.every;
                if (slot >= 0 && slot < R.capacity) {
                    uint16_t* f = R.frames + ((size_t)slot * K + c) * (size_t)m;
                    for (int j = lane; j < m; j += 64) f[j] = s_pop[j];
                    if (lane == 0) R.frec[(size_t)slot * K + c] = ceg_site_frame_record_t{cc, energy};
                    flags |= CEG_SITE_FRAME_TAKEN;
                } else {
                    flags |= CEG_SITE_FRAME_DROPPED;
                }
            }
            if (R.track_min && energy < mine) {
                mine = energy;
                uint16_t* f = R.best + (size_t)c * (size_t)m;
                for (int j = lane; j < m; j += 64) f[j] = s_pop[j];
                if (lane == 0) { R.mine[c] = energy; R.mink[c] = cc; }
                flags |= CEG_SITE_NEW_MINIMUM;
            }
            if (S.cyc && lane == 0) {
                ceg_site_cycle_record_t r;
                r.cycle = cc; r.temperature = T; r.energy = energy; r.delta = delta;
                r.attempted = attempted; r.accepted = accepted; r.flags = flags; r._pad = 0;
                S.cyc[(size_t)cyc * K + c] = r;
            }
            ++cyc;
            in = 0;
            if (t + 1 < S.t1) T = S.temperature[(size_t)cyc * K + c];
        }
    }
    for (int j = lane; j < m; j += 64) gpop[j] = s_pop[j];
    if (lane == 0) {
        S.energy[c] = energy; S.delta[c] = delta;
        S.attempted[c] = attempted; S.accepted[c] = accepted;
    }
}

struct SiteLadders {                             // by value (kernarg): the tempering of the group, include/ceg_hip.h "tempering"
    const double* pair_cdf;                      // [R-1]
    const uint32_t* ladder_stream;               // [K/R]
    int64_t *pt_attempted, *pt_accepted;         // [K/R][R-1]
    int32_t* replica;                            // [K]
    int32_t rungs, pop_stride;                   // R; the uint16 entries between two populations in LDS (pop_lds(m) / 2)
};

struct SiteHop {
    int i, old, nw;
    double before, after, u;
    bool ok;
};

// The step of k_site_sweep on the population `pop` (LDS), operation for operation: the lane stride, the xor butterfly and the rule.
// Wave-uniform but for the lane's share of the two sums; on acceptance lane 0 writes pop[i] and the caller adds after - before.
__device__ __forceinline__ SiteHop site_hop(const SiteSweep& S, uint16_t* pop, uint64_t s, uint32_t stream, double T, int lane)
{
    const int m = S.m;
    const size_t n = (size_t)S.n;
    const ceg_philox::Block a = ceg_philox::draw(S.seed, s, stream, SITE_SELECT);
    const ceg_philox::Block b = ceg_philox::draw(S.seed, s, stream, ceg_philox::ACCEPT);
    SiteHop h;
    h.i = min((int)floor(ceg_philox::uniform(a.w[0], a.w[1]) * (double)m), m - 1);
    h.nw = min((int)floor(ceg_philox::uniform(a.w[2], a.w[3]) * (double)S.n), S.n - 1);
    h.u = ceg_philox::uniform(b.w[0], b.w[1]);
    h.old = (int)pop[h.i];
    const double* __restrict__ row_old = S.interactions + (size_t)h.old * n;
    const double* __restrict__ row_new = S.interactions + (size_t)h.nw * n;
    const double f_old = S.framework[h.old], f_new = S.framework[h.nw];
    double so = 0.0, sn = 0.0;
    for (int j = lane; j < m; j += 64) {
        const size_t p = (size_t)pop[j];
        double x = row_old[p], y = row_new[p];
        if (j == h.i) { x = 0.0; y = 0.0; }
        so += x;
        sn += y;
    }
    so += __shfl_xor(so, 32); sn += __shfl_xor(sn, 32);
    so += __shfl_xor(so, 16); sn += __shfl_xor(sn, 16);
    so += from_lane_xor<8>(so); sn += from_lane_xor<8>(sn);
    so += from_lane_xor<4>(so); sn += from_lane_xor<4>(sn);
    so += from_lane_xor<2>(so); sn += from_lane_xor<2>(sn);
    so += from_lane_xor<1>(so); sn += from_lane_xor<1>(sn);
    h.before = f_old + so;
    h.after = f_new + sn;
    h.ok = h.after < h.before;
    if (!h.ok) h.ok = h.u < exp((h.before - h.after) / T);
    if (h.ok && lane == 0) pop[h.i] = (uint16_t)h.nw;
    return h;
}

// Workgroup l = ladder l, wave r = rung r = chain l R + r (blockDim = 64 R).  The R populations sit in dynamic LDS, `slot` says
// which one the rung owns; energy, delta, slot and the replica entry belong to the configuration and change hands in an exchange,
// everything else in the wave's registers belongs to the rung.  The counters of pair j live in wave j.
// Protocol, ONE workgroup barrier per step, double-buffered by the step's parity p = t & 1: lane 0 of every wave publishes
// (energy, delta, slot, replica) into s_pub*[p][r], then the barrier, then the step.  The two waves of an attempted pair read the
// partner's entry of s_pub*[p] and come to the same decision from the same bits; nobody writes s_pub*[p] again before the barrier
// of step t + 1 has passed, which every reader of step t reaches only after its reads, so a late reader never meets step t + 2's
// values.  The same barrier orders a lane-0 population write of step t before every read of step t + 1, whichever wave owns the
// slot by then.  The barrier is the first statement of the loop body and the one after the loop: no branch that depends on the
// rung, the pair or the cycle contains one, and the end-of-cycle code has none -- it patches this step's hop into what it copies
// (pop_at) instead of waiting for lane 0's write.
// Indices: as k_site_sweep; slot < R as published by waves of this workgroup; pair < R - 1, so pair + 1 is a rung; the counters
// inside [K/R][R-1].
__global__ __launch_bounds__(1024) void k_site_sweep_pt(const SiteSweep S, const SiteLadders P)
{
    extern __shared__ uint16_t s_pop[];
    __shared__ double s_pub_e[2][PT_MAX_RUNGS], s_pub_d[2][PT_MAX_RUNGS], s_cdf[PT_MAX_RUNGS];
    __shared__ int32_t s_pub_slot[2][PT_MAX_RUNGS], s_pub_rep[2][PT_MAX_RUNGS];
    const int R = P.rungs, l = (int)blockIdx.x, r = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int c = l * R + r, m = S.m;
    const size_t K = (size_t)S.k;
    uint16_t* gpop = S.pop + (size_t)c * (size_t)m;
    int slot = r;                                // between launches the populations lie by rung
    for (int j = lane; j < m; j += 64) s_pop[(size_t)slot * P.pop_stride + j] = gpop[j];
    if ((int)threadIdx.x < R - 1) s_cdf[threadIdx.x] = P.pair_cdf[threadIdx.x];
    double energy = S.energy[c], delta = S.delta[c];
    int32_t rep = P.replica[c];
    int64_t attempted = S.attempted[c], accepted = S.accepted[c];
    int64_t pt_att = 0, pt_acc = 0;              // of the pair (r, r + 1)
    if (r < R - 1) { pt_att = P.pt_attempted[(size_t)l * (R - 1) + r]; pt_acc = P.pt_accepted[(size_t)l * (R - 1) + r]; }
    const uint32_t stream = S.stream[c], lstream = P.ladder_stream[l];
    int64_t cyc = S.t0 / S.spc, in = S.t0 - cyc * S.spc;
    double T = S.temperature[(size_t)cyc * K + c];
    double mine = S.rec.track_min ? S.rec.mine[c] : 0.0;
    for (int64_t t = S.t0; t < S.t1; ++t) {
        const int p = (int)(t & 1);
        if (lane == 0) { s_pub_e[p][r] = energy; s_pub_d[p][r] = delta; s_pub_slot[p][r] = slot; s_pub_rep[p][r] = rep; }
        __syncthreads();                         // the step's only barrier
        const uint64_t s = S.first_step + (uint64_t)t;
        const ceg_philox::Block x = ceg_philox::draw(S.seed, s, lstream, SITE_EXCHANGE);
        const double v = ceg_philox::uniform(x.w[0], x.w[1]);
        int pair = 0;                            // the first j with v < pair_cdf[j] (non-decreasing: the entries <= v come first)
        while (pair < R - 1 && !(v < s_cdf[pair])) ++pair;
        int hop_i = -1, hop_nw = 0;              // this step's accepted hop, for the copies at the cycle's end
        if (pair < R - 1 && (r == pair || r == pair + 1)) {
            const int q = r == pair ? pair + 1 : pair;
            const double u = ceg_philox::uniform(x.w[2], x.w[3]);
            const double E_a = s_pub_e[p][pair], E_b = s_pub_e[p][pair + 1];
            const double T_a = S.temperature[(size_t)cyc * K + (size_t)(l * R + pair)], T_b = S.temperature[(size_t)cyc * K + (size_t)(l * R + pair + 1)];
            bool ok = E_b < E_a;
            if (!ok) {
                const double Tx = 1.0 / (1.0 / T_a - 1.0 / T_b);
                ok = u < exp((E_a - E_b) / Tx);
            }
            if (r == pair) { ++pt_att; if (ok) ++pt_acc; }
            if (ok) {
                energy = s_pub_e[p][q];
                delta = s_pub_d[p][q];
                slot = s_pub_slot[p][q];
                rep = s_pub_rep[p][q];
            }
            if (S.log && lane == 0) {
                ceg_site_record_t rec;
                rec.molecule = r == pair ? -1 : -2; rec.old_site = -1; rec.new_site = -1; rec.accepted = ok ? 1 : 0;
                rec.before = E_a; rec.after = E_b; rec.u = u;
                S.log[(size_t)t * K + c] = rec;
            }
        } else {
            const SiteHop h = site_hop(S, s_pop + (size_t)slot * P.pop_stride, s, stream, T, lane);
            ++attempted;
            if (h.ok) {
                const double d = h.after - h.before;
                energy = energy + d;
                delta = delta + d;
                ++accepted;
                hop_i = h.i;
                hop_nw = h.nw;
            }
            if (S.log && lane == 0) {
                ceg_site_record_t rec;
                rec.molecule = h.i; rec.old_site = h.old; rec.new_site = h.nw; rec.accepted = h.ok ? 1 : 0;
                rec.before = h.before; rec.after = h.after; rec.u = h.u;
                S.log[(size_t)t * K + c] = rec;
            }
        }
        if (++in == S.spc) {                     // ---- the end of cycle cc, by rung, with what sits on the rung now (no barrier here)
            const uint16_t* pop = s_pop + (size_t)slot * P.pop_stride;
            auto pop_at = [&](int j) { return j == hop_i ? (uint16_t)hop_nw : pop[j]; };
            const int64_t cc = S.cycle0 + cyc;
            int32_t flags = 0;
            const SiteRecorderView& V = S.rec;
            if (V.every > 0 && cc >= V.origin && (cc - V.origin) % V.every == 0) {
                const int64_t fs = V.frame0 + (cc - V.first_due) / V.every;
                if (fs >= 0 && fs < V.capacity) {
                    uint16_t* f = V.frames + ((size_t)fs * K + c) * (size_t)m;
                    for (int j = lane; j < m; j += 64) f[j] = pop_at(j);
                    if (lane == 0) V.frec[(size_t)fs * K + c] = ceg_site_frame_record_t{cc, energy};
                    flags |= CEG_SITE_FRAME_TAKEN;
                } else {
                    flags |= CEG_SITE_FRAME_DROPPED;
                }
            }
            if (V.track_min && energy < mine) {
                mine = energy;
                uint16_t* f = V.best + (size_t)c * (size_t)m;
                for (int j = lane; j < m; j += 64) f[j] = pop_at(j);
                if (lane == 0) { V.mine[c] = energy; V.mink[c] = cc; }
                flags |= CEG_SITE_NEW_MINIMUM;
            }
            if (S.cyc && lane == 0) {
                ceg_site_cycle_record_t rec;
                rec.cycle = cc; rec.temperature = T; rec.energy = energy; rec.delta = delta;
                rec.attempted = attempted; rec.accepted = accepted; rec.flags = flags; rec._pad = 0;
                S.cyc[(size_t)cyc * K + c] = rec;
            }
            ++cyc;
            in = 0;
            if (t + 1 < S.t1) T = S.temperature[(size_t)cyc * K + c];
        }
    }
    __syncthreads();                             // the last step's population writes, before any wave copies a slot out
    const uint16_t* pop = s_pop + (size_t)slot * P.pop_stride;
    for (int j = lane; j < m; j += 64) gpop[j] = pop[j];
    if (lane == 0) {
        S.energy[c] = energy; S.delta[c] = delta;
        S.attempted[c] = attempted; S.accepted[c] = accepted;
        P.replica[c] = rep;
        if (r < R - 1) { P.pt_attempted[(size_t)l * (R - 1) + r] = pt_att; P.pt_accepted[(size_t)l * (R - 1) + r] = pt_acc; }
    }
}

// ---- grouped cycles (ceg_site_group_sweep_grouped; run_montecarlo!(::SiteHopping; groupcycles, restartgroupcycle), simulation.jl:917-982)
static_assert(sizeof(ceg_site_grouped_record_t) == 48, "a layout the bindings restate");

constexpr uint32_t SITE_GROUP = 13;              // the purpose of a grouped cycle's decision draw
constexpr uint32_t SITE_RESTART = 14;            // entry j of a restart's shuffle: counter word 3 = 14 | (j << 8)

struct SiteGrouped {                             // by value (kernarg): what a grouped call adds to SiteSweep
    uint16_t* p0;                                // [K][m] P0, the population at the start of the cycle in flight
    double *e0, *d0, *er;                        // [K] E0, D0 and Er of the cycle in flight
    int64_t* hops;                               // [K] the hops accepted in it so far
    ceg_site_grouped_record_t* out;              // [ncycles][K] or nullptr
    double tail;
    int32_t restart, pop_stride;                 // pop_stride: the uint16 entries between s_pop and the r_j of a restart in LDS
};

// baseline_energy of the population `pop` (LDS) by one wave, in the order include/ceg_hip.h writes down ("grouped cycles", restart):
// lane l adds framework[pop[j]] for j = l, l + 64, ... onto +0.0 (F); row by row, i = 0 .. m - 2, lane l adds
// interactions[pop[i]][pop[j]] for j = i + 1 + l, i + 1 + l + 64, ... onto ONE accumulator that starts at +0.0 (E); both meet by the xor
// butterfly of the row sum; the result is (tail + F) + E.  Every lane returns it.
__device__ __forceinline__ double site_baseline_wave(const SiteSweep& S, const uint16_t* pop, double tail, int lane)
{
    const int m = S.m;
    const size_t n = (size_t)S.n;
    double f = 0.0, e = 0.0;
    for (int j = lane; j < m; j += 64) f += S.framework[pop[j]];
    int i = 0;
    for (; m - (i + 1) > 64; ++i) {
        const double* __restrict__ row = S.interactions + (size_t)pop[i] * n;
        for (int j = i + 1 + lane; j < m; j += 64) e += row[pop[j]];
    }
    // the last rows hold one term per lane at the most: eight rows' gathers in flight, added in the rows' order, +0.0 where the lane
    // has no term (the same bits: e is never -0.0)
    for (; i + 1 < m; i += 8) {
        double t[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int j = i + r + 1 + lane;
            t[r] = j < m ? S.interactions[(size_t)pop[i + r] * n + (size_t)pop[j]] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) e += t[r];
    }
    f += __shfl_xor(f, 32); e += __shfl_xor(e, 32);
    f += __shfl_xor(f, 16); e += __shfl_xor(e, 16);
    f += from_lane_xor<8>(f); e += from_lane_xor<8>(e);
    f += from_lane_xor<4>(f); e += from_lane_xor<4>(e);
    f += from_lane_xor<2>(f); e += from_lane_xor<2>(e);
    f += from_lane_xor<1>(f); e += from_lane_xor<1>(e);
    return (tail + f) + e;
}

// Workgroup = wave c = chain c, as k_site_sweep; the hop is site_hop.  What a grouped cycle adds happens at its first step (save,
// restart) and after its last (decision, restore), by the rule of include/ceg_hip.h "grouped cycles".  A launch may end inside a
// cycle: P0 sits in device memory from the cycle's start on, E0, D0 and Er are written there at the start and the hop count at the
// end of every launch, and a launch that begins inside a cycle reads them back.
// The restart never builds the n-entry permutation.  Pass 1, lane-strided: r_j of entry j from its own Philox block, into s_r.
// Pass 2, lane-strided: entry j ends as the value that position r_j held just before exchange j.  That value is p itself unless an
// earlier exchange q < j had r_q == p; the latest such q put there what position q held just before exchange q, and so on down
// (q falls strictly, so the walk ends).  Positions >= j are touched by earlier exchanges only as their r_q, which is all the walk
// looks at.
// Indices: as k_site_sweep; s_r[j] and the walk's q stay inside [0, m); p0 inside [K][m]; the grouped record inside [ncycles][K].
__global__ __launch_bounds__(64) void k_site_sweep_grouped(const SiteSweep S, const SiteGrouped G)
{
    extern __shared__ uint16_t s_pop[];
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int m = S.m;
    const size_t K = (size_t)S.k;
    uint16_t* s_r = s_pop + G.pop_stride;
    uint16_t* gpop = S.pop + (size_t)c * (size_t)m;
    uint16_t* gp0 = G.p0 + (size_t)c * (size_t)m;
    for (int j = lane; j < m; j += 64) s_pop[j] = gpop[j];
    double energy = S.energy[c], delta = S.delta[c];
    int64_t attempted = S.attempted[c], accepted = S.accepted[c];
    const uint32_t stream = S.stream[c];
    int64_t cyc = S.t0 / S.spc, in = S.t0 - cyc * S.spc;
    double T = S.temperature[(size_t)cyc * K + c];
    double mine = S.rec.track_min ? S.rec.mine[c] : 0.0;
    double E0 = 0.0, D0 = 0.0, Er = 0.0;
    int64_t hops = 0;
    if (in != 0) { E0 = G.e0[c]; D0 = G.d0[c]; Er = G.er[c]; hops = G.hops[c]; }      // the launch begins inside a cycle
    __syncthreads();
    for (int64_t t = S.t0; t < S.t1; ++t) {
        const uint64_t s = S.first_step + (uint64_t)t;
        if (in == 0) {                           // ---- the start of a cycle: save, restart
            E0 = energy; D0 = delta; hops = 0;
            for (int j = lane; j < m; j += 64) gp0[j] = s_pop[j];
            if (G.restart) {
                for (int j = lane; j < m; j += 64) {
                    const ceg_philox::Block b = ceg_philox::draw(S.seed, s, stream, ceg_philox::attempt_purpose(SITE_RESTART, (uint32_t)j));
                    const int left = S.n - j;
                    s_r[j] = (uint16_t)(j + min((int)floor(ceg_philox::uniform(b.w[0], b.w[1]) * (double)left), left - 1));
                }
                __syncthreads();
                for (int j = lane; j < m; j += 64) {
                    int p = (int)s_r[j], top = j;
                    for (;;) {
                        int q = top - 1;
                        while (q >= 0 && (int)s_r[q] != p) --q;
                        if (q < 0) break;
                        p = q;
                        top = q;
                    }
                    s_pop[j] = (uint16_t)p;
                }
                __syncthreads();
                energy = site_baseline_wave(S, s_pop, G.tail, lane);
            }
            Er = energy;
            if (lane == 0) { G.e0[c] = E0; G.d0[c] = D0; G.er[c] = Er; }
        }
        const SiteHop h = site_hop(S, s_pop, s, stream, T, lane);
        if (h.ok) {
            energy = energy + (h.after - h.before);
            ++hops;
        }
        if (S.log && lane == 0) {
            ceg_site_record_t r;
            r.molecule = h.i; r.old_site = h.old; r.new_site = h.nw; r.accepted = h.ok ? 1 : 0;
            r.before = h.before; r.after = h.after; r.u = h.u;
            S.log[(size_t)t * K + c] = r;
        }
        __syncthreads();
        if (++in == S.spc) {                     // ---- the decision, then the end of cycle cc on what it leaves
            const ceg_philox::Block g = ceg_philox::draw(S.seed, s, stream, SITE_GROUP);
            const double u = ceg_philox::uniform(g.w[0], g.w[1]), E1 = energy;
            bool ok = E1 < E0;
            if (!ok) ok = u < exp((E0 - E1) / T);
            ++attempted;
            if (ok) {
                ++accepted;
                delta = D0 + (E1 - E0);
            } else {
                for (int j = lane; j < m; j += 64) s_pop[j] = gp0[j];
                energy = E0;
                delta = D0;
            }
            __syncthreads();
            if (G.out && lane == 0) {
                ceg_site_grouped_record_t r;
                r.before = E0; r.restart_energy = Er; r.after = E1; r.u = u;
                r.accepted = ok ? 1 : 0; r.restarted = G.restart ? 1 : 0; r.hops_accepted = hops;
                G.out[(size_t)cyc * K + c] = r;
            }
            const int64_t cc = S.cycle0 + cyc;
            int32_t flags = (ok ? CEG_SITE_GROUP_ACCEPTED : 0) | (G.restart ? CEG_SITE_GROUP_RESTARTED : 0);
            const SiteRecorderView& R = S.rec;
            if (R.every > 0 && cc >= R.origin && (cc - R.origin) % R.every == 0) {
                const int64_t slot = R.frame0 + (cc - R.first_due) / R.every;
                if (slot >= 0 && slot < R.capacity) {
                    uint16_t* f = R.frames + ((size_t)slot * K + c) * (size_t)m;
                    for (int j = lane; j < m; j += 64) f[j] = s_pop[j];
                    if (lane == 0) R.frec[(size_t)slot * K + c] = ceg_site_frame_record_t{cc, energy};
                    flags |= CEG_SITE_FRAME_TAKEN;
                } else {
                    flags |= CEG_SITE_FRAME_DROPPED;
                }
            }
            if (R.track_min && energy < mine) {
                mine = energy;
                uint16_t* f = R.best + (size_t)c * (size_t)m;
                for (int j = lane; j < m; j += 64) f[j] = s_pop[j];
                if (lane == 0) { R.mine[c] = energy; R.mink[c] = cc; }
                flags |= CEG_SITE_NEW_MINIMUM;
            }
            if (S.cyc && lane == 0) {
                ceg_site_cycle_record_t r;
                r.cycle = cc; r.temperature = T; r.energy = energy; r.delta = delta;
                r.attempted = attempted; r.accepted = accepted; r.flags = flags; r._pad = 0;
                S.cyc[(size_t)cyc * K + c] = r;
            }
            ++cyc;
            in = 0;
            if (t + 1 < S.t1) T = S.temperature[(size_t)cyc * K + c];
        }
    }
    for (int j = lane; j < m; j += 64) gpop[j] = s_pop[j];
    if (lane == 0) {
        S.energy[c] = energy; S.delta[c] = delta;
        S.attempted[c] = attempted; S.accepted[c] = accepted;
        G.hops[c] = hops;
    }
}

// Workgroup c: baseline_energy (sitehopping.jl:105-112) of chain c.  Thread t takes the rows i = t, t + 256, ... and in each the
// pairs j = i + 1 .. m - 1 in rising order; the partial sums meet by an xor butterfly per wave and then wave by wave.
__global__ __launch_bounds__(BASE_THREADS) void k_site_baseline(const double* __restrict__ framework, const double* __restrict__ interactions,
                                                                const uint16_t* __restrict__ pop, int n, int m, double tail,
                                                                double* __restrict__ out, double* __restrict__ energy)
{
    extern __shared__ uint16_t s_pop[];
    __shared__ double s_f[BASE_THREADS / 64], s_e[BASE_THREADS / 64];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
    const uint16_t* gpop = pop + (size_t)c * (size_t)m;
    for (int j = tid; j < m; j += BASE_THREADS) s_pop[j] = gpop[j];
    __syncthreads();
    double f = 0.0, e = 0.0;
    for (int i = tid; i < m; i += BASE_THREADS) {
        const size_t pi = (size_t)s_pop[i];
        f += framework[pi];
        const double* __restrict__ row = interactions + pi * (size_t)n;
        for (int j = i + 1; j < m; ++j) e += row[s_pop[j]];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        f += __shfl_xor(f, o);
        e += __shfl_xor(e, o);
    }
    if ((tid & 63) == 0) { s_f[tid >> 6] = f; s_e[tid >> 6] = e; }
    __syncthreads();
    if (tid == 0) {
        double F = 0.0, E = 0.0;
        for (int w = 0; w < BASE_THREADS / 64; ++w) { F += s_f[w]; E += s_e[w]; }
        const double total = (tail + F) + E;
        if (out) out[c] = total;
        if (energy) energy[c] = total;
    }
}

struct SiteRecorder {
    int64_t every = 0, origin = 0, capacity = 0, frames = 0;
    bool track_min = false;
    uint16_t* d_frames = nullptr;
    ceg_site_frame_record_t* d_frec = nullptr;
    uint16_t* d_best = nullptr;
    double* d_mine = nullptr;
    int64_t* d_mink = nullptr;
};

void recorder_free(SiteRecorder* r)
{
    if (!r) return;
    for (void* p : {(void*)r->d_frames, (void*)r->d_frec, (void*)r->d_best, (void*)r->d_mine, (void*)r->d_mink})
        if (p) (void)hipFree(p);
    delete r;
}

struct SiteTempering {                           // ceg_site_group_set_tempering: L = K / rungs ladders
    int rungs = 0;
    double* d_cdf = nullptr;                     // [R-1]
    uint32_t* d_lstream = nullptr;               // [L]
    int64_t *d_attempted = nullptr, *d_accepted = nullptr;   // [L][R-1]
    int32_t* d_replica = nullptr;                // [K]
};

void tempering_free(SiteTempering* t)
{
    if (!t) return;
    for (void* p : {(void*)t->d_cdf, (void*)t->d_lstream, (void*)t->d_attempted, (void*)t->d_accepted, (void*)t->d_replica})
        if (p) (void)hipFree(p);
    delete t;
}

// the first cycle >= from at whose end a frame is due (every > 0)
int64_t first_due(const SiteRecorder* r, int64_t from)
{
    const int64_t lo = std::max(from, r->origin);
    return r->origin + (lo - r->origin + r->every - 1) / r->every * r->every;
}

// frames due at the ends of the cycles [cycle0, cycle0 + ncycles)
int64_t frames_due(const SiteRecorder* r, int64_t cycle0, int64_t ncycles)
{
    if (r->every <= 0 || ncycles <= 0) return 0;
    const int64_t end = cycle0 + ncycles, first = first_due(r, cycle0);
    return first < end ? (end - 1 - first) / r->every + 1 : 0;
}

int64_t env_int(const char* name, int64_t fallback, int64_t lo, int64_t hi)
{
    const char* e = getenv(name);
    if (!e || !*e) return fallback;
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return (end && *end == 0 && v >= lo && v <= hi) ? (int64_t)v : fallback;
}

// every site < n and no site twice within a chain; `seen` is scratch of n entries
int check_populations(const uint16_t* pop, int n, int m, int k)
{
    std::vector<int32_t> seen((size_t)n, -1);
    for (int c = 0; c < k; ++c)
        for (int j = 0; j < m; ++j) {
            const int s = (int)pop[(size_t)c * m + j];
            if (s >= n) return fail(CEG_ERR_INVALID, "site group: chain %d, molecule %d sits on site %d of %d", c, j, s, n);
            if (seen[s] == c) return fail(CEG_ERR_INVALID, "site group: chain %d uses site %d twice", c, s);
            seen[s] = c;
        }
    return CEG_OK;
}

}  // namespace

struct ceg_site_group {
    int device = 0, n = 0, m = 0, k = 0;
    double tail = 0.0;
    bool own_tables = false, poisoned = false;
    const double *d_fw = nullptr, *d_inter = nullptr;
    uint16_t* d_pop = nullptr;
    double *d_energy = nullptr, *d_delta = nullptr, *d_scratch = nullptr;
    int64_t *d_attempted = nullptr, *d_accepted = nullptr;
    hipStream_t stream = nullptr;
    SiteRecorder* rec = nullptr;
    SiteTempering* pt = nullptr;
};

namespace {

void group_free(ceg_site_group* g)
{
    if (!g) return;
    recorder_free(g->rec);
    tempering_free(g->pt);
    if (g->own_tables)
        for (const void* p : {(const void*)g->d_fw, (const void*)g->d_inter})
            if (p) (void)hipFree(const_cast<void*>(p));
    for (void* p : {(void*)g->d_pop, (void*)g->d_energy, (void*)g->d_delta, (void*)g->d_scratch, (void*)g->d_attempted, (void*)g->d_accepted})
        if (p) (void)hipFree(p);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

size_t pop_lds(int m) { return ((size_t)m * sizeof(uint16_t) + 15) & ~(size_t)15; }

// baseline of every chain into `out` and / or the running energies (device pointers); enqueued on the group's stream
hipError_t launch_baseline(ceg_site_group* g, double* d_out, double* d_energy)
{
    hipLaunchKernelGGL(k_site_baseline, dim3((unsigned)g->k), dim3(BASE_THREADS), pop_lds(g->m), g->stream, g->d_fw, g->d_inter, g->d_pop, g->n, g->m,
                       g->tail, d_out, d_energy);
    return hipGetLastError();
}

int poisoned(ceg_site_group* g, const char* what)
{
    g->poisoned = true;
    return fail(CEG_ERR_HIP, "site group: %s failed: %s; the group is inconsistent", what, hipGetErrorString(hipGetLastError()));
}

// replica[l R + r] = r: every configuration sits on its own rung (the stream is idle: a synchronous copy)
bool identity_replica(ceg_site_group* g)
{
    std::vector<int32_t> id((size_t)g->k);
    for (int c = 0; c < g->k; ++c) id[(size_t)c] = c % g->pt->rungs;
    return hipMemcpy(g->pt->d_replica, id.data(), sizeof(int32_t) * id.size(), hipMemcpyHostToDevice) == hipSuccess;
}

// dynamic LDS of k_site_sweep_pt beside its static tables; false with the figures in *need / *have where it does not fit
bool ladder_lds_fits(const ceg_site_group* g, int rungs, size_t* need, size_t* have)
{
    hipFuncAttributes fa{};
    int limit = 0;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_site_sweep_pt)) != hipSuccess ||
        hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, g->device) != hipSuccess)
        limit = 0;
    *need = (size_t)rungs * pop_lds(g->m) + fa.sharedSizeBytes;
    *have = (size_t)std::max(limit, 0);
    return *need <= *have;
}

#define SITE_ENTER(g)                                                                                                     \
    if (!(g)) return fail(CEG_ERR_INVALID, "site group: bad argument");                                                   \
    if ((g)->poisoned) return fail(CEG_ERR_HIP, "site group: the group is inconsistent after a failed call: destroy it"); \
    ceg_host::DeviceGuard guard((g)->device);                                                                             \
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice failed")

}  // namespace

extern "C" int ceg_site_group_create(int32_t device, int32_t n, int32_t m, int32_t k, const double* framework, const double* interactions,
                                     int32_t tables_on_device, const uint16_t* populations, double tailcorrection, ceg_site_group_t** group)
{
    if (!group) return fail(CEG_ERR_INVALID, "site group: bad argument");
    *group = nullptr;
    if (!framework || !interactions || !populations) return fail(CEG_ERR_INVALID, "site group: a table or the populations are missing");
    if (n < 1 || n > 65535) return fail(CEG_ERR_INVALID, "site group: n = %d sites, outside 1..65535 (sites are UInt16)", n);
    if (m < 1 || m > CEG_SITE_MAX_MOLECULES) return fail(CEG_ERR_INVALID, "site group: m = %d molecules, outside 1..%d", m, CEG_SITE_MAX_MOLECULES);
    if (k < 1) return fail(CEG_ERR_INVALID, "site group: K = %d chains", k);
    if (!std::isfinite(tailcorrection)) return fail(CEG_ERR_INVALID, "site group: the tail correction is not finite");
    if (int rc = check_populations(populations, n, m, k)) return rc;
    const int64_t limit_mb = env_int("CEG_HIP_SITE_TABLE_LIMIT_MB", 2048, 1, (int64_t)1 << 30);
    const size_t table_bytes = (size_t)n * (size_t)n * sizeof(double);
    if (table_bytes > (size_t)limit_mb << 20)
        return fail(CEG_ERR_UNSUPPORTED, "site group: interactions of %d sites take %zu bytes, above CEG_HIP_SITE_TABLE_LIMIT_MB = %lld MiB", n, table_bytes,
                    (long long)limit_mb);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(CEG_ERR_NO_DEVICE, "site group: device %d is not present", device);
    ceg_host::DeviceGuard guard(device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice failed");
    ceg_site_group* g = new ceg_site_group();
    g->device = device; g->n = n; g->m = m; g->k = k; g->tail = tailcorrection;
    const size_t K = (size_t)k, pop_bytes = K * (size_t)m * sizeof(uint16_t);
    bool ok = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess;
    if (tables_on_device) {
        g->d_fw = framework;
        g->d_inter = interactions;
    } else {
        g->own_tables = true;
        ok = ok && hipMalloc((void**)&g->d_fw, sizeof(double) * (size_t)n) == hipSuccess && hipMalloc((void**)&g->d_inter, table_bytes) == hipSuccess &&
             hipMemcpy((void*)g->d_fw, framework, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy((void*)g->d_inter, interactions, table_bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && hipMalloc((void**)&g->d_pop, pop_bytes) == hipSuccess && hipMalloc((void**)&g->d_energy, sizeof(double) * K) == hipSuccess &&
         hipMalloc((void**)&g->d_delta, sizeof(double) * K) == hipSuccess && hipMalloc((void**)&g->d_scratch, sizeof(double) * K) == hipSuccess &&
         hipMalloc((void**)&g->d_attempted, sizeof(int64_t) * K) == hipSuccess && hipMalloc((void**)&g->d_accepted, sizeof(int64_t) * K) == hipSuccess &&
         hipMemcpy(g->d_pop, populations, pop_bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset(g->d_delta, 0, sizeof(double) * K) == hipSuccess &&
         hipMemset(g->d_attempted, 0, sizeof(int64_t) * K) == hipSuccess && hipMemset(g->d_accepted, 0, sizeof(int64_t) * K) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess && launch_baseline(g, nullptr, g->d_energy) == hipSuccess && hipStreamSynchronize(g->stream) == hipSuccess;
    if (!ok) {
        const int rc = fail(CEG_ERR_HIP, "site group: could not set up the device state: %s", hipGetErrorString(hipGetLastError()));
        group_free(g);
        return rc;
    }
    *group = g;
    return CEG_OK;
}

extern "C" int ceg_site_group_destroy(ceg_site_group_t* g)
{
    if (!g) return CEG_OK;
    ceg_host::DeviceGuard guard(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    group_free(g);
    return CEG_OK;
}

extern "C" int ceg_site_group_baseline(ceg_site_group_t* g, double* out)
{
    SITE_ENTER(g);
    if (!out) return fail(CEG_ERR_INVALID, "site group: bad argument");
    if (launch_baseline(g, g->d_scratch, nullptr) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) return poisoned(g, "the baseline launch");
    HIP_TRY(hipMemcpy(out, g->d_scratch, sizeof(double) * (size_t)g->k, hipMemcpyDeviceToHost));
    return CEG_OK;
}

extern "C" int ceg_site_group_rebase(ceg_site_group_t* g)
{
    SITE_ENTER(g);
    if (launch_baseline(g, nullptr, g->d_energy) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) return poisoned(g, "the baseline launch");
    return CEG_OK;
}

extern "C" int ceg_site_group_get_populations(ceg_site_group_t* g, uint16_t* out)
{
    SITE_ENTER(g);
    if (!out) return fail(CEG_ERR_INVALID, "site group: bad argument");
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(out, g->d_pop, (size_t)g->k * (size_t)g->m * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return CEG_OK;
}

extern "C" int ceg_site_group_set_populations(ceg_site_group_t* g, const uint16_t* populations)
{
    SITE_ENTER(g);
    if (!populations) return fail(CEG_ERR_INVALID, "site group: bad argument");
    if (int rc = check_populations(populations, g->n, g->m, g->k)) return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (hipMemcpy(g->d_pop, populations, (size_t)g->k * (size_t)g->m * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) return poisoned(g, "the upload of the populations");
    if (launch_baseline(g, nullptr, g->d_energy) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) return poisoned(g, "the baseline launch");
    if (g->pt && !identity_replica(g)) return poisoned(g, "the reset of the replica map");
    return CEG_OK;
}

namespace {

struct GroupedCall {                             // what ceg_site_group_sweep_grouped adds to a sweep
    int32_t restart;
    ceg_site_grouped_record_t* out;              // [ncycles][K] host, or nullptr
};

// ceg_site_group_sweep_cycles (grouped == nullptr) and ceg_site_group_sweep_grouped: one validation, one staging, one launch loop
int sweep_call(ceg_site_group_t* g, const ceg_site_params_t* params, const ceg_site_cycles_t* cy, ceg_site_stats_t* stats_out,
               ceg_site_cycle_record_t* cycles_out, ceg_site_record_t* log_out, const GroupedCall* grouped)
{
    SITE_ENTER(g);
    if (grouped && g->pt) return fail(CEG_ERR_UNSUPPORTED, "site sweep: grouped cycles while tempering is installed (run_parallel_tempering has no group cycles)");
    if (grouped && grouped->restart != 0 && grouped->restart != 1) return fail(CEG_ERR_INVALID, "site sweep: restart = %d, outside {0, 1}", grouped->restart);
    if (!params || !cy) return fail(CEG_ERR_INVALID, "site sweep: params or cycles are missing");
    if (cy->ncycles < 0 || cy->steps_per_cycle < 1) return fail(CEG_ERR_INVALID, "site sweep: ncycles >= 0 and steps_per_cycle >= 1");
    const size_t K = (size_t)g->k;
    const int64_t top = INT64_MAX;
    if (cy->cycle0 < 0 ? false : cy->ncycles > top - cy->cycle0) return fail(CEG_ERR_INVALID, "site sweep: cycle0 + ncycles is beyond 2^63 - 1");
    if (cy->ncycles > 0 && cy->steps_per_cycle > top / cy->ncycles) return fail(CEG_ERR_INVALID, "site sweep: ncycles * steps_per_cycle is beyond 2^63 - 1");
    const int64_t total = cy->ncycles * cy->steps_per_cycle;
    if (params->first_step > (uint64_t)top || total > top - (int64_t)params->first_step) return fail(CEG_ERR_INVALID, "site sweep: first_step + the steps is beyond 2^63 - 1");
    if (cy->ncycles > CEG_MC_CYCLES_MAX_RECORDS / (int64_t)K) return fail(CEG_ERR_INVALID, "site sweep: more than CEG_MC_CYCLES_MAX_RECORDS cycle records (ncycles * K)");
    if (log_out && total > CEG_MC_CYCLES_MAX_RECORDS / (int64_t)K) return fail(CEG_ERR_INVALID, "site sweep: more than CEG_MC_CYCLES_MAX_RECORDS log records (steps * K)");
    if (cy->ncycles > 0) {
        if (!cy->temperature) return fail(CEG_ERR_INVALID, "site sweep: the temperatures are missing");
        for (size_t e = 0; e < (size_t)cy->ncycles * K; ++e)
            if (!(std::isfinite(cy->temperature[e]) && cy->temperature[e] > 0.0))
                return fail(CEG_ERR_INVALID, "site sweep: the temperature of cycle %lld, chain %lld is not finite and > 0", (long long)(e / K), (long long)(e % K));
        if (g->pt)                               // the reference sorts Ts: inside a ladder the rungs' temperatures rise strictly
            for (size_t e = 0; e < (size_t)cy->ncycles * K; ++e)
                if (e % K % (size_t)g->pt->rungs != 0 && !(cy->temperature[e - 1] < cy->temperature[e]))
                    return fail(CEG_ERR_INVALID, "site sweep: cycle %lld, chain %lld: the temperatures of a ladder must rise strictly with the rung",
                                (long long)(e / K), (long long)(e % K));
    }
    const int64_t per_launch = env_int("CEG_HIP_SITE_STEPS_PER_LAUNCH", 4096, 1, (int64_t)1 << 30);

    double* d_temp = nullptr;
    uint32_t* d_stream = nullptr;
    ceg_site_cycle_record_t* d_cyc = nullptr;
    ceg_site_record_t* d_log = nullptr;
    uint16_t* d_p0 = nullptr;                    // grouped: the cycle in flight (SiteGrouped)
    double* d_saved = nullptr;                   // grouped: [3][K] E0, D0, Er
    int64_t* d_hops = nullptr;
    ceg_site_grouped_record_t* d_grouped = nullptr;
    auto release = [&]() {
        for (void* p : {(void*)d_temp, (void*)d_stream, (void*)d_cyc, (void*)d_log, (void*)d_p0, (void*)d_saved, (void*)d_hops, (void*)d_grouped})
            if (p) (void)hipFree(p);
    };
    if (total > 0) {
        std::vector<uint32_t> ids(K);
        for (size_t c = 0; c < K; ++c) ids[c] = params->stream_id ? params->stream_id[c] : (uint32_t)c;
        const size_t ncyc = (size_t)cy->ncycles;
        bool ok = hipMalloc((void**)&d_temp, sizeof(double) * ncyc * K) == hipSuccess && hipMalloc((void**)&d_stream, sizeof(uint32_t) * K) == hipSuccess &&
                  (!cycles_out || hipMalloc((void**)&d_cyc, sizeof(ceg_site_cycle_record_t) * ncyc * K) == hipSuccess) &&
                  (!log_out || hipMalloc((void**)&d_log, sizeof(ceg_site_record_t) * (size_t)total * K) == hipSuccess) &&
                  hipMemcpy(d_temp, cy->temperature, sizeof(double) * ncyc * K, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(d_stream, ids.data(), sizeof(uint32_t) * K, hipMemcpyHostToDevice) == hipSuccess;
        if (grouped)
            ok = ok && hipMalloc((void**)&d_p0, K * (size_t)g->m * sizeof(uint16_t)) == hipSuccess && hipMalloc((void**)&d_saved, sizeof(double) * 3 * K) == hipSuccess &&
                 hipMalloc((void**)&d_hops, sizeof(int64_t) * K) == hipSuccess &&
                 (!grouped->out || hipMalloc((void**)&d_grouped, sizeof(ceg_site_grouped_record_t) * ncyc * K) == hipSuccess);
        if (!ok) {
            const int rc = fail(CEG_ERR_HIP, "site sweep: could not stage the call: %s", hipGetErrorString(hipGetLastError()));
            release();
            return rc;
        }
        SiteSweep S{};
        S.framework = g->d_fw; S.interactions = g->d_inter; S.pop = g->d_pop;
        S.energy = g->d_energy; S.delta = g->d_delta; S.attempted = g->d_attempted; S.accepted = g->d_accepted;
        S.temperature = d_temp; S.stream = d_stream; S.cyc = d_cyc; S.log = d_log;
        S.seed = params->seed; S.first_step = params->first_step;
        S.cycle0 = cy->cycle0; S.spc = cy->steps_per_cycle;
        S.n = g->n; S.m = g->m; S.k = g->k;
        if (const SiteRecorder* r = g->rec) {
            S.rec = SiteRecorderView{r->every, r->origin, r->capacity, r->frames, r->every > 0 ? first_due(r, cy->cycle0) : 0, r->d_frames, r->d_frec,
                                     r->d_best, r->d_mine, r->d_mink, r->track_min ? 1 : 0};
        }
        for (int64_t t0 = 0; t0 < total; t0 += per_launch) {
            S.t0 = t0;
            S.t1 = std::min(total, t0 + per_launch);
            if (grouped) {
                const SiteGrouped G{d_p0, d_saved, d_saved + K, d_saved + 2 * K, d_hops, d_grouped, g->tail, grouped->restart, (int32_t)(pop_lds(g->m) / sizeof(uint16_t))};
                hipLaunchKernelGGL(k_site_sweep_grouped, dim3((unsigned)g->k), dim3(64), 2 * pop_lds(g->m), g->stream, S, G);
            } else if (const SiteTempering* pt = g->pt) {
                const SiteLadders P{pt->d_cdf, pt->d_lstream, pt->d_attempted, pt->d_accepted, pt->d_replica, pt->rungs, (int32_t)(pop_lds(g->m) / sizeof(uint16_t))};
                hipLaunchKernelGGL(k_site_sweep_pt, dim3((unsigned)(g->k / pt->rungs)), dim3(64u * (unsigned)pt->rungs), (size_t)pt->rungs * pop_lds(g->m), g->stream, S, P);
            } else
                hipLaunchKernelGGL(k_site_sweep, dim3((unsigned)g->k), dim3(64), pop_lds(g->m), g->stream, S);
            if (hipGetLastError() != hipSuccess) {
                release();
                return poisoned(g, "a sweep launch");
            }
        }
        if (hipStreamSynchronize(g->stream) != hipSuccess) {
            release();
            return poisoned(g, "the sweep");
        }
        if (g->rec) g->rec->frames = std::min(g->rec->capacity, g->rec->frames + frames_due(g->rec, cy->cycle0, cy->ncycles));
        ok = (!cycles_out || hipMemcpy(cycles_out, d_cyc, sizeof(ceg_site_cycle_record_t) * ncyc * K, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!log_out || hipMemcpy(log_out, d_log, sizeof(ceg_site_record_t) * (size_t)total * K, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!d_grouped || hipMemcpy(grouped->out, d_grouped, sizeof(ceg_site_grouped_record_t) * ncyc * K, hipMemcpyDeviceToHost) == hipSuccess);
        release();
        if (!ok) return fail(CEG_ERR_HIP, "site sweep: D2H of the records failed");
    }
    if (stats_out) {
        std::vector<double> e(K), d(K);
        std::vector<int64_t> at(K), ac(K);
        HIP_TRY(hipStreamSynchronize(g->stream));
        HIP_TRY(hipMemcpy(e.data(), g->d_energy, sizeof(double) * K, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(d.data(), g->d_delta, sizeof(double) * K, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(at.data(), g->d_attempted, sizeof(int64_t) * K, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ac.data(), g->d_accepted, sizeof(int64_t) * K, hipMemcpyDeviceToHost));
        for (size_t c = 0; c < K; ++c) stats_out[c] = ceg_site_stats_t{at[c], ac[c], d[c], e[c]};
    }
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_site_group_sweep_cycles(ceg_site_group_t* g, const ceg_site_params_t* params, const ceg_site_cycles_t* cy, ceg_site_stats_t* stats_out,
                                           ceg_site_cycle_record_t* cycles_out, ceg_site_record_t* log_out)
{
    return sweep_call(g, params, cy, stats_out, cycles_out, log_out, nullptr);
}

extern "C" int ceg_site_group_sweep_grouped(ceg_site_group_t* g, const ceg_site_params_t* params, const ceg_site_cycles_t* cy, int32_t restart,
                                            ceg_site_stats_t* stats_out, ceg_site_cycle_record_t* cycles_out, ceg_site_record_t* log_out,
                                            ceg_site_grouped_record_t* grouped_out)
{
    const GroupedCall call{restart, grouped_out};
    return sweep_call(g, params, cy, stats_out, cycles_out, log_out, &call);
}

extern "C" int ceg_site_group_set_recorder(ceg_site_group_t* g, const ceg_site_recorder_t* spec)
{
    SITE_ENTER(g);
    if (spec && (spec->every < 0 || spec->origin < 0 || spec->frame_capacity < 0))
        return fail(CEG_ERR_INVALID, "site recorder: every, origin and frame_capacity must be >= 0");
    const size_t K = (size_t)g->k, row = K * (size_t)g->m * sizeof(uint16_t);
    if (spec && ((double)spec->frame_capacity + 1.0) * (double)(row + K * sizeof(ceg_site_frame_record_t)) > (double)CEG_MC_RECORDER_MAX_BYTES)
        return fail(CEG_ERR_INVALID, "site recorder: the store is too large (more than CEG_MC_RECORDER_MAX_BYTES over all frames and chains)");
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (!spec) {
        recorder_free(g->rec);
        g->rec = nullptr;
        return CEG_OK;
    }
    SiteRecorder* r = new SiteRecorder();
    r->every = spec->every; r->origin = spec->origin; r->capacity = spec->frame_capacity; r->track_min = spec->track_min != 0;
    const size_t cap = (size_t)r->capacity;
    std::vector<int64_t> never(K, -1);
    bool ok = hipMalloc((void**)&r->d_frames, std::max(cap * row, (size_t)16)) == hipSuccess &&
              hipMalloc((void**)&r->d_frec, std::max(cap * K * sizeof(ceg_site_frame_record_t), (size_t)16)) == hipSuccess &&
              hipMalloc((void**)&r->d_best, row) == hipSuccess && hipMalloc((void**)&r->d_mine, sizeof(double) * K) == hipSuccess &&
              hipMalloc((void**)&r->d_mink, sizeof(int64_t) * K) == hipSuccess && hipMemset(r->d_frames, 0, std::max(cap * row, (size_t)16)) == hipSuccess &&
              hipMemset(r->d_frec, 0, std::max(cap * K * sizeof(ceg_site_frame_record_t), (size_t)16)) == hipSuccess &&
              hipMemcpy(r->d_best, g->d_pop, row, hipMemcpyDeviceToDevice) == hipSuccess &&
              hipMemcpy(r->d_mine, g->d_energy, sizeof(double) * K, hipMemcpyDeviceToDevice) == hipSuccess &&
              hipMemcpy(r->d_mink, never.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        const int rc = fail(CEG_ERR_HIP, "site recorder: could not set up the device buffers: %s", hipGetErrorString(hipGetLastError()));
        recorder_free(r);
        return rc;
    }
    recorder_free(g->rec);
    g->rec = r;
    return CEG_OK;
}

extern "C" int ceg_site_group_recorder_read(ceg_site_group_t* g, int64_t first_frame, int64_t nframes, ceg_site_frame_record_t* records_out,
                                            uint16_t* populations_out, int64_t* frames_out)
{
    SITE_ENTER(g);
    const SiteRecorder* r = g->rec;
    if (!r) return fail(CEG_ERR_INVALID, "site recorder: the group has no recorder (ceg_site_group_set_recorder)");
    if (first_frame < 0 || nframes < 0 || first_frame > r->frames || nframes > r->frames - first_frame)
        return fail(CEG_ERR_INVALID, "site recorder: the window [first_frame, first_frame + nframes) lies outside the %lld frames held", (long long)r->frames);
    HIP_TRY(hipStreamSynchronize(g->stream));
    const size_t K = (size_t)g->k, row = K * (size_t)g->m, f = (size_t)first_frame, nf = (size_t)nframes;
    if (records_out && nf) HIP_TRY(hipMemcpy(records_out, r->d_frec + f * K, nf * K * sizeof(ceg_site_frame_record_t), hipMemcpyDeviceToHost));
    if (populations_out && nf) HIP_TRY(hipMemcpy(populations_out, r->d_frames + f * row, nf * row * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (frames_out) *frames_out = r->frames;
    return CEG_OK;
}

extern "C" int ceg_site_group_recorder_min(ceg_site_group_t* g, int64_t* mink_out, double* mine_out, uint16_t* populations_out)
{
    SITE_ENTER(g);
    const SiteRecorder* r = g->rec;
    if (!r) return fail(CEG_ERR_INVALID, "site recorder: the group has no recorder (ceg_site_group_set_recorder)");
    if (!r->track_min) return fail(CEG_ERR_INVALID, "site recorder: the recorder keeps no minimum (track_min)");
    HIP_TRY(hipStreamSynchronize(g->stream));
    const size_t K = (size_t)g->k;
    if (mink_out) HIP_TRY(hipMemcpy(mink_out, r->d_mink, sizeof(int64_t) * K, hipMemcpyDeviceToHost));
    if (mine_out) HIP_TRY(hipMemcpy(mine_out, r->d_mine, sizeof(double) * K, hipMemcpyDeviceToHost));
    if (populations_out) HIP_TRY(hipMemcpy(populations_out, r->d_best, K * (size_t)g->m * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return CEG_OK;
}

extern "C" int ceg_site_group_set_tempering(ceg_site_group_t* g, const ceg_site_tempering_t* spec)
{
    SITE_ENTER(g);
    if (!spec) {
        HIP_TRY(hipStreamSynchronize(g->stream));
        tempering_free(g->pt);
        g->pt = nullptr;
        return CEG_OK;
    }
    const int R = spec->rungs;
    if (R < 2 || R > PT_MAX_RUNGS) return fail(CEG_ERR_INVALID, "site tempering: %d rungs, outside 2..%d", R, PT_MAX_RUNGS);
    if (g->k % R != 0) return fail(CEG_ERR_INVALID, "site tempering: K = %d chains are no whole number of ladders of %d rungs", g->k, R);
    if (spec->_reserved != 0) return fail(CEG_ERR_INVALID, "site tempering: _reserved must be 0");
    if (!spec->pair_cdf) return fail(CEG_ERR_INVALID, "site tempering: the pair table is missing");
    for (int j = 0; j < R - 1; ++j) {
        const double v = spec->pair_cdf[j];
        if (!(std::isfinite(v) && v >= 0.0 && v <= 1.0) || (j > 0 && v < spec->pair_cdf[j - 1]))
            return fail(CEG_ERR_INVALID, "site tempering: pair_cdf[%d] is not finite, outside [0, 1] or below the entry before it", j);
    }
    size_t need = 0, have = 0;
    if (!ladder_lds_fits(g, R, &need, &have))
        return fail(CEG_ERR_UNSUPPORTED, "site tempering: %d populations of %d molecules take %zu bytes of LDS, the device gives a workgroup %zu", R, g->m, need, have);
    const size_t K = (size_t)g->k, L = K / (size_t)R, npairs = L * (size_t)(R - 1);
    std::vector<uint32_t> ls(L);
    for (size_t l = 0; l < L; ++l) ls[l] = spec->ladder_stream ? spec->ladder_stream[l] : (uint32_t)l;
    HIP_TRY(hipStreamSynchronize(g->stream));
    SiteTempering* t = new SiteTempering();
    t->rungs = R;
    SiteTempering* old = g->pt;
    g->pt = t;                                   // (identity_replica writes the group's)
    const bool ok = hipMalloc((void**)&t->d_cdf, sizeof(double) * (size_t)(R - 1)) == hipSuccess && hipMalloc((void**)&t->d_lstream, sizeof(uint32_t) * L) == hipSuccess &&
                    hipMalloc((void**)&t->d_attempted, sizeof(int64_t) * npairs) == hipSuccess && hipMalloc((void**)&t->d_accepted, sizeof(int64_t) * npairs) == hipSuccess &&
                    hipMalloc((void**)&t->d_replica, sizeof(int32_t) * K) == hipSuccess &&
                    hipMemcpy(t->d_cdf, spec->pair_cdf, sizeof(double) * (size_t)(R - 1), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(t->d_lstream, ls.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(t->d_attempted, 0, sizeof(int64_t) * npairs) == hipSuccess && hipMemset(t->d_accepted, 0, sizeof(int64_t) * npairs) == hipSuccess &&
                    identity_replica(g) && hipDeviceSynchronize() == hipSuccess &&
                    // (above 64 KiB of dynamic LDS the runtime wants to be told; the size was checked against the device's limit)
                    ((size_t)R * pop_lds(g->m) <= 64 * 1024 ||
                     hipFuncSetAttribute(reinterpret_cast<const void*>(k_site_sweep_pt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)R * pop_lds(g->m))) == hipSuccess);
    if (!ok) {
        const int rc = fail(CEG_ERR_HIP, "site tempering: could not set up the device buffers: %s", hipGetErrorString(hipGetLastError()));
        g->pt = old;
        tempering_free(t);
        return rc;
    }
    tempering_free(old);
    return CEG_OK;
}

extern "C" int ceg_site_group_tempering_read(ceg_site_group_t* g, int64_t* attempted, int64_t* accepted, int32_t* replica)
{
    SITE_ENTER(g);
    const SiteTempering* t = g->pt;
    if (!t) return fail(CEG_ERR_INVALID, "site tempering: the group has no tempering (ceg_site_group_set_tempering)");
    HIP_TRY(hipStreamSynchronize(g->stream));
    const size_t K = (size_t)g->k, npairs = K / (size_t)t->rungs * (size_t)(t->rungs - 1);
    if (attempted) HIP_TRY(hipMemcpy(attempted, t->d_attempted, sizeof(int64_t) * npairs, hipMemcpyDeviceToHost));
    if (accepted) HIP_TRY(hipMemcpy(accepted, t->d_accepted, sizeof(int64_t) * npairs, hipMemcpyDeviceToHost));
    if (replica) HIP_TRY(hipMemcpy(replica, t->d_replica, sizeof(int32_t) * K, hipMemcpyDeviceToHost));
    return CEG_OK;
}

// ------------------------------------------------------------------ the tables (sitehopping.jl:41-82, telescoped)
namespace {

using namespace ceg_mcs;
typedef double double4_t __attribute__((ext_vector_type(4)));

// Workgroup i: site i as ceg_mc_trial_insert sees a placement in the guest-free box -- framework_interactions atom by atom (one grid
// corner per thread, montecarlo.jl:490-504) and the structure factor S_i over the handle's k-vectors (molecule_sf, the trial row's),
// kept as St[q][i] for the contraction.  rec = 2 sum kf Re(conj(F) S_i) + sum kf |S_i|^2 + off1; framework = (fv + fd) + rec.
__global__ __launch_bounds__(MC_THREADS) void k_site_points(const McView v, const McMolecule nm, const double* __restrict__ positions, int n_pad, int stride,
                                                            double off1, double2* __restrict__ St, double* __restrict__ framework, double* __restrict__ recip)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_pos[MC_MAX_ATOMS * 3];
    __shared__ double s_q[MC_MAX_ATOMS];
    __shared__ int32_t s_kind[MC_MAX_ATOMS];
    __shared__ double s_red[MC_THREADS / 64][4];
    const int tid = threadIdx.x, m = nm.m;
    const size_t i = blockIdx.x;
    if (tid < 3 * m) s_pos[tid] = positions[i * (size_t)m * 3 + tid];
    if (tid < m) {
        s_kind[tid] = nm.kinds[tid];
        s_q[tid] = v.kind_charge[nm.kinds[tid]];
    }
    __syncthreads();
    double fv = 0.0, fd = 0.0, rs = 0.0, ss = 0.0;
    {
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
    if (v.nk > 0) {
        double2* tab = reinterpret_cast<double2*>(s_raw);
        fill_tables(v, s_pos, m, tab, stride, tid, MC_THREADS);
        __syncthreads();
        for (int64_t q = tid; q < v.nk; q += MC_THREADS) {
            const double2 S = molecule_sf(v, tab, stride, s_q, m, q);
            const double2 F = v.sf_fw[q];
            const double kf = v.kf[q];
            St[(size_t)q * (size_t)n_pad + i] = S;
            rs += kf * (F.x * S.x + F.y * S.y);
            ss += kf * (S.x * S.x + S.y * S.y);
        }
    }
    double vals[4] = {fv, fd, rs, ss};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vals[c] += __shfl_xor(vals[c], o);
    if ((tid & 63) == 0)
        for (int c = 0; c < 4; ++c) s_red[tid >> 6][c] = vals[c];
    __syncthreads();
    if (tid == 0) {
        double tot[4] = {0, 0, 0, 0};
        for (int w = 0; w < MC_THREADS / 64; ++w)
            for (int c = 0; c < 4; ++c) tot[c] += s_red[w][c];
        const double rec = (2.0 * tot[2] + tot[3]) + off1;
        if (recip) recip[i] = rec;
        framework[i] = (tot[0] + tot[1]) + rec;
    }
}

// Wave (ti, tj), ti <= tj: out[i][j] = 2 sum_k kf_k Re(S_i conj(S_j)) for the 16 x 16 sites of the tile with i < j.
// MFMA operand maps (v_mfma_f64_16x16x4): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D register v: row
// (lane >> 4) + 4 v, column lane & 15.  St is [nk][n_pad], n_pad a multiple of 16 and zero beyond n: every load is in bounds.
__global__ __launch_bounds__(64) void k_site_recip_pairs(const double2* __restrict__ St, const double* __restrict__ kf, int nk, int n, int n_pad,
                                                         double* __restrict__ out)
{
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (ti > tj) return;
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int i0 = 16 * ti, j0 = 16 * tj;
    double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < nk; kc += 4) {
        const int k = kc + lk;
        const bool in = k < nk;
        const size_t kk = in ? (size_t)k : 0;
        const double w = in ? 2.0 * kf[kk] : 0.0;
        const double2 a = St[kk * (size_t)n_pad + i0 + li], b = St[kk * (size_t)n_pad + j0 + li];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w * a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w * a.y, b.y, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + lk + 4 * r, j = j0 + li;
        if (i < j && j < n) out[(size_t)i * (size_t)n + j] = acc[r];
    }
}

// Workgroup (ti, tj), ti <= tj, thread (a, b) = site pair (16 ti + a, 16 tj + b) with i < j: the molecule-pair sum of
// single_contribution_vdw (energy.jl:407-427) -- the literal pair distance and the exact rule energies of the trial row -- plus the
// reciprocal term already in out[i][j] (with_recip) plus off2, written to [i][j] and [j][i]; the diagonal gets 1e100.
__global__ __launch_bounds__(256) void k_site_real_pairs(const McView v, const McMolecule nm, const double* __restrict__ positions, int n, int with_recip,
                                                         double off2, double* __restrict__ out)
{
    __shared__ double s_pi[16][MC_MAX_ATOMS * 3], s_pj[16][MC_MAX_ATOMS * 3];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (ti > tj) return;
    const int tid = threadIdx.x, m = nm.m;
    for (int e = tid; e < 16 * 3 * m; e += 256) {
        const int s = e / (3 * m), c = e - s * 3 * m;
        const int si = 16 * ti + s, sj = 16 * tj + s;
        s_pi[s][c] = si < n ? positions[(size_t)si * (size_t)m * 3 + c] : 0.0;
        s_pj[s][c] = sj < n ? positions[(size_t)sj * (size_t)m * 3 + c] : 0.0;
    }
    __syncthreads();
    const int a = tid >> 4, b = tid & 15;
    const int i = 16 * ti + a, j = 16 * tj + b;
    if (i >= n || j >= n || i > j) return;
    if (i == j) {
        out[(size_t)i * (size_t)n + i] = 1e100;
        return;
    }
    const double* M = v.mat;
    const double* I = v.invmat;
    double inter = 0.0;
    for (int aj = 0; aj < m; ++aj) {
        const double ax = s_pj[b][3 * aj], ay = s_pj[b][3 * aj + 1], az = s_pj[b][3 * aj + 2];
        const int kind1 = nm.kinds[aj];
        for (int ai = 0; ai < m; ++ai) {
            double r2;
            {
#pragma clang fp contract(off)
                const double dx = s_pi[a][3 * ai] - ax, dy = s_pi[a][3 * ai + 1] - ay, dz = s_pi[a][3 * ai + 2] - az;
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
            if (!(r2 < v.cutoff2)) continue;
            const int t = kind1 * v.nkinds + nm.kinds[ai];
            for (int q = v.rule_offset[t]; q < v.rule_offset[t + 1]; ++q) inter += rule_energy(v.rules[q], r2, v.coulombic);
        }
    }
    const size_t ij = (size_t)i * (size_t)n + j, ji = (size_t)j * (size_t)n + i;
    const double total = (inter + (with_recip ? out[ij] : 0.0)) + off2;
    out[ij] = total;
    out[ji] = total;
}

int tables_check(const ceg_mc_t* h, const int32_t* kinds, int32_t m_atoms, const double* positions, int32_t n, const void* framework, const void* interactions,
                 McMolecule* nm)
{
    if (!h || !positions || !framework || !interactions) return fail(CEG_ERR_INVALID, "site tables: bad argument");
    if (h->poisoned) return fail(CEG_ERR_HIP, "site tables: the handle is inconsistent after a failed call");
    if (h->group) return fail(CEG_ERR_INVALID, "site tables: the handle belongs to a chain group");
    if (h->v.nmol != 0 || !h->h_mol.empty()) return fail(CEG_ERR_UNSUPPORTED, "site tables: the handle holds %d guests; the tables are those of the guest-free framework", h->v.nmol);
    if (n < 1 || n > 65535) return fail(CEG_ERR_INVALID, "site tables: n = %d sites, outside 1..65535 (sites are UInt16)", n);
    if (int rc = check_molecule(h, kinds, m_atoms, nm)) return rc;
    if (h->v.nk > 0 && tables_bytes(h, m_atoms) > 64 * 1024) return fail(CEG_ERR_UNSUPPORTED, "site tables: k-space tables of the molecule do not fit in LDS");
    const int64_t limit_mb = env_int("CEG_HIP_SITE_TABLE_LIMIT_MB", 2048, 1, (int64_t)1 << 30);
    const size_t limit = (size_t)limit_mb << 20, n_pad = ((size_t)n + 15) & ~(size_t)15;
    if ((size_t)n * (size_t)n * sizeof(double) > limit)
        return fail(CEG_ERR_UNSUPPORTED, "site tables: interactions of %d sites take %zu bytes, above CEG_HIP_SITE_TABLE_LIMIT_MB = %lld MiB", n,
                    (size_t)n * (size_t)n * sizeof(double), (long long)limit_mb);
    if ((size_t)h->v.nk * n_pad * sizeof(double2) > limit)
        return fail(CEG_ERR_UNSUPPORTED, "site tables: the structure factors of %d sites over %d k-vectors take %zu bytes, above CEG_HIP_SITE_TABLE_LIMIT_MB = %lld MiB", n,
                    h->v.nk, (size_t)h->v.nk * n_pad * sizeof(double2), (long long)limit_mb);
    for (size_t e = 0; e < (size_t)n * (size_t)m_atoms * 3; ++e)
        if (!std::isfinite(positions[e])) return fail(CEG_ERR_INVALID, "site tables: a position is not finite");
    return CEG_OK;
}

}  // namespace

extern "C" int ceg_site_tables_device(ceg_mc_t* h, const int32_t* kinds, int32_t m_atoms, const double* positions, int32_t n, double offset_one,
                                      double offset_pair, double* d_framework, double* d_recip, double* d_interactions)
{
    McMolecule nm{};
    if (int rc = tables_check(h, kinds, m_atoms, positions, n, d_framework, d_interactions, &nm)) return rc;
    if (!std::isfinite(offset_one) || !std::isfinite(offset_pair)) return fail(CEG_ERR_INVALID, "site tables: an offset is not finite");
    ceg_host::DeviceGuard guard(h->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice failed");
    const int nk = h->v.nk, n_pad = (n + 15) & ~15, tiles = n_pad / 16;
    const size_t pos_bytes = sizeof(double) * (size_t)n * (size_t)m_atoms * 3, st_bytes = sizeof(double2) * (size_t)std::max(nk, 1) * (size_t)n_pad;
    double* d_pos = nullptr;
    double2* d_st = nullptr;
    auto release = [&]() {
        if (d_pos) (void)hipFree(d_pos);
        if (d_st) (void)hipFree(d_st);
    };
    bool ok = hipMalloc((void**)&d_pos, pos_bytes) == hipSuccess && hipMalloc((void**)&d_st, st_bytes) == hipSuccess &&
              hipMemcpy(d_pos, positions, pos_bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemsetAsync(d_st, 0, st_bytes, h->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_site_points, dim3((unsigned)n), dim3(MC_THREADS), nk > 0 ? tables_bytes(h, m_atoms) : 0, h->stream, h->v, nm, d_pos, n_pad, h->stride,
                           offset_one, d_st, d_framework, d_recip);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && nk > 0) {
        hipLaunchKernelGGL(k_site_recip_pairs, dim3((unsigned)tiles, (unsigned)tiles), dim3(64), 0, h->stream, d_st, h->v.kf, nk, n, n_pad, d_interactions);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok) {
        hipLaunchKernelGGL(k_site_real_pairs, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, h->stream, h->v, nm, d_pos, n, nk > 0 ? 1 : 0, offset_pair,
                           d_interactions);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = hipStreamSynchronize(h->stream) == hipSuccess && ok;
    const int rc = ok ? CEG_OK : fail(CEG_ERR_HIP, "site tables: the build failed: %s", hipGetErrorString(hipGetLastError()));
    release();
    return rc;
}

extern "C" int ceg_site_tables(ceg_mc_t* h, const int32_t* kinds, int32_t m_atoms, const double* positions, int32_t n, double offset_one, double offset_pair,
                               double* framework, double* recip, double* interactions)
{
    McMolecule nm{};
    if (int rc = tables_check(h, kinds, m_atoms, positions, n, framework, interactions, &nm)) return rc;
    ceg_host::DeviceGuard guard(h->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice failed");
    const size_t N = (size_t)n;
    double *d_fw = nullptr, *d_rec = nullptr, *d_it = nullptr;
    auto release = [&]() {
        for (void* p : {(void*)d_fw, (void*)d_rec, (void*)d_it})
            if (p) (void)hipFree(p);
    };
    if (hipMalloc((void**)&d_fw, sizeof(double) * N) != hipSuccess || hipMalloc((void**)&d_rec, sizeof(double) * N) != hipSuccess ||
        hipMalloc((void**)&d_it, sizeof(double) * N * N) != hipSuccess) {
        release();
        return fail(CEG_ERR_HIP, "site tables: could not allocate the device tables");
    }
    int rc = ceg_site_tables_device(h, kinds, m_atoms, positions, n, offset_one, offset_pair, d_fw, d_rec, d_it);
    if (rc == CEG_OK && (hipMemcpy(framework, d_fw, sizeof(double) * N, hipMemcpyDeviceToHost) != hipSuccess ||
                         (recip && hipMemcpy(recip, d_rec, sizeof(double) * N, hipMemcpyDeviceToHost) != hipSuccess) ||
                         hipMemcpy(interactions, d_it, sizeof(double) * N * N, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(CEG_ERR_HIP, "site tables: D2H of the tables failed");
    release();
    return rc;
}
