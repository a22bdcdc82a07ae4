// ceg_mc_cycles.hip -- the cycle end of ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles: the end-of-cycle block of
// run_montecarlo! (src/simulation.jl:727-728, 818-827) as one small launch per cycle (k_mcg_cycle_end) on the group's stream.  The
// sweeps of ceg_mc_sweep.hip enqueue it behind the accept launch (and the sampler frame) of a cycle's last step; it writes the cycle's
// record and the next cycle's temperature, dmax and thetamax into the chain's parameter slot, which the next step's launches read.
#include "ceg_mc_state.h"

using namespace ceg_mcs;

namespace {

static_assert(sizeof(ceg_mc_cycles_t) == 48 && sizeof(ceg_mc_cycle_record_t) == 96, "layouts the bindings restate");

struct CycleEnd {                                // by value (kernarg)
    CycleSource src;
    CycleRun run;
    int64_t j;                                   // cycle of the call
    int32_t k, _pad;
};

template <class T>
__device__ __forceinline__ T cycle_at(const T* base, int c, int stride)
{
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)c * (size_t)stride);
}

__device__ __forceinline__ double cycle_clamp(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

// simulation.jl:818-822
__device__ __forceinline__ double cycle_adapt_dmax(double dmax, int64_t accepted, int64_t trials, int64_t cc)
{
#pragma clang fp contract(off)
    const double r = (double)accepted / (double)trials;
    const double q = 10.0 / (double)(99 + cc);
    const double s = sqrt(q);
    const double f = (r - 0.25) * s;
    const double g = 1.0 + f;
    return cycle_clamp(dmax * g, 0.1, 3.0);
}

// simulation.jl:823-826 in radians: 120, 10 and 180 degrees
__device__ __forceinline__ double cycle_adapt_thetamax(double thetamax, int64_t accepted, int64_t trials, int64_t cc)
{
#pragma clang fp contract(off)
    const double r = (double)accepted / (double)trials;
    const double a = (r - 0.5) / (double)cc;
    const double b = a * 2.0943951023931953;
    return cycle_clamp(thetamax + b, 0.17453292519943295, 3.141592653589793);
}

// one workgroup, lane c on chain c: the record of cycle j, then the chain's parameters of cycle j + 1.  Ordinary loads and stores:
// the launches before and after it on the stream are whole kernels.
__global__ __launch_bounds__(CEG_MC_GROUP_MAX) void k_mcg_cycle_end(const McView* __restrict__ views, const CycleEnd E)
{
    const int c = (int)threadIdx.x;
    if (c >= E.k) return;
    const CycleSource& S = E.src;
    const CycleRun& R = E.run;
    const int64_t* prior = R.d_prior + 4 * (size_t)c;
    const int64_t tt = prior[0] + cycle_at(S.translation_trials, c, S.stats_stride), ta = prior[1] + cycle_at(S.translation_accepted, c, S.stats_stride);
    const int64_t rt = prior[2] + cycle_at(S.rotation_trials, c, S.stats_stride), ra = prior[3] + cycle_at(S.rotation_accepted, c, S.stats_stride);
    const int nmol = S.nmol ? cycle_at(S.nmol, c, S.nmol_stride) : as_constant(views)[c].nmol;
    double* triple = reinterpret_cast<double*>(reinterpret_cast<char*>(S.triple) + (size_t)c * (size_t)S.triple_stride);
    const double temperature = triple[0], dmax = triple[1], thetamax = triple[2];
    const int64_t cc = R.cycle0 + E.j;
    double dmax_next = dmax, thetamax_next = thetamax;
    const bool adapts = nmol > 0 && !(S.stop && S.last_step >= (uint64_t)S.stop[c]);      // (not a chain that stopped in or before this cycle)
    if (adapts && (R.adapt & CEG_MC_ADAPT_DMAX) && tt > 0) dmax_next = cycle_adapt_dmax(dmax, ta, tt, cc);
    if (adapts && (R.adapt & CEG_MC_ADAPT_THETAMAX) && rt > 0) thetamax_next = cycle_adapt_thetamax(thetamax, ra, rt, cc);
    ceg_mc_cycle_record_t rec;
    rec.temperature = temperature; rec.dmax = dmax; rec.thetamax = thetamax;
    rec.dmax_next = dmax_next; rec.thetamax_next = thetamax_next;
    rec.delta_moves = cycle_at(S.delta_moves, c, S.stats_stride);
    rec.delta_swaps = S.delta_swaps ? cycle_at(S.delta_swaps, c, S.stats_stride) : 0.0;
    rec.translation_trials = tt; rec.translation_accepted = ta; rec.rotation_trials = rt; rec.rotation_accepted = ra;
    rec.nmol = nmol; rec._pad = 0;
    R.d_records[(size_t)E.j * (size_t)E.k + (size_t)c] = rec;
    triple[1] = dmax_next;
    triple[2] = thetamax_next;
    if (R.d_table && E.j + 1 < R.ncycles) triple[0] = R.d_table[(size_t)(E.j + 1) * (size_t)E.k + (size_t)c];
}

int bad_cycles(const char* what)
{
    char msg[200];
    std::snprintf(msg, sizeof msg, "cycles: %s", what);
    return merr(CEG_ERR_INVALID, msg);
}

}  // namespace

int ceg_mcs::cycles_check(const ceg_mc_cycles_t* cy, int k, uint64_t first_step, bool constant_columns, const void* cycles_out, int64_t* nsteps)
{
    if (!cy) return bad_cycles("no ceg_mc_cycles_t");
    if (cy->ncycles < 0 || cy->steps_per_cycle < 1 || cy->cycle0 < 1) return bad_cycles("ncycles >= 0, steps_per_cycle >= 1 and cycle0 >= 1");
    if (cy->adapt & ~(CEG_MC_ADAPT_DMAX | CEG_MC_ADAPT_THETAMAX)) return bad_cycles("unknown adapt bits");
    if (cy->ncycles > 0 && !cycles_out) return bad_cycles("cycles_out is missing");
    if (cy->ncycles > INT64_MAX / cy->steps_per_cycle) return bad_cycles("ncycles * steps_per_cycle exceeds 2^63 - 1");
    const int64_t total = cy->ncycles * cy->steps_per_cycle;
    if (first_step > (uint64_t)INT64_MAX || (uint64_t)total > (uint64_t)INT64_MAX - first_step) return bad_cycles("the call must end before step 2^63");
    if (cy->cycle0 > INT64_MAX - 99 - cy->ncycles) return bad_cycles("99 + cycle0 + ncycles is not representable");
    if (cy->ncycles > CEG_MC_CYCLES_MAX_RECORDS / (int64_t)k) return bad_cycles("more than CEG_MC_CYCLES_MAX_RECORDS records (ncycles * K) in one call: split the run");
    if (cy->temperatures)
        for (int64_t j = 0; j < cy->ncycles; ++j)
            for (int c = 0; c < k; ++c) {
                const double t = cy->temperatures[(size_t)j * (size_t)k + (size_t)c];
                if (!std::isfinite(t) || !(t > 0.0)) return bad_cycles("every temperature of the table must be finite and > 0");
                if (constant_columns && t != cy->temperatures[c])
                    return bad_cycles("a species has a swap probability > 0: the temperature of every chain must be constant over the cycles");
            }
    if (cy->prior)
        for (int c = 0; c < k; ++c) {
            const int64_t* q = cy->prior + 4 * (size_t)c;
            if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || q[1] > q[0] || q[3] > q[2])
                return bad_cycles("the prior counters must be >= 0 with accepted <= trials");
        }
    *nsteps = total;
    return CEG_OK;
}

void ceg_mcs::cycles_enqueue(hipStream_t stream, const McView* d_views, int k, const CycleRun& run, int64_t j, const CycleSource& src)
{
    const CycleEnd E{src, run, j, k, 0};
    hipLaunchKernelGGL(k_mcg_cycle_end, dim3(1u), dim3((unsigned)CEG_MC_GROUP_MAX), 0, stream, d_views, E);
}
