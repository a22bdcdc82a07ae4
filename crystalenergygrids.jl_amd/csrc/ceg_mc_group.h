// ceg_mc_group.h -- a chain group on the host: what ceg_mc_group.hip (the group itself and its one-step calls) and ceg_mc_sweep.hip
// (the sweeps) share, and nobody else includes.  The other files of a group's features see a group through GroupRef (ceg_mc_state.h).
#pragma once
#include "ceg_mc_state.h"

// ---- chain groups: one step of K Markov chains (handles on one device) per trial launch and per accept launch.  The members' own
// asynchronous work runs on the group's stream while they are grouped, so per-handle calls and group calls stay in order.
struct ceg_mc_group {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<ceg_mc*> chains;
    std::vector<uint64_t> uploaded;              // v_version of each member's view in d_views (0: never uploaded)
    ceg_mcs::McView* d_views = nullptr;          // [K] device memory, read by k_mcg_trial / k_mcg_accept
    ceg_mcs::McView* h_views = nullptr;          // [K] pinned staging of the view uploads
    bool uploads_pending = false;                // an upload out of h_views may not have run yet
    // per-call staging, pinned and device-mapped: trial entries + row prefixes + placements in, rows out; accept entries
    unsigned char *h_in = nullptr, *dm_in = nullptr;
    double *h_out = nullptr, *dm_out = nullptr;
    void *h_acc = nullptr, *dm_acc = nullptr;    // [K] McGroupAccept of ceg_mc_group.hip
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
    ceg_mcs::GroupSampler* sampler = nullptr;    // density maps and series taken during sweeps (ceg_mc_sample.hip); nullptr: none
    ceg_mcs::GroupTempering* tempering = nullptr;    // rungs, energies and exchange records of the *_cycles sweeps (ceg_mc_temper.hip); nullptr: none
    ceg_mcs::GroupRecorder* recorder = nullptr;  // frames and minimum taken at the cycle ends of the *_cycles sweeps (ceg_mc_record.hip); nullptr: none
    // chain plan (ceg_mc_group_set_chain_plan): the host's copy for the checks and the launch lists, the device's for the kernels
    std::vector<double> plan_phi;                // [K][plan_species], empty: the species table's value for every chain
    std::vector<int64_t> plan_stop;              // [K], empty: no chain stops
    int plan_species = 0;
    double* d_plan_phi = nullptr;
    int64_t* d_plan_stop = nullptr;
    // device cells (ceg_mc_group_set_device_cells): ceg_mc_group_sweep / _cycles take the chains with neighbour cells
    bool device_cells = false;
    bool sweep_enqueued = false;                 // the last run_sweep got as far as its steps (a failure before that has launched and changed nothing)
    std::vector<int64_t> halted;                 // [K] of the last sweep call: the step at which a full cell halted the chain, -1: none
};

namespace ceg_mcs {

// defined in ceg_mc_group.hip
int chain_err(int code, int c, const char* sep, const char* what);        // "chain <c><sep><what>"
int group_bad(int c, const char* what);                                   // CEG_ERR_INVALID, "chain <c>: <what>"
// the views of chains `used` (used[c] != 0) into d_views where they changed since their last upload, in stream order
bool group_upload_views(ceg_mc_group* g, const std::vector<char>& used);

}  // namespace ceg_mcs
