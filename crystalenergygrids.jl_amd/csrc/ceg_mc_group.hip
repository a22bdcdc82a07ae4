// ceg_mc_group.hip -- chain groups (ceg_mc_group_*): K Markov chains, each a ceg_mc handle of ceg_mc.hip, driven together.  Here the
// group itself (struct ceg_mc_group, ceg_mc_group.h) and its one-step calls:
//   ceg_mc_group_create / _destroy
//   ceg_mc_group_trial / _accept   one step of K chains in one launch per class: the bodies of k_mc_trial / k_mc_accept (ceg_mc_state.h)
//   ceg_mc_group_set_blocks        block pockets: inblockpocket and the retry loop of choose_step!, resolved inside the GCMC trial launch
//   ceg_mc_group_set_chain_plan    per chain: the phiPV_div_k of the swap rules and the absolute step at which the chain stops (isotherms)
//   ceg_mc_group_set_device_cells / _halted
// The sweeps (ceg_mc_group_sweep, _sweep_gcmc and their *_cycles forms) are in ceg_mc_sweep.hip; sampler, tempering, recorder and
// baseline of a group in ceg_mc_sample.hip, ceg_mc_temper.hip, ceg_mc_record.hip and ceg_mc_baseline.hip.
#include "ceg_mc_gcmc.h"
#include "ceg_mc_group.h"

using namespace ceg_mcs;

namespace {

// ---- a chain group (ceg_mc_group_*): one step of K chains in one launch per (FAST, INSERT, CELLS) class.  What a chain of the
// launch needs travels in mapped host memory like a small batch of k_mc_trial; the views stay in device memory.
struct McGroupRow {
    int32_t view, molecule, stride, _pad;    // view: index of the chain in the group (views[view]); molecule -1 for an insertion
    int64_t trial, out;                      // offsets of the chain's placements (doubles) and of its first row (rows)
    McLocal L;
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
    temper_free(g->tempering);
    recorder_free(g->recorder);
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

}  // namespace

int ceg_mcs::chain_err(int code, int c, const char* sep, const char* what)        // "chain <c><sep><what>"
{
    char msg[160];
    std::snprintf(msg, sizeof msg, "chain %d%s%s", c, sep, what);
    return merr(code, msg);
}

int ceg_mcs::group_bad(int c, const char* what) { return chain_err(CEG_ERR_INVALID, c, ": ", what); }

bool ceg_mcs::group_upload_views(ceg_mc_group* g, const std::vector<char>& used)
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

int ceg_mcs::group_refuse_poisoned(int c)
{
    return chain_err(CEG_ERR_HIP, c, " of the group is inconsistent after an earlier failure of accept / insert / remove: call ceg_mc_set_guests on it", "");
}

ceg_mcs::GroupRef ceg_mcs::group_ref(ceg_mc_group* g)
{
    return GroupRef{g->device, g->stream, g->chains.data(), (int)g->chains.size(), g->d_views, &g->d_baseline, &g->baseline_cap, &g->sampler, &g->tempering, &g->recorder};
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
        McGroupAccept& A = static_cast<McGroupAccept*>(g->h_acc)[e++];
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
    hipLaunchKernelGGL(k_mcg_accept, dim3((unsigned)count), dim3(MC_THREADS), lds, g->stream, g->d_views, static_cast<const McGroupAccept*>(g->dm_acc));
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

// ---- device cells of a group: the plain sweeps take the chains with neighbour cells
extern "C" int ceg_mc_group_set_device_cells(ceg_mc_group_t* g, int32_t on, int32_t min_capacity)
{
    if (!g || min_capacity < 0 || min_capacity > (1 << 20)) return merr(CEG_ERR_INVALID, "bad argument (0 <= min_capacity <= 2^20)");
    Guard guard(g->device);
    if (!guard.ok) return merr(CEG_ERR_HIP, "hipSetDevice failed");
    if (hipStreamSynchronize(g->stream) != hipSuccess) return merr(CEG_ERR_HIP, "stream synchronisation failed");
    group_stream_idle(g);
    for (size_t c = 0; on && min_capacity > 0 && c < g->chains.size(); ++c) {
        ceg_mc* h = g->chains[c];
        if (!h->cm.on || h->cm.cap >= min_capacity) continue;
        if (h->poisoned) return group_refuse_poisoned((int)c);
        h->cm.min_cap = min_capacity;
        if (int rc = rebuild_cells(h)) { h->poisoned = true; return rc; }
    }
    g->device_cells = on != 0;
    return CEG_OK;
}

extern "C" int ceg_mc_group_halted(ceg_mc_group_t* g, int64_t* halted_step_out)
{
    if (!g || !halted_step_out) return merr(CEG_ERR_INVALID, "bad argument");
    for (size_t c = 0; c < g->chains.size(); ++c) halted_step_out[c] = c < g->halted.size() ? g->halted[c] : -1;
    return CEG_OK;
}

