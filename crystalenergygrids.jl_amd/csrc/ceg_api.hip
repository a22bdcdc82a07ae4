// ceg_api.hip -- C ABI of libceg_hip.so (include/ceg_hip.h): plan management, host-side
// preparation of the lattice-image list and bins, the build launches.  The one-shot entry
// points (slab scheduling over devices, D2H pipelines, .grid files) are in ceg_oneshot.hip.
//
// Replaces the loop nests of create_grid_vdw / create_grid_coulomb
// (src/grids.jl:144-150, 171-177 of CrystalEnergyGrids.jl).  No CPU compute path exists
// here: without a HIP device every build entry point fails with CEG_ERR_NO_DEVICE.
#include "ceg_internal.h"
#include "ceg_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

using namespace ceg;
using ceg_host::check_common;
using ceg_host::DeviceGuard;
using ceg_host::fail;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err = "";

int ceg_host::fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// used by the other translation units (ceg_interp.hip) to report through ceg_last_error()
extern "C" void ceg_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }

extern "C" int ceg_abi_version(void) { return CEG_ABI_VERSION; }

extern "C" const char* ceg_last_error(void) { return g_err.c_str(); }

extern "C" int ceg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

namespace ceg {
UniformClass detect_uniform_class(const FastVdw* fast, int32_t nkinds, const int32_t* kind, const double* charge, int64_t natoms)
{
    UniformClass u;
    std::vector<char> present((size_t)std::max(nkinds, 1), 0);
    for (int64_t a = 0; a < natoms; ++a)
        if (kind[a] >= 0 && kind[a] < nkinds) present[kind[a]] = 1;
    const FastVdw* first = nullptr;
    for (int32_t k = 0; k < nkinds; ++k) {
        const FastVdw& f = fast[k];
        if (!present[k] || f.cls == 0) continue;          // absent, or no rule with this probe: not a VdW-active kind
        if (f.cls != 1) return u;
        if (!first) first = &f;
        else if (memcmp(&first->p0, &f.p0, 4 * sizeof(double)) != 0) return u;      // bit-identical {4 eps, sigma^2, sigma^6, shift}
    }
    if (!first) return u;
    const double e4 = first->p0, s6 = first->p2, sh = first->shift;
    if (!(std::fabs(e4) >= 1e-9 && std::fabs(e4) <= 1e9) || !(s6 >= 1e-9 && s6 <= 1e9) || !std::isfinite(sh)) return u;
    u.cls = 1; u.eps4 = e4; u.s6 = s6; u.shift = sh;
    if (!charge) return u;
    bool have = false;
    double q = 0.0;
    for (int64_t a = 0; a < natoms; ++a) {
        const int32_t k = kind[a];
        if (k < 0 || k >= nkinds || fast[k].cls == 0) continue;
        if (!have) { q = charge[a]; have = true; }
        else if (memcmp(&q, &charge[a], sizeof(double)) != 0) return u;
    }
    if (have && std::fabs(q) >= 1e-6 && std::fabs(q) <= 1e6) { u.cls = 2; u.q = q; }
    return u;
}
}  // namespace ceg

// ------------------------------------------------------------------ plan
struct ceg_plan {
    int device = 0;
    Geom g{};
    int64_t natoms = 0;
    bool has_rules = false, has_charge = false;
    bool can_cull = false;
    // host copies (needed to (re)build the image list)
    std::vector<double> h_pos, h_charge;
    std::vector<int32_t> h_kind;           // 0-based, -1 if none
    std::vector<DevRule> h_rules;
    std::vector<int32_t> h_offset;
    std::vector<int32_t> h_offset_union;   // multi-probe plans: offsets of a table with one entry per kind that has a rule with ANY probe
    int32_t nkinds = 0;
    // device
    double4* d_atoms = nullptr;
    int32_t* d_kind = nullptr;
    DevRule* d_rules = nullptr;
    int32_t* d_offset = nullptr;
    double4* d_images = nullptr;    // (views into `images`, which owns them)
    int32_t* d_imgkind = nullptr;
    int32_t* d_imgatom = nullptr;
    int32_t* d_binstart = nullptr;
    std::shared_ptr<void> images;          // owner of the lattice-image list + bins on the device (an ImageSet, shared between plans: image cache)
    ImageBins ib{};
    bool images_built = false;
    bool images_from_cache = false;
    PlanConst* d_pc = nullptr;   // device copy of {g, ib, rt, tables}
    double* d_erfcx = nullptr;
    double* d_exp2 = nullptr;
    int vdwk = 0;                // hot-loop VdW variant: 0 generic, 1 LJ-only, 2 LJ/Buckingham classes, 3 one tabulated Buckingham class
    bool single_buck = false;    // every present kind with a VdW rule is the same Buckingham (+ hard sphere) -> candidate for vdwk 3
    double bk[4] = {0, 0, 0, 0}; // its A, B, C, shift
    double* d_bk2 = nullptr;
    UniformClass uni;            // one Lennard-Jones record (+ one charge) for every VdW-active atom: k_culled VDWK 4 / 5 (0: none)
    double r_exact2 = CEG_R_EXACT2;
    std::vector<FastVdw> h_fast;
    FastVdw* d_fast = nullptr;
    bool fast_ewald = false;     // alpha*cutoff within the erfcx polynomial's domain
    bool ew2 = false;            // r^2-indexed Ewald tables built (hot-loop variant EWK = 2)
    double* d_ew2 = nullptr;
    bool ew2f = false;           // and the fine layout beside them (EWK = 3 where a variant can hold it)
    double* d_ew2f = nullptr;
    // multi-probe plans (ceg_plan_create_multi): the rule tables of every probe; d_pc holds probe 0 in its single-probe slots and
    // all of them in rtm / fastm, d_pc_probe[p] is the same block with probe p in the single-probe slots (launches of one probe)
    struct ProbeTab {
        std::vector<DevRule> rules;
        std::vector<int32_t> offset;
        std::vector<FastVdw> fast;
        DevRule* d_rules = nullptr;
        int32_t* d_offset = nullptr;
        FastVdw* d_fast = nullptr;
        PlanConst* d_pc = nullptr;
        // the probe's own hot-loop class (round 4: probes of several classes in one plan): 1 Lennard-Jones-only -- shares launches
        // with other such probes --, 3 one tabulated Buckingham class, 2 / 0 as in an ordinary plan: single-probe launches
        int vdwk = 0;
        bool single_buck = false;
        double bk[4] = {0, 0, 0, 0};
        double* d_bk2 = nullptr;
        UniformClass uni;               // the probe's own uniform class: the plain builds on the plan run probe 0 with it
        int32_t* d_imgkind = nullptr;   // per image: kind | "the kind has a rule with THIS probe" (the shared list carries the union)
    };
    int nprobes = 0;             // 0: ordinary plan
    std::vector<ProbeTab> probes;
};

namespace {

inline void matvec(const double* m, const double v[3], double o[3])
{
    for (int i = 0; i < 3; ++i) o[i] = m[i] * v[0] + m[i + 3] * v[1] + m[i + 6] * v[2];
}

// perpendicular widths of the cell (src/utils.jl:10-29)
void perpendicular_widths(const double* m, double w[3])
{
    const double* a = m;
    const double* b = m + 3;
    const double* c = m + 6;
    auto cross = [](const double* u, const double* v, double* o) {
        o[0] = u[1] * v[2] - u[2] * v[1];
        o[1] = u[2] * v[0] - u[0] * v[2];
        o[2] = u[0] * v[1] - u[1] * v[0];
    };
    auto norm = [](const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); };
    double axb[3], bxc[3], cxa[3];
    cross(a, b, axb);
    cross(b, c, bxc);
    cross(c, a, cxa);
    const double vol = std::fabs(a[0] * bxc[0] + a[1] * bxc[1] + a[2] * bxc[2]);
    w[0] = vol / norm(bxc);
    w[1] = vol / norm(cxa);
    w[2] = vol / norm(axb);
}

// Translate the public rule table into device rules.  Only kinds that occur in the atom list
// are validated, mirroring the reference where derivativesGrid raises lazily
// (src/interactions.jl:442-443,462-467).
int convert_rules(ceg_plan* p, const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds)
{
    std::vector<char> present(nkinds, 0);
    for (int64_t a = 0; a < p->natoms; ++a) present[p->h_kind[a]] = 1;
    p->h_offset.assign(nkinds + 1, 0);
    p->h_rules.clear();
    for (int32_t k = 0; k < nkinds; ++k) {
        p->h_offset[k] = (int32_t)p->h_rules.size();
        for (int32_t t = rule_offset[k]; t < rule_offset[k + 1]; ++t) {
            const ceg_rule_t& r = rules[t];
            DevRule d{};
            d.kind = r.kind;
            d.shift = r.shift;
            switch (r.kind) {
            case CEG_NOINTERACTION:
            case CEG_COULOMB_EWALD_DIRECT:
                continue;  // exact zeros in a VdW grid
            case CEG_LENNARDJONES:
                d.p0 = r.p[0];
                d.p1 = r.p[1] * r.p[1];
                break;
            case CEG_BUCKINGHAM:
                d.p0 = r.p[0];
                d.p1 = r.p[1];
                d.p2 = r.p[2];
                break;
            case CEG_HARDSPHERE: {
                const double rr = r.p[0] + r.p[1];
                d.p0 = rr * rr;
                break;
            }
            default:
                if (present[k])
                    return fail(CEG_ERR_RULE,
                                "interaction kind %d (force-field index %d) is not valid in a VdW grid "
                                "(src/interactions.jl:442-467)", r.kind, k + 1);
                continue;
            }
            p->h_rules.push_back(d);
        }
    }
    p->h_offset[nkinds] = (int32_t)p->h_rules.size();
    p->nkinds = nkinds;
    // classify every kind for the hot loop of k_culled
    p->h_fast.assign(nkinds, FastVdw{});
    bool all_lj = true, all_fast = true;
    double hs_max2 = 0.0;
    for (int32_t k = 0; k < nkinds; ++k) {
        const int32_t b = p->h_offset[k], e = p->h_offset[k + 1];
        FastVdw f{};
        int nlj = 0, nbuck = 0, nhs = 0, nother = 0;
        for (int32_t t = b; t < e; ++t) {
            const DevRule& r = p->h_rules[t];
            if (r.kind == CEG_LENNARDJONES) { ++nlj; f.p0 = 4.0 * r.p0; f.p1 = r.p1; f.p2 = r.p1 * r.p1 * r.p1; f.shift += r.shift; }
            else if (r.kind == CEG_BUCKINGHAM) { ++nbuck; f.p0 = r.p0; f.p1 = r.p1; f.p2 = r.p2; f.shift += r.shift; }
            else if (r.kind == CEG_HARDSPHERE) { ++nhs; f.shift += r.shift; if (present[k]) hs_max2 = std::max(hs_max2, r.p0); }
            else ++nother;
        }
        if (e == b) f.cls = 0;
        else if (nlj == 1 && nbuck == 0 && nhs == 0 && nother == 0) f.cls = 1;
        else if (nbuck == 1 && nlj == 0 && nother == 0) f.cls = 2;
        else f.cls = 3;
        p->h_fast[k] = f;
        if (!present[k]) continue;
        if (f.cls > 1) all_lj = false;
        if (f.cls > 2) all_fast = false;
    }
    p->vdwk = all_lj ? 1 : (all_fast ? 2 : 0);
    // one Buckingham parameter set for every present VdW-active kind (the Na probe of the fixture force field: Na-O only)
    if (p->vdwk == 2) {
        bool first = true, same = true;
        for (int32_t k = 0; k < nkinds && same; ++k) {
            const FastVdw& f = p->h_fast[k];
            if (!present[k] || f.cls == 0) continue;
            if (f.cls != 2) { same = false; break; }
            if (first) { p->bk[0] = f.p0; p->bk[1] = f.p1; p->bk[2] = f.p2; p->bk[3] = f.shift; first = false; }
            else same = f.p0 == p->bk[0] && f.p1 == p->bk[1] && f.p2 == p->bk[2] && f.shift == p->bk[3];
        }
        p->single_buck = same && !first && p->bk[1] > 0.0 && p->bk[2] != 0.0 && std::isfinite(1.0 / p->bk[2]);
    }
    // hard spheres must lie inside the exact-path radius for the fast Buckingham class
    p->r_exact2 = std::max(CEG_R_EXACT2, hs_max2 * (1.0 + 1e-9) + 1e-9);
    if (p->r_exact2 >= p->g.cutoff2) p->vdwk = 0, p->r_exact2 = CEG_R_EXACT2;
    return CEG_OK;
}

// The uniform class of a Lennard-Jones-only plan (vdwk == 1) for the hot loops of k_culled:
//   1 (uni_lj): every kind that is present and has a rule with the probe carries a bit-identical fast record {4 eps, sigma^2, sigma^6,
//               shift} -- the hot loop then sums the channels in units of 4 eps sigma^6 and applies that and count * shift once per tile;
//   2 (uni_q):  1, and every atom of such a kind carries a bit-identical charge (per ATOM: charges are not a property of the kind) --
//               the Coulomb channels of the VdW-active group are summed in units of q.
// The sums are divided by 4 eps sigma^6 (q) on the exact path and multiplied back at the end of a tile, so these must be ordinary
// numbers of moderate size: |4 eps| and sigma^6 in [1e-9, 1e9], |q| in [1e-6, 1e6] (force fields hold 1e-2 .. 1e3 K, 1 .. 5 A and
// 1e-2 .. 4 e); all finite.
void set_uniform_class(ceg_plan* p)
{
    p->uni = UniformClass{};
    if (p->vdwk != 1 || p->natoms <= 0) return;
    p->uni = detect_uniform_class(p->h_fast.data(), p->nkinds, p->h_kind.data(), p->h_charge.empty() ? nullptr : p->h_charge.data(), p->natoms);
}

// what PlanConst carries of it
void fill_uniform_class(PlanConst& c, const UniformClass& u)
{
    c.uni_class = u.cls;
    if (u.cls == 0) return;
    const double unit = u.eps4 * u.s6;
    c.uni_unit = unit; c.uni_s6 = u.s6; c.uni_shift = u.shift;
    c.uni_k1 = 2.0 * u.s6; c.uni_k2 = 3.5 * u.s6; c.uni_k3 = 5.6 * u.s6;
    c.uni_sv = 1.0 / unit; c.uni_s1 = -1.0 / (6.0 * unit); c.uni_s2 = 1.0 / (48.0 * unit); c.uni_s3 = -1.0 / (480.0 * unit);
    if (u.cls == 2) {
        c.uni_q = u.q; c.uni_inv_q = 1.0 / u.q; c.uni_qs2 = 1.0 / (3.0 * u.q); c.uni_qs3 = 1.0 / (15.0 * u.q);
    }
}

// ---- small-block cache for the plan tables.  A plan is a dozen small device arrays; hipMalloc +
// hipFree of those cost ~3 ms per plan, a third of the one-shot VdW build.  Blocks are kept by
// (device, power-of-two size class) and handed back by ceg_plan_destroy after a device
// synchronisation (hipFree's implicit one), so a cached block is never still in use by a kernel.
struct BlockCache {
    std::mutex m;
    std::map<std::pair<int, size_t>, std::vector<void*>> idle;
    std::unordered_map<void*, std::pair<int, size_t>> owner;
    size_t idle_bytes = 0;
};
BlockCache g_blocks;
constexpr size_t BLOCK_CACHE_LIMIT = 256ull << 20;

hipError_t cached_malloc(void** out, size_t bytes)
{
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    size_t cls = 512;
    while (cls < bytes) cls <<= 1;
    std::lock_guard<std::mutex> lock(g_blocks.m);
    auto& list = g_blocks.idle[{dev, cls}];
    if (!list.empty()) {
        *out = list.back();
        list.pop_back();
        g_blocks.idle_bytes -= cls;
        return hipSuccess;
    }
    if (hipError_t e = hipMalloc(out, cls); e != hipSuccess) return e;
    g_blocks.owner[*out] = {dev, cls};
    return hipSuccess;
}

void cached_free(void* ptr)         // caller has synchronised the device
{
    if (!ptr) return;
    std::lock_guard<std::mutex> lock(g_blocks.m);
    auto it = g_blocks.owner.find(ptr);
    if (it == g_blocks.owner.end()) { (void)hipFree(ptr); return; }
    const size_t cls = it->second.second;
    if (g_blocks.idle_bytes + cls > BLOCK_CACHE_LIMIT) {
        g_blocks.owner.erase(it);
        (void)hipFree(ptr);
        return;
    }
    g_blocks.idle[it->second].push_back(ptr);
    g_blocks.idle_bytes += cls;
}

void block_cache_release()
{
    std::lock_guard<std::mutex> lock(g_blocks.m);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto& kv : g_blocks.idle) {
        if (hipSetDevice(kv.first.first) != hipSuccess) continue;
        for (void* ptr : kv.second) {
            g_blocks.owner.erase(ptr);
            (void)hipFree(ptr);
        }
        kv.second.clear();
    }
    g_blocks.idle_bytes = 0;
    if (prev >= 0) (void)hipSetDevice(prev);
}

}  // namespace

namespace ceg_host {          // the same pool for the other translation units of the library (ceg_host.h)
hipError_t pool_malloc(void** out, size_t bytes) { return cached_malloc(out, bytes); }
void pool_free(void* ptr) { cached_free(ptr); }
}

namespace ceg {
struct ImgBox {
    double mat[9], invmat[9];
    double lo[3], hi[3], bin[3];
    int32_t nb[3];
    int32_t has_rules, has_charge, vdw_only;
    int32_t nkinds;
    uint64_t hasbits[16];
};
hipError_t build_images_device(const ImgBox& B, const double4* d_atoms, const int32_t* d_kind, const int32_t* d_has, int64_t natoms,
                               double4** out_xyzq, int32_t** out_kind, int32_t** out_atom, int32_t** out_binstart, int64_t* out_n);
}

namespace {

// The tables of a plan are a dozen uploads of a few hundred bytes to a few hundred kilobytes; a synchronous hipMemcpy from pageable memory
// costs 15-20 us each whatever its size (a fifth of a plan creation on a new framework).  They go through a page-locked staging area
// instead -- a host memcpy and an asynchronous copy on the null stream each -- and ONE synchronisation at the end of the creation
// (flush_uploads; also before the staging area wraps around).  Larger arrays keep the synchronous copy.  The areas live in a small
// process-wide pool: a plan creation borrows one for its duration (StagingLease), so threads that come and go do not each leave
// page-locked memory behind.
struct UploadStaging {
    char* h = nullptr;
    size_t cap = 0, used = 0;
    bool pending = false;
};
constexpr size_t UPLOAD_STAGING_BYTES = 4u << 20, UPLOAD_STAGED_MAX = 1u << 20;
struct StagingPool {
    std::mutex m;
    std::vector<char*> idle;           // (kept until the process ends: the HIP runtime may be gone when static destructors run)
};
StagingPool g_staging_pool;
thread_local UploadStaging* g_staging = nullptr;      // the area of the plan creation running on this thread, if any

struct StagingLease {
    UploadStaging st;
    UploadStaging* outer;
    StagingLease() : outer(g_staging)
    {
        if (!std::getenv("CEG_HIP_SYNC_UPLOADS")) {
            {
                std::lock_guard<std::mutex> lock(g_staging_pool.m);
                if (!g_staging_pool.idle.empty()) { st.h = g_staging_pool.idle.back(); g_staging_pool.idle.pop_back(); }
            }
            if (!st.h && hipHostMalloc((void**)&st.h, UPLOAD_STAGING_BYTES, hipHostMallocPortable) != hipSuccess) { st.h = nullptr; (void)hipGetLastError(); }
            if (st.h) st.cap = UPLOAD_STAGING_BYTES;
        }
        g_staging = &st;
    }
    ~StagingLease()
    {
        if (st.pending) (void)hipStreamSynchronize(nullptr);
        g_staging = outer;
        if (st.h) {
            std::lock_guard<std::mutex> lock(g_staging_pool.m);
            if (g_staging_pool.idle.size() < 8) g_staging_pool.idle.push_back(st.h);
            else (void)hipHostFree(st.h);
        }
    }
};

inline hipError_t flush_uploads()
{
    UploadStaging* st = g_staging;
    if (!st || !st->pending) return hipSuccess;
    st->pending = false;
    st->used = 0;
    return hipStreamSynchronize(nullptr);
}

template <class T>
int upload(T** dst, const T* src, size_t n)
{
    *dst = nullptr;
    if (n == 0) n = 1;  // keep pointers valid
    HIP_TRY(cached_malloc((void**)dst, n * sizeof(T)));
    if (!src) return CEG_OK;
    const size_t bytes = n * sizeof(T);
    UploadStaging* st = g_staging;
    if (st && st->h && bytes <= UPLOAD_STAGED_MAX) {
        if (st->used + bytes > st->cap) HIP_TRY(flush_uploads());
        memcpy(st->h + st->used, src, bytes);
        HIP_TRY(hipMemcpyAsync(*dst, st->h + st->used, bytes, hipMemcpyHostToDevice, nullptr));
        st->used += (bytes + 255) & ~(size_t)255;
        st->pending = true;
        return CEG_OK;
    }
    HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return CEG_OK;
}

// ---- image cache.  The lattice-image list of a plan depends on the framework (positions, cell), the cutoff, the grid's
// bounding box and, per atom, on what travels with an image: its kind + "has a VdW rule" flag, its charge, and whether atoms
// without a rule are left out (VdW-only plans).  setup_RASPA builds several grids of ONE framework one after the other
// (src/raspa.jl:497-520) and every one-shot call used to enumerate, sort and upload the same images again (1.0-1.4 ms of host time
// for the 11 664-atom workload: as long as a whole rank's compute at N = 8).  Finished lists are kept on the device, keyed by a
// 128-bit hash of everything they depend on, and shared by reference between plans; the cache holds the last few (CEG_HIP_IMAGE_CACHE
// = number of entries, 0 switches it off).
struct ImageSet {
    int device = 0;
    uint64_t key[2] = {0, 0};
    int64_t natoms = 0;             // compared on a hit together with the 128-bit (non-cryptographic) key: a collision must also
    double cutoff2 = 0.0;           // reproduce the atom count, the cutoff and the box to be taken for a hit
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    double4* d_images = nullptr;
    int32_t* d_imgkind = nullptr;
    int32_t* d_imgatom = nullptr;
    int32_t* d_binstart = nullptr;
    ImageBins ib{};                 // geometry of the bins + the pointers above (ib.atoms is per plan)
    size_t bytes = 0;
    ~ImageSet()
    {
        DeviceGuard guard(device);
        (void)hipDeviceSynchronize();          // no kernel still reads the arrays
        for (void* ptr : {(void*)d_images, (void*)d_imgkind, (void*)d_imgatom, (void*)d_binstart}) cached_free(ptr);
    }
};
std::mutex g_image_mutex;
// (heap-allocated and never destroyed: a static destructor would run ~ImageSet -- HIP calls -- after the runtime may be gone at exit)
std::vector<std::shared_ptr<ImageSet>>& g_image_cache = *new std::vector<std::shared_ptr<ImageSet>>();       // most recently used last
std::atomic<long> g_image_hits{0}, g_image_misses{0};

struct Hash128 {
    uint64_t a = 0x243F6A8885A308D3ull, b = 0x13198A2E03707344ull;
    void word(uint64_t w)
    {
        a = (a ^ w) * 0x9E3779B97F4A7C15ull; a ^= a >> 29;
        b = (b + w) * 0xC2B2AE3D27D4EB4Full; b ^= b >> 31; b += a;
    }
    void bytes(const void* ptr, size_t n)
    {
        const unsigned char* c = static_cast<const unsigned char*>(ptr);
        size_t i = 0;
        for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, c + i, 8); word(w); }
        uint64_t w = 0;
        if (i < n) memcpy(&w, c + i, n - i);
        word(w ^ ((uint64_t)n << 56));
    }
    template <class T> void pod(const T& v) { bytes(&v, sizeof v); }
};

int image_cache_capacity()
{
    if (const char* e = std::getenv("CEG_HIP_IMAGE_CACHE")) return std::max(0, atoi(e));
    return 6;
}

void image_cache_release()
{
    std::lock_guard<std::mutex> lock(g_image_mutex);
    g_image_cache.clear();
}

// Expand the atoms into every lattice image that can be within the cutoff of a grid point
// (grid bounding box grown by the cutoff), bin them on a cartesian lattice and upload.
#ifndef CEG_BIN_Z
#define CEG_BIN_Z 1.5
#endif
int build_images(ceg_plan* p)
{
    const Geom& g = p->g;
    const double cutoff = std::sqrt(g.cutoff2);
    const double margin = cutoff * (1.0 + 1e-6) + 1e-6;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = g.shift[a] - margin;
        hi[a] = g.shift[a] + g.size[a] + margin;
    }
    // bins: ~4.5 A edge in x and y (a tile's neighbourhood is then <= 64 bin rows (bx, by): one row per lane); z is the
    // contiguous direction of a row, where a finer bin only tightens the [bz0, bz1] range a row contributes
    double target[3] = {4.5, 4.5, CEG_BIN_Z};
    if (const char* e = std::getenv("CEG_HIP_BIN_XY")) target[0] = target[1] = std::max(0.5, atof(e));
    if (const char* e = std::getenv("CEG_HIP_BIN_Z")) target[2] = std::max(0.25, atof(e));
    int nb[3];
    double bin[3];
    for (int a = 0; a < 3; ++a) {
        nb[a] = std::max(1, (int)std::floor((hi[a] - lo[a]) / target[a]));
        bin[a] = (hi[a] - lo[a]) / nb[a];
    }
    // "the kind has a VdW rule": with the plan's probe, or with any probe of a multi-probe plan
    const std::vector<int32_t>& off = p->nprobes > 0 ? p->h_offset_union : p->h_offset;
    auto kind_has_rule = [&](int32_t k) { return k >= 0 && k + 1 < (int32_t)off.size() && off[k + 1] > off[k]; };
    // ---- cache look-up: everything the list below is a function of
    Hash128 hk;
    std::shared_ptr<ImageSet> hit;
    const int cap = image_cache_capacity();
    if (cap > 0) {
        hk.pod(p->device); hk.pod(p->natoms);
        hk.bytes(g.mat, sizeof g.mat); hk.bytes(g.invmat, sizeof g.invmat);
        hk.bytes(lo, sizeof lo); hk.bytes(hi, sizeof hi); hk.bytes(target, sizeof target);
        hk.bytes(p->h_pos.data(), p->h_pos.size() * sizeof(double));
        const int32_t mode = (p->has_rules ? 1 : 0) | (p->has_charge ? 2 : 0);
        hk.pod(mode);
        if (p->has_charge) hk.bytes(p->h_charge.data(), p->h_charge.size() * sizeof(double));
        if (p->has_rules)
            for (int64_t a = 0; a < p->natoms; ++a) {
                const int32_t k = p->h_kind[a];
                hk.pod((int32_t)(k < 0 ? -1 : (k | (kind_has_rule(k) ? (1 << 25) : 0))));
            }
        std::lock_guard<std::mutex> lock(g_image_mutex);
        for (size_t t = 0; t < g_image_cache.size(); ++t) {
            const std::shared_ptr<ImageSet> c = g_image_cache[t];
            if (c->device == p->device && c->key[0] == hk.a && c->key[1] == hk.b && c->natoms == p->natoms && c->cutoff2 == g.cutoff2 &&
                memcmp(c->lo, lo, sizeof lo) == 0 && memcmp(c->hi, hi, sizeof hi) == 0) {
                hit = c;
                std::rotate(g_image_cache.begin() + t, g_image_cache.begin() + t + 1, g_image_cache.end());      // most recently used last
                break;
            }
        }
    }
    if (hit) {
        g_image_hits.fetch_add(1);
        p->images = hit;
        const ImageSet& c = *hit;
        p->d_images = c.d_images; p->d_imgkind = c.d_imgkind; p->d_imgatom = c.d_imgatom; p->d_binstart = c.d_binstart;
        p->ib = c.ib;
        p->ib.kind = p->has_rules ? p->d_imgkind : nullptr;
        p->ib.atoms = p->d_atoms;
        p->images_built = true;
        p->images_from_cache = true;
        return CEG_OK;
    }
    if (cap > 0) g_image_misses.fetch_add(1);
    if (!std::getenv("CEG_HIP_IMAGES_ON_HOST")) {
        // round 4: the list is built on the device from the atom table that is already there (ceg_images.hip) -- byte-identical to
        // the host loop below, 1.0-1.4 ms -> ~0.2 ms for the 11 664-atom framework; CEG_HIP_IMAGES_ON_HOST=1 keeps the host build
        ceg::ImgBox B{};
        memcpy(B.mat, g.mat, sizeof B.mat);
        memcpy(B.invmat, g.invmat, sizeof B.invmat);
        for (int a = 0; a < 3; ++a) { B.lo[a] = lo[a]; B.hi[a] = hi[a]; B.bin[a] = bin[a]; B.nb[a] = nb[a]; }
        B.has_rules = p->has_rules ? 1 : 0;
        B.has_charge = p->has_charge ? 1 : 0;
        B.vdw_only = (p->has_rules && !p->has_charge) ? 1 : 0;
        B.nkinds = p->nkinds;
        int32_t* d_has = nullptr;
        if (p->has_rules && p->nkinds <= 1024) {
            for (int32_t k = 0; k < p->nkinds; ++k)
                if (kind_has_rule(k)) B.hasbits[k >> 6] |= 1ull << (k & 63);
        } else if (p->has_rules) {
            std::vector<int32_t> has((size_t)std::max(p->nkinds, 1), 0);
            for (int32_t k = 0; k < p->nkinds; ++k) has[k] = kind_has_rule(k) ? 1 : 0;
            if (int rc = upload(&d_has, has.data(), has.size())) return rc;
        }
        auto set = std::make_shared<ImageSet>();
        set->device = p->device;
        set->key[0] = hk.a; set->key[1] = hk.b;
        set->natoms = p->natoms; set->cutoff2 = g.cutoff2;
        memcpy(set->lo, lo, sizeof lo); memcpy(set->hi, hi, sizeof hi);
        int64_t n = 0;
        const hipError_t e = ceg::build_images_device(B, p->d_atoms, p->has_rules ? p->d_kind : nullptr, d_has, p->natoms, &set->d_images, &set->d_imgkind,
                                                      &set->d_imgatom, &set->d_binstart, &n);
        if (d_has) cached_free(d_has);          // (build_images_device has synchronised)
        if (e != hipSuccess) return fail(CEG_ERR_HIP, "building the lattice-image list on the device failed: %s", hipGetErrorString(e));
        set->bytes = (size_t)n * (sizeof(double4) + 2 * sizeof(int32_t)) + (size_t)(nb[0] * nb[1] * nb[2] + 1) * sizeof(int32_t);
        p->images = set;
        p->d_images = set->d_images; p->d_imgkind = set->d_imgkind; p->d_imgatom = set->d_imgatom; p->d_binstart = set->d_binstart;
        ImageBins& ib = p->ib;
        ib.xyzq = p->d_images;
        ib.kind = p->has_rules ? p->d_imgkind : nullptr;
        ib.atom = p->d_imgatom;
        ib.atoms = p->d_atoms;
        ib.bin_start = p->d_binstart;
        for (int a = 0; a < 3; ++a) {
            ib.lo[a] = lo[a];
            ib.bin[a] = bin[a];
            ib.inv_bin[a] = 1.0 / bin[a];
            ib.nb[a] = nb[a];
        }
        ib.nimages = (int32_t)n;
        p->images_built = true;
        set->ib = ib;
        if (cap > 0) {
            std::lock_guard<std::mutex> lock(g_image_mutex);
            g_image_cache.push_back(set);
            while ((int)g_image_cache.size() > cap) g_image_cache.erase(g_image_cache.begin());
        }
        return CEG_OK;
    }
    struct Img { double x, y, z, q; int32_t kind; int32_t bin; int32_t atom; };
    std::vector<Img> imgs;
    imgs.reserve((size_t)p->natoms * 8);
    const double* M = g.mat;
    const double* I = g.invmat;
    for (int64_t a = 0; a < p->natoms; ++a) {
        if (p->has_rules && !p->has_charge) {
            // a VdW-only plan (create_grid_vdw: one probe atom against the framework): atoms whose kind has no rule for the probe
            // contribute exact zeros (an empty rule run, src/interactions.jl:599-610) -- they need not be staged at all
            // (Si / Al against Ar or Na in the fixture force field: a third of the framework)
            if (!kind_has_rule(p->h_kind[a])) continue;
        }
        const double pa[3] = {p->h_pos[3 * a], p->h_pos[3 * a + 1], p->h_pos[3 * a + 2]};
        double fmin[3] = {1e300, 1e300, 1e300}, fmax[3] = {-1e300, -1e300, -1e300};
        for (int c = 0; c < 8; ++c) {
            const double d[3] = {((c & 1) ? hi[0] : lo[0]) - pa[0], ((c & 2) ? hi[1] : lo[1]) - pa[1],
                                 ((c & 4) ? hi[2] : lo[2]) - pa[2]};
            double f[3];
            matvec(I, d, f);
            for (int q = 0; q < 3; ++q) {
                fmin[q] = std::min(fmin[q], f[q]);
                fmax[q] = std::max(fmax[q], f[q]);
            }
        }
        int n0[3], n1[3];
        // an image pa + M n lies in the box only if n = I (P - pa) is inside the fractional hull of
        // the box corners, i.e. fmin <= n <= fmax componentwise (1e-9 guards the rounding of I*d)
        for (int q = 0; q < 3; ++q) {
            n0[q] = (int)std::ceil(fmin[q] - 1e-9);
            n1[q] = (int)std::floor(fmax[q] + 1e-9);
        }
        for (int nx = n0[0]; nx <= n1[0]; ++nx)
            for (int ny = n0[1]; ny <= n1[1]; ++ny)
                for (int nz = n0[2]; nz <= n1[2]; ++nz) {
                    const double P[3] = {pa[0] + (nx * M[0] + ny * M[3] + nz * M[6]),
                                         pa[1] + (nx * M[1] + ny * M[4] + nz * M[7]),
                                         pa[2] + (nx * M[2] + ny * M[5] + nz * M[8])};
                    if (P[0] < lo[0] || P[0] > hi[0] || P[1] < lo[1] || P[1] > hi[1] || P[2] < lo[2] ||
                        P[2] > hi[2])
                        continue;
                    int b[3];
                    for (int q = 0; q < 3; ++q) {
                        b[q] = (int)std::floor((P[q] - lo[q]) / bin[q]);
                        b[q] = std::min(std::max(b[q], 0), nb[q] - 1);
                    }
                    Img im;
                    im.x = P[0]; im.y = P[1]; im.z = P[2];
                    im.q = p->has_charge ? p->h_charge[a] : 0.0;
                    // kind (low 24 bits) + bit 25: the kind has at least one VdW rule (= META_HASVDW of the kernel), so that the
                    // staging loop does not have to look the rule offsets up per image
                    im.kind = -1;
                    if (p->has_rules) {
                        const int32_t k = p->h_kind[a];
                        im.kind = k < 0 ? -1 : (k | (kind_has_rule(k) ? (1 << 25) : 0));
                    }
                    im.bin = (b[0] * nb[1] + b[1]) * nb[2] + b[2];
                    im.atom = (int32_t)a;
                    imgs.push_back(im);
                }
    }
    if (imgs.size() > 0x7ffffff0ull) return fail(CEG_ERR_UNSUPPORTED, "too many lattice images");
    const size_t nbins = (size_t)nb[0] * nb[1] * nb[2];
    std::vector<int32_t> start(nbins + 1, 0);
    for (const Img& im : imgs) start[im.bin + 1]++;
    for (size_t b = 0; b < nbins; ++b) start[b + 1] += start[b];
    std::vector<int32_t> cursor(start.begin(), start.end() - 1);
    std::vector<double4> xyzq(imgs.size());
    std::vector<int32_t> kind(imgs.size());
    std::vector<int32_t> atom(imgs.size());
    for (const Img& im : imgs) {       // stable: atom order, then lattice order, inside each bin
        const int32_t s = cursor[im.bin]++;
        xyzq[s] = make_double4(im.x, im.y, im.z, im.q);
        kind[s] = im.kind;
        atom[s] = im.atom;
    }
    auto set = std::make_shared<ImageSet>();
    set->device = p->device;
    set->key[0] = hk.a; set->key[1] = hk.b;
    set->natoms = p->natoms; set->cutoff2 = g.cutoff2;
    memcpy(set->lo, lo, sizeof lo); memcpy(set->hi, hi, sizeof hi);
    if (int rc = upload(&set->d_images, xyzq.data(), xyzq.size())) return rc;
    if (int rc = upload(&set->d_imgkind, kind.data(), kind.size())) return rc;
    if (int rc = upload(&set->d_imgatom, atom.data(), atom.size())) return rc;
    if (int rc = upload(&set->d_binstart, start.data(), start.size())) return rc;
    set->bytes = xyzq.size() * sizeof(double4) + (kind.size() + atom.size() + start.size()) * sizeof(int32_t);
    p->images = set;
    p->d_images = set->d_images; p->d_imgkind = set->d_imgkind; p->d_imgatom = set->d_imgatom; p->d_binstart = set->d_binstart;
    ImageBins& ib = p->ib;
    ib.xyzq = p->d_images;
    ib.kind = p->has_rules ? p->d_imgkind : nullptr;
    ib.atom = p->d_imgatom;
    ib.atoms = p->d_atoms;
    ib.bin_start = p->d_binstart;
    for (int a = 0; a < 3; ++a) {
        ib.lo[a] = lo[a];
        ib.bin[a] = bin[a];
        ib.inv_bin[a] = 1.0 / bin[a];
        ib.nb[a] = nb[a];
    }
    ib.nimages = (int32_t)imgs.size();
    p->images_built = true;
    set->ib = ib;
    if (cap > 0) {
        std::lock_guard<std::mutex> lock(g_image_mutex);
        g_image_cache.push_back(set);
        while ((int)g_image_cache.size() > cap) g_image_cache.erase(g_image_cache.begin());     // (freed when the last plan lets go)
    }
    return CEG_OK;
}

// Function tables of the fast real-space Ewald term (csrc/ceg_math.h): erfcx on
// [alpha*R_EXACT, alpha*cutoff] as ERFCX_TAB_N degree-5 pieces (Chebyshev-node interpolation in
// long double), and 2^(j/64).  Returns false (fast path disabled, libm-grade erfc used instead)
// if the fit does not reach 1e-14.
bool build_ewald_tables_uncached(double alpha, double cutoff2, std::vector<double>& tab, std::vector<double>& exp2_tab,
                                 double* inv_h_out, double* mx0_inv_h_out);

// the long-double fit takes ~2 ms; every Coulomb grid of a run uses the same (alpha, cutoff)
bool build_ewald_tables(double alpha, double cutoff2, std::vector<double>& tab, std::vector<double>& exp2_tab,
                        double* inv_h_out, double* mx0_inv_h_out)
{
    struct Memo { bool valid = false, ok = false; double alpha = 0, cutoff2 = 0, inv_h = 0, mx0 = 0; std::vector<double> tab, e2; };
    static std::mutex m;
    static Memo memo;
    std::lock_guard<std::mutex> lock(m);
    if (!(memo.valid && memo.alpha == alpha && memo.cutoff2 == cutoff2)) {
        memo.tab.clear(); memo.e2.clear();
        memo.ok = build_ewald_tables_uncached(alpha, cutoff2, memo.tab, memo.e2, &memo.inv_h, &memo.mx0);
        memo.alpha = alpha; memo.cutoff2 = cutoff2; memo.valid = true;
    }
    tab = memo.tab; exp2_tab = memo.e2; *inv_h_out = memo.inv_h; *mx0_inv_h_out = memo.mx0;
    return memo.ok;
}

bool build_ewald_tables_uncached(double alpha, double cutoff2, std::vector<double>& tab, std::vector<double>& exp2_tab,
                                 double* inv_h_out, double* mx0_inv_h_out)
{
    const int N = CEG_ERFCX_TAB_N;
    const long double x0 = (long double)alpha * std::sqrt((long double)CEG_R_EXACT2) * (1.0L - 1e-6L);
    const long double x1 = (long double)alpha * std::sqrt((long double)cutoff2 * (1.0L + 2e-9L)) * (1.0L + 1e-6L);
    if (!(x1 > x0) || x1 > 5.0L * (1.0L - 1e-9L)) return false;   // 5 = ERFCX_XMAX of the slow path's polynomial
    const long double h = (x1 - x0) / N;
    auto erfcx = [](long double x) { return expl(x * x) * erfcl(x); };
    tab.assign((size_t)N * 6, 0.0);
    const long double PI = 3.14159265358979323846264338327950288L;
    long double node[6];
    for (int k = 0; k < 6; ++k) node[k] = 0.5L + 0.5L * cosl(PI * (k + 0.5L) / 6.0L);   // s in [0, 1]
    double worst = 0.0;
    for (int i = 0; i < N; ++i) {
        const long double lo = x0 + i * h;
        long double V[6][7];
        for (int r = 0; r < 6; ++r) {
            long double pw = 1.0L;
            for (int c = 0; c < 6; ++c) { V[r][c] = pw; pw *= node[r]; }
            V[r][6] = erfcx(lo + node[r] * h);
        }
        for (int c = 0; c < 6; ++c) {                       // Gauss-Jordan with partial pivoting
            int piv = c;
            for (int r = c + 1; r < 6; ++r) if (fabsl(V[r][c]) > fabsl(V[piv][c])) piv = r;
            for (int q = 0; q < 7; ++q) std::swap(V[c][q], V[piv][q]);
            const long double d = V[c][c];
            for (int q = 0; q < 7; ++q) V[c][q] /= d;
            for (int r = 0; r < 6; ++r) if (r != c) {
                const long double f = V[r][c];
                for (int q = 0; q < 7; ++q) V[r][q] -= f * V[c][q];
            }
        }
        for (int c = 0; c < 6; ++c) tab[(size_t)i * 6 + c] = (double)V[c][6];
        for (int t = 0; t <= 8; ++t) {                      // accuracy check with a double Horner
            const double sl = t / 8.0;
            double pv = tab[(size_t)i * 6 + 5];
            for (int c = 4; c >= 0; --c) pv = pv * sl + tab[(size_t)i * 6 + c];
            const long double ref = erfcx(lo + (long double)sl * h);
            worst = std::max(worst, (double)fabsl(((long double)pv - ref) / ref));
        }
    }
    if (!(worst < 1e-14)) return false;
    exp2_tab.resize(64);
    for (int j = 0; j < 64; ++j) exp2_tab[j] = (double)exp2l((long double)j / 64.0L);
    *inv_h_out = (double)(1.0L / h);
    *mx0_inv_h_out = (double)(-x0 / h);
    return true;
}

// r^2-indexed tables of B0(s) = erfc(alpha sqrt(s))/sqrt(s) and C(s) = 2 alpha/sqrt(pi) exp(-alpha^2 s) (ceg_internal.h,
// CEG_EW2_* / CEG_EW2F_*): per interval an interpolant of the layout's degree at the Chebyshev nodes of the interval, in long double,
// expressed in t = s - s_lo (the interval's lower end: clearing the low bits of s gives it).  Returns false if the range needs more
// than the layout's ni_max intervals or a polynomial misses the tolerance (relative) anywhere -- the caller then keeps the erfcx /
// libm variants (coarse layout) or the coarse table (fine layout).
// `which` 0: the two Ewald functions (record = 2 (degree + 1) doubles, tolerance relative);  1: G0(s) = A exp(-B sqrt(s)) of a
// Buckingham class with alpha := B, record = CEG_BK2_STRIDE doubles, tolerance relative to G0 at the start of the table + the
// dispersion term C/s^3 it is added to (exp(-B r) spans 17 decades up to the cutoff).
struct Ew2Layout {
    int logm;          // 2^logm intervals per octave of s
    int degree;        // of each polynomial
    int ni_max;        // intervals the kernels have room for
    int cover_logm;    // the table ends where a table with 2^cover_logm intervals per octave ends (<= logm)
    constexpr int shift() const { return 20 - logm; }              // bits of the high word below the interval key
    constexpr int nd() const { return degree + 1; }                // coefficients per polynomial = Chebyshev nodes per interval
    constexpr int stride() const { return 2 * nd(); }              // doubles per record of the Ewald pair
    bool operator==(const Ew2Layout& o) const { return logm == o.logm && degree == o.degree && ni_max == o.ni_max && cover_logm == o.cover_logm; }
};
constexpr Ew2Layout EW2_COARSE{CEG_EW2_LOGM, 6, CEG_EW2_NI_MAX, CEG_EW2_LOGM};
// (the fine table covers the range of the ordinary one, two intervals for each of its: 330 for 165 at 12 A, at most 352 for 176)
constexpr Ew2Layout EW2_FINE{CEG_EW2F_LOGM, CEG_EW2F_ND - 1, CEG_EW2F_NI_MAX, CEG_EW2_LOGM};
constexpr Ew2Layout BK2_LAYOUT{CEG_BK2_LOGM, CEG_BK2_ND - 1, CEG_BK2_NI_MAX, CEG_BK2_LOGM};
static_assert(EW2_COARSE.stride() == CEG_EW2_STRIDE && EW2_COARSE.shift() == CEG_EW2_SHIFT, "coarse layout");
static_assert(EW2_FINE.stride() == CEG_EW2F_STRIDE && EW2_FINE.shift() == CEG_EW2F_SHIFT, "fine layout");
static_assert(BK2_LAYOUT.nd() <= CEG_BK2_STRIDE && BK2_LAYOUT.shift() == CEG_BK2_SHIFT, "Buckingham layout");

bool build_ew2_table_uncached(double alpha, double r_exact2, double cutoff2, const Ew2Layout& lay, std::vector<double>& tab, int32_t* base_out,
                              int32_t* ni_out, double* worst_out, int which = 0, double bkA = 0.0, double bkC = 0.0)
{
    const int SHIFT = lay.shift(), ni_max = lay.ni_max;
    auto key_of = [SHIFT](double s) { uint64_t b; memcpy(&b, &s, 8); return (int32_t)((uint32_t)(b >> 32) >> SHIFT); };
    *base_out = 0; *ni_out = 0; *worst_out = 0.0;
    if (!(alpha > 0.0) || !(r_exact2 >= 1.0) || !(cutoff2 > r_exact2) || lay.degree < 1 || lay.logm < 0 || lay.logm > 12 || lay.cover_logm < 0 ||
        lay.cover_logm > lay.logm)
        return false;
    const int up = lay.logm - lay.cover_logm;              // last interval: the one that ends where the covering layout's last one ends
    const int32_t base = key_of(r_exact2), last = (((key_of(cutoff2 * (1.0 + 4e-9) + 4e-9) >> up) + 1) << up) - 1;
    const int32_t ni = last - base + 1;
    *base_out = base; *ni_out = ni;
    if (ni < 1 || ni > ni_max) return false;
    const long double a = alpha, ka = 2.0L * a / sqrtl(3.14159265358979323846264338327950288L);
    auto B0 = [&](long double s) { const long double r = sqrtl(s); return which == 0 ? erfcl(a * r) / r : (long double)bkA * expl(-a * r); };
    auto Cf = [&](long double s) { return ka * expl(-a * a * s); };
    const int nf = which == 0 ? 2 : 1, stride = which == 0 ? lay.stride() : CEG_BK2_STRIDE;
    const int ND = lay.nd();                               // coefficients per polynomial: degree 6 / 5 (Ewald pair, 14 / 12 doubles) / degree 7
    const int NC = ND + 1;                                 // columns of the augmented Vandermonde matrix
    const long double PI = 3.14159265358979323846264338327950288L;
    std::vector<long double> node((size_t)ND), Vm((size_t)ND * NC), cu((size_t)ND), ct((size_t)ND);
    auto V = [&](int r, int c) -> long double& { return Vm[(size_t)r * NC + c]; };
    for (int k = 0; k < ND; ++k) node[k] = cosl(PI * (k + 0.5L) / (long double)ND);       // u in [-1, 1]
    tab.assign((size_t)ni * stride, 0.0);
    double worst = 0.0;
    for (int32_t i = 0; i < ni; ++i) {
        const uint64_t lo_bits = (uint64_t)(uint32_t)((base + i) << SHIFT) << 32;
        const uint64_t mid_bits = lo_bits | ((uint64_t)1 << (32 + SHIFT - 1));
        const uint64_t hi_bits = (uint64_t)(uint32_t)((base + i + 1) << SHIFT) << 32;
        double s_lo, s_mid, s_hi;
        memcpy(&s_lo, &lo_bits, 8); memcpy(&s_mid, &mid_bits, 8); memcpy(&s_hi, &hi_bits, 8);
        const long double hh = 0.5L * ((long double)s_hi - (long double)s_lo);           // half width; s_mid is the exact centre
        for (int f = 0; f < nf; ++f) {
            for (int r = 0; r < ND; ++r) {
                long double pw = 1.0L;
                for (int c = 0; c < ND; ++c) { V(r, c) = pw; pw *= node[r]; }
                const long double s = (long double)s_mid + node[r] * hh;
                V(r, ND) = f == 0 ? B0(s) : Cf(s);
            }
            for (int c = 0; c < ND; ++c) {                      // Gauss-Jordan with partial pivoting
                int piv = c;
                for (int r = c + 1; r < ND; ++r) if (fabsl(V(r, c)) > fabsl(V(piv, c))) piv = r;
                for (int q = 0; q <= ND; ++q) std::swap(V(c, q), V(piv, q));
                const long double d = V(c, c);
                for (int q = 0; q <= ND; ++q) V(c, q) /= d;
                for (int r = 0; r < ND; ++r) if (r != c) {
                    const long double g = V(r, c);
                    for (int q = 0; q <= ND; ++q) V(r, q) -= g * V(c, q);
                }
            }
            // P(u), u = (t - hh)/hh with t = s - s_lo  ->  coefficients in t (binomial expansion in long double)
            std::fill(ct.begin(), ct.end(), 0.0L);
            long double sc = 1.0L;
            for (int c = 0; c < ND; ++c) { cu[c] = V(c, ND) * sc; sc /= hh; }             // in (t - hh)
            for (int c = 0; c < ND; ++c) {                                                 // (t - hh)^c = sum_k C(c,k) t^k (-hh)^(c-k)
                long double binom = 1.0L;
                for (int k = 0; k <= c; ++k) {
                    ct[k] += cu[c] * binom * powl(-hh, c - k);
                    binom = binom * (c - k) / (k + 1);
                }
            }
            double* co = &tab[(size_t)i * stride + ND * f];
            for (int c = 0; c < ND; ++c) co[c] = (double)ct[c];
            for (int q = 0; q <= 16; ++q) {                      // accuracy check with the kernel's double Horner
                const double t = (double)(((long double)q / 16.0L) * 2.0L * hh * (1.0L - 1e-12L));
                double pv = co[ND - 1];
                for (int c = ND - 2; c >= 0; --c) pv = __builtin_fma(pv, t, co[c]);
                const long double s = (long double)s_lo + (long double)t;
                const long double ref = f == 0 ? B0(s) : Cf(s);
                const long double scale = which == 0 ? fabsl(ref) : fabsl(ref) + fabsl((long double)bkC) / (s * s * s);
                worst = std::max(worst, (double)fabsl(((long double)pv - ref) / scale));
            }
        }
    }
    *worst_out = worst;
    return worst < 5e-11;
}

// memoised per layout: a plan asks for the coarse and for the fine table of the same (alpha, r_exact2, cutoff2)
bool build_ew2_table(double alpha, double r_exact2, double cutoff2, const Ew2Layout& lay, std::vector<double>& tab, int32_t* base_out,
                     int32_t* ni_out, double* worst_out = nullptr)
{
    struct Memo { bool valid = false, ok = false; Ew2Layout lay{0, 0, 0, 0}; double alpha = 0, r_exact2 = 0, cutoff2 = 0, worst = 0; int32_t base = 0, ni = 0; std::vector<double> tab; };
    static std::mutex m;
    static Memo memos[2];
    std::lock_guard<std::mutex> lock(m);
    Memo& memo = memos[lay == EW2_COARSE ? 0 : 1];
    if (!(memo.valid && memo.lay == lay && memo.alpha == alpha && memo.r_exact2 == r_exact2 && memo.cutoff2 == cutoff2)) {
        memo.tab.clear();
        memo.ok = build_ew2_table_uncached(alpha, r_exact2, cutoff2, lay, memo.tab, &memo.base, &memo.ni, &memo.worst);
        memo.lay = lay; memo.alpha = alpha; memo.r_exact2 = r_exact2; memo.cutoff2 = cutoff2; memo.valid = true;
        if (std::getenv("CEG_HIP_TRACE"))
            fprintf(stderr, "[ceg_hip] r^2-indexed Ewald table (%d per octave, degree %d): %d intervals, worst relative error %.2e -> %s\n",
                    1 << lay.logm, lay.degree, memo.ni, memo.worst, memo.ok ? "used" : "not used");
    }
    tab = memo.tab; *base_out = memo.base; *ni_out = memo.ni;
    if (worst_out) *worst_out = memo.worst;
    return memo.ok;
}

bool build_bk2_table(double A, double B, double C, double r_exact2, double cutoff2, std::vector<double>& tab, int32_t* base_out, int32_t* ni_out)
{
    struct Memo { bool valid = false, ok = false; double A = 0, B = 0, C = 0, r_exact2 = 0, cutoff2 = 0; int32_t base = 0, ni = 0; std::vector<double> tab; };
    static std::mutex m;
    static Memo memo;
    std::lock_guard<std::mutex> lock(m);
    if (!(memo.valid && memo.A == A && memo.B == B && memo.C == C && memo.r_exact2 == r_exact2 && memo.cutoff2 == cutoff2)) {
        memo.tab.clear();
        double worst = 0.0;
        memo.ok = build_ew2_table_uncached(B, r_exact2, cutoff2, BK2_LAYOUT, memo.tab, &memo.base, &memo.ni, &worst, 1, A, C) && worst < CEG_BK2_TOL;
        memo.A = A; memo.B = B; memo.C = C; memo.r_exact2 = r_exact2; memo.cutoff2 = cutoff2; memo.valid = true;
        if (std::getenv("CEG_HIP_TRACE"))
            fprintf(stderr, "[ceg_hip] r^2-indexed Buckingham table: %d intervals, worst error %.2e of the pair energy -> %s\n", memo.ni, worst,
                    memo.ok ? "used" : "not used");
    }
    tab = memo.tab; *base_out = memo.base; *ni_out = memo.ni;
    return memo.ok;
}

}  // namespace

int ceg_host::check_common(const double* pos, int64_t natoms, const double* mat, const double* invmat,
                           const int32_t* dims, const double* size, const double* shift, const double* delta)
{
    if (!pos && natoms > 0) return fail(CEG_ERR_INVALID, "pos is NULL");
    if (natoms < 0) return fail(CEG_ERR_INVALID, "natoms < 0");
    if (!mat || !invmat || !dims || !size || !shift || !delta)
        return fail(CEG_ERR_INVALID, "NULL geometry argument");
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1) return fail(CEG_ERR_INVALID, "dims[%d] = %d < 1", a, dims[a]);
    return CEG_OK;
}

// out[i] = kind of image i | META_HASVDW iff has[kind] (the flag bit is bit 25: what build_images sets for the union of the probes)
__global__ void k_probe_image_flags(const int32_t* __restrict__ kind_union, const int32_t* __restrict__ has, int32_t nkinds, int32_t* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t kw = kind_union[i];
    if (kw < 0) { out[i] = kw; return; }
    const int32_t k = kw & ((1 << 24) - 1);
    out[i] = k | ((k < nkinds && has[k]) ? (1 << 25) : 0);
}

static int probe_image_flags(const int32_t* d_union, const int32_t* d_has, int32_t nkinds, int32_t* d_out, int64_t n)
{
    if (n <= 0) return CEG_OK;
    hipLaunchKernelGGL(k_probe_image_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d_union, d_has, nkinds, d_out, n);
    return hipGetLastError() == hipSuccess ? CEG_OK : fail(CEG_ERR_HIP, "image-flag kernel launch failed");
}

// nprobes == 0: the ordinary plan of ceg_plan_create (rules / rule_offset may be NULL: Coulomb only);
// nprobes >= 1: a multi-probe plan, mrules / moffset [nprobes], probes of any rule class ceg_plan_create takes
static int create_impl(ceg_plan_t** plan, int32_t device,
                       const double* pos, const int64_t* atomkind, const double* charge,
                       int64_t natoms,
                       const double mat[9], const double invmat[9],
                       int32_t ortho, double safemin2, double cutoff2,
                       const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                       int32_t nprobes, const ceg_rule_t* const* mrules, const int32_t* const* moffset,
                       double alpha,
                       const int32_t dims[3], const double size[3], const double shift[3],
                       const double delta[3])
{
    if (!plan) return fail(CEG_ERR_INVALID, "plan is NULL");
    *plan = nullptr;
    if (int rc = check_common(pos, natoms, mat, invmat, dims, size, shift, delta)) return rc;
    if (nprobes < 0 || nprobes > CEG_MAX_PROBES) return fail(CEG_ERR_INVALID, "nprobes = %d outside 1..%d", nprobes, CEG_MAX_PROBES);
    if (nprobes > 0) {
        if (!mrules || !moffset || !atomkind || nkinds <= 0) return fail(CEG_ERR_INVALID, "rule tables / atomkind missing");
        for (int q = 0; q < nprobes; ++q)
            if (!mrules[q] || !moffset[q]) return fail(CEG_ERR_INVALID, "rule table of probe %d is NULL", q);
        rules = mrules[0];
        rule_offset = moffset[0];
    }
    const bool trace = std::getenv("CEG_HIP_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (trace)
            fprintf(stderr, "[ceg plan] %-28s %8.3f ms\n", what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    const int ndev = ceg_device_count();
    if (ndev <= 0) return fail(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(CEG_ERR_NO_DEVICE, "device %d not present (%d devices)", device, ndev);
    const bool has_rules = rules && rule_offset && atomkind && nkinds > 0;
    if (!has_rules && !charge) return fail(CEG_ERR_INVALID, "plan needs rules+atomkind and/or charges");

    ceg_plan* p = new ceg_plan();
    p->device = device;
    p->natoms = natoms;
    p->has_rules = has_rules;
    p->has_charge = charge != nullptr;
    Geom& g = p->g;
    memcpy(g.mat, mat, sizeof g.mat);
    memcpy(g.invmat, invmat, sizeof g.invmat);
    for (int a = 0; a < 3; ++a) {
        g.size[a] = size[a];
        g.shift[a] = shift[a];
        g.delta[a] = delta[a];
        g.dims[a] = dims[a];
    }
    g.ortho = ortho ? 1 : 0;
    g.safemin2 = safemin2;
    g.cutoff2 = cutoff2;
    g.alpha = alpha;
    g.diag = (mat[1] == 0 && mat[2] == 0 && mat[3] == 0 && mat[5] == 0 && mat[6] == 0 && mat[7] == 0) ? 1 : 0;

    p->h_pos.assign(pos, pos + 3 * natoms);
    if (charge) p->h_charge.assign(charge, charge + natoms);
    p->h_kind.assign(natoms, -1);
    if (has_rules) {
        for (int64_t a = 0; a < natoms; ++a) {
            const int64_t k = atomkind[a];
            if (k < 1 || k > nkinds) {
                delete p;
                return fail(CEG_ERR_INVALID, "atomkind[%lld] = %lld outside 1..%d", (long long)a, (long long)k, nkinds);
            }
            p->h_kind[a] = (int32_t)(k - 1);
        }
        if (int rc = convert_rules(p, rules, rule_offset, nkinds)) {
            delete p;
            return rc;
        }
        if (nprobes > 0) {
            // every probe through the same classification; the plan keeps probe 0 in its single-probe fields and the union of the
            // probes' "kind has a rule" sets in h_offset (what build_images turns into the per-image flag)
            p->nprobes = nprobes;
            p->probes.resize(nprobes);
            std::vector<int32_t> any(nkinds, 0);
            double r_exact2 = CEG_R_EXACT2;
            for (int q = 0; q < nprobes; ++q) {
                if (q > 0)
                    if (int rc = convert_rules(p, mrules[q], moffset[q], nkinds)) { delete p; return rc; }
                // Probes of any rule class share the plan (round 4: the grids of Na + CO2, src/raspa.jl:497-520, from one image list).
                // The Lennard-Jones-only ones share accumulating loops (ceg_plan_build_multi); a probe of another class -- a
                // Buckingham cation -- runs the single-probe kernels of its class from the same list, alone or fused with the Coulomb grid.
                ceg_plan::ProbeTab& t = p->probes[q];
                t.rules = p->h_rules; t.offset = p->h_offset; t.fast = p->h_fast;
                t.vdwk = p->vdwk; t.single_buck = p->single_buck;
                set_uniform_class(p);
                t.uni = p->uni;
                for (int c = 0; c < 4; ++c) t.bk[c] = p->bk[c];
                r_exact2 = std::max(r_exact2, p->r_exact2);          // ONE exact-path radius for the plan: the largest any probe asks for
                for (int32_t k = 0; k < nkinds; ++k) any[k] |= (t.offset[k + 1] > t.offset[k]) ? 1 : 0;
            }
            p->r_exact2 = r_exact2;
            if (!(r_exact2 < p->g.cutoff2)) {
                delete p;
                return fail(CEG_ERR_UNSUPPORTED, "a hard sphere of one of the probes reaches the cutoff: build that grid with a plan of its own");
            }
            p->h_rules = p->probes[0].rules; p->h_fast = p->probes[0].fast;
            p->vdwk = p->probes[0].vdwk; p->single_buck = p->probes[0].single_buck;
            for (int c = 0; c < 4; ++c) p->bk[c] = p->probes[0].bk[c];
            p->h_offset_union.assign(nkinds + 1, 0);
            for (int32_t k = 0; k < nkinds; ++k) p->h_offset_union[k + 1] = p->h_offset_union[k] + any[k];
            p->h_offset = p->probes[0].offset;
            p->uni = UniformClass{};      // the plan-level block serves the multi-probe launches and the Coulomb grid: per-candidate records
        } else {
            set_uniform_class(p);
        }
        // CEG_HIP_UNIFORM_CLASS=0 keeps the per-candidate records (one library runs both paths: tests, A/B); =1 defers the
        // Lennard-Jones constants only
        if (const char* e = std::getenv("CEG_HIP_UNIFORM_CLASS")) {
            const int cap = std::max(0, atoi(e));
            auto limit = [cap](UniformClass& u) { if (u.cls > cap) u.cls = cap; if (u.cls == 0) u = UniformClass{}; };
            limit(p->uni);
            for (auto& t : p->probes) limit(t.uni);
        }
    }
    // culling needs: finite cutoff, every perpendicular width >= 2*cutoff (two images of one atom
    // are then never both inside the cutoff), which ProbeSystem guarantees (src/probes.jl:24)
    double w[3];
    perpendicular_widths(g.mat, w);
    const double cutoff = std::sqrt(cutoff2);
    p->can_cull = std::isfinite(cutoff2) && cutoff2 > 0 &&
                  std::min(w[0], std::min(w[1], w[2])) >= 2.0 * cutoff * (1.0 - 1e-12);

    stamp("host: rules, geometry");
    DeviceGuard guard(device);
    if (!guard.ok) {
        delete p;
        return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", device);
    }
    StagingLease lease;                 // the page-locked area the uploads below go through
    std::vector<double4> xyzq((size_t)natoms);
    for (int64_t a = 0; a < natoms; ++a)
        xyzq[a] = make_double4(pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], charge ? charge[a] : 0.0);
    int rc = upload(&p->d_atoms, xyzq.data(), xyzq.size());
    if (!rc) rc = upload(&p->d_kind, p->h_kind.data(), p->h_kind.size());
    if (!rc) rc = upload(&p->d_rules, p->h_rules.data(), p->h_rules.size());
    if (!rc) {
        if (p->h_offset.empty()) p->h_offset.assign(1, 0);
        rc = upload(&p->d_offset, p->h_offset.data(), p->h_offset.size());
    }
    stamp("atom / rule tables uploaded");
    if (!rc && p->can_cull) rc = build_images(p);
    stamp(p->images_from_cache ? "images: cache hit" : "images built + uploaded");
    if (!rc && p->can_cull) {
        PlanConst hc{};
        hc.g = p->g;
        hc.ib = p->ib;
        hc.rt = RuleTable{p->d_rules, p->d_offset, p->nkinds};
        hc.alpha2 = alpha * alpha;
        hc.r_exact2 = p->r_exact2;
        {   // |f_k(centre - image)| <= |row_k(invmat)| (reach of a kept image from the tile centre) for every image a 4x4x4 tile can
            // keep; if that plus the fractional half-extent of the tile stays below 1/2 on all three axes the kernel skips the test
            // (the tile's extent follows from size / dims, which is what grid_coord steps by -- NOT from the caller's `delta`, which
            // only scales the derivative channels, grids.jl:126-133, and may be anything)
            const double hx = 1.5 * size[0] / dims[0], hy = 1.5 * size[1] / dims[1], hz = 1.5 * size[2] / dims[2];
            const double reach = std::sqrt(cutoff2 * (1.0 + 1e-9) + 1e-9) + std::sqrt(hx * hx + hy * hy + hz * hz);
            bool all = true;
            for (int k = 0; k < 3; ++k) {
                const double rown = std::sqrt(invmat[k] * invmat[k] + invmat[k + 3] * invmat[k + 3] + invmat[k + 6] * invmat[k + 6]);
                const double ek = std::fabs(invmat[k]) * hx + std::fabs(invmat[k + 3]) * hy + std::fabs(invmat[k + 6]) * hz + 1e-9;
                if (!(rown * reach + ek < 0.5 - 1e-6)) all = false;
            }
            hc.all_simple = all ? 1 : 0;
        }
        if (p->h_fast.empty()) p->h_fast.assign(1, FastVdw{});
        rc = upload(&p->d_fast, p->h_fast.data(), p->h_fast.size());
        hc.fastvdw = p->d_fast;
        fill_uniform_class(hc, p->uni);
        p->fast_ewald = false;
        bool any_vdwk2 = p->vdwk == 2;
        for (const auto& t : p->probes) any_vdwk2 = any_vdwk2 || t.vdwk == 2;
        if (!rc && ((p->has_charge && std::isfinite(alpha) && alpha > 0) || any_vdwk2)) {
            std::vector<double> tab, e2;
            double inv_h = 0, mx0 = 0;
            const bool want_ewald = p->has_charge && std::isfinite(alpha) && alpha > 0;
            const bool ok = build_ewald_tables(want_ewald ? alpha : 0.25, cutoff2, tab, e2, &inv_h, &mx0);
            if (!ok && p->vdwk == 2) p->vdwk = 0;       // no exp table: Buckingham stays on the generic path
            if (!ok)
                for (auto& t : p->probes)
                    if (t.vdwk == 2) t.vdwk = 0;
            if (ok) {
                rc = upload(&p->d_erfcx, tab.data(), tab.size());
                if (!rc) rc = upload(&p->d_exp2, e2.data(), e2.size());
                hc.erfcx_tab = p->d_erfcx;
                hc.exp2_tab = p->d_exp2;
                hc.erfcx_inv_h = inv_h;
                hc.erfcx_mx0_inv_h = mx0;
                p->fast_ewald = want_ewald;
            }
            hc.ew_k3 = 2.0 * alpha * alpha / 3.0;
            hc.ew_k15 = 4.0 * (alpha * alpha) * (alpha * alpha) / 15.0;
            if (ok && want_ewald && !rc && !std::getenv("CEG_HIP_NO_EW2")) {
                std::vector<double> t2;
                int32_t base = 0, ni = 0;
                if (build_ew2_table(alpha, p->r_exact2, cutoff2, EW2_COARSE, t2, &base, &ni)) {
                    rc = upload(&p->d_ew2, t2.data(), t2.size());
                    hc.ew2_tab = p->d_ew2;
                    hc.ew2_ni = ni;
                    hc.ew2_base = base;
                    p->ew2 = !rc;
                }
                // the fine layout beside it (a cutoff that needs more intervals than the kernels hold has none: nothing else changes).
                // CEG_HIP_EW2_FINE=0 keeps the coarse table alone: one library runs both paths (tests, A/B)
                const char* fine_env = std::getenv("CEG_HIP_EW2_FINE");
                if (p->ew2 && !(fine_env && atoi(fine_env) == 0) && build_ew2_table(alpha, p->r_exact2, cutoff2, EW2_FINE, t2, &base, &ni)) {
                    rc = upload(&p->d_ew2f, t2.data(), t2.size());
                    hc.ew2f_tab = p->d_ew2f;
                    hc.ew2f_ni = ni;
                    hc.ew2f_base = base;
                    p->ew2f = !rc;
                }
            }
        }
        // the r^2-indexed table of ONE Buckingham class (VDWK = 3): G0/C, the hot loop accumulates the channels divided by C, 6C, -48C,
        // 480C (ceg_kernels.hip); `target` receives the table and its scalar constants
        auto setup_bk2 = [&](int& vdwk, bool single_buck, const double bk[4], double** d_tab, PlanConst& target) {
            if (rc || vdwk != 2 || !single_buck || std::getenv("CEG_HIP_NO_BK2")) return;
            std::vector<double> tb;
            int32_t base = 0, ni = 0;
            if (!build_bk2_table(bk[0] / bk[2], bk[1], 1.0, p->r_exact2, cutoff2, tb, &base, &ni)) return;
            rc = upload(d_tab, tb.data(), tb.size());
            target.bk2_tab = *d_tab;
            target.bk2_ni = ni;
            target.bk2_base = base;
            const double B = bk[1], C = bk[2];
            target.bk_B = B; target.bk_C = C; target.bk_invC = 1.0 / C; target.bk_nshift = -bk[3] / C;
            target.bk_c1 = -B / 6.0; target.bk_c2 = -B / 48.0; target.bk_c3 = B * B / 3.0; target.bk_c4 = -B / 160.0;
            target.bk_s1 = 1.0 / (6.0 * C); target.bk_s2 = -1.0 / (48.0 * C); target.bk_s3 = 1.0 / (480.0 * C);
            if (!rc) vdwk = 3;
        };
        if (p->nprobes == 0) setup_bk2(p->vdwk, p->single_buck, p->bk, &p->d_bk2, hc);
        if (!rc && p->nprobes > 0) {
            // (without the r^2-indexed Ewald tables -- alpha * cutoff > 5, or a fit that misses its tolerance -- the Coulomb grid is
            //  built by its own launch with the erfcx / libm-grade arithmetic and only the VdW grids share a pass: ceg_plan_build_multi)
            hc.nprobes = p->nprobes;
            for (int q = 0; q < p->nprobes && !rc; ++q) {
                ceg_plan::ProbeTab& t = p->probes[q];
                rc = upload(&t.d_rules, t.rules.data(), t.rules.size());
                if (!rc) rc = upload(&t.d_offset, t.offset.data(), t.offset.size());
                if (!rc) rc = upload(&t.d_fast, t.fast.data(), t.fast.size());
                hc.rtm[q] = RuleTable{t.d_rules, t.d_offset, p->nkinds};
                hc.fastm[q] = t.d_fast;
            }
            for (int q = 0; q < p->nprobes && !rc; ++q) {        // the block with probe q in the single-probe slots
                ceg_plan::ProbeTab& t = p->probes[q];
                PlanConst hq = hc;
                hq.rt = hc.rtm[q];
                hq.fastvdw = hc.fastm[q];
                fill_uniform_class(hq, t.uni);
                setup_bk2(t.vdwk, t.single_buck, t.bk, &t.d_bk2, hq);
                // per image: does ITS kind have a rule with this probe?  The shared list carries the union of the probes (what the
                // launches of several Lennard-Jones probes stage by); a single-probe launch drops / declasses the images that are
                // inactive for its probe -- the tabulated Buckingham class carries no per-candidate parameters that could be zero.
                if (!rc && p->nprobes > 1) {
                    std::vector<int32_t> has((size_t)p->nkinds);
                    for (int32_t k = 0; k < p->nkinds; ++k) has[k] = t.offset[k + 1] > t.offset[k] ? 1 : 0;
                    int32_t* d_has = nullptr;
                    rc = upload(&d_has, has.data(), has.size());
                    if (!rc) {
                        void* raw = nullptr;
                        const int64_t n = p->ib.nimages;
                        if (cached_malloc(&raw, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess) rc = fail(CEG_ERR_HIP, "hipMalloc failed");
                        else {
                            t.d_imgkind = (int32_t*)raw;
                            rc = probe_image_flags(p->d_imgkind, d_has, p->nkinds, t.d_imgkind, n);
                        }
                    }
                    if (d_has) { (void)hipDeviceSynchronize(); cached_free(d_has); }
                    hq.ib.kind = t.d_imgkind;
                }
                if (!rc) rc = upload(&t.d_pc, &hq, 1);
                if (q == 0) { p->vdwk = t.vdwk; }
            }
            hc.rt = hc.rtm[0];
            hc.fastvdw = hc.fastm[0];
        }
        if (!rc) rc = upload(&p->d_pc, &hc, 1);
    } else if (!rc && p->nprobes > 0) {
        rc = fail(CEG_ERR_UNSUPPORTED, "multi-probe plans need every perpendicular cell width >= 2*cutoff (what a ProbeSystem guarantees)");
    }
    if (flush_uploads() != hipSuccess && !rc) rc = fail(CEG_ERR_HIP, "uploading the plan's tables failed");       // (also before a failed plan's blocks go back to the pool)
    stamp("function tables, constants");
    if (rc) {
        ceg_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return CEG_OK;
}

extern "C" int ceg_plan_create(ceg_plan_t** plan, int32_t device,
                               const double* pos, const int64_t* atomkind, const double* charge,
                               int64_t natoms,
                               const double mat[9], const double invmat[9],
                               int32_t ortho, double safemin2, double cutoff2,
                               const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                               double alpha,
                               const int32_t dims[3], const double size[3], const double shift[3],
                               const double delta[3])
{
    return create_impl(plan, device, pos, atomkind, charge, natoms, mat, invmat, ortho, safemin2, cutoff2, rules, rule_offset, nkinds, 0,
                       nullptr, nullptr, alpha, dims, size, shift, delta);
}

extern "C" int ceg_plan_create_multi(ceg_plan_t** plan, int32_t device, const double* pos, const int64_t* atomkind, const double* charge,
                                     int64_t natoms, const double mat[9], const double invmat[9], int32_t ortho, double safemin2,
                                     double cutoff2, int32_t nprobes, const ceg_rule_t* const* rules,
                                     const int32_t* const* rule_offset, int32_t nkinds, double alpha, const int32_t dims[3],
                                     const double size[3], const double shift[3], const double delta[3])
{
    if (nprobes < 1) return fail(CEG_ERR_INVALID, "nprobes = %d < 1", nprobes);
    return create_impl(plan, device, pos, atomkind, charge, natoms, mat, invmat, ortho, safemin2, cutoff2, nullptr, nullptr, nkinds, nprobes,
                       rules, rule_offset, alpha, dims, size, shift, delta);
}

extern "C" int ceg_plan_num_probes(const ceg_plan_t* p) { return p ? p->nprobes : 0; }

extern "C" int ceg_plan_destroy(ceg_plan_t* p)
{
    if (!p) return CEG_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();          // what hipFree would do: no kernel of this plan is still running
    p->images.reset();                     // the image arrays belong to the (possibly cached, possibly shared) ImageSet
    for (void* ptr : {(void*)p->d_atoms, (void*)p->d_kind, (void*)p->d_rules, (void*)p->d_offset, (void*)p->d_pc, (void*)p->d_erfcx,
                      (void*)p->d_exp2, (void*)p->d_fast, (void*)p->d_ew2, (void*)p->d_ew2f, (void*)p->d_bk2})
        cached_free(ptr);
    for (auto& t : p->probes)
        for (void* ptr : {(void*)t.d_rules, (void*)t.d_offset, (void*)t.d_fast, (void*)t.d_pc, (void*)t.d_bk2, (void*)t.d_imgkind}) cached_free(ptr);
    delete p;
    return CEG_OK;
}

extern "C" int ceg_image_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries)
{
    std::lock_guard<std::mutex> lock(g_image_mutex);
    if (hits) *hits = g_image_hits.load();
    if (misses) *misses = g_image_misses.load();
    if (entries) *entries = (int64_t)g_image_cache.size();
    return CEG_OK;
}

extern "C" int ceg_plan_can_cull(const ceg_plan_t* p) { return (p && p->can_cull) ? 1 : 0; }

extern "C" int ceg_plan_uniform_class(const ceg_plan_t* p)
{
    if (!p) return 0;
    return p->nprobes > 0 ? p->probes[0].uni.cls : p->uni.cls;
}

extern "C" int ceg_plan_ew2_fine(const ceg_plan_t* p) { return (p && p->ew2f) ? 1 : 0; }

// host only: the r^2-indexed Ewald table a plan with these parameters builds, coarse (fine == 0) or fine layout
extern "C" int ceg_ew2_table(double alpha, double r_exact2, double cutoff2, int32_t fine, double* table, int64_t capacity, int32_t* base,
                             int32_t* ni, int32_t* stride, double* worst)
{
    const Ew2Layout& lay = fine ? EW2_FINE : EW2_COARSE;
    std::vector<double> t;
    int32_t b = 0, n = 0;
    double w = 0.0;
    const bool ok = build_ew2_table(alpha, r_exact2, cutoff2, lay, t, &b, &n, &w);
    if (base) *base = b;
    if (ni) *ni = n;
    if (stride) *stride = t.empty() ? 0 : lay.stride();
    if (worst) *worst = w;
    if (table && !t.empty()) {          // (a fit that misses the tolerance is still returned: its errors are what a test looks at)
        if (capacity < (int64_t)t.size()) return fail(CEG_ERR_INVALID, "table needs %lld doubles, capacity %lld", (long long)t.size(), (long long)capacity);
        memcpy(table, t.data(), t.size() * sizeof(double));
    }
    return ok ? 1 : 0;
}

// host only: the classification of convert_rules + detect_uniform_class on a caller's tables
extern "C" int ceg_uniform_class(const int64_t* atomkind, const double* charge, int64_t natoms, const ceg_rule_t* rules,
                                 const int32_t* rule_offset, int32_t nkinds, double cutoff2, double constants[4])
{
    if (!atomkind || natoms <= 0 || !rules || !rule_offset || nkinds <= 0) return fail(CEG_ERR_INVALID, "atom / rule tables missing");
    ceg_plan tmp;
    tmp.natoms = natoms;
    tmp.g.cutoff2 = cutoff2;
    tmp.h_kind.resize((size_t)natoms);
    for (int64_t a = 0; a < natoms; ++a) {
        if (atomkind[a] < 1 || atomkind[a] > nkinds) return fail(CEG_ERR_INVALID, "atomkind[%lld] outside 1..%d", (long long)a, nkinds);
        tmp.h_kind[a] = (int32_t)(atomkind[a] - 1);
    }
    if (charge) tmp.h_charge.assign(charge, charge + natoms);
    if (int rc = convert_rules(&tmp, rules, rule_offset, nkinds)) return rc;
    set_uniform_class(&tmp);
    if (constants) { constants[0] = tmp.uni.eps4; constants[1] = tmp.uni.s6; constants[2] = tmp.uni.shift; constants[3] = tmp.uni.q; }
    return tmp.uni.cls;
}

extern "C" int64_t ceg_plan_num_images(const ceg_plan_t* p) { return (p && p->images_built) ? p->ib.nimages : 0; }

// the lattice-image list of a plan copied to the host (tests: the device build against the host build): xyzq [4 n], kind / atom [n],
// bin_start [nbins + 1] with nbins = nb[0] nb[1] nb[2]; any output may be NULL; nb receives the bin counts
extern "C" int ceg_plan_copy_images(const ceg_plan_t* p, double* xyzq, int32_t* kind, int32_t* atom, int32_t* bin_start, int32_t nb[3])
{
    if (!p || !p->images_built) return fail(CEG_ERR_INVALID, "the plan has no image list");
    DeviceGuard guard(p->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", p->device);
    const size_t n = (size_t)p->ib.nimages;
    const size_t nbins = (size_t)p->ib.nb[0] * p->ib.nb[1] * p->ib.nb[2];
    if (nb) for (int a = 0; a < 3; ++a) nb[a] = p->ib.nb[a];
    bool ok = hipDeviceSynchronize() == hipSuccess;
    if (ok && xyzq && n) ok = hipMemcpy(xyzq, p->d_images, n * sizeof(double4), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && kind && n && p->d_imgkind) ok = hipMemcpy(kind, p->d_imgkind, n * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && atom && n) ok = hipMemcpy(atom, p->d_imgatom, n * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && bin_start) ok = hipMemcpy(bin_start, p->d_binstart, (nbins + 1) * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? CEG_OK : fail(CEG_ERR_HIP, "copying the image list failed");
}

namespace {

int resolve_algo(const ceg_plan* p, int32_t algo, bool* culled)
{
    switch (algo) {
    case CEG_ALGO_AUTO: *culled = p->can_cull; return CEG_OK;
    case CEG_ALGO_BRUTEFORCE: *culled = false; return CEG_OK;
    case CEG_ALGO_CULLED:
        if (!p->can_cull)
            return fail(CEG_ERR_UNSUPPORTED,
                        "culled algorithm needs every perpendicular cell width >= 2*cutoff");
        *culled = true;
        return CEG_OK;
    default: return fail(CEG_ERR_INVALID, "unknown algo %d", algo);
    }
}

int run(ceg_plan* p, int mode, const Output& out, const Points& pts, bool culled, hipStream_t stream)
{
    if (mode != MODE_COULOMB && !p->has_rules) return fail(CEG_ERR_INVALID, "plan was created without rules");
    if (mode != MODE_VDW && !p->has_charge) return fail(CEG_ERR_INVALID, "plan was created without charges");
    RuleTable rt{p->d_rules, p->d_offset, p->nkinds};          // (a multi-probe plan keeps probe 0's rules here: brute force uses probe 0 too)
    hipError_t e;
    if (culled) {
        // a multi-probe plan: the ordinary calls use probe 0, i.e. ITS constant block (rule classes, the tabulated Buckingham
        // class, the per-image flags of that probe) and ITS hot-loop variant -- the plan-level block carries the union image flags
        // and no Buckingham table.  The Coulomb grid alone needs no probe: the plan-level block, as in ceg_plan_build_multi.
        const bool probe0 = p->nprobes > 0 && mode != MODE_COULOMB;
        // (the uniform class of the plan or of probe 0: these calls only; ceg_plan_build_multi keeps the per-candidate records, so that
        //  a grid does not depend on how that call cuts a request into launches)
        e = launch_culled(mode, probe0 ? p->probes[0].d_pc : p->d_pc, p->g, probe0 ? p->probes[0].vdwk : p->vdwk,
                          p->ew2 ? (p->ew2f ? 3 : 2) : (p->fast_ewald ? 1 : 0), out, pts, stream, probe0 ? p->probes[0].uni.cls : p->uni.cls);
    } else {
        AtomTable at{p->d_atoms, p->has_rules ? p->d_kind : nullptr, p->natoms};
        e = launch_bruteforce(mode, p->g, at, rt, out, pts, stream);
    }
    if (e != hipSuccess) return fail(CEG_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return CEG_OK;
}

int build_common(ceg_plan* p, int mode, double lv, double tv, double lc, double tc, int32_t i_begin,
                 int32_t i_end, float* d_v, float* d_c, int64_t channel_stride, int32_t i_origin,
                 int32_t algo, void* stream)
{
    if (!p) return fail(CEG_ERR_INVALID, "plan is NULL");
    if (i_begin < 0 || i_end > p->g.dims[0] + 1 || i_begin > i_end)
        return fail(CEG_ERR_INVALID, "bad x-plane range [%d,%d) for dims[0]+1 = %d", i_begin, i_end, p->g.dims[0] + 1);
    if (i_origin > i_begin) return fail(CEG_ERR_INVALID, "i_origin %d > i_begin %d", i_origin, i_begin);
    if ((mode != MODE_COULOMB && !d_v) || (mode != MODE_VDW && !d_c)) return fail(CEG_ERR_INVALID, "output pointer is NULL");
    const int64_t plane = (int64_t)(p->g.dims[1] + 1) * (p->g.dims[2] + 1);
    if (channel_stride < (int64_t)(i_end - i_origin) * plane)
        return fail(CEG_ERR_INVALID, "channel_stride %lld too small", (long long)channel_stride);
    bool culled;
    if (int rc = resolve_algo(p, algo, &culled)) return rc;
    Output out{};
    out.vdw = d_v;
    out.coulomb = d_c;
    out.channel_stride = channel_stride;
    out.i_origin = i_origin;
    out.i_begin = i_begin;
    out.i_end = i_end;
    out.lambda_vdw = lv;
    out.thr_vdw = tv;
    out.lambda_coulomb = lc;
    out.thr_coulomb = tc;
    DeviceGuard guard(p->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", p->device);
    return run(p, mode, out, Points{nullptr, 0}, culled, (hipStream_t)stream);
}

}  // namespace

extern "C" int ceg_plan_build_vdw(ceg_plan_t* plan, double lambda, double threshold, int32_t i_begin,
                                  int32_t i_end, float* d_out, int64_t channel_stride, int32_t i_origin,
                                  int32_t algo, void* stream)
{
    return build_common(plan, MODE_VDW, lambda, threshold, 0, 0, i_begin, i_end, d_out, nullptr, channel_stride,
                        i_origin, algo, stream);
}

extern "C" int ceg_plan_build_coulomb(ceg_plan_t* plan, double lambda, double threshold, int32_t i_begin,
                                      int32_t i_end, float* d_out, int64_t channel_stride, int32_t i_origin,
                                      int32_t algo, void* stream)
{
    return build_common(plan, MODE_COULOMB, 0, 0, lambda, threshold, i_begin, i_end, nullptr, d_out,
                        channel_stride, i_origin, algo, stream);
}

extern "C" int ceg_plan_build_fused(ceg_plan_t* plan, double lambda_vdw, double threshold_vdw,
                                    double lambda_coulomb, double threshold_coulomb, int32_t i_begin,
                                    int32_t i_end, float* d_out_vdw, float* d_out_coulomb,
                                    int64_t channel_stride, int32_t i_origin, int32_t algo, void* stream)
{
    return build_common(plan, MODE_FUSED, lambda_vdw, threshold_vdw, lambda_coulomb, threshold_coulomb, i_begin,
                        i_end, d_out_vdw, d_out_coulomb, channel_stride, i_origin, algo, stream);
}

// K VdW grids + the Coulomb grid of one framework from one image list (the grids setup_RASPA asks for one after the other,
// src/raspa.jl:497-520).  The requested set is cut into launches of the multi-probe kernels: with the Coulomb grid the first two
// probes ride in the fused launch (48 accumulator registers: 3 waves per SIMD), the others in VdW launches of up to four probes.
// Whatever the cut, every grid is bit-identical to the one a launch of that grid alone produces (same per-pair arithmetic, same
// order of the sums; ceg_kernels.hip).
extern "C" int ceg_plan_build_multi(ceg_plan_t* p, double lambda_vdw, double threshold_vdw, double lambda_coulomb, double threshold_coulomb,
                                    int32_t i_begin, int32_t i_end, float* const* d_out_vdw, float* d_out_coulomb,
                                    int64_t channel_stride, int32_t i_origin, void* stream)
{
    if (!p) return fail(CEG_ERR_INVALID, "plan is NULL");
    if (p->nprobes < 1) return fail(CEG_ERR_INVALID, "not a multi-probe plan (ceg_plan_create_multi)");
    if (i_begin < 0 || i_end > p->g.dims[0] + 1 || i_begin > i_end)
        return fail(CEG_ERR_INVALID, "bad x-plane range [%d,%d) for dims[0]+1 = %d", i_begin, i_end, p->g.dims[0] + 1);
    if (i_origin > i_begin) return fail(CEG_ERR_INVALID, "i_origin %d > i_begin %d", i_origin, i_begin);
    const int64_t plane = (int64_t)(p->g.dims[1] + 1) * (p->g.dims[2] + 1);
    if (channel_stride < (int64_t)(i_end - i_origin) * plane) return fail(CEG_ERR_INVALID, "channel_stride %lld too small", (long long)channel_stride);
    if (d_out_coulomb && !p->has_charge) return fail(CEG_ERR_INVALID, "plan was created without charges");
    std::vector<int> req;
    for (int q = 0; q < p->nprobes; ++q)
        if (d_out_vdw && d_out_vdw[q]) req.push_back(q);
    if (req.empty() && !d_out_coulomb) return CEG_OK;
    Output base{};
    base.channel_stride = channel_stride;
    base.i_origin = i_origin;
    base.i_begin = i_begin;
    base.i_end = i_end;
    base.lambda_vdw = lambda_vdw;
    base.thr_vdw = threshold_vdw;
    base.lambda_coulomb = lambda_coulomb;
    base.thr_coulomb = threshold_coulomb;
    DeviceGuard guard(p->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", p->device);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    // real-space Ewald arithmetic available to this plan (never the fine table: the fused multi-probe variants cannot hold it, and the
    // Coulomb grid must not depend on how this call cuts a request into launches)
    const int ewk = p->ew2 ? 2 : (p->fast_ewald ? 1 : 0);
    auto single = [&](int mode, int q) {          // one probe (q >= 0) and / or the Coulomb grid: the single-probe kernels of the probe's class
        Output o = base;
        o.vdw = q >= 0 ? d_out_vdw[q] : nullptr;
        o.coulomb = mode != MODE_VDW ? d_out_coulomb : nullptr;
        return launch_culled(mode, q >= 0 ? p->probes[q].d_pc : p->d_pc, p->g, q >= 0 ? p->probes[q].vdwk : 1, ewk, o, Points{nullptr, 0}, st);
    };
    auto multi = [&](int mode, const int* idx, int np) {
        Output o = base;
        for (int t = 0; t < np; ++t) { o.vdwm[t] = d_out_vdw[idx[t]]; o.probe_idx[t] = idx[t]; }
        o.coulomb = mode == MODE_FUSED ? d_out_coulomb : nullptr;
        return launch_culled_multi(mode, np, p->d_pc, p->g, o, st);
    };
    // the Lennard-Jones-only probes can share accumulating loops; a probe of another class launches alone (or fused with the Coulomb grid)
    std::vector<int> lj, other;
    for (int q : req) (p->probes[q].vdwk == 1 ? lj : other).push_back(q);
    if (d_out_coulomb) {
        int fused_np = CEG_MAX_PROBES_FUSED;          // probes that share the Coulomb launch (CEG_HIP_MULTI_FUSED_NP = 0 | 1 | 2: measurement aid)
        if (const char* env = std::getenv("CEG_HIP_MULTI_FUSED_NP")) fused_np = std::max(0, std::min(CEG_MAX_PROBES_FUSED, atoi(env)));
        if (!p->ew2 && p->nprobes > 1) fused_np = 0;  // the fused multi-probe variants are built on the r^2-indexed tables
        // what rides with the Coulomb grid, by what it saves on the roofline workload (profiles/r04_multi_probe_timing.txt): two
        // Lennard-Jones probes (25.3 -> 18.1 ms), else one probe of another class (18.2 -> 15.5 ms), else one Lennard-Jones probe
        if (fused_np >= 2 && lj.size() >= 2) {
            e = multi(MODE_FUSED, &lj[0], 2);
            lj.erase(lj.begin(), lj.begin() + 2);
        } else if (fused_np >= 1 && !other.empty()) {
            e = single(MODE_FUSED, other[0]);
            other.erase(other.begin());
        } else if (fused_np >= 1 && !lj.empty()) {
            e = single(MODE_FUSED, lj[0]);
            lj.erase(lj.begin());
        } else {
            e = single(MODE_COULOMB, -1);
        }
    }
    size_t at = 0;
    while (e == hipSuccess && at < lj.size()) {
        const int n = (int)std::min<size_t>(CEG_MAX_PROBES, lj.size() - at);
        e = n == 1 ? single(MODE_VDW, lj[at]) : multi(MODE_VDW, &lj[at], n);
        at += (size_t)n;
    }
    for (size_t t = 0; e == hipSuccess && t < other.size(); ++t) e = single(MODE_VDW, other[t]);
    if (e != hipSuccess) return fail(CEG_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return CEG_OK;
}

extern "C" int ceg_plan_eval_points(ceg_plan_t* p, int32_t which, int32_t algo, const double* points,
                                    int64_t npoints, double* out)
{
    if (!p) return fail(CEG_ERR_INVALID, "plan is NULL");
    if (npoints < 0 || (npoints > 0 && (!points || !out))) return fail(CEG_ERR_INVALID, "bad points/out");
    if (which != 0 && which != 1) return fail(CEG_ERR_INVALID, "which must be 0 (vdw) or 1 (coulomb)");
    if (npoints == 0) return CEG_OK;
    bool culled;
    if (int rc = resolve_algo(p, algo, &culled)) return rc;
    if (culled) {
        // the image list only covers the grid's bounding box grown by the cutoff
        bool inside = true;
        for (int64_t q = 0; q < npoints && inside; ++q)
            for (int a = 0; a < 3; ++a) {
                const double x = points[3 * q + a];
                if (!(x >= p->g.shift[a] - 1e-9 && x <= p->g.shift[a] + p->g.size[a] + 1e-9)) inside = false;
            }
        if (!inside) {
            if (algo == CEG_ALGO_CULLED)
                return fail(CEG_ERR_UNSUPPORTED, "culled evaluation needs points inside the grid bounding box");
            culled = false;
        }
    }
    DeviceGuard guard(p->device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", p->device);
    double* d_pts = nullptr;
    double* d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_pts, sizeof(double) * 3 * npoints));
    if (hipMalloc((void**)&d_out, sizeof(double) * 8 * npoints) != hipSuccess) {
        (void)hipFree(d_pts);
        return fail(CEG_ERR_HIP, "hipMalloc failed");
    }
    int rc = CEG_OK;
    if (hipMemcpy(d_pts, points, sizeof(double) * 3 * npoints, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(CEG_ERR_HIP, "hipMemcpy H2D failed");
    if (!rc) {
        Output o{};
        if (which == 0) o.raw_vdw = d_out; else o.raw_coulomb = d_out;
        rc = run(p, which == 0 ? MODE_VDW : MODE_COULOMB, o, Points{d_pts, npoints}, culled, nullptr);
    }
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(CEG_ERR_HIP, "kernel execution failed: %s", hipGetErrorString(hipGetLastError()));
    if (!rc && hipMemcpy(out, d_out, sizeof(double) * 8 * npoints, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(CEG_ERR_HIP, "hipMemcpy D2H failed");
    (void)hipFree(d_pts);
    (void)hipFree(d_out);
    return rc;
}

extern "C" int ceg_release_cached_buffers(void)
{
    ceg_host::oneshot_pools_release();
    image_cache_release();
    block_cache_release();
    return CEG_OK;
}
