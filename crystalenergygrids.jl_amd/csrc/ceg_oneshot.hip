// ceg_oneshot.hip -- the one-shot entry points of libceg_hip.so (include/ceg_hip.h): ceg_grid_vdw / _coulomb [+ _file, _device],
// ceg_grids_multi, the page-locked result arrays and the cached .grid file -> interpolation handle.  Host code only: every
// kernel is launched through the plan API of ceg_api.hip (ceg_plan_create[_multi], ceg_plan_build_*).
//
//   entry point -> Framework (the arguments of the plan) + Enqueue (the build call of one chunk) + outputs
//   fan_out_*   -> one x-slab per device, one host thread per extra device
//   host_pipeline / resident_pipeline -> one slab: plan, chunks, copies
#include "ceg_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

using ceg_host::DeviceGuard;
using ceg_host::fail;

namespace {

// x-planes [begin,end) of device `d` out of `n`
inline void slab(int nx, int n, int d, int* begin, int* end)
{
    const int base = nx / n, rem = nx % n;
    *begin = d * base + std::min(d, rem);
    *end = *begin + base + (d < rem ? 1 : 0);
}

// ---- pinned staging buffers, kept across calls (page-locking costs more than the copy it serves)
struct PinnedBuf { void* ptr; size_t bytes; bool busy; bool user = false; };     // user: handed to a caller by ceg_host_grid_alloc
std::mutex g_pinned_mutex;
std::vector<PinnedBuf> g_pinned;

// ---- device output slabs, kept across calls as well (hipMalloc + hipFree of 0.5 GB cost ~8 ms, as
// much as the VdW kernel itself); one idle buffer per device is retained, see ceg_release_cached_buffers
struct DeviceBuf { int device; void* ptr; size_t bytes; bool busy; };
std::vector<DeviceBuf> g_devbufs;      // guarded by g_pinned_mutex

// streams are expensive to create on ROCm (an HSA queue each, ~2 ms): keep a pair per device
struct StreamPair { int device; hipStream_t comp, copy; bool busy; };
std::vector<StreamPair> g_streams;     // guarded by g_pinned_mutex

bool streams_acquire(int device, hipStream_t* comp, hipStream_t* copy)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_streams)
        if (p.device == device && !p.busy) { p.busy = true; *comp = p.comp; *copy = p.copy; return true; }
    StreamPair sp{device, nullptr, nullptr, true};
    if (hipStreamCreateWithFlags(&sp.comp, hipStreamNonBlocking) != hipSuccess) return false;
    if (hipStreamCreateWithFlags(&sp.copy, hipStreamNonBlocking) != hipSuccess) { (void)hipStreamDestroy(sp.comp); return false; }
    g_streams.push_back(sp);
    *comp = sp.comp; *copy = sp.copy;
    return true;
}

void streams_release(hipStream_t comp)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_streams)
        if (p.comp == comp) p.busy = false;
}

void* device_acquire(int device, size_t bytes)     // current device must be `device`
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_devbufs)
        if (p.device == device && !p.busy && p.bytes >= bytes) { p.busy = true; return p.ptr; }
    for (size_t t = 0; t < g_devbufs.size(); ++t)
        if (g_devbufs[t].device == device && !g_devbufs[t].busy) {
            (void)hipFree(g_devbufs[t].ptr);
            g_devbufs.erase(g_devbufs.begin() + t);
            break;
        }
    void* ptr = nullptr;
    if (hipMalloc(&ptr, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    g_devbufs.push_back({device, ptr, bytes, true});
    return ptr;
}

void device_release(void* ptr)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_devbufs)
        if (p.ptr == ptr) p.busy = false;
}

void* pinned_acquire(size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_pinned)
        if (!p.busy && p.bytes >= bytes) { p.busy = true; return p.ptr; }
    for (size_t t = 0; t < g_pinned.size(); ++t)          // replace an idle, too small buffer
        if (!g_pinned[t].busy) {
            (void)hipHostFree(g_pinned[t].ptr);
            g_pinned.erase(g_pinned.begin() + t);
            break;
        }
    void* ptr = nullptr;
    if (hipHostMalloc(&ptr, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    g_pinned.push_back({ptr, bytes, true});
    return ptr;
}

// true when [ptr, ptr + bytes) lies inside a page-locked buffer this library handed out (ceg_host_grid_alloc): the one-shot
// pipelines then copy D2H straight to where the data belongs instead of through the ring + host threads
bool pinned_owns(const void* ptr, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    const char* q = static_cast<const char*>(ptr);
    for (const auto& p : g_pinned) {
        const char* base = static_cast<const char*>(p.ptr);
        if (p.busy && q >= base && q + bytes <= base + p.bytes) return true;
    }
    return false;
}

void pinned_release(void* ptr)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto& p : g_pinned)
        if (p.ptr == ptr) { p.busy = false; p.user = false; }
}

// copy `nseg` segments in parallel; first touch of a fresh destination is page-fault bound, and the
// faults of different threads proceed in parallel
struct Segment { float* dst; const float* src; size_t n; int64_t file_offset; };
// fd >= 0: every piece is also written to the file at its byte offset (pwrite is thread-safe); dst may be null.
// Returns false if a write failed.
bool parallel_copy(const std::vector<Segment>& segs, int nthreads, int fd = -1)
{
    // cut every segment into pieces of <= 1 MiB so that all threads have work
    std::vector<Segment> pieces;
    const size_t piece = 256 * 1024;
    for (const auto& sg : segs)
        for (size_t o = 0; o < sg.n; o += piece)
            pieces.push_back({sg.dst ? sg.dst + o : nullptr, sg.src + o, std::min(piece, sg.n - o), sg.file_offset + (int64_t)(o * sizeof(float))});
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&]() {
        for (;;) {
            const size_t t = next.fetch_add(1);
            if (t >= pieces.size()) return;
            const Segment& pc = pieces[t];
            if (pc.dst) std::memcpy(pc.dst, pc.src, pc.n * sizeof(float));
            if (fd >= 0) {
                const char* ptr = reinterpret_cast<const char*>(pc.src);
                size_t left = pc.n * sizeof(float);
                int64_t off = pc.file_offset;
                while (left > 0) {
                    const ssize_t w = pwrite(fd, ptr, left, (off_t)off);
                    if (w <= 0) { ok.store(false); break; }
                    ptr += w; left -= (size_t)w; off += w;
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    return ok.load();
}

// ---- what an entry point hands down
// The framework and grid description: the arguments that travel unchanged from the C entry point to ceg_plan_create[_multi].
struct Framework {
    const double* pos; const int64_t* atomkind; const double* charge; int64_t natoms;
    const double* mat; const double* invmat; int32_t ortho; double safemin2, cutoff2;
    int32_t nprobes;                                                    // 0: one rule table (ceg_plan_create); >= 1: one per probe (ceg_plan_create_multi)
    const ceg_rule_t* rules; const int32_t* rule_offset;                // nprobes == 0
    const ceg_rule_t* const* mrules; const int32_t* const* mrule_offset;  // nprobes >= 1
    int32_t nkinds; double alpha;
    const int32_t* dims; const double* size; const double* shift; const double* delta;

    int nx() const { return dims[0] + 1; }
    int64_t plane() const { return (int64_t)(dims[1] + 1) * (dims[2] + 1); }
};

int create_plan(const Framework& f, int device, ceg_plan_t** plan)
{
    if (f.nprobes == 0)
        return ceg_plan_create(plan, device, f.pos, f.atomkind, f.charge, f.natoms, f.mat, f.invmat, f.ortho, f.safemin2, f.cutoff2,
                               f.rules, f.rule_offset, f.nkinds, f.alpha, f.dims, f.size, f.shift, f.delta);
    return ceg_plan_create_multi(plan, device, f.pos, f.atomkind, f.charge, f.natoms, f.mat, f.invmat, f.ortho, f.safemin2, f.cutoff2,
                                 f.nprobes, f.mrules, f.mrule_offset, f.nkinds, f.alpha, f.dims, f.size, f.shift, f.delta);
}

// Enqueues the build of x-planes [cb, ce) on `stream`.  d_out is one slab of 8 channels per output grid, one after the other, with
// `stride` points per channel and x-plane `origin` at its start (ceg_plan_build_*'s channel_stride / i_origin).
using Enqueue = std::function<int(ceg_plan_t* plan, int cb, int ce, float* d_out, int64_t stride, int origin, hipStream_t stream)>;

Enqueue single_grid(bool vdw, double lambda, double threshold)
{
    return [=](ceg_plan_t* plan, int cb, int ce, float* d_out, int64_t stride, int origin, hipStream_t stream) {
        return vdw ? ceg_plan_build_vdw(plan, lambda, threshold, cb, ce, d_out, stride, origin, CEG_ALGO_AUTO, stream)
                   : ceg_plan_build_coulomb(plan, lambda, threshold, cb, ce, d_out, stride, origin, CEG_ALGO_AUTO, stream);
    };
}

// chunk of a slab [b, e) = a multiple of 4 planes (the kernel's tile edge) of about 32 MB over the ngrids x 8 channels
int chunk_planes(int64_t plane, int ngrids, int b, int e)
{
    const int cx = (int)std::max<int64_t>(4, ((32ll << 20) / (plane * 8 * ngrids * (int64_t)sizeof(float))) / 4 * 4);
    return std::min(cx, (e - b + 3) / 4 * 4);
}

// ---- slabs over devices
struct FanOut { int ndev, nslabs, first_device, copy_threads; };

// Slab t of `ngpus` is built on device (first_device + t) % ndev.  CEG_HIP_OVERSUBSCRIBE=1 (a rehearsal aid for one-GPU boxes)
// admits more slabs than devices, so the multi-device scheduling -- one host thread, one plan, one slab per "device" -- can run
// on a single card.
int fan_out_plan(const Framework& f, int32_t ngpus, int first_device, FanOut* fo)
{
    const int ndev = ceg_device_count();
    if (ndev <= 0) return fail(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (first_device < 0 || first_device >= ndev) return fail(CEG_ERR_NO_DEVICE, "target device %d not present (%d devices)", first_device, ndev);
    const bool oversubscribe = std::getenv("CEG_HIP_OVERSUBSCRIBE") != nullptr;
    if (ngpus < 1 || (ngpus > ndev && !oversubscribe))
        return fail(CEG_ERR_NO_DEVICE, "ngpus = %d but %d HIP devices are present", ngpus, ndev);
    ngpus = std::min(ngpus, f.nx());
    // host threads that move finished chunks from the pinned ring into the caller's array
    int copy_threads = 8;
    if (const char* env = std::getenv("CEG_HIP_COPY_THREADS")) copy_threads = std::max(1, atoi(env));
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw > 0) copy_threads = std::min<int>(copy_threads, (int)hw);
    *fo = {ndev, ngpus, first_device, std::max(1, copy_threads / ngpus)};
    return CEG_OK;
}

// work(slab index, device, x-planes [b, e), error text): one call per slab, each on a host thread of its own; the calling thread's
// device is restored and the first failure becomes the call's error
using SlabWork = std::function<int(int t, int device, int b, int e, std::string* err)>;

int fan_out_run(const Framework& f, const FanOut& fo, const SlabWork& work)
{
    int prev = -1;
    (void)hipGetDevice(&prev);
    std::vector<int> rcs(fo.nslabs, CEG_OK);
    std::vector<std::string> errs(fo.nslabs);
    auto run = [&](int t) {
        int b, e;
        slab(f.nx(), fo.nslabs, t, &b, &e);
        rcs[t] = work(t, (fo.first_device + t) % fo.ndev, b, e, &errs[t]);
    };
    std::vector<std::thread> workers;
    for (int t = 1; t < fo.nslabs; ++t) workers.emplace_back(run, t);      // one host thread per extra device
    run(0);
    for (auto& w : workers) w.join();
    if (prev >= 0) (void)hipSetDevice(prev);
    for (int t = 0; t < fo.nslabs; ++t)
        if (rcs[t]) return fail(rcs[t], "%s", errs[t].c_str());
    return CEG_OK;
}

// ---- host arrays out
struct HostOutput { float* host; int64_t file_offset; };      // host may be NULL when a file is written; file_offset: byte offset of the payload

// One device's share of a one-shot build: x-planes [b, e) of every output grid, computed in chunks of `cx` planes; chunk j is
// copied D2H into a pinned ring slot (copy stream) and from there into the caller's arrays and / or the file (host threads) while
// chunks j+1.. are being computed.
int host_pipeline(const Framework& f, const Enqueue& enqueue, const std::vector<HostOutput>& outs, int fd, int copy_threads,
                  int d, int b, int e, std::string* err)
{
    auto bad = [&](int code, const char* what) {
        *err = std::string(what) + " (device " + std::to_string(d) + "): " + hipGetErrorString(hipGetLastError());
        return code;
    };
    const int NG = (int)outs.size();
    const int64_t plane = f.plane();
    const int64_t npts = plane * f.nx();
    const int64_t slab_pts = (int64_t)(e - b) * plane;
    if (slab_pts <= 0) return CEG_OK;
    const bool trace = std::getenv("CEG_HIP_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (trace)
            fprintf(stderr, "[ceg one-shot dev %d] %-28s %8.3f ms\n", d, what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    if (hipSetDevice(d) != hipSuccess) return bad(CEG_ERR_HIP, "hipSetDevice failed");
    ceg_plan_t* plan = nullptr;
    int rc = create_plan(f, d, &plan);
    if (rc) { *err = ceg_last_error(); return rc; }
    stamp("plan created");
    const int cx = chunk_planes(plane, NG, b, e);
    const int nchunks = (e - b + cx - 1) / cx;
    const int R = std::min(3, nchunks);
    const size_t grid_slot = (size_t)8 * cx * plane;           // floats of one grid in a ring slot
    const size_t slot_floats = grid_slot * NG;
    // Every output is page-locked memory of this library (ceg_host_grid_alloc) and no file is written on the way: every chunk is
    // copied D2H straight to its place -- no ring, no host threads, no second pass over the 537 MB.
    bool direct = fd < 0;
    for (const auto& o : outs) direct = direct && o.host != nullptr && pinned_owns(o.host, sizeof(float) * 8 * (size_t)npts);
    float* d_all = nullptr;                                     // NG slabs of 8 * slab_pts floats
    float* h_ring = nullptr;
    hipStream_t s_comp = nullptr, s_copy = nullptr;
    std::vector<hipEvent_t> ev_comp(nchunks, nullptr), ev_copy(nchunks, nullptr);
    std::thread drain;
    std::atomic<int> drained{0}, enqueued{0};
    std::atomic<int> drain_rc{CEG_OK};
    bool ok = streams_acquire(d, &s_comp, &s_copy) &&
              (d_all = static_cast<float*>(device_acquire(d, sizeof(float) * 8 * slab_pts * NG))) != nullptr;
    for (int j = 0; j < nchunks && ok; ++j)
        ok = hipEventCreateWithFlags(&ev_comp[j], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ev_copy[j], hipEventDisableTiming) == hipSuccess;
    if (ok && !direct) {
        h_ring = static_cast<float*>(pinned_acquire(sizeof(float) * slot_floats * R));
        ok = h_ring != nullptr;
    }
    if (!ok) rc = bad(CEG_ERR_HIP, "allocation of streams / buffers failed");
    stamp("streams, buffers, pinned ring");
    // all kernels up front: the compute stream runs them back to back
    for (int j = 0; j < nchunks && !rc; ++j) {
        const int cb = b + j * cx, ce = std::min(e, cb + cx);
        rc = enqueue(plan, cb, ce, d_all, slab_pts, b, s_comp);
        if (rc) { *err = ceg_last_error(); break; }
        if (hipEventRecord(ev_comp[j], s_comp) != hipSuccess) rc = bad(CEG_ERR_HIP, "hipEventRecord failed");
    }
    stamp("kernels enqueued");
    if (!rc && !direct)
        drain = std::thread([&]() {
            (void)hipSetDevice(d);
            for (int j = 0; j < nchunks; ++j) {
                while (j >= enqueued.load()) std::this_thread::yield();
                if (drain_rc.load() != CEG_OK) { drained.store(j + 1); continue; }
                if (hipEventSynchronize(ev_copy[j]) != hipSuccess) { drain_rc.store(CEG_ERR_HIP); drained.store(j + 1); continue; }
                const int cb = b + j * cx, ce = std::min(e, cb + cx);
                const size_t cpts = (size_t)(ce - cb) * plane;
                const float* slot = h_ring + (size_t)(j % R) * slot_floats;
                std::vector<Segment> segs;
                for (int g = 0; g < NG; ++g)
                    for (int c = 0; c < 8; ++c) {
                        const size_t at = (size_t)c * npts + (size_t)cb * plane;           // float offset inside the grid
                        segs.push_back({outs[g].host ? outs[g].host + at : nullptr, slot + (size_t)g * grid_slot + (size_t)c * cpts, cpts,
                                        outs[g].file_offset + (int64_t)(at * sizeof(float))});
                    }
                if (!parallel_copy(segs, copy_threads, fd)) drain_rc.store(CEG_ERR_INVALID);
                drained.store(j + 1);
            }
        });
    for (int j = 0; j < nchunks && !rc; ++j) {
        if (!direct)
            while (j - drained.load() >= R) std::this_thread::yield();        // ring slot still being emptied
        const int cb = b + j * cx, ce = std::min(e, cb + cx);
        const size_t cpts = (size_t)(ce - cb) * plane;
        if (hipStreamWaitEvent(s_copy, ev_comp[j], 0) != hipSuccess) rc = bad(CEG_ERR_HIP, "hipStreamWaitEvent failed");
        // per grid the 8 channel segments of the chunk as ONE strided copy (rows of cpts floats, source pitch = channel stride of the
        // slab), to their place in the caller's array (direct) or packed into the ring slot ([NG][8][cpts])
        for (int g = 0; g < NG && !rc; ++g) {
            float* dst = direct ? outs[g].host + (size_t)cb * plane : h_ring + (size_t)(j % R) * slot_floats + (size_t)g * grid_slot;
            if (hipMemcpy2DAsync(dst, sizeof(float) * (direct ? (size_t)npts : cpts), d_all + (size_t)g * 8 * slab_pts + (size_t)(cb - b) * plane,
                                 sizeof(float) * (size_t)slab_pts, sizeof(float) * cpts, 8, hipMemcpyDeviceToHost, s_copy) != hipSuccess)
                rc = bad(CEG_ERR_HIP, "hipMemcpy2DAsync D2H failed");
        }
        if (direct) continue;
        if (!rc && hipEventRecord(ev_copy[j], s_copy) != hipSuccess) rc = bad(CEG_ERR_HIP, "hipEventRecord failed");
        if (rc) drain_rc.store(rc);
        enqueued.store(j + 1);
    }
    stamp("copies enqueued");
    if (drain.joinable()) {
        if (rc) enqueued.store(nchunks);       // let the drain thread run to its end
        drain.join();
        stamp("drained into caller arrays");
        if (!rc && drain_rc.load() == CEG_ERR_INVALID) { *err = "writing the grid file failed"; rc = CEG_ERR_INVALID; }
        if (!rc && drain_rc.load() != CEG_OK) rc = bad(CEG_ERR_HIP, "kernel execution or D2H copy failed");
    } else if (direct) {
        if (hipStreamSynchronize(s_copy) != hipSuccess && !rc) rc = bad(CEG_ERR_HIP, "kernel execution or D2H copy failed");
        stamp("grids in the caller's page-locked arrays");
    }
    (void)hipStreamSynchronize(s_comp);
    (void)hipStreamSynchronize(s_copy);
    for (int j = 0; j < nchunks; ++j) {
        if (ev_comp[j]) (void)hipEventDestroy(ev_comp[j]);
        if (ev_copy[j]) (void)hipEventDestroy(ev_copy[j]);
    }
    if (h_ring) pinned_release(h_ring);
    if (d_all) device_release(d_all);
    if (s_comp) streams_release(s_comp);
    ceg_plan_destroy(plan);
    stamp("cleaned up");
    return rc;
}

// The one-shot build into host arrays (`grids`, each 8 * npts floats) and, with `path`, into a .grid file: header, the payload of the
// grids one after the other, trailer.  An entry of `grids` may be NULL only when a file is written.
int oneshot(const Framework& f, const Enqueue& enqueue, const std::vector<float*>& grids, int32_t ngpus, const char* path = nullptr,
            const void* header = nullptr, int64_t header_bytes = 0, const void* trailer = nullptr, int64_t trailer_bytes = 0)
{
    for (float* g : grids)
        if (!g && !path) return fail(CEG_ERR_INVALID, "grid is NULL");
    if (path && (header_bytes < 0 || trailer_bytes < 0 || (header_bytes > 0 && !header) || (trailer_bytes > 0 && !trailer)))
        return fail(CEG_ERR_INVALID, "bad header / trailer");
    if (int rc = ceg_host::check_common(f.pos, f.natoms, f.mat, f.invmat, f.dims, f.size, f.shift, f.delta)) return rc;
    FanOut fo{};
    if (int rc = fan_out_plan(f, ngpus, 0, &fo)) return rc;
    if (grids.empty()) return CEG_OK;

    // optional file: header, payload streamed chunk by chunk at its offsets while the build runs, trailer
    // The reference opens the file only once the whole grid exists (grids.jl:151,178), and its cache looks no
    // further than isfile(path) (raspa.jl:426): a file must never be visible at `path` unless it is complete.
    // Everything goes into `<path>.tmp.<pid>.<n>`, renamed onto `path` after every device pipeline returned
    // CEG_OK and close() succeeded; any failure unlinks the temporary.
    int fd = -1;
    std::string tmp_path;
    const int64_t grid_bytes = (int64_t)sizeof(float) * 8 * f.plane() * f.nx();
    const int64_t payload_bytes = grid_bytes * (int64_t)grids.size();
    if (path) {
        static std::atomic<unsigned> tmp_serial{0};
        tmp_path = std::string(path) + ".tmp." + std::to_string((long long)getpid()) + "." + std::to_string(tmp_serial.fetch_add(1));
        fd = open(tmp_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return fail(CEG_ERR_INVALID, "cannot open %s for writing", tmp_path.c_str());
        bool ok = ftruncate(fd, (off_t)(header_bytes + payload_bytes + trailer_bytes)) == 0;
        ok = ok && (header_bytes == 0 || pwrite(fd, header, (size_t)header_bytes, 0) == (ssize_t)header_bytes);
        ok = ok && (trailer_bytes == 0 ||
                    pwrite(fd, trailer, (size_t)trailer_bytes, (off_t)(header_bytes + payload_bytes)) == (ssize_t)trailer_bytes);
        if (!ok) {
            close(fd);
            (void)unlink(tmp_path.c_str());
            return fail(CEG_ERR_INVALID, "cannot write the header of %s", tmp_path.c_str());
        }
    }
    std::vector<HostOutput> outs;
    for (size_t g = 0; g < grids.size(); ++g) outs.push_back({grids[g], header_bytes + (int64_t)g * grid_bytes});
    int rc = fan_out_run(f, fo, [&](int, int device, int b, int e, std::string* err) {
        return host_pipeline(f, enqueue, outs, fd, fo.copy_threads, device, b, e, err);
    });
    if (fd >= 0 && close(fd) != 0 && !rc) rc = fail(CEG_ERR_INVALID, "closing the grid file failed");
    if (rc) {
        if (path) (void)unlink(tmp_path.c_str());
        return rc;
    }
    if (path && rename(tmp_path.c_str(), path) != 0) {
        (void)unlink(tmp_path.c_str());
        return fail(CEG_ERR_INVALID, "cannot rename %s onto %s", tmp_path.c_str(), path);
    }
    return CEG_OK;
}

// ---- device array out
// One slab of the device-resident one-shot build: slab 0 is built straight into the assembled grid on the target device; the other
// slabs are built on their own devices and travel to the target chunk by chunk with hipMemcpyPeerAsync (xGMI between the GPUs of a
// node) while the later chunks are still being computed.
int resident_pipeline(const Framework& f, const Enqueue& enqueue, float* d_grid, int target, bool direct, int d, int b, int e, std::string* err)
{
    auto bad = [&](int code, const char* what) {
        *err = std::string(what) + " (device " + std::to_string(d) + "): " + hipGetErrorString(hipGetLastError());
        return code;
    };
    const int64_t plane = f.plane();
    const int64_t npts = plane * f.nx();
    const int64_t slab_pts = (int64_t)(e - b) * plane;
    if (slab_pts <= 0) return CEG_OK;
    if (hipSetDevice(d) != hipSuccess) return bad(CEG_ERR_HIP, "hipSetDevice failed");
    ceg_plan_t* plan = nullptr;
    int rc = create_plan(f, d, &plan);
    if (rc) { *err = ceg_last_error(); return rc; }
    hipStream_t s_comp = nullptr, s_copy = nullptr;
    if (!streams_acquire(d, &s_comp, &s_copy)) { ceg_plan_destroy(plan); return bad(CEG_ERR_HIP, "stream creation failed"); }
    const int cx = chunk_planes(plane, 1, b, e);
    const int nchunks = (e - b + cx - 1) / cx;
    float* d_out = nullptr;
    hipEvent_t ev = nullptr;
    // Can this device write into the target's memory?  (xGMI peers of one node: yes.)  If not -- or with CEG_HIP_NO_PEER=1, a
    // rehearsal aid -- the slab is not pushed chunk by chunk with hipMemcpyPeerAsync but travels through a pinned host buffer once
    // it is complete (D2H on this device, H2D on the target), and a note says so.
    bool peer = true;
    if (!direct) {
        if (d != target) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, d, target) != hipSuccess) can = 0;
            (void)hipGetLastError();
            if (can) {
                (void)hipDeviceEnablePeerAccess(target, 0);                 // "already enabled" is fine
                (void)hipGetLastError();
            }
            peer = can != 0;
        }
        if (std::getenv("CEG_HIP_NO_PEER")) peer = false;
        if (!peer) {
            static std::atomic<bool> said{false};
            if (!said.exchange(true))
                fprintf(stderr, "[ceg_hip] note: no peer access from device %d to device %d%s: slabs of the device-resident build travel "
                                "through pinned host memory\n", d, target, std::getenv("CEG_HIP_NO_PEER") ? " (CEG_HIP_NO_PEER)" : "");
        }
        d_out = static_cast<float*>(device_acquire(d, sizeof(float) * 8 * slab_pts));
        if (!d_out || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) rc = bad(CEG_ERR_HIP, "allocation of the slab buffer failed");
    }
    for (int j = 0; j < nchunks && !rc; ++j) {
        const int cb = b + j * cx, ce = std::min(e, cb + cx);
        rc = direct ? enqueue(plan, cb, ce, d_grid, npts, 0, s_comp) : enqueue(plan, cb, ce, d_out, slab_pts, b, s_comp);
        if (rc) { *err = ceg_last_error(); break; }
        if (direct || !peer) continue;
        if (hipEventRecord(ev, s_comp) != hipSuccess || hipStreamWaitEvent(s_copy, ev, 0) != hipSuccess) { rc = bad(CEG_ERR_HIP, "event failed"); break; }
        const size_t cpts = (size_t)(ce - cb) * plane;
        for (int c = 0; c < 8 && !rc; ++c)
            if (hipMemcpyPeerAsync(d_grid + (size_t)c * npts + (size_t)cb * plane, target, d_out + (size_t)c * slab_pts + (size_t)(cb - b) * plane, d,
                                   sizeof(float) * cpts, s_copy) != hipSuccess)
                rc = bad(CEG_ERR_HIP, "hipMemcpyPeerAsync failed");
    }
    if (hipStreamSynchronize(s_comp) != hipSuccess && !rc) rc = bad(CEG_ERR_HIP, "kernel execution failed");
    if (hipStreamSynchronize(s_copy) != hipSuccess && !rc) rc = bad(CEG_ERR_HIP, "peer copy failed");
    if (!rc && !direct && !peer) {                         // host-staged hand-over of the finished slab
        float* h_buf = static_cast<float*>(pinned_acquire(sizeof(float) * 8 * (size_t)slab_pts));
        if (!h_buf) rc = bad(CEG_ERR_HIP, "pinned buffer allocation failed");
        if (!rc && hipMemcpy(h_buf, d_out, sizeof(float) * 8 * (size_t)slab_pts, hipMemcpyDeviceToHost) != hipSuccess) rc = bad(CEG_ERR_HIP, "D2H of the slab failed");
        if (!rc && hipSetDevice(target) != hipSuccess) rc = bad(CEG_ERR_HIP, "hipSetDevice(target) failed");
        for (int c = 0; c < 8 && !rc; ++c)
            if (hipMemcpy(d_grid + (size_t)c * npts + (size_t)b * plane, h_buf + (size_t)c * slab_pts, sizeof(float) * (size_t)slab_pts,
                          hipMemcpyHostToDevice) != hipSuccess)
                rc = bad(CEG_ERR_HIP, "H2D of the slab failed");
        (void)hipSetDevice(d);
        if (h_buf) pinned_release(h_buf);
    }
    if (ev) (void)hipEventDestroy(ev);
    if (d_out) device_release(d_out);
    streams_release(s_comp);
    ceg_plan_destroy(plan);
    return rc;
}

int oneshot_resident(const Framework& f, const Enqueue& enqueue, float* d_grid, int32_t target, int32_t ngpus)
{
    if (!d_grid) return fail(CEG_ERR_INVALID, "d_grid is NULL");
    if (int rc = ceg_host::check_common(f.pos, f.natoms, f.mat, f.invmat, f.dims, f.size, f.shift, f.delta)) return rc;
    FanOut fo{};
    if (int rc = fan_out_plan(f, ngpus, target, &fo)) return rc;
    return fan_out_run(f, fo, [&](int t, int device, int b, int e, std::string* err) {
        return resident_pipeline(f, enqueue, d_grid, target, t == 0, device, b, e, err);
    });
}

}  // namespace

extern "C" int ceg_grid_vdw(const double* pos, const int64_t* atomkind, int64_t natoms,
                            const double mat[9], const double invmat[9],
                            int32_t ortho, double safemin2, double cutoff2,
                            const ceg_rule_t* rules, const int32_t* rule_offset, int32_t nkinds,
                            const int32_t dims[3], const double size[3], const double shift[3],
                            const double delta[3], double lambda, double threshold,
                            float* grid, int32_t ngpus)
{
    if (!rules || !rule_offset || !atomkind || nkinds <= 0) return fail(CEG_ERR_INVALID, "rule table / atomkind missing");
    const Framework f{pos, atomkind, nullptr, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, rules, rule_offset, nullptr, nullptr,
                      nkinds, 0.0, dims, size, shift, delta};
    return oneshot(f, single_grid(true, lambda, threshold), {grid}, ngpus);
}

extern "C" int ceg_grid_coulomb(const double* pos, const double* charge, int64_t natoms,
                                const double mat[9], const double invmat[9],
                                int32_t ortho, double safemin2, double cutoff2, double alpha,
                                const int32_t dims[3], const double size[3], const double shift[3],
                                const double delta[3], double lambda, double threshold,
                                float* grid, int32_t ngpus)
{
    if (!charge) return fail(CEG_ERR_INVALID, "charge is NULL");
    const Framework f{pos, nullptr, charge, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, nullptr, nullptr, nullptr, nullptr,
                      0, alpha, dims, size, shift, delta};
    return oneshot(f, single_grid(false, lambda, threshold), {grid}, ngpus);
}

extern "C" int ceg_grid_vdw_file(const double* pos, const int64_t* atomkind, int64_t natoms, const double mat[9], const double invmat[9],
                                 int32_t ortho, double safemin2, double cutoff2, const ceg_rule_t* rules, const int32_t* rule_offset,
                                 int32_t nkinds, const int32_t dims[3], const double size[3], const double shift[3],
                                 const double delta[3], double lambda, double threshold, float* grid, int32_t ngpus,
                                 const char* path, const void* header, int64_t header_bytes, const void* trailer, int64_t trailer_bytes)
{
    if (!rules || !rule_offset || !atomkind || nkinds <= 0) return fail(CEG_ERR_INVALID, "rule table / atomkind missing");
    if (!path) return fail(CEG_ERR_INVALID, "path is NULL");
    const Framework f{pos, atomkind, nullptr, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, rules, rule_offset, nullptr, nullptr,
                      nkinds, 0.0, dims, size, shift, delta};
    return oneshot(f, single_grid(true, lambda, threshold), {grid}, ngpus, path, header, header_bytes, trailer, trailer_bytes);
}

extern "C" int ceg_grid_coulomb_file(const double* pos, const double* charge, int64_t natoms, const double mat[9], const double invmat[9],
                                     int32_t ortho, double safemin2, double cutoff2, double alpha, const int32_t dims[3],
                                     const double size[3], const double shift[3], const double delta[3], double lambda, double threshold,
                                     float* grid, int32_t ngpus, const char* path, const void* header, int64_t header_bytes,
                                     const void* trailer, int64_t trailer_bytes)
{
    if (!charge) return fail(CEG_ERR_INVALID, "charge is NULL");
    if (!path) return fail(CEG_ERR_INVALID, "path is NULL");
    const Framework f{pos, nullptr, charge, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, nullptr, nullptr, nullptr, nullptr,
                      0, alpha, dims, size, shift, delta};
    return oneshot(f, single_grid(false, lambda, threshold), {grid}, ngpus, path, header, header_bytes, trailer, trailer_bytes);
}

extern "C" int ceg_grid_vdw_device(const double* pos, const int64_t* atomkind, int64_t natoms, const double mat[9], const double invmat[9],
                                   int32_t ortho, double safemin2, double cutoff2, const ceg_rule_t* rules, const int32_t* rule_offset,
                                   int32_t nkinds, const int32_t dims[3], const double size[3], const double shift[3],
                                   const double delta[3], double lambda, double threshold, float* d_grid, int32_t target_device,
                                   int32_t ngpus)
{
    if (!rules || !rule_offset || !atomkind || nkinds <= 0) return fail(CEG_ERR_INVALID, "rule table / atomkind missing");
    const Framework f{pos, atomkind, nullptr, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, rules, rule_offset, nullptr, nullptr,
                      nkinds, 0.0, dims, size, shift, delta};
    return oneshot_resident(f, single_grid(true, lambda, threshold), d_grid, target_device, ngpus);
}

extern "C" int ceg_grid_coulomb_device(const double* pos, const double* charge, int64_t natoms, const double mat[9], const double invmat[9],
                                       int32_t ortho, double safemin2, double cutoff2, double alpha, const int32_t dims[3],
                                       const double size[3], const double shift[3], const double delta[3], double lambda,
                                       double threshold, float* d_grid, int32_t target_device, int32_t ngpus)
{
    if (!charge) return fail(CEG_ERR_INVALID, "charge is NULL");
    const Framework f{pos, nullptr, charge, natoms, mat, invmat, ortho, safemin2, cutoff2, 0, nullptr, nullptr, nullptr, nullptr,
                      0, alpha, dims, size, shift, delta};
    return oneshot_resident(f, single_grid(false, lambda, threshold), d_grid, target_device, ngpus);
}

// Outputs: the requested VdW grids in probe order, then the Coulomb grid -- the order of their slabs on the device and in a ring slot.
extern "C" int ceg_grids_multi(const double* pos, const int64_t* atomkind, const double* charge, int64_t natoms, const double mat[9],
                               const double invmat[9], int32_t ortho, double safemin2, double cutoff2, int32_t nprobes,
                               const ceg_rule_t* const* rules, const int32_t* const* rule_offset, int32_t nkinds, double alpha,
                               const int32_t dims[3], const double size[3], const double shift[3], const double delta[3],
                               double lambda_vdw, double threshold_vdw, double lambda_coulomb, double threshold_coulomb,
                               float* const* grids_vdw, float* grid_coulomb, int32_t ngpus)
{
    if (nprobes < 1 || nprobes > CEG_MAX_PROBES) return fail(CEG_ERR_INVALID, "nprobes = %d outside 1..%d", nprobes, CEG_MAX_PROBES);
    if (!rules || !rule_offset || !atomkind || nkinds <= 0) return fail(CEG_ERR_INVALID, "rule tables / atomkind missing");
    if (grid_coulomb && !charge) return fail(CEG_ERR_INVALID, "charge is NULL");
    std::vector<float*> grids;
    std::vector<int> probe_of;              // per output: probe index, -1 for the Coulomb grid
    for (int q = 0; q < nprobes; ++q)
        if (grids_vdw && grids_vdw[q]) { grids.push_back(grids_vdw[q]); probe_of.push_back(q); }
    if (grid_coulomb) { grids.push_back(grid_coulomb); probe_of.push_back(-1); }
    const Framework f{pos, atomkind, grid_coulomb ? charge : nullptr, natoms, mat, invmat, ortho, safemin2, cutoff2, nprobes, nullptr, nullptr,
                      rules, rule_offset, nkinds, alpha, dims, size, shift, delta};
    const Enqueue enqueue = [=, &probe_of](ceg_plan_t* plan, int cb, int ce, float* d_out, int64_t stride, int origin, hipStream_t stream) {
        float* d_vdw[CEG_MAX_PROBES] = {nullptr, nullptr, nullptr, nullptr};
        float* d_coulomb = nullptr;
        for (size_t g = 0; g < probe_of.size(); ++g)
            (probe_of[g] >= 0 ? d_vdw[probe_of[g]] : d_coulomb) = d_out + g * 8 * (size_t)stride;
        return ceg_plan_build_multi(plan, lambda_vdw, threshold_vdw, lambda_coulomb, threshold_coulomb, cb, ce, d_vdw, d_coulomb, stride, origin,
                                    stream);
    };
    return oneshot(f, enqueue, grids, ngpus);
}

// ------------------------------------------------------------------ page-locked result arrays
// What the one-shot entry points hand back is 537 MB (256^3) per grid; into an ordinary host array that is D2H into a pinned ring
// plus a second pass by host threads (first touch of fresh pages).  A caller that lets the LIBRARY allocate the result gets
// page-locked memory (kept in the per-process cache, so the page-locking is paid once) and the pipelines copy every chunk straight
// to its place: the call is then bounded by the D2H alone.
// Page-locked result arrays in callers' hands are bounded (CEG_HIP_PINNED_LIMIT_MB, default 4096): a garbage-collected caller (the
// Julia shim wraps them as Arrays and returns them with a finalizer) cannot pin host memory without limit while its collector has not
// run yet -- beyond the limit the call fails with CEG_ERR_UNSUPPORTED and the shim falls back to an ordinary array.
extern "C" float* ceg_host_grid_alloc(const int32_t dims[3])
{
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) { (void)fail(CEG_ERR_INVALID, "bad dims"); return nullptr; }
    if (ceg_device_count() <= 0) { (void)fail(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); return nullptr; }
    const size_t bytes = sizeof(float) * 8 * (size_t)(dims[0] + 1) * (size_t)(dims[1] + 1) * (size_t)(dims[2] + 1);
    size_t limit = (size_t)4096 << 20;
    if (const char* e = std::getenv("CEG_HIP_PINNED_LIMIT_MB")) limit = (size_t)std::max(0ll, atoll(e)) << 20;
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        size_t out = 0;
        for (const auto& p : g_pinned)
            if (p.busy && p.user) out += p.bytes;
        if (out + bytes > limit) {
            (void)fail(CEG_ERR_UNSUPPORTED, "page-locked result arrays in use (%zu MB) + this one (%zu MB) exceed CEG_HIP_PINNED_LIMIT_MB = %zu: "
                                            "free some (ceg_host_grid_free) or use an ordinary array", out >> 20, bytes >> 20, limit >> 20);
            return nullptr;
        }
    }
    void* p = pinned_acquire(bytes);
    if (!p) { (void)fail(CEG_ERR_HIP, "page-locked allocation of %zu bytes failed", bytes); return nullptr; }
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        for (auto& q : g_pinned)
            if (q.ptr == p) q.user = true;
    }
    return static_cast<float*>(p);
}

extern "C" int ceg_host_grid_free(float* grid)
{
    if (!grid) return CEG_OK;
    if (!pinned_owns(grid, 1)) return fail(CEG_ERR_INVALID, "not an array of ceg_host_grid_alloc");
    pinned_release(grid);          // back to the cache; ceg_release_cached_buffers unpins it
    return CEG_OK;
}

void ceg_host::oneshot_pools_release()
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (size_t t = g_devbufs.size(); t-- > 0;)
        if (!g_devbufs[t].busy) {
            if (hipSetDevice(g_devbufs[t].device) == hipSuccess) (void)hipFree(g_devbufs[t].ptr);
            g_devbufs.erase(g_devbufs.begin() + t);
        }
    for (size_t t = g_pinned.size(); t-- > 0;)
        if (!g_pinned[t].busy) {
            (void)hipHostFree(g_pinned[t].ptr);
            g_pinned.erase(g_pinned.begin() + t);
        }
    for (size_t t = g_streams.size(); t-- > 0;)
        if (!g_streams[t].busy) {
            if (hipSetDevice(g_streams[t].device) == hipSuccess) {
                (void)hipStreamDestroy(g_streams[t].comp);
                (void)hipStreamDestroy(g_streams[t].copy);
            }
            g_streams.erase(g_streams.begin() + t);
        }
    if (prev >= 0) (void)hipSetDevice(prev);
}

// ------------------------------------------------------------------ cached .grid file -> interpolation handle
// The reference's common case is not "create" but "Retrieved ... grid" (src/raspa.jl:426-438 -> parse_grid, src/grids.jl:61-94):
// the file is read into a host array, multiplied by GRID_TO_KELVIN, and only then would a GPU consumer upload it and make its
// node-major copy.  Here the payload goes file -> pinned ring (parallel pread) -> device while the next chunk is being read,
// is scaled on the device exactly like grids.jl:78 (Float32(Float64(x) * scale)) and handed to ceg_interp_create in place.
extern "C" int ceg_interp_create(ceg_interp_t** handle, int32_t device, const float* grid, int32_t grid_on_device, const int32_t dims[3],
                                 const double size[3], const double shift[3], const double mat[9], const double invmat[9], int32_t is_vdw);
extern "C" int ceg_scale_grid_device(float* d_grid, int64_t nfloats, double scale, int32_t device, void* stream);

extern "C" int ceg_interp_create_from_file(ceg_interp_t** handle, int32_t device, const char* path, int32_t iscoulomb, double scale,
                                           const double* mat, const double* invmat, ceg_grid_header_t* header_out)
{
    if (!handle || !path) return fail(CEG_ERR_INVALID, "NULL argument");
    *handle = nullptr;
    if ((mat == nullptr) != (invmat == nullptr)) return fail(CEG_ERR_INVALID, "mat and invmat go together");
    const int ndev = ceg_device_count();
    if (ndev <= 0) return fail(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(CEG_ERR_NO_DEVICE, "device %d not present (%d devices)", device, ndev);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(CEG_ERR_INVALID, "cannot open %s", path);
    struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
    // header (src/grids.jl:62-75, written by :108-116): f64 spacing, 3 x i32 dims, 3 x f64 size, shift, delta, unitcell lengths,
    // 3 x i32 num_unitcell [, f64 Ewald precision]
    unsigned char hb[136];
    const size_t hbytes = iscoulomb ? 136 : 128;
    if (pread(fd, hb, hbytes, 0) != (ssize_t)hbytes) return fail(CEG_ERR_INVALID, "%s: truncated header", path);
    ceg_grid_header_t H{};
    size_t o = 0;
    auto rd = [&](void* dst, size_t n) { memcpy(dst, hb + o, n); o += n; };
    rd(&H.spacing, 8); rd(H.dims, 12); rd(H.size, 24); rd(H.shift, 24); rd(H.delta, 24); rd(H.unitcell, 24); rd(H.num_unitcell, 12);
    H.ewald_precision = std::numeric_limits<double>::infinity();          // EnergyGrid(..., Inf, ...) for a VdW grid (grids.jl:92)
    if (iscoulomb) rd(&H.ewald_precision, 8);
    for (int a = 0; a < 3; ++a)
        if (H.dims[a] < 1 || H.dims[a] > (1 << 20) || !(H.size[a] > 0.0)) return fail(CEG_ERR_INVALID, "%s: not a .grid header (dims / size)", path);
    // the node count is bounded by the FILE SIZE before anything is multiplied: with dims up to 2^20 per axis the product
    // reaches 2^60 and nodes * 32 wraps around int64, so that a crafted header could satisfy the size check below with a small file
    const off_t fsize = lseek(fd, 0, SEEK_END);
    const int64_t max_nodes = fsize > (off_t)hbytes ? (int64_t)(fsize - (off_t)hbytes) / 32 : 0;
    int64_t nodes = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t ext = (int64_t)H.dims[a] + 1;
        if (nodes > max_nodes / ext) return fail(CEG_ERR_INVALID, "%s: file shorter than its header says", path);
        nodes *= ext;
    }
    const int64_t nfl = 8 * nodes;
    const int64_t payload = nfl * (int64_t)sizeof(float);
    if (fsize < (off_t)(hbytes + payload)) return fail(CEG_ERR_INVALID, "%s: file shorter than its header says", path);
    // header + payload [+ the 72-byte cell matrix] and nothing else: a VdW file opened as a Coulomb one (or the reverse) is off by the
    // 8 bytes of the Ewald precision and is refused here instead of being read 8 bytes out of step
    if (fsize != (off_t)(hbytes + payload) && fsize != (off_t)(hbytes + payload + 72))
        return fail(CEG_ERR_INVALID, "%s: %lld bytes do not make a %s grid of %d x %d x %d points (wrong iscoulomb?)", path, (long long)fsize,
                    iscoulomb ? "Coulomb" : "VdW", H.dims[0] + 1, H.dims[1] + 1, H.dims[2] + 1);
    H.has_mat = 0;
    if (fsize == (off_t)(hbytes + payload + 72) && pread(fd, H.mat, 72, (off_t)(hbytes + payload)) == 72) H.has_mat = 1;   // :154 / :182
    double M[9], I[9];
    if (mat) { memcpy(M, mat, sizeof M); memcpy(I, invmat, sizeof I); }
    else {
        if (!H.has_mat) return fail(CEG_ERR_INVALID, "%s carries no cell matrix: pass mat / invmat (parse_grid's `mat` argument, grids.jl:80-90)", path);
        memcpy(M, H.mat, sizeof M);
        const double* m = M;                         // column-major: m[i + 3 j]
        const double c00 = m[4] * m[8] - m[7] * m[5], c01 = m[7] * m[2] - m[1] * m[8], c02 = m[1] * m[5] - m[4] * m[2];
        const double det = m[0] * c00 + m[3] * c01 + m[6] * c02;
        if (!(std::fabs(det) > 0.0)) return fail(CEG_ERR_INVALID, "%s: singular cell matrix", path);
        const double id = 1.0 / det;
        I[0] = c00 * id; I[1] = c01 * id; I[2] = c02 * id;
        I[3] = (m[6] * m[5] - m[3] * m[8]) * id; I[4] = (m[0] * m[8] - m[6] * m[2]) * id; I[5] = (m[3] * m[2] - m[0] * m[5]) * id;
        I[6] = (m[3] * m[7] - m[6] * m[4]) * id; I[7] = (m[6] * m[1] - m[0] * m[7]) * id; I[8] = (m[0] * m[4] - m[3] * m[1]) * id;
    }
    if (header_out) *header_out = H;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(CEG_ERR_HIP, "hipSetDevice(%d) failed", device);
    float* d_raw = nullptr;
    HIP_TRY(hipMalloc((void**)&d_raw, (size_t)payload));
    hipStream_t s_comp = nullptr, s_copy = nullptr;
    if (!streams_acquire(device, &s_comp, &s_copy)) { (void)hipFree(d_raw); return fail(CEG_ERR_HIP, "stream creation failed"); }
    const size_t slot = 32ull << 20;
    const int nchunks = (int)((payload + (int64_t)slot - 1) / (int64_t)slot);
    const int R = std::min(3, nchunks);
    char* ring = static_cast<char*>(pinned_acquire(slot * R));
    std::vector<hipEvent_t> ev(R, nullptr);
    int rc = ring ? CEG_OK : fail(CEG_ERR_HIP, "pinned buffer allocation failed");
    for (int t = 0; t < R && !rc; ++t)
        if (hipEventCreateWithFlags(&ev[t], hipEventDisableTiming) != hipSuccess) rc = fail(CEG_ERR_HIP, "event creation failed");
    int nthreads = 8;
    if (const char* env = std::getenv("CEG_HIP_COPY_THREADS")) nthreads = std::max(1, atoi(env));
    for (int j = 0; j < nchunks && !rc; ++j) {
        char* buf = ring + (size_t)(j % R) * slot;
        if (j >= R && hipEventSynchronize(ev[j % R]) != hipSuccess) { rc = fail(CEG_ERR_HIP, "H2D copy failed"); break; }
        const int64_t off = (int64_t)j * (int64_t)slot, len = std::min<int64_t>((int64_t)slot, payload - off);
        std::atomic<bool> ok{true};
        std::atomic<int64_t> next{0};
        const int64_t piece = 1 << 20;
        auto work = [&]() {
            for (;;) {
                const int64_t b = next.fetch_add(piece);
                if (b >= len) return;
                int64_t left = std::min(piece, len - b), at = b;
                while (left > 0) {
                    const ssize_t got = pread(fd, buf + at, (size_t)left, (off_t)(hbytes + off + at));
                    if (got <= 0) { ok.store(false); return; }
                    left -= got; at += got;
                }
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nthreads; ++t) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
        if (!ok.load()) { rc = fail(CEG_ERR_INVALID, "%s: read error", path); break; }
        if (hipMemcpyAsync(reinterpret_cast<char*>(d_raw) + off, buf, (size_t)len, hipMemcpyHostToDevice, s_copy) != hipSuccess ||
            hipEventRecord(ev[j % R], s_copy) != hipSuccess)
            rc = fail(CEG_ERR_HIP, "hipMemcpyAsync H2D failed");
    }
    if (hipStreamSynchronize(s_copy) != hipSuccess && !rc) rc = fail(CEG_ERR_HIP, "H2D copy failed");
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (ring) pinned_release(ring);
    if (!rc && scale != 1.0) {                       // grid .*= GRID_TO_KELVIN (grids.jl:78)
        rc = ceg_scale_grid_device(d_raw, nfl, scale, device, s_copy);
        if (!rc && hipStreamSynchronize(s_copy) != hipSuccess) rc = fail(CEG_ERR_HIP, "scaling kernel failed");
    }
    streams_release(s_comp);
    if (!rc) rc = ceg_interp_create(handle, device, d_raw, 1, H.dims, H.size, H.shift, M, I, iscoulomb ? 0 : 1);
    (void)hipFree(d_raw);
    return rc;
}
