// Host-side runtime plumbing: error strings, RAII device buffers, launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mmw_hip.h"
#include "device_utils.h"
#include "switches.h"

namespace mmw {

inline std::string& last_error_ref() {
    static thread_local std::string e;
    return e;
}
inline int fail(int code, const std::string& msg) {
    last_error_ref() = msg;
    return code;
}

#define MMW_HIP(call)                                                                                         \
    do {                                                                                                      \
        hipError_t err__ = (call);                                                                            \
        if (err__ != hipSuccess) {                                                                            \
            char buf__[512];                                                                                  \
            snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, \
                     __LINE__);                                                                               \
            return ::mmw::fail(MMW_ERR_HIP, buf__);                                                           \
        }                                                                                                     \
    } while (0)

#define MMW_TRY(expr)              \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != MMW_OK) return rc__; \
    } while (0)

// No C++ exception (std::bad_alloc from a host vector, ...) crosses the C boundary: every extern "C" entry runs its body inside this.
// `prefix` names the entry (the batch entries share their handle's name) in front of the exception's text.
template <typename F> int guarded(const char* prefix, F&& f) {
    try {
        return f();
    } catch (const std::exception& ex) {
        return fail(MMW_ERR_ARG, std::string(prefix) + ": " + ex.what());
    } catch (...) {
        return fail(MMW_ERR_ARG, std::string(prefix) + ": unknown exception");
    }
}

// an entry that refuses null pointers (`bad`) with `msg` and then is one call: both inside the guard, under the name `who`
template <typename F> int entry(const char* who, bool bad, const char* msg, F&& call) {
    return guarded(who, [&]() -> int { return bad ? fail(MMW_ERR_ARG, msg) : call(); });
}

inline int device_count(int* n) {
    if (!n) return fail(MMW_ERR_ARG, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(MMW_ERR_HIP, std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
    }
    *n = c;
    return MMW_OK;
}
// `device` names a visible HIP device, or the entry `who` refuses it; the entries differ in how much the refusal says
enum DeviceText { DEV_BARE, DEV_ID, DEV_ID_VISIBLE };
inline int check_device(const char* who, int device, DeviceText text) {
    int ndev = 0;
    MMW_TRY(device_count(&ndev));
    if (device >= 0 && device < ndev) return MMW_OK;
    std::string msg = std::string(who) + ": no such HIP device";
    if (text != DEV_BARE) msg += " " + std::to_string(device);
    if (text == DEV_ID_VISIBLE) msg += " (" + std::to_string(ndev) + " visible)";
    return fail(MMW_ERR_HIP, msg);
}
struct ScopedStream {  // a stream of a handle-less call
    hipStream_t s = nullptr;
    ~ScopedStream() { if (s) (void)hipStreamDestroy(s); }
};

// Per-device one-time setup.  A kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) and the CU count belong to the
// CURRENT device, and handles of one process may sit on different devices and be driven from different host threads (bench.py's
// resident instances, the speculative search): both are keyed by the device id and guarded.
inline int set_max_lds(const void* fn, int bytes) {
    int dev = 0;
    MMW_HIP(hipGetDevice(&dev));
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int>* done = new std::map<std::pair<const void*, int>, int>;  // never destroyed (runtime teardown order)
    std::lock_guard<std::mutex> g(mu);
    auto it = done->find({fn, dev});
    if (it != done->end() && it->second >= bytes) return MMW_OK;
    MMW_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    (*done)[{fn, dev}] = bytes;
    return MMW_OK;
}
inline int device_cus() {  // compute units of the current device (256 on MI355X)
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
    c = 256;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cache[dev].store(c, std::memory_order_relaxed);
    return c;
}

// Page-locked host staging for the large transfers of a handle (the factor handed back, the rounding's inputs).  An asynchronous
// copy to or from pageable memory makes the runtime pin the caller's pages and unpin them later, at a moment of its own choosing:
// measured as 20 - 40 ms stalls in front of an unrelated launch of the next probe.  Copies go through this buffer instead.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int ensure(size_t bytes) {
        if (p && bytes <= cap) return MMW_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        if (bytes == 0) bytes = 1;
        MMW_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return MMW_OK;
    }
};

// A small pool of such buffers for the one-off transfers (uploads at creation, API reads): leased for the duration of one copy.
// The pool and its buffers live until the process ends (no destructor races with the HIP runtime's own teardown).
struct StagePool {
    std::mutex m;
    std::vector<PinnedBuf*> idle;
    PinnedBuf* get() {
        std::lock_guard<std::mutex> g(m);
        if (!idle.empty()) { PinnedBuf* b = idle.back(); idle.pop_back(); return b; }
        return new PinnedBuf;
    }
    void put(PinnedBuf* b) { std::lock_guard<std::mutex> g(m); idle.push_back(b); }
};
inline StagePool& stage_pool() { static StagePool* pool = new StagePool; return *pool; }
struct StageLease {
    PinnedBuf* b;
    StageLease() : b(stage_pool().get()) {}
    ~StageLease() { stage_pool().put(b); }
    StageLease(const StageLease&) = delete;
    StageLease& operator=(const StageLease&) = delete;
};
constexpr size_t STAGE_MIN_BYTES = 64 << 10;  // smaller copies go straight: the runtime bounces them through its own pinned chunks
// host -> device and back, synchronous on `st`; large ones through a leased page-locked buffer
inline int copy_h2d(void* dst_dev, const void* src_host, size_t bytes, hipStream_t st) {
    if (bytes == 0) return MMW_OK;
    if (bytes < STAGE_MIN_BYTES) {
        MMW_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st));
        MMW_HIP(hipStreamSynchronize(st));
        return MMW_OK;
    }
    StageLease L;
    MMW_TRY(L.b->ensure(bytes));
    memcpy(L.b->p, src_host, bytes);
    MMW_HIP(hipMemcpyAsync(dst_dev, L.b->p, bytes, hipMemcpyHostToDevice, st));
    MMW_HIP(hipStreamSynchronize(st));
    return MMW_OK;
}
inline int copy_d2h(void* dst_host, const void* src_dev, size_t bytes, hipStream_t st) {
    if (bytes == 0) return MMW_OK;
    if (bytes < STAGE_MIN_BYTES) {
        MMW_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        MMW_HIP(hipStreamSynchronize(st));
        return MMW_OK;
    }
    StageLease L;
    MMW_TRY(L.b->ensure(bytes));
    MMW_HIP(hipMemcpyAsync(L.b->p, src_dev, bytes, hipMemcpyDeviceToHost, st));
    MMW_HIP(hipStreamSynchronize(st));
    memcpy(dst_host, L.b->p, bytes);
    return MMW_OK;
}

// a host vector handed out by a read entry `who`, whose caller must have announced its exact length
template <typename V> int export_vec(const std::vector<V>& v, V* out, int64_t have, const char* who) {
    if ((int64_t)v.size() != have) return fail(MMW_ERR_ARG, std::string(who) + ": wrong length");
    if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(V));
    return MMW_OK;
}

inline int64_t a32(int64_t x) { return (x + 31) & ~(int64_t)31; }  // the batch arenas' arrays start at multiples of 32 elements (fp64: 256 bytes)

template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;    // elements in use
    size_t cap = 0;  // elements allocated
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        cap = 0;
    }
    // Contents are undefined afterwards.  An allocation that is large enough is kept: hipFree waits for the whole device (every
    // stream of every handle), so a handle that shrinks its blocks for the next slot count must not free them.
    int alloc(size_t count) {
        if (p && count <= cap && !live_switch(LIVE_DEVBUF_EXACT)) {
            n = count;
            return MMW_OK;
        }
        release();
        n = count;
        if (count == 0) count = 1;
        MMW_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        cap = count;
        return MMW_OK;
    }
    int upload(const std::vector<T>& h, hipStream_t st) {
        MMW_TRY(alloc(h.size()));
        return copy_h2d(p, h.data(), h.size() * sizeof(T), st);  // synchronous: the source may be a short-lived host vector
    }
    // upload a double host vector converted to T
    template <typename S> int upload_cast(const std::vector<S>& h, hipStream_t st) {
        std::vector<T> tmp(h.size());
        for (size_t i = 0; i < h.size(); ++i) tmp[i] = (T)h[i];
        MMW_TRY(alloc(tmp.size()));
        return copy_h2d(p, tmp.data(), tmp.size() * sizeof(T), st);
    }
};

// Optional per-kernel-class device timers (HIP events on the solver's own stream).  Off by default:
// when off, begin/end cost nothing and no event is recorded.
enum { KT_SPMM = 0, KT_SDDMM = 1, KT_DUAL = 2, KT_LOSS = 3, KT_KRYLOV_VEC = 4, KT_SKETCH = 5, KT_PROJECT = 6, KT_GREEDY = 7,
       KT_FACTOR = 8, KT_NSLOT = 9 };
struct KernelTimers {
    bool on = false;
    hipStream_t st = nullptr;
    struct Rec { int slot; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double total_us[KT_NSLOT] = {0};
    double count[KT_NSLOT] = {0};
    int cur = -1;
    ~KernelTimers() {
        for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
    int get(hipEvent_t* e) {
        if (!pool.empty()) { *e = pool.back(); pool.pop_back(); return MMW_OK; }
        MMW_HIP(hipEventCreate(e));
        return MMW_OK;
    }
    int begin(int slot) {
        if (!on) return MMW_OK;
        Rec r; r.slot = slot;
        MMW_TRY(get(&r.a)); MMW_TRY(get(&r.b));
        MMW_HIP(hipEventRecord(r.a, st));
        recs.push_back(r);
        return MMW_OK;
    }
    int end() {
        if (!on || recs.empty()) return MMW_OK;
        if (attached) { attached = false; return MMW_OK; }  // the launch itself records the pair (begin_attached)
        MMW_HIP(hipEventRecord(recs.back().b, st));
        return MMW_OK;
    }
    // A bracket of ONE launch whose events the launch carries itself (hipExtLaunchKernelGGL's start / stop events: the dispatch's own
    // begin and end, what a kernel trace reports) instead of two marker packets around it, which add the marker's and the dispatch's
    // latency (2-3 us) to a 17 us kernel.  `attach` is set for the profiling mode that times the shipped path as launched.
    bool attach = false, attached = false;
    int begin_attached(int slot, hipEvent_t* a, hipEvent_t* b) {
        *a = nullptr; *b = nullptr;
        if (!on) return MMW_OK;
        if (!attach) return begin(slot);
        Rec r; r.slot = slot;
        MMW_TRY(get(&r.a)); MMW_TRY(get(&r.b));
        recs.push_back(r);
        *a = r.a; *b = r.b;
        attached = true;
        return MMW_OK;
    }
    int flush() {  // call after the stream has been synchronised
        for (auto& r : recs) {
            float ms = 0;
            MMW_HIP(hipEventElapsedTime(&ms, r.a, r.b));
            total_us[r.slot] += ms * 1e3; count[r.slot] += 1;
            pool.push_back(r.a); pool.push_back(r.b);
        }
        recs.clear();
        return MMW_OK;
    }
    void clear() { for (int i = 0; i < KT_NSLOT; ++i) { total_us[i] = 0; count[i] = 0; } }
};

// Phase timers of the loop (mmw_set_timing): four events per timed iteration on the solver's stream, one row of MMW_F_PHASE_US per iteration.
// Timing every iteration costs the loop four event records per iteration (each one a barrier packet between two launches of
// the dependent chain).  With a stride S > 1 only iteration 0 and the iterations i = S/2 (mod S) carry events; every other row of
// MMW_F_PHASE_US repeats the sample of its group of S iterations (the harness takes means over the rows, sim_mmw_time.py:48-52).
struct PhaseTimers {
    bool timing = false;
    int timing_stride = 1;
    std::vector<hipEvent_t> events;      // 4 per timed iteration
    std::vector<hipEvent_t> event_pool;  // events of earlier runs, kept for reuse
    std::vector<int> ev_iter;            // iteration of every group of four pending events
    struct PhaseSample { int it; double us[4]; };
    std::vector<PhaseSample> phase_samples;  // the iterations that carried events (set_timing)
    std::vector<double> phase_us;
    ~PhaseTimers() {
        for (auto e : events) (void)hipEventDestroy(e);
        for (auto e : event_pool) (void)hipEventDestroy(e);
    }
    bool timed(int iter) const { return timing && (timing_stride <= 1 || iter == 0 || iter % timing_stride == timing_stride / 2); }
    void clear_samples() { phase_us.clear(); phase_samples.clear(); }
    int record(int slot, int iter, hipStream_t st) {
        if (!timed(iter)) return MMW_OK;
        if (slot == 0) ev_iter.push_back(iter);
        hipEvent_t e;
        if (!event_pool.empty()) {  // events are kept across runs: creating four per iteration cost the class path ~20 us per iteration
            e = event_pool.back();
            event_pool.pop_back();
        } else
            MMW_HIP(hipEventCreate(&e));
        MMW_HIP(hipEventRecord(e, st));
        events.push_back(e);
        return MMW_OK;
    }
    // the events recorded so far / dropping those recorded since (the timers of a discarded chunk; earlier chunks keep theirs)
    size_t mark() const { return events.size(); }
    int drop_since(size_t mark0, hipStream_t st) {
        if (!timing) return MMW_OK;
        MMW_HIP(hipStreamSynchronize(st));
        for (size_t i = mark0; i < events.size(); ++i) event_pool.push_back(events[i]);
        events.resize(std::min(events.size(), mark0));
        ev_iter.resize(events.size() / 4);
        return MMW_OK;
    }
    int flush(int iter, hipStream_t st) {  // `iter`: iterations done
        if (events.empty()) return MMW_OK;
        MMW_HIP(hipStreamSynchronize(st));
        for (size_t i = 0; i + 3 < events.size(); i += 4) {
            float a = 0, b = 0, c = 0, t = 0;
            MMW_HIP(hipEventElapsedTime(&a, events[i], events[i + 1]));
            MMW_HIP(hipEventElapsedTime(&b, events[i + 1], events[i + 2]));
            MMW_HIP(hipEventElapsedTime(&c, events[i + 2], events[i + 3]));
            MMW_HIP(hipEventElapsedTime(&t, events[i], events[i + 3]));
            phase_samples.push_back({ev_iter[i / 4], {a * 1e3, b * 1e3, c * 1e3, t * 1e3}});
        }
        for (auto e : events) event_pool.push_back(e);
        events.clear();
        ev_iter.clear();
        // one row per iteration done: its own sample, else the sample of its group of `timing_stride` iterations, else the nearest one
        phase_us.clear();
        if (phase_samples.empty()) return MMW_OK;
        std::sort(phase_samples.begin(), phase_samples.end(), [](const PhaseSample& x, const PhaseSample& y) { return x.it < y.it; });
        const int S = std::max(1, timing_stride);
        for (int i = 0; i < iter; ++i) {
            const int want = (i == 0 || S <= 1) ? i : (i / S) * S + S / 2;
            const PhaseSample* best = nullptr;
            for (const PhaseSample& q : phase_samples) {
                if (q.it == want) { best = &q; break; }
                if (q.it == 0 && i != 0 && phase_samples.size() > 1) continue;  // the first iteration of a run is not like the others
                if (!best || std::abs(q.it - i) < std::abs(best->it - i)) best = &q;
            }
            for (int k = 0; k < 4; ++k) phase_us.push_back(best->us[k]);
        }
        return MMW_OK;
    }
};

inline double tnow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }  // seconds, monotonic

inline int grid_rows(int rows) {  // one wavefront per row, 4 rows per workgroup, grid-stride beyond the cap
    int g = (rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (g < 1) g = 1;
    return g > ROW_GRID_MAX ? ROW_GRID_MAX : g;  // short rows are latency chains: one row per wave beats grid-striding
}
inline int grid_slabs(int rows) { return std::min(grid_rows(rows), MAX_PART); }  // kernels that write a Dpad-wide slab per workgroup
inline int grid_elems(size_t n) {
    size_t g = (n + BLOCK - 1) / BLOCK;
    if (g < 1) g = 1;
    return (int)(g > 2048 ? 2048 : g);
}

}  // namespace mmw
