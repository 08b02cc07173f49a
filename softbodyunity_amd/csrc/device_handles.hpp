// device_handles.hpp — the owners of what the HIP runtime hands out: events, streams, device memory, pinned host memory, the ring of
// mapped pinned tables the kinematic targets and the impulses travel in, and the cache of sb_step's graph executables. Plain types,
// move-only or fixed in place, whose destructor gives the resource back; included by solver_internal.hpp (after HIP_CHECK).
// No other file of the plugin creates or destroys one of these resources by hand (the peer mailbox, which has two ways to be
// allocated and mappings in other processes, is PeerState's own business).
//
// FIRST USE. Much of the solver's device state is made at the first call that needs it, inside `if (!x) { ... }`. Such a block is ALL OR
// NOTHING: either it is keyed on the thing it creates LAST (every step before it may then simply be done again: create() is idempotent,
// alloc() and upload() free first), or it builds into locals and moves them into place at the end. Either way, after a thrown HipError
// the next call runs the block again and never meets a half-made state -- a key that is set first would let it skip the block and hand
// a null pointer to a kernel. The types below keep their own side of it: a failed alloc() / upload() leaves the buffer empty, pointer
// and count never disagree.
#pragma once

namespace sbi {

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { destroy(); e = o.e; o.e = nullptr; } return *this; }
    void create(unsigned flags = hipEventDefault) { if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, flags)); }
    void destroy() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
    ~Event() { destroy(); }
};

struct Stream {                  // a non-blocking stream
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { destroy(); s = o.s; o.s = nullptr; } return *this; }
    void create() { if (!s) HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    void destroy() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    operator hipStream_t() const { return s; }
    ~Stream() { destroy(); }
};

template <class T>
struct DevBuf {
    T *p = nullptr;
    T *base = nullptr;           // what hipMalloc returned (p = base + lead: placement experiments, sb_tuning.prev_offset_bytes)
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;                 // owns device memory
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), base(o.base), count(o.count) { o.p = o.base = nullptr; o.count = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { free(); p = o.p; base = o.base; count = o.count; o.p = o.base = nullptr; o.count = 0; } return *this; }
    void alloc(size_t n, int64_t &acct, size_t lead_elems = 0) {
        free();
        if (!n) return;
        HIP_CHECK(hipMalloc((void **)&base, (n + lead_elems) * sizeof(T)));
        p = base + lead_elems; count = n; acct += (int64_t)((n + lead_elems) * sizeof(T));
    }
    void upload(const std::vector<T> &h, int64_t &acct) {       // (a failed copy leaves no buffer behind: `if (!x.p) x.upload(..)` stays a sound first-use test)
        alloc(h.size(), acct);
        try { if (!h.empty()) HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
        catch (...) { free(); throw; }
    }
    void free() { if (base) { (void)hipFree(base); } base = nullptr; p = nullptr; count = 0; }
    ~DevBuf() { free(); }
};

// Pinned host memory; mapped (hipHostMallocMapped): kernels read it in place through `dev`, the device-side alias of the allocation.
template <class T>
struct HostBuf {
    T *p = nullptr;
    T *dev = nullptr;            // mapped memory only
    size_t count = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept : p(o.p), dev(o.dev), count(o.count) { o.p = o.dev = nullptr; o.count = 0; }
    HostBuf &operator=(HostBuf &&o) noexcept { if (this != &o) { free(); p = o.p; dev = o.dev; count = o.count; o.p = o.dev = nullptr; o.count = 0; } return *this; }
    void alloc(size_t n, bool mapped = false) {
        free();
        void *h = nullptr, *d = nullptr;
        HIP_CHECK(hipHostMalloc(&h, n * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault));
        const hipError_t e = mapped ? hipHostGetDevicePointer(&d, h, 0) : hipSuccess;
        if (e != hipSuccess) {
            (void)hipHostFree(h);
            throw HipError(SB_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
        }
        p = (T *)h; dev = (T *)d; count = n;
    }
    void free() { if (p) (void)hipHostFree(p); p = dev = nullptr; count = 0; }
    ~HostBuf() { free(); }
};

// A device buffer and its pinned host twin of the same size (at least one element), for results that leave by an asynchronous copy.
template <class T>
struct Mirror {
    DevBuf<T> d;
    HostBuf<T> h;
    void pin() { h.alloc(std::max<size_t>(d.count, 1)); }      // the host side alone, sized like the device side
    void alloc(size_t count, int64_t &acct) {                  // both or neither: a caller may key on either side
        try { d.alloc(count, acct); pin(); }
        catch (...) { release(); throw; }
    }
    void copy_out(hipStream_t st, size_t count) { if (count) HIP_CHECK(hipMemcpyAsync(h.p, d.p, count * sizeof(T), hipMemcpyDeviceToHost, st)); }
    void release() { d.free(); h.free(); }
};

// N mapped pinned tables that kernels read in place, one per call: the caller fills host(q), launches its readers with device(q) and then
// records the slot's event behind the last of them (retire); a table is reused -- N calls later -- only after that event.
template <int N>
struct TableRing {
    static constexpr size_t kFloorBytes = 4096;      // (= 256 kinematic targets of 16 bytes)
    HostBuf<char> table[N];
    Event done[N];               // behind the last reader of the slot's table
    int next = 0;
    int acquire(size_t bytes) {
        const int q = next;
        next = (q + 1) % N;
        if (!done[q]) done[q].create(hipEventDisableTiming);
        else HIP_CHECK(hipEventSynchronize(done[q]));          // (the call that used this table, N calls ago)
        if (table[q].count < bytes) table[q].alloc(std::max(kFloorBytes, bytes * 2), /*mapped=*/true);
        return q;
    }
    char *host(int q) { return table[q].p; }
    const char *device(int q) const { return table[q].dev; }
    void retire(int q, hipStream_t st) { HIP_CHECK(hipEventRecord(done[q], st)); }
};

// The instantiated graphs of sb_step, one per key (a tick flavour): at most kMaxGraphs are kept, the least recently used one goes when
// another arrives (a host that varies substeps). The executables are destroyed with the cache, or earlier by clear().
struct GraphCache {
    static constexpr size_t kMaxGraphs = 8;
    struct Entry { hipGraphExec_t exec; uint64_t last_use; };
    std::map<int, Entry> entries;
    uint64_t clock = 0;
    GraphCache() = default;
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    hipGraphExec_t find(int key) {               // null: not instantiated yet (or evicted since)
        auto it = entries.find(key);
        if (it == entries.end()) return nullptr;
        it->second.last_use = ++clock;
        return it->second.exec;
    }
    // Instantiates the captured graph `g` under `key` and destroys g; `st` is the stream an evicted executable may still be running on.
    hipGraphExec_t add(int key, hipGraph_t g, hipStream_t st) {
        hipGraphExec_t ge = nullptr;
        hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) throw HipError(SB_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        if (entries.size() >= kMaxGraphs) {
            auto old = entries.begin();
            for (auto q = entries.begin(); q != entries.end(); ++q) if (q->second.last_use < old->second.last_use) old = q;
            HIP_CHECK(hipStreamSynchronize(st));
            (void)hipGraphExecDestroy(old->second.exec);
            entries.erase(old);
        }
        entries.emplace(key, Entry{ge, ++clock});
        return ge;
    }
    void clear() { for (auto &g : entries) (void)hipGraphExecDestroy(g.second.exec); entries.clear(); }
    ~GraphCache() { clear(); }
};

}  // namespace sbi
