// hs_dev_runtime.inc -- part of hs_capi.hip (one translation unit): the device-side plumbing of the library -- pooled device / pinned
// blocks (BlockPool, DBuf, HBuf), transfers queued as kernels (UploadPack, Shipment), host waits, timing events and the
// per-kernel accounting (KernelClock), device binding.
namespace {

// Size-class pool of device / pinned-host blocks: the stage drivers allocate dozens of temporaries per call and
// hipMalloc/hipFree (which synchronises) would dominate small batches. Blocks are kept for the life of the process.
// set when a host wait gave up on the device (stream_wait_impl): kernels may still be writing the blocks of the failed call, so
// from then on nothing is handed back to the pools (the blocks leak; the process is expected to report the error and end)
static std::atomic<bool> g_device_lost{false};
static std::atomic<long> g_pool_miss_dev{0}, g_pool_miss_host{0};      // blocks the pools did not have (hipMalloc / hipHostMalloc calls): HS_POOL_STATS=1 prints them per pipeline call
struct BlockPool {
    std::mutex mu;
    std::vector<std::pair<size_t, void*>> free_dev, free_host;
    static size_t round_up(size_t n) { size_t c = 4096; while (c < n) c <<= 1; return c; }
    int get(bool host, size_t n, void** out, size_t* cap) {
        const size_t c = round_up(n);
        {
            std::lock_guard<std::mutex> g(mu);
            auto& fl = host ? free_host : free_dev;
            for (size_t i = 0; i < fl.size(); ++i)
                if (fl[i].first == c) { *out = fl[i].second; *cap = c; fl[i] = fl.back(); fl.pop_back(); return HS_OK; }
        }
        (host ? g_pool_miss_host : g_pool_miss_dev).fetch_add(1, std::memory_order_relaxed);
        if (host) { if (int rc = pinned_block(c, out)) return rc; } else HS_HIP(hipMalloc(out, c));
        *cap = c;
        return HS_OK;
    }
    // A pinned block of 2 MB and more: anonymous memory on transparent huge pages, registered with the runtime (mapped for the device at
    // its own address) -- 11 ms per 256 MB against 34 ms for hipHostMalloc and half of its cost when the process ends (512 times fewer
    // pages to pin and to give back; tools/probes/pin_cost*.hip: the same 56 GB/s from kernels and copies). Where the kernel grants no huge
    // pages the registration pins 4-KB pages, which is what hipHostMalloc does. HS_PINNED_HOSTMALLOC=1: hipHostMalloc for every block.
    std::vector<std::pair<void*, std::pair<void*, size_t>>> registered;      // block -> (mapping, its length): what the exit probe gives back
    int pinned_block(size_t c, void** out) {
        static const bool plain = std::getenv("HS_PINNED_HOSTMALLOC") != nullptr;
        const size_t H = (size_t)2 << 20;
        if (!plain && c >= H) {
            void* m = ::mmap(nullptr, c + H, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (m != MAP_FAILED) {
                void* q = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(m) + H - 1) & ~(uintptr_t)(H - 1));
                (void)::madvise(q, c, MADV_HUGEPAGE);
                if (hipHostRegister(q, c, hipHostRegisterMapped | hipHostRegisterPortable) == hipSuccess) {
                    std::lock_guard<std::mutex> g(mu);
                    registered.push_back(std::make_pair(q, std::make_pair(m, c + H)));
                    *out = q;
                    return HS_OK;
                }
                (void)hipGetLastError();
                ::munmap(m, c + H);
            }
        }
        HS_HIP(hipHostMalloc(out, c, hipHostMallocDefault));
        return HS_OK;
    }
    void release_host(void* p) {      // (the exit probe only: blocks live as long as the process)
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < registered.size(); ++i)
                if (registered[i].first == p) {
                    (void)hipHostUnregister(p);
                    ::munmap(registered[i].second.first, registered[i].second.second);
                    registered[i] = registered.back(); registered.pop_back();
                    return;
                }
        }
        (void)hipHostFree(p);
    }
    void put(bool host, void* p, size_t cap) {
        if (g_device_lost.load(std::memory_order_relaxed)) return;
        std::lock_guard<std::mutex> g(mu);
        (host ? free_host : free_dev).push_back(std::make_pair(cap, p));
    }
};
// one pool per device: a block belongs to the device (and, for pinned host blocks, is mapped for the device) that was current
// when it was allocated; the host threads of a shard stay on one device (hs_set_device / the sharded stage calls below)
static std::atomic<bool>& g_pool_made_flag() { static std::atomic<bool> f{false}; return f; }      // a pool exists: this process has used a device
BlockPool& pool() {
    static BlockPool* pools[64] = {};
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    dev &= 63;
    BlockPool* p = __atomic_load_n(&pools[dev], __ATOMIC_ACQUIRE);
    if (!p) {
        std::lock_guard<std::mutex> g(mu);
        if (!pools[dev]) { __atomic_store_n(&pools[dev], new BlockPool(), __ATOMIC_RELEASE); g_pool_made_flag().store(true); }
        p = pools[dev];
    }
    return *p;
}

// HS_EXIT_PROBE=1 (diagnostic, called by the drop-in executables before they leave): gives the pooled blocks back and resets the
// device, timing every step -- what the process would otherwise leave to the kernel's teardown after _exit
extern "C" int hs_device_was_used(void) { return g_pool_made_flag().load() ? 1 : 0; }
extern "C" void hs_teardown_probe(void) {
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (!g_pool_made_flag().load()) return;      // (nothing of this process ever touched a device: it stays that way)
    BlockPool& p = pool();
    size_t db = 0, hb = 0, dn = 0, hn = 0;
    const double t0 = now();
    for (auto& b : p.free_dev) { db += b.first; dn++; (void)hipFree(b.second); }
    const double t1 = now();
    for (auto& b : p.free_host) { hb += b.first; hn++; p.release_host(b.second); }
    const double t2 = now();
    (void)hipDeviceReset();
    const double t3 = now();
    if (std::getenv("HS_EXIT_PROBE") || std::getenv("HS_TIMING"))
        std::fprintf(stderr, "[hs exit probe] pooled device blocks: %zu, %.1f MB, hipFree %.1f ms; pooled pinned blocks: %zu, %.1f MB, hipHostFree %.1f ms; hipDeviceReset %.1f ms\n",
                     dn, db / 1e6, t1 - t0, hn, hb / 1e6, t2 - t1, t3 - t2);
}

// RAII device buffer (pooled). A block goes back to the pool it came from (`owner`), whatever device is current on the thread
// that releases it.
struct DBuf {
    void* p = nullptr;
    size_t bytes = 0, cap = 0;
    bool view = false;             // points into an UploadPack: not owned
    BlockPool* owner = nullptr;
    ~DBuf() { release(); }
    void release() { if (p && !view && owner) owner->put(false, p, cap); p = nullptr; view = false; }
    int alloc(size_t n) {
        release();
        bytes = n;
        owner = &pool();
        return owner->get(false, n ? n : 16, &p, &cap);
    }
    template <class T> int upload(const std::vector<T>& v);
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    void take(DBuf& o) { release(); p = o.p; bytes = o.bytes; cap = o.cap; view = o.view; owner = o.owner; o.p = nullptr; o.view = false; }      // (the block changes hands)
};

// pinned host buffer (pooled) for large downloads
struct HBuf {
    void* p = nullptr;
    size_t cap = 0;
    BlockPool* owner = nullptr;
    ~HBuf() { release(); }
    void release() { if (p && owner) owner->put(true, p, cap); p = nullptr; }
    int alloc(size_t n) {
        release();
        owner = &pool();
        return owner->get(true, n ? n : 16, &p, &cap);
    }
    void take(HBuf& o) { release(); p = o.p; cap = o.cap; owner = o.owner; o.p = nullptr; o.cap = 0; }      // (the block changes hands)
    HBuf() = default;
    HBuf(const HBuf&) = delete;
    HBuf& operator=(const HBuf&) = delete;
};

template <class T> int DBuf::upload(const std::vector<T>& v) {
    int rc = alloc(v.size() * sizeof(T));
    if (rc) return rc;
    const size_t n = v.size() * sizeof(T);
    if (n == 0) return HS_OK;
    if (n >= (128u << 10)) {     // large: stage through pinned memory (pageable sources get pinned page by page otherwise)
        HBuf h;
        if (int r2 = h.alloc(n)) return r2;
        std::memcpy(h.p, v.data(), n);
        HS_HIP(hipMemcpy(p, h.p, n, hipMemcpyHostToDevice));
    } else {
        HS_HIP(hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice));
    }
    return HS_OK;
}

// Many small host arrays -> ONE pinned staging buffer -> ONE asynchronous host-to-device copy. Every hipMemcpy of a small
// pageable array costs 10-20 us of latency on the calling thread (a blit kernel each); a stage call used to issue a dozen.
// The DBufs handed to add() become views into the pack's device block; the pack (and its pinned buffer) must outlive the copy:
// keep it in the scope that ends with a synchronising call, or as a member.
// HS_COPY_STATS=1: how often every hipMemcpyAsync call site ran, printed when the library is unloaded (diagnostic for the copy count)
static std::atomic<long> g_copy_sites[4096];
static const bool g_copy_stats = [] {
    const bool on = std::getenv("HS_COPY_STATS") != nullptr;
    if (on) std::atexit([] { for (int i = 0; i < 4096; ++i) { const long n = g_copy_sites[i].load(); if (n) std::fprintf(stderr, "[hs copies] hs_capi.hip:%d %ld\n", i, n); } });
    return on;
}();
#define HS_COPY_ASYNC(...) ((g_copy_stats ? (void)g_copy_sites[__LINE__ & 4095].fetch_add(1, std::memory_order_relaxed) : (void)0), hipMemcpyAsync(__VA_ARGS__))

static int ship_kernel(void* dst, const void* src, size_t bytes, hipStream_t stream);      // (hsdev::k_ship, below the kernels)
struct UploadPack {
    struct Item { const void* src; size_t bytes, off; DBuf* dst; };
    std::vector<Item> items;
    size_t total = 0;
    DBuf dev;
    HBuf host;
    template <class T> void add(const std::vector<T>& v, DBuf& dst) {
        items.push_back(Item{v.data(), v.size() * sizeof(T), total, &dst});
        total = (total + v.size() * sizeof(T) + 255) & ~(size_t)255;
    }
    template <class T> void add(const hs::ArrayView<T>& v, DBuf& dst) {
        items.push_back(Item{v.data(), v.size() * sizeof(T), total, &dst});
        total = (total + v.size() * sizeof(T) + 255) & ~(size_t)255;
    }
    int commit(hipStream_t stream) {
        if (int rc = dev.alloc(total ? total : 256)) return rc;
        if (int rc = host.alloc(total ? total : 256)) return rc;
        for (const Item& it : items) {
            if (it.bytes) std::memcpy((char*)host.p + it.off, it.src, it.bytes);
            it.dst->release();
            it.dst->p = (char*)dev.p + it.off; it.dst->bytes = it.bytes; it.dst->cap = 0; it.dst->view = true;
        }
        if (total) { if (int rc = ship_kernel(dev.p, host.p, total, stream)) return rc; }
        items.clear(); total = 0;
        return HS_OK;
    }
};

// Host waits = polling hipStreamQuery with a 25-us sleep between two looks (HS_WAIT_SLEEP_US; the polling thread's timer slack set
// to 1 us for the duration of the wait, HS_TIMER_SLACK_NS, so that 25 us are 25 us and not 75 -- the thread's own value is put back): about 1 % of a core instead of 100 %, the host learns of the
// end of the work 30 us late -- which the other contig groups cover. No events, no interrupts, no device-wide
// scheduling flag. HS_SPIN_WAIT=1 polls back to back instead (measured on the 16-core box, 500-contig job: the same step time,
// 60-80 CPU-ms more per step; it only pays when a single chain owns the device). A wait that has lasted HS_WAIT_TIMEOUT_S
// seconds (default 1800, 0 = no limit) returns an error instead of hanging the caller for ever; the blocks of that call are
// then leaked, not recycled (g_device_lost), because the device may still be writing them.
static bool blocking_wait() { static const bool spin = std::getenv("HS_SPIN_WAIT") != nullptr; return !spin; }
static bool spin_wait() { return !blocking_wait(); }
static std::atomic<long> g_waits{0}, g_wait_us{0};     // HS_TIMING: host waits and the wall time spent in them
static int stream_wait_impl(hipStream_t s);
static int stream_wait(hipStream_t s) {
    static const bool timed = std::getenv("HS_TIMING") != nullptr;
    if (!timed) { g_waits.fetch_add(1, std::memory_order_relaxed); return stream_wait_impl(s); }
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = stream_wait_impl(s);
    g_waits.fetch_add(1); g_wait_us.fetch_add((long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}
// a wait that is nearly always over already (the work was behind an earlier wait of the same stream): one look first, the counted wait only if needed
static int stream_wait_quiet(hipStream_t s) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return HS_OK;
    if (e != hipErrorNotReady) { HS_HIP(e); }
    (void)hipGetLastError();
    return stream_wait(s);
}
static long wait_timeout_s() {
    static const long v = []() { const char* e = std::getenv("HS_WAIT_TIMEOUT_S"); return e ? std::atol(e) : 1800l; }();
    return v;
}
template <class Query> static int poll_wait_impl(Query query, const char* what);
static int stream_wait_impl(hipStream_t s) { return poll_wait_impl([s] { return hipStreamQuery(s); }, "hipStreamQuery: "); }
// the same wait for an event in the middle of a stream's queue (what was queued before it is done, what follows may still run)
static int event_wait(hipEvent_t e) {
    g_waits.fetch_add(1, std::memory_order_relaxed);
    return poll_wait_impl([e] { return hipEventQuery(e); }, "hipEventQuery: ");
}
template <class Query> static int poll_wait_impl(Query query, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    const long limit = wait_timeout_s();
    // the kernel's default timer slack adds up to 50 us to every sleep: while it polls, the thread asks for 1 us -- and gets its own
    // setting back when the wait returns (the caller's thread may be anybody's: a Python main thread, an OpenMP master)
    struct SlackGuard {
        long old = -1;
        void set(long ns) { if (old < 0) { old = prctl(PR_GET_TIMERSLACK); if (old >= 0) prctl(PR_SET_TIMERSLACK, (unsigned long)ns); } }
        ~SlackGuard() { if (old >= 0) prctl(PR_SET_TIMERSLACK, (unsigned long)old); }
    } slack;
    for (unsigned long looks = 1;; ++looks) {
        const hipError_t e = query();
        if (e == hipSuccess) return HS_OK;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); set_error(std::string(what) + hipGetErrorString(e)); return HS_EHIP; }
        (void)hipGetLastError();      // (hipErrorNotReady is sticky otherwise)
        if (blocking_wait()) {
            static const long sleep_ns = []() { const char* e = std::getenv("HS_WAIT_SLEEP_US"); return e ? std::atol(e) * 1000l : 25000l; }();
            static const long slack_ns = []() { const char* e = std::getenv("HS_TIMER_SLACK_NS"); return e ? std::atol(e) : 1000l; }();
            if (slack_ns > 0) slack.set(slack_ns);
            struct timespec ts = {0, sleep_ns}; nanosleep(&ts, nullptr);
        }
        else { for (int i = 0; i < 16; ++i) __builtin_ia32_pause(); }
        if (limit > 0 && (looks & 4095ul) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(limit)) {
            g_device_lost.store(true);
            set_error("the device did not finish the queued work within " + std::to_string(limit) + " s (HS_WAIT_TIMEOUT_S)");
            return HS_EHIP;
        }
    }
}
static int copy_d2h(void* h, const void* d, size_t n, hipStream_t s) {
    if (n) HS_HIP(HS_COPY_ASYNC(h, d, n, hipMemcpyDeviceToHost, s));
    return stream_wait(s);
}

// Timing events are recycled per host thread: creating and destroying a few hundred (interrupt-backed) events per step makes
// the runtime stall for tens of milliseconds every few dozen steps.
// Device -> host into pageable memory through a pooled pinned buffer. A direct copy makes the runtime pin the destination on
// the fly (a "userptr" mapping); when that memory is later freed the kernel driver has to evict and restore the process's
// GPU queues to drop the mapping -- tens of milliseconds during which nothing runs.
static int d2h_pinned(void* dst, const void* d, size_t n, hipStream_t s) {
    if (!n) return stream_wait(s);
    HBuf h;
    if (int rc = h.alloc(n)) return rc;
    if (int rc = copy_d2h(h.p, d, n, s)) return rc;
    std::memcpy(dst, h.p, n);
    return HS_OK;
}

static int ship_kernel(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    hsdev::ShipList L; L.n = 1;
    L.seg[0].src = src; L.seg[0].dst = dst; L.seg[0].bytes = (long long)bytes; L.seg[0].count = nullptr; L.seg[0].stride = 0; L.seg[0].cap = 0; L.seg[0].extra = 0;
    hipLaunchKernelGGL(hsdev::k_ship, dim3((unsigned)std::max<size_t>(1, std::min<size_t>(256, bytes / 4096 + 1))), dim3(256), 0, stream, L);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
// a transfer queued as a kernel (hsdev::k_ship: pinned host memory is mapped into the device's address space); segments whose length
// is a count on the device take it from there when the kernel runs
struct Shipment {
    hsdev::ShipList L;
    bool too_many = false;      // a segment beyond the list's: launch() refuses
    Shipment() { L.n = 0; }
    void seg(const hsdev::ShipSeg& g) { if (L.n < (int)(sizeof L.seg / sizeof L.seg[0])) L.seg[L.n++] = g; else too_many = true; }
    void add(void* dst, const void* src, size_t bytes) { if (bytes) seg(hsdev::ShipSeg{src, dst, (long long)bytes, nullptr, 0, 0, 0}); }
    void add_counted(void* dst, const void* src, const long long* d_count, size_t stride, long long cap, size_t extra = 0) {
        seg(hsdev::ShipSeg{src, dst, 0, d_count, (long long)stride, cap, (long long)extra});
    }
    // one 8-byte word of the device: a shipment moves 16-byte pieces, so the aligned piece that holds it goes to dst (16 bytes);
    // returns where the word then lies on the host
    const int64_t* add_word(void* dst, const int64_t* d_word) {
        const uintptr_t in_piece = reinterpret_cast<uintptr_t>(d_word) & 15;
        add(dst, reinterpret_cast<const char*>(d_word) - in_piece, 16);
        return reinterpret_cast<const int64_t*>((const char*)dst + in_piece);
    }
    int launch(hipStream_t s, int blocks = 256) {
        if (too_many) { set_error("a shipment of more segments than its list holds"); return HS_EINVAL; }
        if (L.n == 0) return HS_OK;
        hipLaunchKernelGGL(hsdev::k_ship, dim3((unsigned)blocks), dim3(256), 0, s, L);
        HS_HIP(hipGetLastError());
        L.n = 0;
        return HS_OK;
    }
};

// Timing events (the EventPairs of the stage code and the KernelClock's two per launch) are recorded on every step by default; a caller
// that times many steps asks for every n-th one (hs_kernel_stats_every: bench.py) -- with ~1200 event records per C4 step the records
// themselves cost the step 1.3 ms (alternating runs on one box: 15.6 against 16.9 ms), each being a packet of its own between two
// kernels of a stream. The pipeline calls timing_next_step() when a step begins (no launch of the previous one is in flight then).
static std::atomic<int> g_timing_every{1};
static std::atomic<long> g_timing_step{0};
static std::atomic<bool> g_timing_on{true};
static bool timing_on() { return g_timing_on.load(std::memory_order_relaxed); }
static void timing_next_step() { const int n = g_timing_every.load(); g_timing_on.store(n <= 1 || g_timing_step.fetch_add(1) % n == 0); }
static hipError_t ev_rec(hipEvent_t e, hipStream_t s) { return e ? hipEventRecord(e, s) : hipSuccess; }      // (an EventPair of an untimed step holds no events)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    static std::vector<hipEvent_t>& cache() { static thread_local std::vector<hipEvent_t> c; return c; }
    ~EventPair() { if (a) cache().push_back(a); if (b) cache().push_back(b); }
    static int get(hipEvent_t* e) {
        std::vector<hipEvent_t>& c = cache();
        if (!c.empty()) { *e = c.back(); c.pop_back(); return HS_OK; }
        HS_HIP(hipEventCreateWithFlags(e, hipEventDefault));
        return HS_OK;
    }
    int take() { if (int rc = get(&a)) return rc; return get(&b); }      // (whatever the step: a caller that times every call)
    int init() { return timing_on() ? take() : HS_OK; }
    // (called after the stream has been waited for: the events are complete and no synchronising call -- an ioctl in the
    // runtime -- is needed; one that is not yet complete is waited for the slow way)
    int ms(float* out) {
        if (!a || !b) { *out = 0; return HS_OK; }      // (untimed step)
        hipError_t e = hipEventElapsedTime(out, a, b);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); HS_HIP(hipEventSynchronize(b)); e = hipEventElapsedTime(out, a, b); }
        HS_HIP(e);
        return HS_OK;
    }
};

// Per-kernel accounting (include/hairsplitter_hip.h: hs_kernel_stats). A KernelClock belongs to one host thread / stream;
// begin() / end() bracket a launch (or a short run of launches of one family) with events, flush() -- called once the stream
// has been waited for -- turns them into durations and adds them to the process-wide table.
struct KernelTable {
    std::mutex mu;
    hs_kernel_stats st;
    KernelTable() { std::memset(&st, 0, sizeof st); }
};
KernelTable& kernel_table() { static KernelTable* t = new KernelTable(); return *t; }
struct KernelClock {
    struct Item { int k; hipEvent_t a, b; int64_t bytes; };
    std::vector<Item> items;
    hipEvent_t open_a = nullptr;
    int open_k = -1;
    static bool enabled() { static const bool on = std::getenv("HS_NO_KERNEL_STATS") == nullptr; return on && timing_on(); }
    int begin(int k, hipStream_t s) {
        if (!enabled()) return HS_OK;
        if (open_a) { EventPair::cache().push_back(open_a); open_a = nullptr; }      // (a begin() without its end(): an error path)
        if (int rc = EventPair::get(&open_a)) return rc;
        open_k = k;
        HS_HIP(ev_rec(open_a, s));
        return HS_OK;
    }
    // (end / end_prepare follow what begin() did, not the process-wide flag: another pipeline's step may have flipped it in between)
    int end(int64_t bytes, hipStream_t s) {
        if (!open_a) return HS_OK;
        hipEvent_t b = nullptr;
        if (int rc = EventPair::get(&b)) return rc;
        HS_HIP(ev_rec(b, s));
        items.push_back(Item{open_k, open_a, b, bytes});
        open_a = nullptr; open_k = -1;
        return HS_OK;
    }
    // for launches whose closing event is recorded by the callee: the item is queued, *b is recorded by the caller's callee
    int end_prepare(int64_t bytes, hipEvent_t* b) {
        if (!open_a) { *b = nullptr; return HS_OK; }
        if (int rc = EventPair::get(b)) return rc;
        items.push_back(Item{open_k, open_a, *b, bytes});
        open_a = nullptr; open_k = -1;
        return HS_OK;
    }
    static void add_bytes(int k, int64_t bytes) { if (!enabled()) return; KernelTable& t = kernel_table(); std::lock_guard<std::mutex> g(t.mu); t.st.bytes[k] += bytes; }      // (bytes the kernels count themselves: of the timed steps only, like the launches)
    void flush() {
        if (items.empty()) return;
        KernelTable& t = kernel_table();
        std::lock_guard<std::mutex> g(t.mu);
        for (Item& it : items) {
            float ms = 0;
            hipError_t e = hipEventElapsedTime(&ms, it.a, it.b);
            if (e == hipErrorNotReady) { (void)hipGetLastError(); e = hipEventSynchronize(it.b) == hipSuccess ? hipEventElapsedTime(&ms, it.a, it.b) : hipErrorUnknown; }
            if (e == hipSuccess) {
                t.st.ms[it.k] += ms; t.st.launches[it.k] += 1; t.st.bytes[it.k] += it.bytes;
            } else (void)hipGetLastError();
            if (it.a) EventPair::cache().push_back(it.a);
            if (it.b) EventPair::cache().push_back(it.b);
        }
        items.clear();
    }
    ~KernelClock() { flush(); if (open_a) EventPair::cache().push_back(open_a); }
};

// a launch (or a short run of launches of one family) between the two records of a caller's EventPair and the KernelClock's, under
// HS_K_OTHER. `bytes` is read when the launch has returned: one that learns its size on the way (the minimizers' count) sets it then.
template <class Launch> static int timed_launch(KernelClock& kc, EventPair& ev, hipStream_t st, const int64_t& bytes, Launch launch) {
    HS_HIP(ev_rec(ev.a, st));
    if (int rc = kc.begin(HS_K_OTHER, st)) return rc;
    if (int rc = launch()) return rc;
    if (int rc = kc.end(bytes, st)) return rc;
    HS_HIP(ev_rec(ev.b, st));
    return HS_OK;
}

static int host_threads() { return hs::host_threads(); }      // usable cores (hs_driver.cpp)

// How a caller's pageable array goes up, stated once: into a block of its own, `before` zero bytes in front and `behind` zero bytes
// behind it (a job's sequences carry HS_SEQ_PAD readable bytes on either side). Below 64 MB a plain hipMemcpy. Read bases and CIGAR ops
// are gigabytes: from 64 MB on the array goes through two pinned 32-MB buffers, a chunk copied into one on several host threads while
// the other is on its way (a plain hipMemcpy from pageable memory stages through the runtime's own buffers with one copying thread:
// 12-15 GB/s when batch creation was measured; at 115 MB the two are level, DESIGN 4.9d). Synchronous on the calling thread's default stream.
static int upload_pageable(DBuf& d, const void* src, size_t bytes, size_t before = 0, size_t behind = 0) {
    if (int rc = d.alloc(before + bytes + behind)) return rc;
    char* dst = (char*)d.p + before;
    if (before) HS_HIP(hipMemset(d.p, 0, before));
    if (behind) HS_HIP(hipMemset(dst + bytes, 0, behind));
    if (!bytes) return HS_OK;
    if (bytes < ((size_t)64 << 20)) { HS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return HS_OK; }
    const size_t CH = (size_t)32 << 20;
    HBuf stage[2];
    EventPair done;      // a: the copy that last used stage[0], b: stage[1]'s
    if (int rc = done.take()) return rc;
    const hipEvent_t stage_done[2] = {done.a, done.b};
    for (int k = 0; k < 2; ++k) if (int rc = stage[k].alloc(CH)) return rc;
    int k = 0;
    for (size_t off = 0; off < bytes; off += CH, k ^= 1) {
        const size_t n = std::min(CH, bytes - off);
        if (off >= 2 * CH) HS_HIP(hipEventSynchronize(stage_done[k]));      // (the copy that last used this buffer)
        const int parts = 8;
        hs::hs_parallel_for(parts, std::min(parts, host_threads()), [&](int q) {
            const size_t a = n * (size_t)q / parts, e = n * ((size_t)q + 1) / parts;
            std::memcpy((char*)stage[k].p + a, (const char*)src + off + a, e - a);
        });
        HS_HIP(hipMemcpyAsync(dst + off, stage[k].p, n, hipMemcpyHostToDevice, nullptr));
        HS_HIP(ev_rec(stage_done[k], nullptr));
    }
    HS_HIP(hipStreamSynchronize(nullptr));
    return HS_OK;
}

// a vector's elements in a malloc'd array of the C ABI's results (one element of room at least); nullptr: out of memory
template <class T> static T* malloc_copy(const std::vector<T>& v) {
    T* p = static_cast<T*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// K2 of one contig group at a time: the kernel fills the device on its own; eight of them side by side only slow each other
// down (0.29 ms alone, 1.0 ms each among eight) and every group would get its selection at the same late moment, whereas one
// after the other the groups' chains start 0.3 ms apart and their host work spreads out (44.5 -> 39.7 ms per C4 step). Taking
// turns for EVERY device phase of the groups was tried too: 52 ms per step -- the later phases are short, the lock then mostly
// adds its own queueing. HS_DEVICE_TURNS=0: no turns.
struct DeviceTurn {
    static std::mutex& mu() { static std::mutex m; return m; }
    static bool on() { static const bool v = []() { const char* e = std::getenv("HS_DEVICE_TURNS"); return !(e && e[0] == '0'); }(); return v; }
    std::unique_lock<std::mutex> lk;
    DeviceTurn() { if (on()) lk = std::unique_lock<std::mutex>(mu()); }
};

static void set_wait_policy() {}   // (the wait mode is no device state: see stream_wait)

int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available: the HairSplitter MI355X path has no CPU fallback");
        return HS_ENODEVICE;
    }
    static std::once_flag once;
    std::call_once(once, set_wait_policy);
    return HS_OK;
}

// The HIP current device is a per-thread setting (0 on a new thread): every thread that works on a batch -- the caller's, the
// contig-group threads of a pipeline -- binds itself to the batch's device first
static int bind_device(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return HS_OK;
    HS_HIP(hipSetDevice(device));
    return HS_OK;
}

}  // namespace

