// ngs_abi.cpp — the C ABI (include/ngram_search.h): handle registry, device residency of the
// index, per-call search contexts (stream + scratch) and result marshalling.
//
// Mirrors nGramSearch/dllmain.cpp (paths under /root/reference): the global shared_mutex
// (:22), smallest-free-handle allocation (:41-46), shared locks for searches (:63,84,100,122,
// 135,147) and exclusive locks for indexN/dispose (:39,112).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/ngram_search.h"
#include "ngs_build.h"
#include "ngs_index.h"
#include "ngs_join.h"
#include "ngs_kernels.h"
#include "ngs_match.h"
#include "ngs_set.h"
#include "ngs_sim.h"
#include "ngs_token.h"
#include "ngs_utf8.h"

namespace ngs {
namespace {

constexpr char kDefaultValid[] = ".%$ @0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
constexpr uint32_t kInt32Max = (uint32_t)std::numeric_limits<int32_t>::max();
constexpr size_t kOutBudget = size_t(1) << 30;       // bytes of (key, score) output per chunk
constexpr size_t kGeneralBudget = size_t(2) << 30;   // bytes of dense general-path state
constexpr uint32_t kSmallBatch = 16;                 // host batches up to this many queries take the latency path
constexpr size_t kSmallBlock = size_t(1) << 20;      // ... if their output block is at most this many bytes
constexpr size_t kPartBudget = size_t(1) << 30;      // bytes of sliced tier-1b partial results per call
constexpr uint32_t kSmallSlices = 32;                // ... or term-id slices per query (sliced k_wave)
constexpr size_t kSmallQ = size_t(64) << 10;         // ... and if their offsets + bytes fit this many bytes
// the latency path's one block, device and pinned host: statistics | results | queries
constexpr size_t kSioStats = sizeof(StatsBlock);
constexpr size_t kSioBytes = kSioStats + kSmallBlock + kSmallQ;
constexpr int kRetryQcap = -6;                       // finish_search: rerun with the batch's byte count
constexpr uint32_t kCalmCalls = 16;                  // grown survivor slots unused this many calls: halved

// the last HIP failure on this thread (ngsLastError): the reference's entry points answer 0 on
// failure, indistinguishable from "no results", so callers that care ask afterwards
thread_local int t_last_error = 0;
// failures that are not HIP errors (include/ngram_search.h: NGS_ERR_*)
constexpr int kErrInternal = 0x10001;     // a kernel reported an internal error (finish_search -5)
constexpr int kErrQueryBuffer = 0x10002;  // the batch outgrew the normalised-query buffer twice
constexpr int kErrRerankLimit = 0x10003;  // scoreBatchSim*: the effective limit is above kRerankMaxStride

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    std::fprintf(stderr, "ngram_search: %s failed: %s\n", what, hipGetErrorString(e));
    t_last_error = (int)e;
    return false;
}
#define HIP_CHECK(expr) hip_ok((expr), #expr)

// Phases of the host batch path (scoreBatch / searchBatch): nanoseconds summed over the calls since
// the last reset, read by ngsHostPhases (bench.py's detail.dropin). NGS_HOST_TIMING=1 also prints
// each phase (microseconds since the previous mark) to stderr.
enum HostPhase : int {
    kHpPack = 0,      // query lengths, offsets and bytes packed into pinned staging
    kHpQueue,         // H2D copies and the kernels queued
    kHpWait,          // the kernels, waited for
    kHpPackBack,      // the device pack of the results and the offsets back
    kHpRecords,       // the records back, marshalled into the new[]'d arrays as they land
    kHpCall,          // the whole call (scoreBatch / searchBatch)
    kHpCalls,         // (count) calls
    kHpReplays,       // (count) one-stream calls replayed from a graph (queue_search)
    kHpN
};
std::atomic<uint64_t> g_host_phase[kHpN];
struct HostTimer {
    bool on;
    std::chrono::steady_clock::time_point t;
    HostTimer() : on(std::getenv("NGS_HOST_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void mark(int id, const char* what) {
        const auto n = std::chrono::steady_clock::now();
        g_host_phase[id].fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(),
                                   std::memory_order_relaxed);
        if (on)
            std::fprintf(stderr, "[ngs host] %-28s %9.1f us\n", what,
                         std::chrono::duration<double, std::micro>(n - t).count());
        t = n;
    }
};

// Largest host batch (queries x limit entries) whose result arrays are allocated at capacity and
// filled as chunks finish (batch_query); larger ones collect the records first
constexpr uint64_t kDirectMax = uint64_t(1) << 25;


// body(lo, hi) over [0, n) on up to 8 host threads (one below `serial_below` items)
// A fixed pool of host worker threads for the batch path's packing and marshalling: spawning
// eight threads per use cost ~50 us each time (the pool's workers wait on a condition variable).
class HostPool {
  public:
    static HostPool& get() {
        static HostPool p;
        return p;
    }
    size_t size() const { return workers_.size() + 1; }
    // runs task(i) for i in [0, n) on the workers and the caller; returns when all are done
    void run(size_t n, const std::function<void(size_t)>& task) {
        std::unique_lock<std::mutex> lk(mu_);
        busy_.wait(lk, [&] { return !task_; });  // one parallel section at a time
        task_ = &task;
        n_ = n;
        next_ = 0;
        left_ = n;
        ++gen_;
        work_.notify_all();
        while (next_ < n_) {  // the caller takes items too
            const size_t i = next_++;
            lk.unlock();
            task(i);
            lk.lock();
            --left_;
        }
        done_.wait(lk, [&] { return left_ == 0; });
        task_ = nullptr;
        busy_.notify_all();
    }

  private:
    HostPool() {
        const size_t nt = std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
        for (size_t t = 1; t < nt; ++t) workers_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
        }
        work_.notify_all();
        for (auto& w : workers_) w.join();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        uint64_t seen = 0;
        for (;;) {
            work_.wait(lk, [&] { return quit_ || (task_ && gen_ != seen && next_ < n_); });
            if (quit_) return;
            seen = gen_;
            while (task_ && next_ < n_) {
                const size_t i = next_++;
                const std::function<void(size_t)>* t = task_;
                lk.unlock();
                (*t)(i);
                lk.lock();
                if (--left_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable work_, done_, busy_;
    const std::function<void(size_t)>* task_ = nullptr;
    size_t n_ = 0, next_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};

// body(lo, hi) over [0, n) on the host pool (serially below `serial_below` items)
template <class F>
void parallel_ranges(size_t n, size_t serial_below, F&& body) {
    HostPool& pool = HostPool::get();
    const size_t nt = n < serial_below ? 1 : pool.size();
    if (nt <= 1) {
        body(size_t(0), n);
        return;
    }
    const std::function<void(size_t)> task = [&](size_t t) { body(n * t / nt, n * (t + 1) / nt); };
    pool.run(nt, task);
}

// Persistent host threads for the parts of a batch split over replicas (dllmain.cpp:82-90 callers
// on an index placed on several devices): part 0 runs on the calling thread, part i on worker i - 1,
// each on its replica's device and contexts. One split at a time; a call that finds the workers
// busy (another thread's split) spawns threads of its own for that call.
class PartWorkers {
  public:
    explicit PartWorkers(size_t n) : n_(n), todo_(n, false) {
        for (size_t i = 0; i < n; ++i) th_.emplace_back([this, i] { loop(i); });
    }
    ~PartWorkers() {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
        }
        work_.notify_all();
        for (auto& t : th_) t.join();
    }
    size_t size() const { return n_; }
    // f(i) for i in [0, parts): i = 0 here, the rest on the workers; false if busy (nothing ran)
    bool try_run(size_t parts, const std::function<void(size_t)>& f) {
        std::unique_lock<std::mutex> call(call_mu_, std::try_to_lock);
        if (!call.owns_lock() || parts > n_ + 1) return false;
        {
            std::lock_guard<std::mutex> g(mu_);
            f_ = &f;
            left_ = parts - 1;
            for (size_t i = 0; i + 1 < parts; ++i) todo_[i] = true;
        }
        work_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return left_ == 0; });
        f_ = nullptr;
        return true;
    }

  private:
    void loop(size_t i) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            work_.wait(lk, [&] { return quit_ || todo_[i]; });
            if (quit_) return;
            todo_[i] = false;
            const std::function<void(size_t)>* f = f_;
            lk.unlock();
            (*f)(i + 1);
            lk.lock();
            if (--left_ == 0) done_.notify_all();
        }
    }
    size_t n_;
    std::vector<char> todo_;
    std::vector<std::thread> th_;
    std::mutex mu_, call_mu_;
    std::condition_variable work_, done_;
    const std::function<void(size_t)>* f_ = nullptr;
    size_t left_ = 0;
    bool quit_ = false;
};

// f(i) for the parts of a split: on the library's persistent workers, or threads of this call's own
template <class Workers>
void run_parts(Workers& w, size_t parts, const std::function<void(size_t)>& f) {
    if (w && w->try_run(parts, f)) return;
    std::vector<std::thread> th;
    for (size_t i = 1; i < parts; ++i) th.emplace_back(f, i);
    f(0);
    for (auto& t : th) t.join();
}

template <class T>
bool dev_alloc(T** p, size_t n) {
    *p = nullptr;
    return HIP_CHECK(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
}

template <class T>
bool dev_upload(T** p, const std::vector<T>& v, std::vector<void*>& owned, size_t pad = 0) {
    if (!dev_alloc(p, v.size() + pad)) return false;
    owned.push_back(*p);
    if (pad && !HIP_CHECK(hipMemset(*p + v.size(), 0, pad * sizeof(T)))) return false;
    return v.empty() || HIP_CHECK(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

// A page-locked host buffer, grown geometrically: the host entry points stage queries and
// results through these (asynchronous DMA at full PCIe rate instead of pageable bounce copies).
struct Pinned {
    void* p = nullptr;
    size_t cap = 0;
    bool grow(size_t bytes) {
        if (bytes <= cap) return true;
        const size_t nb = std::max<size_t>(bytes, cap * 2);
        if (p) hipHostFree(p);
        p = nullptr;
        cap = 0;
        if (!HIP_CHECK(hipHostMalloc(&p, std::max<size_t>(nb, 64), hipHostMallocDefault))) return false;
        cap = nb;
        return true;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    ~Pinned() {
        if (p) hipHostFree(p);
    }
};

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;      // the heavy list (cmin 2) beside tier 1a
    hipStream_t side2 = nullptr;     // tier 1b on the full list (cmin 1, short search) beside both
    hipEvent_t join = nullptr, join2 = nullptr;
    hipEvent_t prep_ev = nullptr, lists_ev = nullptr;  // k_prep done (s), heavy / full lists merged (side)
    hipEvent_t in_ev = nullptr;   // ngsSearchDeviceAsync: the caller's stream up to the call
    // d_stats needs no reset before the next call's k_prep (kPrepZero): k_prep zeroes the statistics
    // and the path counts, k_lists the list counters after reading them; false until a call has
    // queued both, and after a call that flagged *oflow
    bool stats_clean = false;
    // the latency path's block (d_sio): the statistics slots the context's last small batch added to,
    // which the next one's k_prep has to zero beside its own
    uint32_t sio_slots = 0;
    hipEvent_t ev[6] = {};
    hipEvent_t piece_ev[kBackPieces] = {};  // finish_host_chunk: the read-back's pieces landed
    size_t qcap = 0, bcap = 0, ncap = 0, ocap = 0;
    uint32_t ecap = kEmitCap;  // survivor slots per query in d_est / d_esc (ensure_queries, emit_cap)
    uint32_t ecap_grow = 0;    // slots later calls ask for: raised when tier 1a ran out of them
    size_t ebcap = 0;          // ... for this many queries
    uint32_t calm = 0;         // calls in a row with grown slots that no query filled
    bool shrink = false;       // ... enough of them: the next call gives half the slots back
    uint8_t* d_raw = nullptr;
    uint64_t* d_off = nullptr;
    uint8_t* d_norm = nullptr;
    uint32_t* d_qm = nullptr;
    uint32_t* d_glist = nullptr;
    uint32_t* d_list2 = nullptr;
    uint32_t* d_gcount = nullptr;  // the path counts behind d_stats' slots (PathCounts); not read
    uint32_t* d_fb = nullptr;      // queries tier 1a handed to tier 1b
    uint32_t* d_fb2 = nullptr;     // ... from the heavy list (side stream)
    uint32_t* d_heavy = nullptr;   // queries the prep kernel listed as heavy (cmin 2)
    uint32_t* d_full = nullptr;    // ... for tier 1b (cmin 1, short search)
    uint32_t* d_lslots = nullptr;  // k_prep's slot lists of both (2 * kListSlots * ceil(B / kListSlots))
    uint32_t* d_esn = nullptr;     // tier 1a survivor lists for k_emit: count per query,
    uint32_t* d_est = nullptr;     // kEmitCap terms and
    uint8_t* d_esc = nullptr;      // kEmitCap hit counts per query
    // the survivor arena (SearchParams.at): ablocks blocks of kArenaBlock entries, a chain link per
    // block and a first block per query (ebcap rows); grown (arena_grow) after a call ran out of it
    uint32_t* d_eovf = nullptr;
    uint32_t* d_anext = nullptr;
    uint32_t* d_at = nullptr;
    uint8_t* d_ac = nullptr;
    uint32_t ablocks = 0, arena_grow = 0;
    // arena_calm: calls in a row that used under a quarter of a grown arena (kCalmCalls: halved);
    // arena_off: calls left to run without an arena after its allocation failed
    uint32_t arena_calm = 0, arena_off = 0, arena_shrink_to = 0;
    uint32_t heavy_items = 0;      // (query, slice) items of the last call's heavy launch (SearchParams.hgrid)
    size_t eorows = 0;
    uint64_t* d_prec = nullptr;    // sliced tier 1b: top-L records per (query, slice)
    uint32_t* d_pcnt = nullptr;    // ... and their counts
    size_t pcap = 0, pncap = 0;    // records d_prec holds, counts d_pcnt holds
    uint32_t* d_group = nullptr;
    // a StatsBlock (the statistics slots and the path counts: one memset, one read-back), then the
    // 2 * kListSlots counter lines of k_prep's slot lists (d_lctr; same memset, not read back)
    DevStats* d_stats = nullptr;
    uint32_t* d_lctr = nullptr;
    DevStats* h_stats = nullptr;   // pinned host copy of the same
    // host-path outputs, one block holding [n (B + 1) | k (B * stride) | s (B * stride)] for the
    // call's B and stride, so that a small batch reads all of it back in one copy; packed copies
    // (launch_pack) for large batches
    uint32_t* d_out = nullptr;
    uint32_t* d_n = nullptr;
    uint32_t* d_k = nullptr;
    float* d_s = nullptr;
    uint32_t* d_pos = nullptr;  // [ncap + 1] packed offsets
    uint32_t* d_pk = nullptr;   // [2 * ocap] packed keys, or (pointer mode) u64 result pointers
    float* d_ps = nullptr;      // [ocap] packed scores
    void* d_ptemp = nullptr;    // scan scratch
    size_t ptemp_bytes = 0;
    GeneralBuffers gen;
    Pinned h_off, h_raw, h_res;  // queries in; results out
    // the U8 entry points: a batch's UTF-8 bytes and byte offsets as copied in, and the decoder's
    // scratch; the decoder writes the UTF-32 batch into d_raw / d_off (ensure_u8)
    uint8_t* d_u8 = nullptr;
    uint64_t* d_u8off = nullptr;
    void* d_u8temp = nullptr;
    size_t u8cap = 0, u8ncap = 0, u8temp_bytes = 0;
    uint8_t* d_sio = nullptr;     // the latency path's block (kSioBytes): one copy in, one copy out
    uint8_t* h_sio = nullptr;     // ... its pinned host image
    // one-stream calls (queue_search): calls built as graphs, replayed when a call's launch
    // arguments (the signature) repeat one of them; gseen: recent signatures, a call is built on
    // its second occurrence. Up to kGraphs of each (a pipelined caller rotates its output buffers
    // over the contexts in flight: C2's bench loop, 4 buffers over 3 contexts)
    static constexpr size_t kGraphs = 8;
    std::vector<std::pair<std::vector<uint8_t>, hipGraphExec_t>> graphs;
    std::vector<std::vector<uint8_t>> gseen;
    bool gfail = false;  // a graph failed to build: this context queues its calls one by one

    ~Context() {
        hipSetDevice(device);
        for (void* p : {(void*)d_raw, (void*)d_off, (void*)d_norm, (void*)d_qm, (void*)d_glist, (void*)d_list2, (void*)d_fb, (void*)d_fb2, (void*)d_heavy, (void*)d_full, (void*)d_lslots,
                        (void*)d_esn, (void*)d_est, (void*)d_esc, (void*)d_prec, (void*)d_pcnt,
                        (void*)d_eovf, (void*)d_anext, (void*)d_at, (void*)d_ac,
                        (void*)d_group, (void*)d_stats, (void*)d_sio, (void*)d_out, (void*)d_pos, (void*)d_pk, (void*)d_ps, d_ptemp, (void*)d_u8, (void*)d_u8off, d_u8temp, (void*)gen.cnt,
                        (void*)gen.kenc, (void*)gen.list, (void*)gen.sorted, (void*)gen.lcount, gen.temp})
            if (p) hipFree(p);
        for (auto& g : graphs) hipGraphExecDestroy(g.second);
        if (h_stats) hipHostFree(h_stats);
        if (h_sio) hipHostFree(h_sio);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : {join, join2, prep_ev, lists_ev, in_ev})
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : piece_ev)
            if (e) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
        if (side && side != stream && !side_shared) hipStreamDestroy(side);
        if (side2 && side2 != side && side2 != stream) hipStreamDestroy(side2);
    }
    bool side_shared = false;  // side is the replica's (shared by its contexts)
};

// The side stream runs the heavy list's chain and then the full list's tier 1b (cmin 1, short
// search) beside tier 1a, at normal priority (at the highest one the main launches' streams starved:
// rejected in round 1 and again in round 5). A third stream per context for the full list made one
// context's main stream share a hardware queue (HIP's default is four, one of them the null
// stream's) with the other's side work (a pipelined scoreBatch measured 2x slower that way); the
// side stream is also shared by the replica's contexts (queue_search).
hipError_t make_side_stream(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }

// One copy of the index in one device's HBM, with its pool of per-call contexts. An index built
// after ngsSetDevices has one replica per listed device; batches are split across them.
struct Replica {
    int device = 0;
    DevIndex dev{};
    const float* wild_w = nullptr;  // the keys' wildcard weights (ngsSaveIndex reads them back)
    // dictionary indexes: gram ids (rows of gram_off) and slots of ghash_key / ghash_val as uploaded
    // (ngsReplicaDigest; the host's copies are freed after the upload)
    uint64_t n_gram_ids = 0, ghash_slots = 0;
    std::vector<void*> owned;
    std::mutex pool_mu;
    std::vector<std::unique_ptr<Context>> pool;
    // DevIndex.kt_flag per validChar set in use (indexes with kt_off only): made once per set, kept
    // until dispose (a launch in flight may still read an older set's)
    std::mutex kflag_mu;
    std::vector<std::pair<std::array<uint32_t, 8>, uint8_t*>> kflags;
    // the last main tier-1a launch of any call on this replica (launch_fast orders the next after it)
    std::mutex main_mu;
    hipEvent_t main_ev = nullptr;
    bool main_rec = false;
    hipStream_t shared_side = nullptr;  // one side stream for every context (made under main_mu)
    // the similarity stage's key -> term map of an index whose keys have one pair each (no kt_off):
    // built from tk on the device by the first similarity call on the replica (sim_key_term)
    std::mutex sim_mu;
    const uint32_t* key_term = nullptr;
    // the token-sorted terms (NGS_SIM_TOKEN_SORT): term_off / term_bytes of the terms' sorted forms,
    // built from the device's term arrays by the first flagged call on the replica (sim_sorted_terms)
    const uint64_t* ts_off = nullptr;
    const uint8_t* ts_bytes = nullptr;

    // the index as the kernels of a search under `valid` see it (kt_flag for that set); false on a
    // HIP failure
    bool index_for(const uint32_t valid[8], DevIndex& X) {
        X = dev;
        X.kt_flag = nullptr;
        if (!dev.kt_off) return true;
        std::array<uint32_t, 8> v;
        std::copy(valid, valid + 8, v.begin());
        std::lock_guard<std::mutex> g(kflag_mu);
        for (auto& e : kflags)
            if (e.first == v) {
                X.kt_flag = e.second;
                return true;
            }
        uint8_t* f = nullptr;
        if (!HIP_CHECK(hipSetDevice(device)) || !HIP_CHECK(hipMalloc(&f, std::max<size_t>(dev.n_keys, 1)))) return false;
        owned.push_back(f);
        // synchronously: a search on another stream may use the set as soon as it is listed
        if (!HIP_CHECK(build_key_flags(dev, valid, f, nullptr)) || !HIP_CHECK(hipStreamSynchronize(nullptr))) return false;
        kflags.emplace_back(v, f);
        X.kt_flag = f;
        return true;
    }

    // The similarity entry points queue kernels that read the index on the caller's stream and
    // return: the device is drained before the index arrays go, so dispose() does not free one
    // under such a kernel (hipFree waits for the device as well; this states it).
    ~Replica() {
        pool.clear();
        hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (main_ev) hipEventDestroy(main_ev);
        if (shared_side) hipStreamDestroy(shared_side);
        for (void* p : owned) hipFree(p);
    }

    std::unique_ptr<Context> acquire() {
        {
            std::lock_guard<std::mutex> g(pool_mu);
            if (!pool.empty()) {
                auto c = std::move(pool.back());
                pool.pop_back();
                return c;
            }
        }
        auto c = std::make_unique<Context>();
        c->device = device;
        // (the side streams are made by the first call whose batch needs them, queue_search)
        if (!HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) ||
            !HIP_CHECK(hipEventCreateWithFlags(&c->join, hipEventDisableTiming)) ||
            !HIP_CHECK(hipEventCreateWithFlags(&c->join2, hipEventDisableTiming)) ||
            !HIP_CHECK(hipEventCreateWithFlags(&c->prep_ev, hipEventDisableTiming)) ||
            !HIP_CHECK(hipEventCreateWithFlags(&c->lists_ev, hipEventDisableTiming)) ||
            !HIP_CHECK(hipEventCreateWithFlags(&c->in_ev, hipEventDisableTiming)))
            return nullptr;
        for (hipEvent_t& e : c->ev)
            if (!HIP_CHECK(hipEventCreate(&e))) return nullptr;
        for (hipEvent_t& e : c->piece_ev)
            if (!HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return nullptr;
        if (!dev_alloc(&c->d_group, kGeneralMaxGroup) || !dev_alloc(&c->d_stats, sizeof(StatsBlock) / sizeof(DevStats) + 2 * kListSlots) ||
            !dev_alloc(&c->d_sio, kSioBytes) ||
            !HIP_CHECK(hipMemsetAsync(c->d_sio, 0, kSioStats, c->stream)) ||
            !HIP_CHECK(hipStreamSynchronize(c->stream)) ||
            !HIP_CHECK(hipHostMalloc((void**)&c->h_sio, kSioBytes, hipHostMallocDefault)) ||
            !HIP_CHECK(hipHostMalloc((void**)&c->h_stats, sizeof(StatsBlock), hipHostMallocDefault)))
            return nullptr;
        StatsBlock* const sb = reinterpret_cast<StatsBlock*>(c->d_stats);
        c->d_gcount = &sb->paths.general;
        c->d_lctr = reinterpret_cast<uint32_t*>(sb + 1);
        return c;
    }
    void give_back(std::unique_ptr<Context> c) {
        std::lock_guard<std::mutex> g(pool_mu);
        pool.push_back(std::move(c));
    }
};

// ngsServe: the low-latency score() path. A persistent kernel (k_serve) on a stream of its own,
// one wave per request slot, polls request blocks in coherent pinned host memory; score() takes a
// free slot, writes the normalised query there, publishes a request number and spins until the
// kernel publishes it back with the results: no launch, no copy, no stream wait per call, and up
// to kServeSlots callers served side by side. The kernel exits on stop, after kServeIdleMs without
// a request or after kServeLifeMs, and is relaunched on demand.
constexpr uint32_t kServeIdleMs = 200;
constexpr uint32_t kServeLifeMs = 10000;
// score()/search() start the server by themselves (no ngsServe call) from this many single-query
// calls on a library the server can answer (fewer than 16 skip buckets, narrow strings)
constexpr uint32_t kAutoServeAfter = 4;

struct Server {
    int device = 0;
    hipStream_t stream = nullptr;
    ServeBlock* h = nullptr;  // kServeSlots request blocks, coherent pinned host memory
    ServeBlock* d = nullptr;  // their device view
    DevStats* scratch = nullptr;
    uint32_t* list2 = nullptr;
    unsigned long long* t_any = nullptr;  // the latest request time of any slot (device memory)
    uint64_t seq[kServeSlots] = {};
    std::mutex slot_mu[kServeSlots];  // one request per slot at a time
    std::mutex launch_mu;             // one (re)launch at a time
    std::atomic<bool> launched{false};
    uint32_t launch_valid[8] = {};  // the validChar set of its DevIndex.kt_flag

    bool init(int dev) {
        device = dev;
        const size_t nst = (size_t)kServeSlots * (sizeof(StatsBlock) / sizeof(DevStats));  // a StatsBlock per slot
        if (!HIP_CHECK(hipSetDevice(dev)) || !HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) ||
            !HIP_CHECK(hipHostMalloc((void**)&h, sizeof(ServeBlock) * kServeSlots,
                                     hipHostMallocCoherent | hipHostMallocMapped)) ||
            !HIP_CHECK(hipHostGetDevicePointer((void**)&d, h, 0)) ||
            !HIP_CHECK(hipMalloc((void**)&scratch, sizeof(DevStats) * nst)) ||
            !HIP_CHECK(hipMalloc((void**)&list2, sizeof(uint32_t) * 4 * kServeSlots)) ||
            !HIP_CHECK(hipMalloc((void**)&t_any, sizeof(unsigned long long))))
            return false;
        std::memset((void*)h, 0, sizeof(ServeBlock) * kServeSlots);
        return HIP_CHECK(hipMemset(scratch, 0, sizeof(DevStats) * nst)) &&
               HIP_CHECK(hipMemset(t_any, 0, sizeof(unsigned long long)));
    }
    // the kernel has left (idle, lifetime, stop) or was never launched
    bool stopped() { return !launched || hipStreamQuery(stream) == hipSuccess; }
    void stop() {
        if (!h) return;
        __atomic_store_n(&h->stop, 1u, __ATOMIC_RELEASE);
        if (stream) hipStreamSynchronize(stream);  // it exits within one poll
        launched = false;
        __atomic_store_n(&h->stop, 0u, __ATOMIC_RELEASE);
    }
    ~Server() {
        if (h) stop();
        hipSetDevice(device);
        if (stream) hipStreamDestroy(stream);
        if (h) hipHostFree(h);
        if (scratch) hipFree(scratch);
        if (list2) hipFree(list2);
        if (t_any) hipFree(t_any);
    }
};

struct Library {
    std::unique_ptr<Server> server;  // ngsServe (null: off)
    std::atomic<bool> serving{false};  // server != null, for the unlocked test in one_query
    std::shared_mutex server_mu;     // creating / dropping / stopping it (exclusive); requests (shared)
    std::atomic<int> serve_pref{0};  // 0: automatic (kAutoServeAfter), 1: ngsServe(h, 1), -1: ngsServe(h, 0)
    std::atomic<uint32_t> single_calls{0};  // score()/search() calls so far (automatic start)
    // batch calls in flight: the server kernel is stopped while any runs and not relaunched until
    // they are done, so no batch kernel queues behind it on a shared hardware queue
    std::atomic<int> batches{0};
    HostIndex host;
    uint64_t serial = 0;                         // this index's own number, never given twice (index sets)
    int device = 0;                              // first replica's device (or the build device)
    std::vector<std::unique_ptr<Replica>> reps;  // empty until the index is on a GPU
    std::mutex valid_mu;
    uint32_t valid[8] = {};
    std::atomic<bool> timing{false};
    std::mutex stats_mu;
    ngs_stats last{};
    bool tk_identity = false;  // DevIndex.tk_identity / tk_monotone / w_max, computed once for every replica
    bool tk_monotone = false;
    float w_max = 0.0f;
    bool rank_lists = false;   // DevIndex.rank_post: one weight (w_uniform), one pair per term, one term per key
    uint32_t w_uniform = 0;
    // DevIndex.kt_off / kt_term (keys with several pairs), built once in upload() for every replica
    std::vector<uint32_t> kt_off, kt_term;
    // the replicas a batch is split over (upload), and host threads for its parts past the first
    std::vector<uint32_t> split;
    std::unique_ptr<PartWorkers> workers;

    // ngsSearchDeviceAsync calls in flight: their context stays out of the pool until
    // ngsSearchDeviceWait (the general path and the statistics need the host afterwards)
    struct Pending {
        Replica* R = nullptr;
        std::unique_ptr<Context> c;
        SearchParams P{};
        const uint8_t* dq = nullptr;
        const uint64_t* doff = nullptr;
        uint32_t B = 0, Lm = 0, stride = 0;
        float thr = 0;
        uint32_t *dn = nullptr, *dk = nullptr;
        float* ds = nullptr;
        int rc = 0;  // queueing already failed
    };
    std::mutex pend_mu;
    std::unordered_map<uint64_t, Pending> pending;

    // The UTF-8 key table of a wide index (the U8 entry points' result strings): every key encoded
    // once (ngs_utf8.h: the decoder's inverse, so an indexU8 key comes back as the bytes indexed),
    // NUL-terminated, and its byte offsets on each replica's device for k_pack's pointer mode. Built
    // by the first U8 call (u8_keys, under the shared lock beside other searches): W-only callers
    // pay nothing. The device arrays are the replicas' (Replica::owned).
    struct U8Keys {
        std::once_flag once;
        bool ok = false;
        std::vector<char> bytes;             // key_bytes8
        std::vector<uint64_t> off;           // n_keys + 1 byte offsets
        std::vector<const uint64_t*> d_off;  // per replica
    } u8;
    uint64_t next_ticket = 1;

    ~Library() {
        workers.reset();  // (idle: dispose holds the exclusive lock, so no split is running)
        server.reset();  // stops the kernel before the index it reads is freed
        for (auto& kv : pending)  // dispose: nothing may still run on the buffers freed below
            if (kv.second.c) hipStreamSynchronize(kv.second.c->stream);
        pending.clear();
        reps.clear();
    }
    // the replica on `dev`, or null
    Replica* replica_at(int dev) {
        for (auto& r : reps)
            if (r->device == dev) return r.get();
        return nullptr;
    }
};

std::shared_mutex g_lock;                                        // dllmain.cpp:22
std::unordered_map<uint32_t, std::unique_ptr<Library>> g_libs;   // dllmain.cpp:24
uint64_t g_next_serial = 1;                                       // Library::serial (under the exclusive lock)
thread_local std::vector<int> t_devices;                          // ngsSetDevice(s): this thread's next builds

Library* find_lib(uint32_t h) {
    auto it = g_libs.find(h);
    return it == g_libs.end() ? nullptr : it->second.get();
}

// Places one copy of the host-built index on device R.device. The host arrays stay until every
// replica is uploaded (free_uploaded).
// `first`: the first replica settles the host index's gram fields (or builds the gram CSR on the
// host when the device build fails); later replicas are placed concurrently and only read them.
bool upload_replica(Library& L, Replica& R, bool keys_unique, bool first) {
    if (!HIP_CHECK(hipSetDevice(R.device))) return false;
    HostIndex& H = L.host;
    DevIndex& X = R.dev;
    X.n_terms = H.n_terms;
    X.n_short = H.n_short;
    X.n_keys = H.n_keys;
    X.keys_unique = keys_unique ? 1u : 0u;
    X.tk_identity = L.tk_identity ? 1u : 0u;
    X.tk_monotone = L.tk_monotone ? 1u : 0u;
    X.w_max = L.w_max;
    const std::vector<char>& kb = H.key_bytes;
    uint64_t *gram_off, *term_off, *key_off;
    uint32_t *post, *tk_off, *wild_key, *gram_row, *skip;
    uint8_t* term_bytes;
    char* key_bytes;
    uint2* tk;
    float *wild_w, *wild_score;
    // from here on the replica's destructor frees what was allocated
    PhaseTimer pt;
    bool ok = dev_upload(&term_off, H.term_off, R.owned) && dev_upload(&term_bytes, H.term_bytes, R.owned, 8) /* whole dwords, and a short term's second dword (myers_short) */ &&
              dev_upload(&tk_off, H.tk_off, R.owned) && dev_upload(&tk, H.tk, R.owned) &&
              dev_upload(&key_off, H.key_off, R.owned) && dev_upload(&key_bytes, kb, R.owned, 4) /* whole dwords (k_key_queries) */ &&
              dev_upload(&wild_w, H.wild_w, R.owned);
    if (!ok) return false;
    pt.mark("replica: arrays to HBM");
    bool dev_built = false;
    uint64_t n_post = H.post.size();
    if (!H.grams_built) {
        // the gram CSR and skip table from the terms now in HBM (ngs_build.hip); dictionary
        // indexes first find their distinct gram keys there and the host lays out the lookup table
        // from them (the first replica; the others reuse it). On failure the host builds them.
        DeviceGrams dg;
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipSuccess;
        uint64_t* dict = nullptr;
        if (H.gram_mode == 1) {
            if (first) {
                std::vector<uint64_t> keys;
                e = gram_keys_device(term_off, term_bytes, H.n_short, H.n_terms, H.csize, H.gsz, keys);
                if (e == hipSuccess) set_gram_dict(H, std::move(keys));
            }
            if (e == hipSuccess) e = hipMalloc(&dict, sizeof(uint64_t) * std::max<size_t>(H.gram_keys.size(), 1));
            if (e == hipSuccess && !H.gram_keys.empty())
                e = hipMemcpy(dict, H.gram_keys.data(), sizeof(uint64_t) * H.gram_keys.size(), hipMemcpyHostToDevice);
        }
        if (e == hipSuccess)
            e = build_grams_device(term_off, term_bytes, H.n_short, H.n_terms, dg, dict, (uint32_t)H.gram_keys.size(),
                                   H.csize, H.gsz);
        if (dict) (void)hipFree(dict);
        if (std::getenv("NGS_BUILD_TIMING"))
            std::fprintf(stderr, "[ngs build] %-22s %8.3f s\n", "gram CSR + skip (GPU)",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (e == hipSuccess) {
            for (void* p : {(void*)dg.gram_off, (void*)dg.post, (void*)dg.gram_row, (void*)dg.skip}) R.owned.push_back(p);
            gram_off = dg.gram_off;
            post = dg.post;
            gram_row = dg.gram_row;
            skip = dg.skip;
            n_post = dg.n_post;
            if (first) {
                H.n_grams = dg.n_grams;
                H.n_buckets = dg.n_buckets;
                H.bucket_span = dg.bucket_span;
            } else if (H.n_grams != dg.n_grams || H.n_buckets != dg.n_buckets || H.bucket_span != dg.bucket_span) {
                return false;  // cannot happen: every device builds the same CSR
            }
            dev_built = true;
        } else {
            (void)hipGetLastError();
            if (!first) return false;  // the host index is shared by the replicas placed concurrently
            build_grams_host(H);
            if (!H.grams_built) return false;
        }
    }
    if (!dev_built)  // host-built gram CSR (NGS_HOST_GRAMS, device-build failure)
        ok = dev_upload(&gram_off, H.gram_off, R.owned) && dev_upload(&post, H.post, R.owned, 4) /* k_wave stages whole 16-byte chunks */ &&
             dev_upload(&gram_row, H.gram_row, R.owned) && dev_upload(&skip, H.skip, R.owned);
    if (!ok) return false;
    uint64_t* ghash_key = nullptr;
    uint32_t* ghash_val = nullptr;
    if (H.gram_mode == 1 && !(dev_upload(&ghash_key, H.ghash_key, R.owned) && dev_upload(&ghash_val, H.ghash_val, R.owned)))
        return false;
    if (H.gram_mode == 1) {
        R.n_gram_ids = H.gram_keys.size();
        R.ghash_slots = H.ghash_key.size();
    }
    X.gsz = H.gsz;
    X.csize = H.csize;
    X.gram_mode = H.gram_mode;
    X.short_query_len = H.short_query_len;
    X.full_scan_len = H.full_scan_len;
    X.ghash_bits = H.ghash_bits;
    X.ghash_key = ghash_key;
    X.ghash_val = ghash_val;
    R.wild_w = wild_w;
    if (!dev_alloc(&wild_key, H.n_keys)) return false;
    R.owned.push_back(wild_key);
    if (!dev_alloc(&wild_score, H.n_keys)) return false;
    R.owned.push_back(wild_score);
    pt.mark("replica: gram CSR");
    if (!HIP_CHECK(build_wildcard(wild_w, H.n_keys, wild_key, wild_score, nullptr))) return false;
    X.kt_off = nullptr;
    X.kt_term = nullptr;
    if (!L.kt_off.empty()) {
        uint32_t *kt_off, *kt_term;
        if (!(dev_upload(&kt_off, L.kt_off, R.owned) && dev_upload(&kt_term, L.kt_term, R.owned))) return false;
        X.kt_off = kt_off;
        X.kt_term = kt_term;
    }
    X.rank_post = nullptr;
    X.w_uniform = L.w_uniform;
    if (L.rank_lists && n_post <= kRankMaxPostings) {
        // the threshold-0 shortcut's rank lists (4 bytes per posting); an index that cannot have them
        // (over 2^31 postings, or no memory for them) searches without them
        const uint32_t n_seg = H.gram_mode == 1 ? (uint32_t)H.gram_keys.size() : (uint32_t)kGramSpace;
        uint32_t* rp = nullptr;
        if (hipMalloc(&rp, sizeof(uint32_t) * (n_post + 4)) == hipSuccess) {
            const hipError_t e = build_rank_post(gram_off, n_seg, post, n_post, tk, H.n_short, H.n_keys, rp, nullptr);
            if (e == hipSuccess) {
                R.owned.push_back(rp);
                X.rank_post = rp;
            } else {
                (void)hipFree(rp);
                if (e != hipErrorNotSupported && !HIP_CHECK(e)) return false;
            }
        }
        (void)hipGetLastError();
        pt.mark("replica: rank lists");
    }
    X.gram_off = gram_off;
    X.post = post;
    X.gram_row = gram_row;
    X.skip = skip;
    X.n_buckets = H.n_buckets;
    X.bucket_span = H.bucket_span;
    X.post_per_row = (uint32_t)std::min<uint64_t>(UINT32_MAX, n_post / std::max<uint64_t>(H.n_grams, 1));
    X.term_off = term_off;
    X.term_bytes = term_bytes;
    X.tk_off = tk_off;
    X.tk = tk;
    X.key_off = key_off;
    X.key_bytes = reinterpret_cast<const uint8_t*>(key_bytes);
    X.wild_key = wild_key;
    X.wild_score = wild_score;
    // the build's null-stream work completes before any search stream (non-blocking) reads it
    const bool synced = HIP_CHECK(hipDeviceSynchronize());
    pt.mark("replica: wildcard answer");
    return synced;
}

// The device copies are authoritative for the search; keep only what marshalling needs.
void free_uploaded(HostIndex& H) {
    std::vector<uint64_t>().swap(H.gram_off);
    std::vector<uint32_t>().swap(H.post);
    std::vector<uint32_t>().swap(H.gram_row);
    std::vector<uint32_t>().swap(H.skip);
    std::vector<uint64_t>().swap(H.term_off);
    std::vector<uint8_t>().swap(H.term_bytes);
    std::vector<uint32_t>().swap(H.tk_off);
    std::vector<uint2>().swap(H.tk);
    std::vector<float>().swap(H.wild_w);
    std::vector<uint64_t>().swap(H.ghash_key);
    std::vector<uint32_t>().swap(H.ghash_val);
    std::vector<uint64_t>().swap(H.gram_keys);
}

// One replica per device in `devs` (repeats allowed: several replicas on one device split a batch
// like several devices do, which the one-GPU tests use).
bool upload(Library& L, const std::vector<int>& devs) {
    const HostIndex& H = L.host;
    PhaseTimer pt;
    bool keys_unique = true;
    {
        std::vector<uint8_t> seen(H.n_keys, 0);
        for (const uint2& kw : H.tk) {
            if (seen[kw.x]) { keys_unique = false; break; }
            seen[kw.x] = 1;
        }
    }
    // term -> pairs shape and the largest weight (term_pairs in ngs_kernels.hip)
    L.tk_identity = H.tk_off.size() == (size_t)H.n_terms + 1;
    for (size_t t = 0; L.tk_identity && t < H.tk_off.size(); ++t) L.tk_identity = H.tk_off[t] == t;
    // term ids in key-rank order: every key rank of term t is below every key rank of t + 1
    // (DevIndex.tk_monotone; the build orders terms by their best key rank, so this fails only
    // where a key has several terms or a short term's key ranks above a long one's)
    L.tk_monotone = true;
    {
        int64_t prev = -1;
        for (size_t t = 0; L.tk_monotone && t + 1 < H.tk_off.size(); ++t) {
            uint32_t lo = UINT32_MAX, hi = 0;
            for (uint32_t p = H.tk_off[t]; p < H.tk_off[t + 1]; ++p) {
                lo = std::min(lo, H.tk[p].x);
                hi = std::max(hi, H.tk[p].x);
            }
            if (lo == UINT32_MAX) continue;  // no pair
            L.tk_monotone = (int64_t)lo > prev;
            prev = hi;
        }
    }
    L.w_max = 0.0f;
    for (const uint2& kw : H.tk) {
        float w;
        std::memcpy(&w, &kw.y, sizeof w);
        if (w > L.w_max) L.w_max = w;  // NaN weights score +0 (pair_enc) and never raise the bound
    }
    // the threshold-0 shortcut (DevIndex.rank_post) needs one record shape per hit count: one weight.
    // Its one-hit prefix entries stand in for multi-hit records only while a one-hit score is at most
    // the record's own: w * fl(1/n) <= 100 (a promoted record) needs w <= 200 (n >= 2)
    L.rank_lists = keys_unique && L.tk_identity && !H.tk.empty() && !std::getenv("NGS_NO_RANK_LISTS");
    L.w_uniform = H.tk.empty() ? 0u : H.tk.front().y;
    for (size_t i = 0; L.rank_lists && i < H.tk.size(); ++i) L.rank_lists = H.tk[i].y == L.w_uniform;
    {
        float wu;
        std::memcpy(&wu, &L.w_uniform, sizeof wu);
        if (!(wu <= 200.0f)) L.rank_lists = false;
    }
    // key -> terms for keys with several pairs (DevIndex.kt_off, key_promoted_long)
    L.kt_off.clear();
    L.kt_term.clear();
    if (!keys_unique) {
        L.kt_off.assign((size_t)H.n_keys + 1, 0);
        for (const uint2& kw : H.tk) L.kt_off[kw.x + 1]++;
        for (uint32_t k = 0; k < H.n_keys; ++k) L.kt_off[k + 1] += L.kt_off[k];
        L.kt_term.resize(H.tk.size() + 1);
        std::vector<uint32_t> fill(L.kt_off.begin(), L.kt_off.end() - 1);
        for (uint32_t t = 0; (size_t)t + 1 < H.tk_off.size(); ++t)
            for (uint32_t p = H.tk_off[t]; p < H.tk_off[t + 1]; ++p) L.kt_term[fill[H.tk[p].x]++] = t;
    }
    pt.mark("upload: index shape checks");
    for (int d : devs) {
        L.reps.push_back(std::make_unique<Replica>());
        L.reps.back()->device = d;
    }
    // the first replica alone (it settles the host index's gram fields), then the others at once,
    // one host thread each: every device has its own PCIe link, so placing n replicas takes about
    // the time of one instead of n (C5 x 8: ~6.5 GB each)
    if (!upload_replica(L, *L.reps.front(), keys_unique, true)) return false;
    if (L.reps.size() > 1) {
        std::vector<char> rok(L.reps.size(), 0);
        std::vector<int> rerr(L.reps.size(), 0);
        std::vector<std::thread> th;
        for (size_t i = 1; i < L.reps.size(); ++i)
            th.emplace_back([&, i] {
                t_last_error = 0;
                rok[i] = upload_replica(L, *L.reps[i], keys_unique, false);
                rerr[i] = t_last_error;
            });
        for (auto& t : th) t.join();
        // a later replica whose device build failed is placed again on this thread, serially, with
        // the host-built gram CSR (what the first replica falls back to) instead of failing indexN
        for (size_t i = 1; i < L.reps.size(); ++i) {
            if (rok[i]) continue;
            if (rerr[i]) t_last_error = rerr[i];
            const int dev = L.reps[i]->device;
            L.reps[i] = std::make_unique<Replica>();
            L.reps[i]->device = dev;
            (void)hipSetDevice(dev);
            (void)hipGetLastError();
            if (!L.host.grams_built) build_grams_host(L.host);
            if (!L.host.grams_built || !upload_replica(L, *L.reps[i], keys_unique, false)) return false;
        }
    }
    L.device = devs.front();
    // the replicas a batch is split over: the first one on each device (NGS_SPLIT_SAME_DEVICE=1, a
    // test hook for one-GPU boxes: every replica). Two replicas on one device add no compute, and
    // their halves' streams share the device's hardware queues: at C3 a forced split ran 1.34x one
    // replica's time (profiles/r06_s2_dropin_replicas.txt)
    static const bool same_dev = [] {
        const char* e = std::getenv("NGS_SPLIT_SAME_DEVICE");
        return e && std::atoi(e) != 0;
    }();
    L.split.clear();
    for (size_t i = 0; i < L.reps.size(); ++i) {
        bool first = true;
        for (size_t j = 0; j < i && !same_dev; ++j) first &= L.reps[j]->device != L.reps[i]->device;
        if (first) L.split.push_back((uint32_t)i);
    }
    if (L.split.size() > 1) L.workers = std::make_unique<PartWorkers>(L.split.size() - 1);
    free_uploaded(L.host);
    std::vector<uint32_t>().swap(L.kt_off);
    std::vector<uint32_t>().swap(L.kt_term);
    pt.mark("upload: replicas placed");
    return true;
}

// Survivor slots per query of tier 1a (d_est / d_esc, 5 bytes each): the wide cap for batches
// up to kEmitWideBatch, at every threshold, halved until the slots fit kEmitWideBytes per context
// (4,096 up to 52,428 queries, 2,048 at 65,536, 1,024 at C5's 131,072). The main launch's queries
// with more survivors go on in the batch's survivor arena (ensure_arena), which holds only what
// they use: C4 (3,960 survivors per query on average, a long tail) takes 1.8 GiB per context this
// way against 2.2 GiB with 4,096 slots and 10 GiB with round 4's slots grown to 32,768
// (profiles/r05_s5_c4_arena.txt). Queries of the heavy list's launch have no arena: past their
// slots they go to tier 1b, and the slots grow when that is frequent (finish_search). Sizing the
// cap by threshold (wide only at thr <= 1/8) handed 26,594 C4 and 7,871 C5 queries per batch to
// tier 1b before the arena (profiles/r03_s4_ab_ecap.txt).
uint32_t emit_cap(size_t B) {
    static const uint32_t init = [] {  // NGS_ECAP_INIT: the slots a context starts with (tests)
        const char* e = std::getenv("NGS_ECAP_INIT");
        return e ? std::max<uint32_t>(kRankInfo + 64, (uint32_t)std::strtoul(e, nullptr, 0)) : 0u;
    }();
    if (init) return init;
    if (B > kEmitWideBatch) return kEmitCap;
    uint32_t cap = std::max(kEmitCap, kEmitCapWide);
    while (cap > kEmitCap && (uint64_t)B * cap * 5ull > kEmitWideBytes) cap /= 2;
    return cap;
}

// The most survivor slots per query a batch of B may grow to: powers of two up to kEmitCapMax,
// within kEmitBudget bytes per context (5 bytes a slot).
uint32_t emit_cap_max(size_t B) {
    uint32_t cap = kEmitCap;
    while (cap < kEmitCapMax && (uint64_t)std::max<size_t>(B, 1) * (cap * 2ull) * 5ull <= kEmitBudget) cap *= 2;
    return cap;
}

bool ensure_queries(Context& c, size_t B, size_t bytes) {
    if (B > c.bcap) {
        for (void** p : {(void**)&c.d_off, (void**)&c.d_qm, (void**)&c.d_glist, (void**)&c.d_list2, (void**)&c.d_fb,
                         (void**)&c.d_fb2, (void**)&c.d_heavy, (void**)&c.d_full, (void**)&c.d_lslots, (void**)&c.d_esn})
            if (*p) { hipFree(*p); *p = nullptr; }
        size_t nb = std::max<size_t>(B, 1024);
        if (!dev_alloc(&c.d_off, nb + 1) || !dev_alloc(&c.d_qm, nb) || !dev_alloc(&c.d_glist, nb) ||
            !dev_alloc(&c.d_list2, nb) || !dev_alloc(&c.d_fb, nb) || !dev_alloc(&c.d_fb2, nb) || !dev_alloc(&c.d_heavy, nb) || !dev_alloc(&c.d_full, nb) ||
            !dev_alloc(&c.d_lslots, 2 * (nb + kListSlots)) || !dev_alloc(&c.d_esn, nb))
            return false;
        c.bcap = nb;
    }
    // the survivor slots: (re)allocated when the batch or the cap this call needs outgrows them,
    // or when a grown cap is given back (finish_search). The rows are this call's batch (or the
    // rows held, if more and the cap is unchanged), and the cap is bounded by kEmitBudget at the
    // rows actually allocated: a context that once ran a large batch must not grow a small
    // batch's cap into rows x cap bytes past the budget.
    uint32_t want = emit_cap(B);
    if (c.ecap_grow > want) want = std::min(c.ecap_grow, std::max(want, emit_cap_max(B)));
    const bool give_back = c.shrink && c.d_est && want < c.ecap;
    c.shrink = false;
    if (!c.d_est || B > c.ebcap || want > c.ecap || give_back) {
        const size_t nb = (want == c.ecap && c.d_est) ? std::max<size_t>({B, 1024, c.ebcap}) : std::max<size_t>(B, 1024);
        want = std::max(emit_cap(B), std::min(want, emit_cap_max(nb)));
        for (void** p : {(void**)&c.d_est, (void**)&c.d_esc})
            if (*p) { hipFree(*p); *p = nullptr; }
        c.ebcap = 0;
        c.ecap = 0;
        if (!dev_alloc(&c.d_est, nb * want) || !dev_alloc(&c.d_esc, nb * want)) return false;
        c.ecap = want;
        c.ebcap = nb;
    }
    if (bytes > c.qcap) {
        for (void** p : {(void**)&c.d_raw, (void**)&c.d_norm})
            if (*p) { hipFree(*p); *p = nullptr; }
        size_t nb = std::max<size_t>(bytes, 1 << 16);
        if (!dev_alloc(&c.d_raw, nb) || !dev_alloc(&c.d_norm, nb)) return false;
        c.qcap = nb;
    }
    return true;
}

// The survivor arena of a context (SearchParams.at): kArenaInit blocks of kArenaBlock entries to
// start with (a C3 query has ~35 survivors, so only outliers ever use it), after a call that ran out
// 5/4 of the blocks it would have needed (each query it ran out for estimates its own need from the
// share of its postings counted), at least 3/2 as many, within
// kArenaBudget bytes. A query's first-block word per row of the batch.
constexpr uint32_t kArenaInit = 1024;                // 1M survivors, 5 MB
constexpr uint64_t kArenaBudget = 4ull << 30;
bool ensure_arena(Context& c, size_t B) {
    static const uint32_t init = [] {  // NGS_ARENA_INIT (tests): a smaller first arena
        const char* e = std::getenv("NGS_ARENA_INIT");
        return e ? std::max<uint32_t>(1, (uint32_t)std::strtoul(e, nullptr, 0)) : kArenaInit;
    }();
    if (!c.d_eovf || B > c.eorows) {  // the first-block words (also the heavy slices' words): required
        if (c.d_eovf) { hipFree(c.d_eovf); c.d_eovf = nullptr; }
        const size_t nb = std::max<size_t>(B, 1024);
        if (!dev_alloc(&c.d_eovf, nb)) return false;
        c.eorows = nb;
    }
    auto free_arena = [&c] {
        for (void** p : {(void**)&c.d_anext, (void**)&c.d_at, (void**)&c.d_ac})
            if (*p) { hipFree(*p); *p = nullptr; }
        c.ablocks = 0;
    };
    if (c.arena_shrink_to && c.arena_shrink_to < c.ablocks) {  // a grown arena left unused (finish_search)
        free_arena();
        c.arena_grow = c.arena_shrink_to;
    }
    c.arena_shrink_to = 0;
    // The arena is optional: the kernels run without one (SearchParams.at null; a query past its slots
    // goes to tier 1b). An allocation that fails leaves the call without it, drops the grown size and
    // waits kCalmCalls calls before trying again, so one out-of-memory event does not fail every later
    // call of the context.
    if (c.arena_off) {
        --c.arena_off;
        return true;
    }
    const uint32_t want = std::max<uint32_t>({init, c.ablocks, c.arena_grow});
    if (!c.d_at || want > c.ablocks) {
        free_arena();
        // plain hipMalloc, not dev_alloc: a refused arena is not an error of the call
        if (hipMalloc((void**)&c.d_anext, (size_t)want * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void**)&c.d_at, (size_t)want * kArenaBlock * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void**)&c.d_ac, (size_t)want * kArenaBlock) != hipSuccess) {
            (void)hipGetLastError();
            free_arena();
            c.arena_grow = 0;
            c.arena_off = kCalmCalls;
            return true;
        }
        c.ablocks = want;
    }
    return true;
}

// Sliced tier 1b's partial results: B * slices * limit records. Within kPartBudget bytes, else the
// call runs tier 1b unsliced (returns the slice count to use).
uint32_t ensure_parts(Context& c, size_t B, uint32_t limit, uint32_t slices) {
    if (slices <= 1 || limit > kWaveMaxLimit) return 1;
    const size_t need = B * slices * limit;
    if (need * sizeof(uint64_t) > kPartBudget) return 1;
    if (need > c.pcap) {
        if (c.d_prec) hipFree(c.d_prec);
        c.d_prec = nullptr;
        c.pcap = 0;
        const size_t nb = std::max<size_t>(need, 1 << 16);
        if (!dev_alloc(&c.d_prec, nb)) return 1;
        c.pcap = nb;
    }
    if (B * slices > c.pncap) {
        if (c.d_pcnt) hipFree(c.d_pcnt);
        c.d_pcnt = nullptr;
        c.pncap = 0;
        const size_t nb = std::max<size_t>(B * slices, 4096);
        if (!dev_alloc(&c.d_pcnt, nb)) return 1;
        c.pncap = nb;
    }
    return slices;
}

bool ensure_outputs(Context& c, size_t B, size_t stride) {
    const size_t need = B * stride;
    if (!c.d_out || B > c.ncap || need > c.ocap) {
        for (void** p : {(void**)&c.d_out, (void**)&c.d_pos, (void**)&c.d_pk, (void**)&c.d_ps, &c.d_ptemp})
            if (*p) { hipFree(*p); *p = nullptr; }
        c.d_n = c.d_k = nullptr;
        c.d_s = nullptr;
        const size_t nb = std::max(B, c.ncap), ob = std::max(need, c.ocap);
        if (!dev_alloc(&c.d_out, nb + 1 + 2 * ob) || !dev_alloc(&c.d_pos, nb + 1) || !dev_alloc(&c.d_pk, 2 * ob) ||
            !dev_alloc(&c.d_ps, ob))
            return false;
        c.ptemp_bytes = pack_temp_bytes((uint32_t)nb);
        if (!HIP_CHECK(hipMalloc(&c.d_ptemp, std::max<size_t>(c.ptemp_bytes, 1)))) return false;
        c.ncap = nb;
        c.ocap = ob;
    }
    // this call's views: [n (B + 1) | k (B * stride) | s (B * stride)] from the block's start
    c.d_n = c.d_out;
    c.d_k = c.d_out + B + 1;
    c.d_s = reinterpret_cast<float*>(c.d_k + need);
    return true;
}

// The U8 batch's staging on the device: its UTF-8 bytes, its B + 1 byte offsets and the
// decoder's scratch. (Replaced only between calls: the context's stream is idle then.)
bool ensure_u8(Context& c, size_t B, size_t bytes) {
    if (bytes > c.u8cap || !c.d_u8) {
        if (c.d_u8) hipFree(c.d_u8);
        c.d_u8 = nullptr;
        c.u8cap = 0;
        const size_t nb = std::max<size_t>(bytes, 1 << 16);
        if (!dev_alloc(&c.d_u8, nb)) return false;
        c.u8cap = nb;
    }
    if (B > c.u8ncap || !c.d_u8off) {
        if (c.d_u8off) hipFree(c.d_u8off);
        if (c.d_u8temp) hipFree(c.d_u8temp);
        c.d_u8off = nullptr;
        c.d_u8temp = nullptr;
        c.u8ncap = 0;
        const size_t nb = std::max<size_t>(B, 1024);
        c.u8temp_bytes = utf8_temp_bytes((uint32_t)nb);
        if (!dev_alloc(&c.d_u8off, nb + 1) || !HIP_CHECK(hipMalloc(&c.d_u8temp, c.u8temp_bytes))) return false;
        c.u8ncap = nb;
    }
    return true;
}

bool ensure_general(const Replica& R, Context& c, hipStream_t s) {
    if (c.gen.G) return true;
    const DevIndex& X = R.dev;
    const uint64_t n_long = X.n_terms - X.n_short;
    const uint64_t kst = gen_kstride(X.n_keys);
    const uint64_t per = n_long * 4 + kst * 4 + (uint64_t)X.n_keys * 8 + 64;
    uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kGeneralMaxGroup, kGeneralBudget / per));
    if ((uint64_t)G * std::max<uint64_t>(kst, 1) > (uint64_t)kInt32Max) G = 1;
    GeneralBuffers& W = c.gen;
    if (!dev_alloc(&W.cnt, (size_t)G * n_long) || !dev_alloc(&W.kenc, (size_t)G * kst) ||
        !dev_alloc(&W.list, (size_t)G * X.n_keys) || !dev_alloc(&W.sorted, X.n_keys) || !dev_alloc(&W.lcount, G))
        return false;
    W.temp_bytes = general_sort_temp_bytes(X.n_keys);
    if (!HIP_CHECK(hipMalloc(&W.temp, std::max<size_t>(W.temp_bytes, 1)))) return false;
    // on the call's stream: a plain hipMemset runs on the null stream, which the context's
    // non-blocking streams do not wait for (the first group's counts raced with it)
    if (!HIP_CHECK(hipMemsetAsync(W.cnt, 0, sizeof(uint32_t) * std::max<size_t>((size_t)G * n_long, 1), s)) ||
        !HIP_CHECK(hipMemsetAsync(W.kenc, 0, sizeof(uint32_t) * std::max<size_t>((size_t)G * kst, 1), s)))
        return false;
    W.G = G;
    return true;
}

// The search pipeline over B queries already in device memory, in two halves: queue_search
// queues the normalisation, the tier kernels and the read-back of the statistics and path
// counts; finish_search waits for them, runs the general path for the queries listed for it
// and records the statistics. small: one kernel per tier on the call's stream (no routing
// lists, no side streams; the latency path of score() and small batches).
int queue_search(Library& L, Replica& R, Context& c, const uint8_t* d_raw, const uint64_t* d_off, uint32_t B,
                 uint64_t qbytes, float thr, uint32_t limit, uint32_t stride, uint32_t* d_n, uint32_t* d_k,
                 float* d_s, hipStream_t s, SearchParams& P, bool small) {
    // small: the statistics go to the latency block (zeroed by k_prep, read back by the caller
    // together with the results)
    DevStats* sd = small ? reinterpret_cast<DevStats*>(c.d_sio) : c.d_stats;
    PathCounts* pc = &reinterpret_cast<StatsBlock*>(sd)->paths;
    std::memset(&P, 0, sizeof(P));  // (padding too: the bytes are a replay signature, Context::gsig)
    P.thr = thr;
    P.limit = limit;
    P.out_stride = stride;
    P.n_queries = B;
    static const uint32_t dbg = [] {
        const char* e = std::getenv("NGS_DEBUG");
        return e ? (uint32_t)std::strtoul(e, nullptr, 0) : 0u;
    }();
    P.dbg = dbg;
    static const uint32_t hslices = [] {  // NGS_HEAVY_SLICES: term-id slices per heavy query (0: auto)
        const char* e = std::getenv("NGS_HEAVY_SLICES");
        return e ? std::min<uint32_t>((uint32_t)std::strtoul(e, nullptr, 0), kHeavyMaxSlices) : 0u;
    }();
    P.hslices = hslices;
    P.hbase = 0;
    P.hgrid = c.heavy_items ? c.heavy_items + c.heavy_items / 8 + 64 : 0u;  // (a margin: batches change)
    // tier 1: the lean kernel with tier 1b on its hand-overs (batches), or tier 1b alone (the latency path)
    P.waves = small ? 1u : 0u;
    {
        std::lock_guard<std::mutex> g(L.valid_mu);
        std::memcpy(P.valid, L.valid, sizeof(P.valid));
    }
    if (!ensure_queries(c, B, qbytes)) return -4;
    P.esn = c.d_esn;
    P.est = c.d_est;
    P.esc = c.d_esc;
    P.ecap = c.ecap;
    if (!small) {  // (the latency path runs tier 1b alone: no tier-1a survivors)
        if (!ensure_arena(c, B)) return -4;
        P.eovf = c.d_eovf;
        P.anext = c.ablocks ? c.d_anext : nullptr;
        P.at = c.ablocks ? c.d_at : nullptr;  // null: no arena this call (ensure_arena)
        P.ac = c.ablocks ? c.d_ac : nullptr;
        P.ablocks = c.ablocks;
        P.actr = &pc->arena_used;
    }
    constexpr uint32_t list_slices = kSlices;        // term-id slices of the hand-over / full lists' tier 1b
    constexpr uint32_t small_slices = kSmallSlices;  // ... and of every query of the latency path
    if (small) {
        // one query's postings over several CUs: a wave per (query, slice of at least 8 skip
        // buckets), then k_merge; a small library stays on one wave per query
        const uint32_t sl = std::min<uint32_t>(small_slices, R.dev.n_buckets / 8);
        P.nslices = sl > 1 ? ensure_parts(c, B, P.limit, sl) : 1u;
        if (P.nslices > 1) P.waves = 1;
    } else {
        P.nslices = ensure_parts(c, B, P.limit, list_slices);
    }
    P.qcap = c.qcap;
    P.oflow = &pc->oflow;
    if (small) {
        P.zero_stats = reinterpret_cast<uint32_t*>(sd);
        // the slots this batch's queries add to (q & (kStatSlots - 1), errors in slot 0) and those the
        // context's last small batch added to (a batch of 3 after one of 14 summed the other 11's
        // slots into its own statistics); the others stay zero from the block's allocation
        const uint32_t mine = (uint32_t)std::min<size_t>(B, kStatSlots);
        P.zero_words = (uint32_t)(std::max(mine, c.sio_slots) * sizeof(DevStats) / sizeof(uint32_t));
        c.sio_slots = mine;
    }
    P.prec = c.d_prec;
    P.pcnt = c.d_pcnt;
    const bool timing = L.timing.load();
    // A small batch whose queries are all on the heavy list (C2: 4,096 queries at threshold 0) is a
    // few waves per CU of long per-query chains, so throughput comes from batches in flight, not from
    // the main and side streams
    // of one call overlapping: its side work goes on the call's own stream, in order, and a context
    // that only ever runs such batches never makes its side streams. Three pipelined calls then hold
    // three hardware queues (HIP maps streams to its four queues round-robin as they are made) instead
    // of six streams sharing four (C2 28.6 -> 34.8 Mq/s at three in flight)
    constexpr uint32_t one_stream_batch = kOneStreamBatch;
    // (only where every lean query is on the heavy list, cmin <= kHeavyCmin for any gram count up to
    // kWaveMaxGrams, as at threshold 0: with a mix, the heavy chain on its own stream overlaps the
    // main launch, and in order after it a call of 8,192 C3-like queries took 0.23 ms longer)
    const bool all_heavy = !((float)kHeavyCmin / (float)kWaveMaxGrams < thr);
    hipStream_t side = s, side2 = s;
    // one side stream for all of the replica's contexts: two calls in flight then hold three streams
    // beside the null stream, one per hardware queue at HIP's default of four; with a side stream per
    // context, one context's main and side streams shared a queue and its tail waited behind its own
    // heavy chain (C3 +1.0 %, six passes on two boxes; profiles/r05_s27_ab_hw_queues.txt)
    if (B > one_stream_batch || !all_heavy) {
        if (!c.side) {
            std::lock_guard<std::mutex> g(R.main_mu);
            if (!R.shared_side && !HIP_CHECK(make_side_stream(&R.shared_side))) return -4;
            c.side = c.side2 = R.shared_side;
            c.side_shared = true;
        }
        side = c.side;
        side2 = c.side2;
    }
    // statistics, path counts and list counters: reset by k_prep and k_lists when the context's last
    // call left them so (the memset's fill kernel waited ~200 us for a workgroup slot behind the
    // previous call's tail in the pipelined trace)
    const bool zero_in_prep = !small && c.stats_clean && P.waves == 0;
    c.stats_clean = false;
    if (zero_in_prep) {
        P.zero_stats = reinterpret_cast<uint32_t*>(c.d_stats);
        P.zero_words = (uint32_t)(kStatSlots * sizeof(DevStats) / sizeof(uint32_t));
    }
    DevIndex X;
    if (!R.index_for(P.valid, X)) return -4;
    // A one-stream call (side == s: batches up to kOneStreamBatch queries that are all heavy, C2) is
    // ~0.1 ms of GPU work for ~12 queued operations, 50 us of host time per call. When a call's
    // launch arguments repeat an earlier call of the context (a server's or a bench's batches into
    // the same buffers), the sequence is built as a graph on the second occurrence and replayed
    // from then on (one submission: ~4 us of host time for 10 launches against ~30,
    // tools/ubench/graph_launch.hip). Such calls leave the replica's main-launch order alone
    // (main_ev): their main launch only routes, every lean query being on the heavy list.
    static const bool no_graphs = std::getenv("NGS_SYNC_DEBUG") != nullptr;
    bool capture = false;
    std::vector<uint8_t> sig;
    // (not on the null stream)
    if (!small && side == s && s && !timing && !no_graphs && !c.gfail) {
        auto put = [&](const void* p, size_t n) {
            sig.insert(sig.end(), static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + n);
        };
        const void* ptrs[] = {d_raw, d_off, d_n, d_k, d_s, s, c.d_norm, c.d_qm, c.d_list2, c.d_fb, c.d_fb2,
                              c.d_heavy, c.d_full, c.d_glist, c.d_lslots, c.d_lctr, c.d_stats, c.h_stats};
        put(ptrs, sizeof(ptrs));
        put(&X, sizeof(X));
        put(&P, sizeof(P));
        const uint32_t flags[] = {B, all_heavy ? 1u : 0u, zero_in_prep ? 1u : 0u};
        put(flags, sizeof(flags));
        for (auto& g : c.graphs) {
            if (g.first != sig) continue;
            if (!HIP_CHECK(hipGraphLaunch(g.second, s))) return -4;
            c.stats_clean = true;
            g_host_phase[kHpReplays].fetch_add(1, std::memory_order_relaxed);
            return 0;
        }
        capture = std::find(c.gseen.begin(), c.gseen.end(), sig) != c.gseen.end();
        if (!capture) {
            if (c.gseen.size() >= Context::kGraphs) c.gseen.erase(c.gseen.begin());
            c.gseen.push_back(sig);
        }
    }
    // the call's operations, queued on s, or with gb appended to a graph being built (one-stream calls)
    auto queue_ops = [&](GraphBuild* gb) -> bool {
        const size_t stat_bytes = sizeof(StatsBlock) + sizeof(DevStats) * 2 * kListSlots;
        if (!zero_in_prep && !small) {
            if (gb) {
                hipMemsetParams mp{};
                mp.dst = c.d_stats;
                mp.value = 0;
                mp.elementSize = 4;
                mp.width = stat_bytes / 4;
                mp.height = 1;
                if (!HIP_CHECK(hipGraphAddMemsetNode(&gb->last, gb->graph, nullptr, 0, &mp))) return false;
            } else if (!HIP_CHECK(hipMemsetAsync(c.d_stats, 0, stat_bytes, s))) {
                return false;
            }
        }
        if (timing) HIP_CHECK(hipEventRecord(c.ev[0], s));
        if (!HIP_CHECK(launch_prep(d_raw, d_off, B, P, c.d_norm, c.d_qm, X.csize, X, c.d_heavy, &pc->heavy, c.d_full,
                                   &pc->full, c.d_lslots, c.d_lctr, s, side, c.prep_ev, c.lists_ev, gb)))
            return false;
        if (timing) HIP_CHECK(hipEventRecord(c.ev[1], s));  // the end of k_prep is the start of the tier-1 phase
        // the main tier-1a launches of this replica's calls one after another: with two calls in flight
        // the second call's main launch otherwise starts in the first one's and the two share the GPU
        // (C3, one box, three passes each: 31.3-31.6 against 30.1-30.6 Mq/s,
        // profiles/r05_s15_ab_serial_main.txt; C5 the same)
        std::unique_lock<std::mutex> g(R.main_mu, std::defer_lock);
        hipEvent_t mev = nullptr;
        bool mwait = false;
        if (!small && !gb) {
            g.lock();
            if (!R.main_ev && !HIP_CHECK(hipEventCreateWithFlags(&R.main_ev, hipEventDisableTiming))) return false;
            mev = R.main_ev;
            mwait = R.main_rec;
            R.main_rec = true;
        }
        if (!HIP_CHECK(launch_fast(X, P, c.d_norm, d_off, c.d_qm, d_n, d_k, d_s, c.d_list2, &pc->tier2, c.d_fb,
                                   &pc->handover, c.d_fb2, &pc->heavy_handover, c.d_heavy, &pc->heavy, c.d_full, &pc->full,
                                   c.d_glist, pc, sd, s, side, side2, c.join, c.join2, c.lists_ev, all_heavy, mev,
                                   mwait, gb)))
            return false;
        if (timing) HIP_CHECK(hipEventRecord(c.ev[3], s));
        // the statistics and the path counts in one read-back (the general path adds no statistics)
        if (small) return true;
        if (gb) {
            hipGraphNode_t n = nullptr;
            if (!HIP_CHECK(hipGraphAddMemcpyNode1D(&n, gb->graph, gb->last ? &gb->last : nullptr, gb->last ? 1 : 0,
                                                   c.h_stats, c.d_stats, kSioStats, hipMemcpyDeviceToHost)))
                return false;
            gb->last = n;
            return true;
        }
        return HIP_CHECK(hipMemcpyAsync(c.h_stats, c.d_stats, kSioStats, hipMemcpyDeviceToHost, s));
    };
    // A graph is built node by node (no stream capture, which in this runtime fails other threads'
    // launches while it is open: the threaded test's scoreBatch calls did) and instantiated
    if (capture) {
        GraphBuild gb;
        hipGraphExec_t exec = nullptr;
        bool made = HIP_CHECK(hipGraphCreate(&gb.graph, 0)) && queue_ops(&gb) &&
                    HIP_CHECK(hipGraphInstantiate(&exec, gb.graph, nullptr, nullptr, 0));
        if (gb.graph) hipGraphDestroy(gb.graph);
        (void)hipGetLastError();
        if (made) {
            c.gseen.erase(std::find(c.gseen.begin(), c.gseen.end(), sig));
            if (c.graphs.size() >= Context::kGraphs) {
                hipGraphExecDestroy(c.graphs.front().second);
                c.graphs.erase(c.graphs.begin());
            }
            c.graphs.emplace_back(std::move(sig), exec);
            if (!HIP_CHECK(hipGraphLaunch(exec, s))) return -4;
        } else {  // nothing of the call ran: queue it one by one, and so from now on
            if (exec) hipGraphExecDestroy(exec);
            c.gfail = true;
            if (!queue_ops(nullptr)) return -4;
        }
    } else if (!queue_ops(nullptr)) {
        return -4;
    }
    c.stats_clean = !small && P.waves == 0;  // k_lists queued: it leaves the list counters zero
    return 0;
}

int finish_search(Library& L, Replica& R, Context& c, uint32_t B, const SearchParams& P, const uint64_t* d_off,
                  uint32_t* d_n, uint32_t* d_k, float* d_s, hipStream_t s, bool small = false) {
    if (!HIP_CHECK(hipStreamSynchronize(s))) return -4;
    const DevStats* hst = small ? reinterpret_cast<const DevStats*>(c.h_sio) : c.h_stats;
    const bool timing = L.timing.load();
    ngs_stats st{};
    st.queries = B;
    const PathCounts& pc = reinterpret_cast<const StatsBlock*>(hst)->paths;
    if (pc.oflow) {  // (the rerun resets the path counts with the memset)
        c.stats_clean = false;
        return kRetryQcap;
    }  // a query past the normalised-query buffer: nothing is valid
    const uint32_t ngen = pc.general;
    if (ngen) {
        std::vector<uint32_t> gl(ngen);
        if (!HIP_CHECK(hipMemcpyAsync(gl.data(), c.d_glist, sizeof(uint32_t) * ngen, hipMemcpyDeviceToHost, s)) ||
            !HIP_CHECK(hipStreamSynchronize(s)))
            return -4;
        std::sort(gl.begin(), gl.end());
        if (!ensure_general(R, c, s)) return -4;
        DevIndex X;
        if (!R.index_for(P.valid, X)) return -4;
        if (timing) HIP_CHECK(hipEventRecord(c.ev[4], s));
        for (uint32_t g0 = 0; g0 < ngen; g0 += c.gen.G) {
            const uint32_t G = std::min(c.gen.G, ngen - g0);
            if (!HIP_CHECK(hipMemcpyAsync(c.d_group, gl.data() + g0, sizeof(uint32_t) * G, hipMemcpyHostToDevice, s)))
                return -4;
            if (!HIP_CHECK(run_general(X, P, c.d_norm, d_off, c.d_qm, c.d_group, gl.data() + g0, G, c.gen, d_n,
                                       d_k, d_s, s)))
                return -4;
        }
        if (timing) HIP_CHECK(hipEventRecord(c.ev[5], s));
        // the last group's k_gen_write still reads c.gen: complete before the context goes back
        // to the pool (and before the call returns, as the ABI promises)
        if (!HIP_CHECK(hipStreamSynchronize(s))) return -4;
    }
    DevStats ds{};
    uint64_t slot_full = 0;
    for (uint32_t i = 0; i < kStatSlots; ++i) {
        const DevStats& x = hst[i];
        ds.postings += x.postings;
        ds.lists += x.lists;
        ds.results += x.results;
        ds.fast += x.fast;
        ds.survivors += x.survivors;
        ds.main_postings += x.main_postings;
        ds.main_lists += x.main_lists;
        ds.errors |= x.errors;
        slot_full += x.slot_full;
    }
    // queries that filled their survivor slots ran again in tier 1b: when that is more than 1/64
    // of the batch, this context's later calls get twice the slots (bounded by emit_cap_max);
    // after kCalmCalls calls in a row that filled none of grown slots, half of them go back
    // the arena's block counter: past its blocks, the arena ran out (those queries went to tier 1b and
    // count as slot_full): later calls get a larger arena, not more slots per query
    // (the queries it ran out for add the blocks they would still need, the next word: the next
    // call's arena is 5/4 of the estimated need, at least 3/2 of this one)
    if (!small) c.heavy_items = pc.heavy * heavy_slices(P, pc.heavy, R.dev);  // the next call's heavy grid
    const uint32_t arena_used = small ? 0u : pc.arena_used;
    const bool arena_out = !small && P.at && arena_used > P.ablocks;
    if (arena_out) {
        const uint64_t need = (uint64_t)P.ablocks + pc.arena_need;
        const uint64_t want = std::max<uint64_t>(3ull * P.ablocks / 2, 5ull * need / 4);
        const uint64_t cap = kArenaBudget / ((uint64_t)kArenaBlock * (sizeof(uint32_t) + sizeof(uint8_t)));
        c.arena_grow = (uint32_t)std::min<uint64_t>(want, cap);
        c.arena_calm = 0;
    } else if (!small && P.at && P.ablocks > kArenaInit && (uint64_t)arena_used * 4 < P.ablocks) {
        // a grown arena mostly unused for kCalmCalls calls in a row: halved (as the survivor slots)
        if (++c.arena_calm >= kCalmCalls) {
            c.arena_calm = 0;
            c.arena_shrink_to = std::max<uint32_t>(kArenaInit, P.ablocks / 2);
        }
    } else if (!small) {
        c.arena_calm = 0;
    }
    if (!small && !arena_out) {
        if (slot_full * 64 > B) {
            c.calm = 0;
            if (c.ecap < emit_cap_max(B)) c.ecap_grow = std::max(c.ecap_grow, c.ecap * 2);
        } else if (slot_full == 0 && c.ecap > emit_cap(B) && ++c.calm >= kCalmCalls) {
            c.calm = 0;
            c.ecap_grow = c.ecap / 2 > emit_cap(B) ? c.ecap / 2 : 0u;
            c.shrink = true;
        }
    }
    if (ds.errors) {
        std::fprintf(stderr, "ngram_search: fused kernel reported internal error 0x%x\n", ds.errors);
        t_last_error = kErrInternal;
        return -5;
    }
    if (timing) {
        float ms = 0;
        st.fast_queries = ds.fast;
        st.general_queries = ngen;
        st.tier2_queries = pc.tier2;
        // queries tier 1b ran: hand-overs of both lean launches and the full list
        st.handover_queries = pc.handover + pc.heavy_handover + pc.full;
        st.heavy_queries = pc.heavy;
        st.full_queries = pc.full;
        st.slot_full_queries = slot_full;
        st.survivor_slots = P.ecap;
        st.survivor_slot_bytes = ((uint64_t)c.ebcap * c.ecap + (uint64_t)c.ablocks * kArenaBlock) *
                                 (sizeof(uint32_t) + sizeof(uint8_t));
        st.arena_blocks = small ? 0u : P.ablocks;
        st.arena_used = arena_used;
        st.postings = ds.postings;
        st.lists = ds.lists;
        st.results = ds.results;
        st.survivors = ds.survivors;
        st.main_postings = ds.main_postings;
        st.main_lists = ds.main_lists;
        if (hipEventElapsedTime(&ms, c.ev[0], c.ev[1]) == hipSuccess) st.prep_kernel_ms = ms;
        if (hipEventElapsedTime(&ms, c.ev[1], c.ev[3]) == hipSuccess) st.fast_kernel_ms = ms;
        if (ngen && hipEventElapsedTime(&ms, c.ev[4], c.ev[5]) == hipSuccess) st.general_ms = ms;
        std::lock_guard<std::mutex> g(L.stats_mu);
        L.last = st;
    }
    return 0;
}

int device_search(Library& L, Replica& R, Context& c, const uint8_t* d_raw, const uint64_t* d_off, uint32_t B,
                  uint64_t qbytes, float thr, uint32_t limit, uint32_t stride, uint32_t* d_n, uint32_t* d_k,
                  float* d_s, hipStream_t s) {
    if (!B) return 0;
    SearchParams P;
    const int rc = queue_search(L, R, c, d_raw, d_off, B, qbytes, thr, limit, stride, d_n, d_k, d_s, s, P, false);
    return rc ? rc : finish_search(L, R, c, B, P, d_off, d_n, d_k, d_s, s);
}

uint32_t effective_limit(const Library& L, uint32_t limit) {
    if (limit == 0) limit = kInt32Max;  // nGramSearch.hpp:420-421
    return std::min<uint32_t>(limit, L.host.n_keys);
}

template <typename CharT>
size_t str_len(const CharT* p) {
    size_t n = 0;
    while (p[n]) ++n;
    return n;
}

// One chunk of a host batch in flight on a context (host_search_one).
struct HostChunk {
    Context* c = nullptr;
    uint32_t q0 = 0, B = 0;
    bool small = false;
    size_t block = 0;
    SearchParams P{};
    const uint8_t* d_raw = nullptr;
    const uint64_t* d_off = nullptr;
    uint32_t *d_n = nullptr, *d_k = nullptr;
    float* d_s = nullptr;
    // pointer mode (pcs != 0): records go out as result pointers pbase + key_off[key] * pcs
    uint64_t pbase = 0;
    uint32_t pcs = 0;
    // ... through these key offsets (the index's own, or the UTF-8 key table's)
    const uint64_t* d_koff = nullptr;
    const uint64_t* h_koff = nullptr;
};

// Queues chunk [q0, q0 + B) on context c: the queries packed into pinned staging, one H2D copy
// (two for large chunks), the search kernels. Nothing waits.
// u8 (CharT = char on a wide index): the queries are UTF-8; their bytes and byte offsets are
// copied in as they are and decoded on the call's stream into the context's query buffer
// (launch_utf8_decode), which the pipeline then reads like a W batch. Result pointers go into the
// UTF-8 key table.
template <typename CharT>
bool queue_host_chunk(Library& L, Replica& R, Context& c, const CharT* const* queries, uint32_t q0, uint32_t B,
                      float thr, uint32_t Lm, HostChunk& h, uint64_t pbase, const Library::U8Keys* u8,
                      size_t replica) {
    constexpr size_t cs = sizeof(CharT);
    const size_t stride = Lm;
    h = HostChunk{};
    h.pbase = pbase;
    h.pcs = pbase ? (uint32_t)cs : 0u;
    h.d_koff = u8 ? u8->d_off[replica] : R.dev.key_off;
    h.h_koff = u8 ? u8->off.data() : L.host.key_off.data();
    h.c = &c;
    h.q0 = q0;
    h.B = B;
    HostTimer ht;
    // query offsets into pinned staging: lengths on up to 8 threads, one prefix pass
    if (!c.h_off.grow(sizeof(uint64_t) * (B + 1))) return false;
    uint64_t* ho = c.h_off.as<uint64_t>();
    ho[0] = 0;
    parallel_ranges(B, 8192, [&](size_t a, size_t e) {
        for (size_t i = a; i < e; ++i) ho[i + 1] = queries[q0 + i] ? str_len(queries[q0 + i]) * cs : 0;
    });
    for (uint32_t i = 0; i < B; ++i) ho[i + 1] += ho[i];
    const uint64_t qbytes = ho[B];
    // small batches (score()'s latency path): one kernel per tier on one stream, the queries
    // in with one copy and the statistics with the whole output block out with one copy,
    // all through the context's latency block [statistics | results | offsets, bytes]
    h.block = sizeof(uint32_t) * (B + 1 + 2 * (size_t)B * stride);
    const size_t qspace = sizeof(uint64_t) * (B + 1) + qbytes;
    h.small = !u8 && B <= kSmallBatch && h.block <= kSmallBlock && qspace <= kSmallQ;
    uint64_t sbytes = qbytes;  // bytes of the batch as the pipeline reads it
    bool ok;
    if (h.small) {
        uint8_t* hq = c.h_sio + kSioStats + kSmallBlock;
        std::memcpy(hq, ho, sizeof(uint64_t) * (B + 1));
        for (uint32_t i = 0; i < B; ++i)
            if (queries[q0 + i])
                std::memcpy(hq + sizeof(uint64_t) * (B + 1) + ho[i], queries[q0 + i], ho[i + 1] - ho[i]);
        uint8_t* dq = c.d_sio + kSioStats + kSmallBlock;
        h.d_off = reinterpret_cast<const uint64_t*>(dq);
        h.d_raw = dq + sizeof(uint64_t) * (B + 1);
        h.d_n = reinterpret_cast<uint32_t*>(c.d_sio + kSioStats);
        h.d_k = h.d_n + B + 1;
        h.d_s = reinterpret_cast<float*>(h.d_k + (size_t)B * stride);
        ok = HIP_CHECK(hipMemcpyAsync(dq, hq, qspace, hipMemcpyHostToDevice, c.stream));
    } else {
        if (!c.h_raw.grow(std::max<uint64_t>(qbytes, 1))) return false;
        uint8_t* hr = c.h_raw.as<uint8_t>();
        parallel_ranges(B, 8192, [&](size_t a, size_t e) {
            for (size_t i = a; i < e; ++i)
                if (queries[q0 + i]) std::memcpy(hr + ho[i], queries[q0 + i], ho[i + 1] - ho[i]);
        });
        ht.mark(kHpPack, "pack queries");
        if (u8) {
            // at most one unit per byte: 4 x bytes always holds the decoded batch (k_prep's *oflow
            // still guards the buffer)
            sbytes = 4 * qbytes;
            ok = ensure_queries(c, B, sbytes) && ensure_outputs(c, B, stride) && ensure_u8(c, B, qbytes) &&
                 HIP_CHECK(hipMemcpyAsync(c.d_u8, c.h_raw.p, qbytes, hipMemcpyHostToDevice, c.stream)) &&
                 HIP_CHECK(hipMemcpyAsync(c.d_u8off, ho, sizeof(uint64_t) * (B + 1), hipMemcpyHostToDevice, c.stream)) &&
                 HIP_CHECK(launch_utf8_decode(c.d_u8, c.d_u8off, B, reinterpret_cast<uint32_t*>(c.d_raw), c.qcap / 4,
                                              c.d_off, c.d_u8temp, c.u8temp_bytes, c.stream));
        } else {
            ok = ensure_queries(c, B, qbytes) && ensure_outputs(c, B, stride) &&
                 HIP_CHECK(hipMemcpyAsync(c.d_raw, c.h_raw.p, qbytes, hipMemcpyHostToDevice, c.stream)) &&
                 HIP_CHECK(hipMemcpyAsync(c.d_off, ho, sizeof(uint64_t) * (B + 1), hipMemcpyHostToDevice, c.stream));
        }
        h.d_raw = c.d_raw;
        h.d_off = c.d_off;
        h.d_n = c.d_n;
        h.d_k = c.d_k;
        h.d_s = c.d_s;
    }
    if (!ok) return false;
    if (queue_search(L, R, c, h.d_raw, h.d_off, B, sbytes, thr, Lm, (uint32_t)stride, h.d_n, h.d_k, h.d_s, c.stream,
                     h.P, h.small) != 0)
        return false;
    ht.mark(kHpQueue, "copy in + queue kernels");
    return !h.small || HIP_CHECK(hipMemcpyAsync(c.h_sio, c.d_sio, kSioStats + h.block, hipMemcpyDeviceToHost, c.stream));
}

// Completes a queued chunk: waits, runs the general path, reads back exactly the results
// (packed on the device for large chunks), fills the chunk's counts and hands its records to
// `emit(recs, scores, n, last, chunk_total)` (in pieces of the chunk's chunk_total records, in order):
// recs are u32 key ranks, or in pointer mode (h.pcs) u64 result
// pointers.
template <class Emit>
bool finish_host_chunk(Library& L, Replica& R, HostChunk& h, uint32_t Lm, std::vector<uint32_t>& counts, bool last,
                       Emit&& emit) {
    Context& c = *h.c;
    const uint32_t B = h.B, q0 = h.q0;
    const size_t stride = Lm;
    HostTimer ht;
    const int frc = finish_search(L, R, c, B, h.P, h.d_off, h.d_n, h.d_k, h.d_s, c.stream, h.small);
    if (frc == kRetryQcap) t_last_error = kErrQueryBuffer;  // cannot happen: the host path sizes the buffer
    if (frc != 0) return false;
    ht.mark(kHpWait, "wait for kernels");
    if (h.small) {
        // the general path ran after the read-back: read the results again
        if (reinterpret_cast<const StatsBlock*>(c.h_sio)->paths.general) {
            if (!HIP_CHECK(hipMemcpyAsync(c.h_sio + kSioStats, c.d_sio + kSioStats, h.block, hipMemcpyDeviceToHost,
                                          c.stream)) ||
                !HIP_CHECK(hipStreamSynchronize(c.stream)))
                return false;
        }
        const uint32_t* hn = reinterpret_cast<const uint32_t*>(c.h_sio + kSioStats);
        const uint32_t* hk = hn + B + 1;
        const float* hs = reinterpret_cast<const float*>(hk + (size_t)B * stride);
        std::vector<uint32_t> k;
        std::vector<float> sc;
        for (uint32_t i = 0; i < B; ++i) {
            counts[q0 + i] = hn[i];
            k.insert(k.end(), hk + (size_t)i * stride, hk + (size_t)i * stride + hn[i]);
            sc.insert(sc.end(), hs + (size_t)i * stride, hs + (size_t)i * stride + hn[i]);
        }
        if (h.pcs) {  // a few records: their pointers made here
            const uint64_t* koff = h.h_koff;
            std::vector<uint64_t> ptr(k.size());
            for (size_t i = 0; i < k.size(); ++i) ptr[i] = h.pbase + koff[k[i]] * h.pcs;
            emit(static_cast<const void*>(ptr.data()), sc.data(), (uint32_t)k.size(), last, (uint32_t)k.size());
        } else {
            emit(static_cast<const void*>(k.data()), sc.data(), (uint32_t)k.size(), last, (uint32_t)k.size());
        }
        return true;
    }
    // large batches: pack on the device (prefix sum of the counts, one copy per query), read
    // back the offsets, then exactly the packed records
    uint64_t* pp = h.pcs ? reinterpret_cast<uint64_t*>(c.d_pk) : nullptr;
    if (!HIP_CHECK(hipMemsetAsync(c.d_n + B, 0, sizeof(uint32_t), c.stream)) ||
        !HIP_CHECK(launch_pack(c.d_n, c.d_k, c.d_s, B, (uint32_t)stride, c.d_pos, c.d_pk, c.d_ps, c.d_ptemp,
                               c.ptemp_bytes, c.stream, h.d_koff, h.pbase, h.pcs, pp)) ||
        !c.h_res.grow(sizeof(uint32_t) * (B + 1)) ||
        !HIP_CHECK(hipMemcpyAsync(c.h_res.p, c.d_pos, sizeof(uint32_t) * (B + 1), hipMemcpyDeviceToHost, c.stream)) ||
        !HIP_CHECK(hipStreamSynchronize(c.stream)))
        return false;
    ht.mark(kHpPackBack, "pack + offsets back");
    const uint32_t total = c.h_res.as<uint32_t>()[B];
    for (uint32_t i = 0; i < B; ++i) counts[q0 + i] = c.h_res.as<uint32_t>()[i + 1] - c.h_res.as<uint32_t>()[i];
    const size_t esz = h.pcs ? sizeof(uint64_t) : sizeof(uint32_t);
    const size_t rb = esz * (size_t)total;  // record bytes
    if (!c.h_res.grow(rb + sizeof(float) * (size_t)total)) return false;
    // the records come back in pieces, each marshalled (straight from the pinned buffer) while the
    // next ones are still on the link: the copy and the host's copy into the caller's arrays overlap
    const uint32_t pieces = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kBackPieces, total / kBackPieceMin));
    const uint32_t per = (total + pieces - 1) / pieces;
    uint8_t* hr = c.h_res.as<uint8_t>();
    for (uint32_t i = 0; i < pieces; ++i) {
        const size_t a = (size_t)i * per, n = std::min<size_t>(per, total - std::min<size_t>(total, a));
        hipStream_t sp = c.stream;  // (pieces alternating over two streams measured slower: 0.47-0.62 ms)
        if (n && !(HIP_CHECK(hipMemcpyAsync(hr + a * esz, reinterpret_cast<const uint8_t*>(c.d_pk) + a * esz, n * esz,
                                            hipMemcpyDeviceToHost, sp)) &&
                   HIP_CHECK(hipMemcpyAsync(hr + rb + a * sizeof(float), c.d_ps + a, n * sizeof(float),
                                            hipMemcpyDeviceToHost, sp))))
            return false;
        if (!HIP_CHECK(hipEventRecord(c.piece_ev[i], sp))) return false;
    }
    for (uint32_t i = 0; i < pieces; ++i) {
        const size_t a = (size_t)i * per, n = std::min<size_t>(per, total - std::min<size_t>(total, a));
        if (!HIP_CHECK(hipEventSynchronize(c.piece_ev[i]))) {
            (void)hipStreamSynchronize(c.stream);  // nothing may still write the buffer
            return false;
        }
        emit(static_cast<const void*>(hr + a * esz), reinterpret_cast<const float*>(hr + rb) + a, (uint32_t)n, last,
             total);
    }
    ht.mark(kHpRecords, "records back + emit");
    return true;
}

// A large host batch can run as about kPipeChunks chunks (of at least kPipeMinChunk queries) over
// two contexts, one queued ahead, so that chunk k's copies and read-back
// overlap chunk k + 1's kernels. Measured slower than one chunk at C3 (the chunks' read-backs
// waited behind the other chunk's kernels), so one chunk is the default; the batch is still cut
// into chunks where its outputs would exceed kOutBudget / kPartBudget.
constexpr uint32_t kPipeChunks = 1;  // measured: 4 chunks 6.1-6.6 ms against 4.4-4.6 for one at C3
constexpr uint32_t kPipeMinChunk = 8192;

// Queries per chunk of a host batch of nq queries at limit Lm: the outputs within kOutBudget and
// sliced tier 1b's partial results within kPartBudget
size_t host_chunk(uint32_t nq, uint32_t Lm) {
    const size_t stride = std::max<uint32_t>(Lm, 1);
    size_t max_chunk = std::max<size_t>(1, std::min<size_t>(1 << 20, kOutBudget / (stride * 8)));
    if (Lm <= kWaveMaxLimit)  // sliced tier 1b's partial results fit the budget
        max_chunk = std::max<size_t>(1, std::min<size_t>(max_chunk, kPartBudget / (sizeof(uint64_t) * kSlices * stride)));
    const size_t want = std::max<size_t>(kPipeMinChunk, (nq + kPipeChunks - 1) / kPipeChunks);
    return std::min(max_chunk, want);
}

// Scores n queries (characters of the index's width) on one replica; fills counts and hands
// each chunk's records, in query order, to emit(keys, scores, n).
template <typename CharT, class Emit>
bool host_search_chunks(Library& L, Replica& R, const CharT* const* queries, uint32_t nq, float thr, uint32_t Lm,
                        std::vector<uint32_t>& counts, Emit&& emit, uint64_t pbase = 0,
                        const Library::U8Keys* u8 = nullptr, size_t replica = 0) {
    counts.assign(nq, 0);
    if (Lm == 0 || nq == 0) return true;
    if (!HIP_CHECK(hipSetDevice(R.device))) return false;
    const size_t chunk = host_chunk(nq, Lm);
    const uint32_t n_chunks = (uint32_t)((nq + chunk - 1) / chunk);
    std::unique_ptr<Context> ctx[2];
    ctx[0] = R.acquire();
    if (!ctx[0]) return false;
    if (n_chunks > 1 && !(ctx[1] = R.acquire())) {
        R.give_back(std::move(ctx[0]));
        return false;
    }
    HostChunk fl[2];
    bool ok = true, pending = false;
    for (uint32_t k = 0; k <= n_chunks && ok; ++k) {
        // queue chunk k, then complete chunk k - 1 while k runs
        if (k < n_chunks) {
            const uint32_t q0 = (uint32_t)(k * chunk), B = (uint32_t)std::min<size_t>(chunk, nq - q0);
            ok = queue_host_chunk(L, R, *ctx[k & 1], queries, q0, B, thr, Lm, fl[k & 1], pbase, u8, replica);
            if (!ok) break;
        }
        if (pending) ok = finish_host_chunk(L, R, fl[(k - 1) & 1], Lm, counts, k == n_chunks, emit);
        pending = k < n_chunks;
    }
    if (!ok)  // a chunk may still be queued: let it drain before its context is reused
        for (auto& c : ctx)
            if (c) hipStreamSynchronize(c->stream);
    for (auto& c : ctx)
        if (c) R.give_back(std::move(c));
    return ok;
}

// ... into flat (key, score) vectors
template <typename CharT>
bool host_search_one(Library& L, Replica& R, const CharT* const* queries, uint32_t nq, float thr, uint32_t Lm,
                     std::vector<uint32_t>& counts, std::vector<uint32_t>& keys, std::vector<float>& scores) {
    keys.clear();
    scores.clear();
    return host_search_chunks(L, R, queries, nq, thr, Lm, counts, [&](const void* recs, const float* sc, uint32_t n,
                                                                       bool, uint32_t) {
        const uint32_t* k = static_cast<const uint32_t*>(recs);
        keys.insert(keys.end(), k, k + n);
        scores.insert(scores.end(), sc, sc + n);
    });
}

// Queries per replica below which a batch is not split (a split costs a host thread and a
// launch sequence per replica). NGS_SPLIT_MIN overrides it (tests split small batches).
uint32_t split_min() {
    static const uint32_t v = [] {
        const char* e = std::getenv("NGS_SPLIT_MIN");
        return e ? std::max<uint32_t>(1, (uint32_t)std::strtoul(e, nullptr, 0)) : 4096u;
    }();
    return v;
}

// Host entry: one replica scores the batch, or (an index on several devices) contiguous slices
// of it go to the replicas, one host thread each, and the slices' results are joined in order.
// Queries are independent, so the joined result is the single-device result.
template <typename CharT>
bool host_search(Library& L, const CharT* const* queries, uint32_t nq, float thr, uint32_t limit,
                 std::vector<uint32_t>& counts, std::vector<uint32_t>& keys, std::vector<float>& scores) {
    const uint32_t Lm = effective_limit(L, limit);
    const size_t nrep = std::max<size_t>(L.split.size(), 1);
    const uint32_t parts = (uint32_t)std::min<uint64_t>(nrep, std::max<uint64_t>(1, nq / split_min()));
    if (parts <= 1) return host_search_one(L, *L.reps.front(), queries, nq, thr, Lm, counts, keys, scores);
    const uint32_t per = (nq + parts - 1) / parts;
    std::vector<std::vector<uint32_t>> pc(parts), pk(parts);
    std::vector<std::vector<float>> ps(parts);
    std::vector<char> pok(parts, 0);
    std::vector<int> perr(parts, 0);  // each worker's ngsLastError, handed to the caller's thread
    const int err0 = t_last_error;
    run_parts(L.workers, parts, [&](size_t i) {
        const uint32_t q0 = (uint32_t)i * per, n = std::min(per, nq - std::min(nq, q0));
        t_last_error = 0;
        pok[i] = host_search_one(L, *L.reps[L.split[i]], queries + q0, n, thr, Lm, pc[i], pk[i], ps[i]);
        perr[i] = pok[i] ? 0 : (t_last_error ? t_last_error : kErrInternal);
    });
    t_last_error = err0;
    for (uint32_t i = 0; i < parts; ++i)
        if (perr[i]) t_last_error = perr[i];
    counts.clear();
    keys.clear();
    scores.clear();
    counts.reserve(nq);
    for (uint32_t i = 0; i < parts; ++i) {
        if (!pok[i]) return false;
        counts.insert(counts.end(), pc[i].begin(), pc[i].end());
        keys.insert(keys.end(), pk[i].begin(), pk[i].end());
        scores.insert(scores.end(), ps[i].begin(), ps[i].end());
    }
    return true;
}

void set_valid(Library& L, const char* chars, int n) {
    uint32_t v[8] = {};
    for (int i = 0; i < n; ++i) {
        const uint8_t c = (uint8_t)chars[i];
        v[c >> 5] |= 1u << (c & 31);
    }
    {
        std::lock_guard<std::mutex> g(L.valid_mu);
        std::memcpy(L.valid, v, sizeof(v));
    }
    // the set's key flags (Replica::index_for) built here, so that the first search under it, an
    // ngsSearchDeviceAsync included, does not build and synchronise them (the caller's device kept)
    int dev = -1;
    (void)hipGetDevice(&dev);
    for (auto& R : L.reps) {
        DevIndex X;
        (void)R->index_for(v, X);
    }
    if (dev >= 0) (void)hipSetDevice(dev);
}

// result strings point into the index's own key storage (valid until dispose, hpp:443-447)
template <typename CharT>
uint32_t marshal(const Library& L, const std::vector<uint32_t>& keys, const std::vector<float>& sc,
                 CharT*** results, float** scores, const Library::U8Keys* u8 = nullptr) {
    const size_t n = keys.size();
    if (scores) *scores = new float[n];
    *results = new CharT*[n];
    CharT** res = *results;
    float* out_s = scores ? *scores : nullptr;
    // (u8, CharT = char: the strings of the UTF-8 key table of a wide index)
    char* base = const_cast<char*>(u8 ? u8->bytes.data() : L.host.key_bytes.data());
    const uint64_t* koff = u8 ? u8->off.data() : L.host.key_off.data();
    auto fill = [&](size_t a, size_t b) {  // key_off is gathered at random: memory-latency bound
        for (size_t i = a; i < b; ++i) {
            res[i] = reinterpret_cast<CharT*>(base + koff[keys[i]] * sizeof(CharT));
            if (out_s) out_s[i] = sc[i];
        }
    };
    // a whole batch's records (1.3M at C3) on several host threads
    const size_t nt = n < (size_t(1) << 18) ? 1 : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
    if (nt <= 1) {
        fill(0, n);
    } else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; ++t) th.emplace_back(fill, n * t / nt, n * (t + 1) / nt);
        for (auto& x : th) x.join();
    }
    return (uint32_t)n;
}

// The query normalised as k_prep does it (escapeBlank with the index's validChar set, C-locale
// trim, toUpper; nGramSearch.hpp:372-376): its length (kQueryWildcard for "" and "*"), false if
// it does not fit `cap` characters.
bool host_normalise(const uint32_t* valid, const char* q, uint8_t* out, uint32_t cap, uint32_t& m) {
    const size_t n = std::strlen(q);
    if (n == 0 || (n == 1 && q[0] == '*')) {  // nGramSearch.hpp:356
        m = kQueryWildcard;
        return true;
    }
    auto esc = [&](uint8_t c) -> uint8_t { return ((valid[c >> 5] >> (c & 31)) & 1u) ? c : (uint8_t)' '; };
    auto space = [](uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); };
    size_t a = 0, e = n;
    while (a < e && space(esc((uint8_t)q[a]))) ++a;
    while (e > a && space(esc((uint8_t)q[e - 1]))) --e;
    if (e - a > cap) return false;
    m = (uint32_t)(e - a);
    for (size_t i = a; i < e; ++i) {
        const uint8_t c = esc((uint8_t)q[i]);
        out[i - a] = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
    }
    return true;
}

// score() through the server (ngsServe): false when the call must take the regular path (a
// limit above the wave search's, a library large enough for the sliced latency path, a query
// the server routes to tier 2 or the general path, or a server that cannot be reached).
bool serve_query(Library& L, const char* query, float thr, uint32_t limit, std::vector<uint32_t>& keys,
                 std::vector<float>& sc) {
    // the server's lifetime (shared: requests of other threads run beside this one)
    std::shared_lock<std::shared_mutex> g(L.server_mu);
    if (L.batches.load(std::memory_order_acquire) > 0) return false;
    Server* sv = L.server.get();
    const uint32_t Lm = effective_limit(L, limit);
    Replica& R = *L.reps.front();
    if (!sv || Lm == 0 || Lm > kWaveMaxLimit || R.dev.n_buckets / 8 > 1) return false;
    // a free request slot, tried from one of this thread's own; all busy: try them again (a request
    // holds its slot ~15 us, and a thread put to sleep on a mutex took ~50 us to wake: 8 threads on
    // 4 slots ran at 84k calls/s blocking, against 240k for 4 threads)
    static std::atomic<uint32_t> next_hint{0};
    thread_local const uint32_t hint = next_hint.fetch_add(1, std::memory_order_relaxed);
    uint32_t slot = 0;
    std::unique_lock<std::mutex> sl;
    for (uint32_t i = 0; !sl.owns_lock(); ++i) {
        const uint32_t k = (hint + i) % kServeSlots;
        sl = std::unique_lock<std::mutex>(sv->slot_mu[k], std::try_to_lock);
        if (sl.owns_lock()) slot = k;
        else if (i % kServeSlots == kServeSlots - 1) {
            if (i > 64 * kServeSlots) std::this_thread::yield();
            else __builtin_ia32_pause();
        }
    }
    ServeBlock* b = sv->h + slot;
    uint32_t m = 0;
    {
        std::lock_guard<std::mutex> gv(L.valid_mu);
        if (!host_normalise(L.valid, query, b->q, kServeMaxQuery, m)) return false;
        std::memcpy(b->valid, L.valid, sizeof(b->valid));
    }
    b->thr = thr;
    b->limit = Lm;
    b->m = m;
    b->off[0] = 0;
    b->off[1] = m == kQueryWildcard ? 0 : m;
    const uint64_t seq = ++sv->seq[slot];
    // (re)launch when the kernel has left; a running server reads the key flags of the validChar set
    // it was launched with, so a new set restarts it (the other slots' requests are answered by
    // the new kernel: theirs stay posted)
    auto launch = [&](bool force) -> bool {
        std::lock_guard<std::mutex> gl(sv->launch_mu);
        if (force && R.dev.kt_off && !sv->stopped()) sv->stop();
        if (!sv->stopped()) return true;
        if (!HIP_CHECK(hipSetDevice(sv->device))) return false;
        SearchParams P{};
        P.n_queries = 1;
        P.nslices = 1;
        DevIndex X;
        if (!R.index_for(b->valid, X)) return false;
        std::memcpy(sv->launch_valid, b->valid, sizeof(sv->launch_valid));
        sv->launched = HIP_CHECK(launch_serve(X, P, sv->d, sv->scratch, sv->list2, sv->t_any, kServeIdleMs,
                                              kServeLifeMs, sv->stream));
        return sv->launched;
    };
    {
        bool stale;
        {
            std::lock_guard<std::mutex> gl(sv->launch_mu);
            stale = R.dev.kt_off && std::memcmp(sv->launch_valid, b->valid, sizeof(b->valid)) != 0;
        }
        if ((stale || sv->stopped()) && !launch(stale)) return false;
    }
    __atomic_store_n(&b->req_seq, seq, __ATOMIC_RELEASE);  // the fields above first (x86 stores stay in order)
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 1; __atomic_load_n(&b->done_seq, __ATOMIC_ACQUIRE) != seq; ++spin) {
        if ((spin & 1023) == 0) {
            // the kernel left (its idle time ran out as the request came in): relaunch, it
            // answers the posted request
            if (sv->stopped() && !launch(false)) return false;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                std::lock_guard<std::mutex> gl(sv->launch_mu);
                sv->stop();  // unreachable: leave it to the regular path
                return false;
            }
        }
        __builtin_ia32_pause();
    }
    if (__atomic_load_n(&b->status, __ATOMIC_ACQUIRE) != 0) return false;
    const uint32_t n = std::min(b->n, Lm);
    keys.assign(b->keys, b->keys + n);
    sc.assign(b->scores, b->scores + n);
    return true;
}

// Starts the server for a library it can answer once kAutoServeAfter single-query calls came in
// (unless ngsServe(h, 0) turned it off): score() at the reference's C1 latency with no opt-in.
void maybe_auto_serve(Library& L) {
    if (L.serve_pref.load(std::memory_order_relaxed) != 0 || L.reps.empty() || L.host.csize != 1) return;
    if (L.reps.front()->dev.n_buckets / 8 > 1) return;  // a large library keeps the sliced latency path
    if (L.single_calls.fetch_add(1, std::memory_order_relaxed) + 1 < kAutoServeAfter) return;
    std::unique_lock<std::shared_mutex> g(L.server_mu, std::try_to_lock);
    if (!g.owns_lock() || L.server || L.serve_pref.load() != 0) return;
    auto sv = std::make_unique<Server>();
    if (!sv->init(L.reps.front()->device)) {
        L.serve_pref.store(-1);  // no server on this device: do not try again
        (void)hipGetLastError();
        t_last_error = 0;
        return;
    }
    L.server = std::move(sv);
    L.serving.store(true, std::memory_order_release);
}

// batches of more than kSmallBatch queries count as batch traffic (smaller ones take the latency
// path, like score())
inline Library* batch_mark(Library* L, uint32_t nq) { return nq > kSmallBatch ? L : nullptr; }

// Marks a batch call in flight for its lifetime: a running server kernel is stopped first (its
// stream may share a hardware queue with the batch's streams) and is not relaunched meanwhile.
struct BatchGuard {
    Library* L;
    explicit BatchGuard(Library* l) : L(l) {
        if (!L) return;
        L->batches.fetch_add(1, std::memory_order_acq_rel);
        if (L->serving.load(std::memory_order_acquire)) {
            std::lock_guard<std::shared_mutex> g(L->server_mu);
            if (L->server && !L->server->stopped()) L->server->stop();
        }
    }
    ~BatchGuard() {
        if (L) L->batches.fetch_sub(1, std::memory_order_acq_rel);
    }
    BatchGuard(const BatchGuard&) = delete;
    BatchGuard& operator=(const BatchGuard&) = delete;
};

// A narrow call on a wide index (or the reverse) is answered like an unknown handle.
template <typename CharT>
uint32_t one_query(uint32_t handle, const CharT* query, CharT*** results, float** scores, float thr,
                   uint32_t limit) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed || !query || L->host.csize != sizeof(CharT)) return 0;  // dllmain.cpp:69, hpp:417-418
    std::vector<uint32_t> counts, keys;
    std::vector<float> sc;
    if (sizeof(CharT) == 1 && !L->serving.load(std::memory_order_acquire)) maybe_auto_serve(*L);
    if (sizeof(CharT) == 1 && L->serving.load(std::memory_order_acquire) && serve_query(*L, reinterpret_cast<const char*>(query), thr, limit, keys, sc))
        return marshal(*L, keys, sc, results, scores);
    // the regular path's kernels while a server exists (it cannot take this query: a limit past the
    // wave search's, tier 2 or the general path): stop it first, since its stream may share a
    // hardware queue with ours and a resident server would hold our launches until its idle exit
    BatchGuard bg(L->serving.load(std::memory_order_acquire) ? L : nullptr);
    if (!host_search(*L, &query, 1, thr, limit, counts, keys, sc)) return 0;
    return marshal(*L, keys, sc, results, scores);
}

// A batch split over the replicas with the one-replica path's pointer mode (dllmain.cpp:82-90 over
// several devices): each replica's part packs its records on its device as result pointers, the
// parts publish their record counts, the last one allocates the caller's arrays at the exact total,
// and every part copies its records into its own slice of them straight from its pinned read-back.
// kNoDirect: a part would take several chunks (the caller's general path then joins vectors).
constexpr uint32_t kNoDirect = 0xFFFFFFFFu;
template <typename CharT>
uint32_t split_direct(Library& L, const CharT* const* queries, uint32_t nq, float thr, uint32_t Lm, uint32_t* counts,
                      CharT*** results, float** scores) {
    const uint32_t parts = (uint32_t)std::min<uint64_t>(L.split.size(), std::max<uint64_t>(1, nq / split_min()));
    const uint32_t per = (nq + parts - 1) / parts;
    if (parts < 2 || host_chunk(per, Lm) < per || (uint64_t)nq * Lm > kDirectMax) return kNoDirect;
    const uint64_t pbase = (uint64_t)(uintptr_t)L.host.key_bytes.data();
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> total(parts, 0), base(parts, 0);
    uint32_t known = 0;
    bool failed = false, ready = false;
    CharT** res = nullptr;
    float* out_s = nullptr;
    // part i knows its record count: the last part to know allocates the arrays for everyone
    auto publish = [&](uint32_t i, uint64_t n, bool fail) {
        std::unique_lock<std::mutex> lk(mu);
        total[i] = n;
        failed |= fail;
        if (++known == parts) {
            uint64_t sum = 0;
            for (uint32_t j = 0; j < parts; ++j) base[j] = sum, sum += total[j];
            if (!failed) {
                res = new CharT*[std::max<uint64_t>(sum, 1)];
                out_s = scores ? new float[std::max<uint64_t>(sum, 1)] : nullptr;
            }
            ready = true;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return ready; });
        }
    };
    std::vector<std::vector<uint32_t>> pc(parts);
    std::vector<int> perr(parts, 0);
    const int err0 = t_last_error;
    run_parts(L.workers, parts, [&](size_t pi) {
        const uint32_t i = (uint32_t)pi, q0 = i * per, n = std::min(per, nq - std::min(nq, q0));
        t_last_error = 0;
        bool seen = false;
        size_t off = 0;
        const bool ok = host_search_chunks(L, *L.reps[L.split[i]], queries + q0, n, thr, Lm, pc[i],
                                           [&](const void* recs, const float* sc, uint32_t m, bool, uint32_t chunk_total) {
            if (!seen) {  // (one chunk: its total is the part's)
                seen = true;
                publish(i, chunk_total, false);
            }
            if (!res) return;  // another part failed
            const uint64_t* p = static_cast<const uint64_t*>(recs);
            CharT** dst = res + base[i] + off;
            float* dsc = out_s ? out_s + base[i] + off : nullptr;
            parallel_ranges(m, size_t(1) << 16, [&](size_t a, size_t e) {
                std::memcpy(dst + a, p + a, (e - a) * sizeof(uint64_t));
                if (dsc) std::memcpy(dsc + a, sc + a, (e - a) * sizeof(float));
            });
            off += m;
        }, pbase);
        if (!seen) publish(i, 0, true);  // (failed before its records: the others must not wait)
        if (!ok) perr[i] = t_last_error ? t_last_error : kErrInternal;
    });
    t_last_error = err0;
    bool bad = failed;
    for (uint32_t i = 0; i < parts; ++i)
        if (perr[i]) bad = true, t_last_error = perr[i];
    if (bad) {
        delete[] res;
        delete[] out_s;
        return 0;
    }
    uint64_t sum = 0;
    for (uint32_t i = 0; i < parts; ++i) {
        std::copy(pc[i].begin(), pc[i].end(), counts + (size_t)i * per);
        sum += total[i];
    }
    *results = res;
    if (scores) *scores = out_s;
    return (uint32_t)sum;
}

// A batch on the first replica, marshalled as the chunks finish, straight into the caller's
// arrays. One chunk (the common case): the arrays at the exact size, filled from the pinned
// read-back; several chunks: at the batch's capacity (nq x limit entries; only the pages written
// are touched). Pointer mode: k_pack writes each record as its result pointer into the host key
// bytes (key_off gathered on the device), so marshalling is two parallel copies. u8: UTF-8
// queries on a wide index, decoded on the device, the pointers into the UTF-8 key table.
template <typename CharT>
uint32_t direct_batch(Library& L, const CharT* const* queries, uint32_t nq, float thr, uint32_t Lm, uint32_t* counts,
                      CharT*** results, float** scores, HostTimer& ht, const Library::U8Keys* u8 = nullptr) {
    std::vector<uint32_t> cnt;
    CharT** res = nullptr;
    float* out_s = nullptr;
    size_t off = 0, cap = 0;
    const uint64_t pbase = (uint64_t)(uintptr_t)(u8 ? u8->bytes.data() : L.host.key_bytes.data());
    static_assert(sizeof(CharT*) == sizeof(uint64_t), "result pointers are 64-bit");
    const bool ok = host_search_chunks(L, *L.reps.front(), queries, nq, thr, Lm, cnt,
                                       [&](const void* recs, const float* sc, uint32_t n, bool last,
                                           uint32_t chunk_total) {
        if (!res) {
            cap = (off == 0 && last) ? std::max<size_t>(chunk_total, 1) : (size_t)nq * Lm;
            res = new CharT*[cap];
            out_s = scores ? new float[cap] : nullptr;
        }
        const uint64_t* p = static_cast<const uint64_t*>(recs);
        parallel_ranges(n, size_t(1) << 16, [&](size_t a, size_t e) {
            std::memcpy(res + off + a, p + a, (e - a) * sizeof(uint64_t));
            if (out_s) std::memcpy(out_s + off + a, sc + a, (e - a) * sizeof(float));
        });
        off += n;
    }, pbase, u8, 0);
    if (ok && !res) {  // no chunk ran (cannot happen with nq >= kSmallBatch): empty arrays
        res = new CharT*[1];
        out_s = scores ? new float[1] : nullptr;
    }
    if (!ok) {
        delete[] res;
        delete[] out_s;
        return 0;
    }
    ht.mark(kHpCall, "search + marshal (chunks)");
    g_host_phase[kHpCalls].fetch_add(1, std::memory_order_relaxed);
    std::copy(cnt.begin(), cnt.end(), counts);
    *results = res;
    if (scores) *scores = out_s;
    return (uint32_t)off;
}

template <typename CharT>
uint32_t batch_query(uint32_t handle, const CharT* const* queries, uint32_t nq, float thr, uint32_t limit,
                     uint32_t* counts, CharT*** results, float** scores) {
    if (counts) std::fill(counts, counts + nq, 0u);
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed || !queries || !counts || L->host.csize != sizeof(CharT)) return 0;
    // (a small batch takes the latency path and stops a running server like score()'s fallback)
    BatchGuard bg(L->serving.load(std::memory_order_acquire) ? L : batch_mark(L, nq));
    std::vector<uint32_t> cnt, keys;
    std::vector<float> sc;
    HostTimer ht;
    const uint32_t Lm = effective_limit(*L, limit);
    const bool one_replica = L->split.size() <= 1 || nq / split_min() <= 1;
    if (one_replica && Lm && (uint64_t)nq * Lm <= kDirectMax && nq >= kSmallBatch)
        return direct_batch(*L, queries, nq, thr, Lm, counts, results, scores, ht);
    if (Lm && nq >= kSmallBatch && !one_replica) {
        const uint32_t n = split_direct(*L, queries, nq, thr, Lm, counts, results, scores);
        if (n != kNoDirect) {
            ht.mark(kHpCall, "search + marshal (replicas)");
            g_host_phase[kHpCalls].fetch_add(1, std::memory_order_relaxed);
            return n;
        }
    }
    if (!host_search(*L, queries, nq, thr, limit, cnt, keys, sc)) return 0;
    std::copy(cnt.begin(), cnt.end(), counts);
    const uint32_t n = marshal(*L, keys, sc, results, scores);
    ht.mark(kHpCall, "search + marshal");
    if (nq >= kSmallBatch) g_host_phase[kHpCalls].fetch_add(1, std::memory_order_relaxed);
    return n;
}

// ---- UTF-8 front end (indexU8 / searchU8 / scoreU8 / the U8 batch calls) ----

// NUL-terminated UTF-8 strings decoded (ngs_utf8.h) into one buffer of NUL-terminated UTF-32
// strings, on the host worker threads; a null string stays null.
struct DecodedStrings {
    std::vector<uint32_t> units;
    std::vector<const uint32_t*> ptr;
};
void decode_strings(const char* const* strs, uint64_t n, DecodedStrings& D) {
    std::vector<uint64_t> off(n + 1, 0);  // room per string: a unit takes at least a byte, and the NUL
    parallel_ranges(n, 8192, [&](size_t a, size_t e) {
        for (size_t i = a; i < e; ++i) off[i + 1] = strs[i] ? std::strlen(strs[i]) + 1 : 0;
    });
    for (uint64_t i = 0; i < n; ++i) off[i + 1] += off[i];
    D.units.resize(std::max<uint64_t>(off[n], 1));
    D.ptr.assign(n, nullptr);
    parallel_ranges(n, 8192, [&](size_t a, size_t e) {
        for (size_t i = a; i < e; ++i) {
            if (!strs[i]) continue;
            uint32_t* out = D.units.data() + off[i];
            const size_t u = utf8_decode(reinterpret_cast<const uint8_t*>(strs[i]), off[i + 1] - off[i] - 1, out);
            out[u] = 0;
            D.ptr[i] = out;
        }
    });
}

// The library's UTF-8 key table, built by the first call that needs it; null on a HIP failure.
const Library::U8Keys* u8_keys(Library& L) {
    Library::U8Keys& T = L.u8;
    std::call_once(T.once, [&] {
        const HostIndex& H = L.host;
        const uint32_t* units = reinterpret_cast<const uint32_t*>(H.key_bytes.data());
        const size_t nk = H.n_keys;
        T.off.assign(nk + 1, 0);
        parallel_ranges(nk, size_t(1) << 14, [&](size_t a, size_t e) {  // (key_off counts the NUL in)
            for (size_t k = a; k < e; ++k)
                T.off[k + 1] = utf8_encoded_len(units + H.key_off[k], H.key_off[k + 1] - 1 - H.key_off[k]) + 1;
        });
        for (size_t k = 0; k < nk; ++k) T.off[k + 1] += T.off[k];
        T.bytes.resize(std::max<uint64_t>(T.off[nk], 1));
        parallel_ranges(nk, size_t(1) << 14, [&](size_t a, size_t e) {
            for (size_t k = a; k < e; ++k) {
                uint8_t* out = reinterpret_cast<uint8_t*>(T.bytes.data()) + T.off[k];
                out[utf8_encode(units + H.key_off[k], H.key_off[k + 1] - 1 - H.key_off[k], out)] = 0;
            }
        });
        // the offsets on every replica's device (the caller's current device kept)
        int dev = -1;
        (void)hipGetDevice(&dev);
        bool ok = true;
        for (auto& R : L.reps) {
            uint64_t* d = nullptr;
            ok = ok && HIP_CHECK(hipSetDevice(R->device)) && dev_alloc(&d, nk + 1);
            if (d) {
                std::lock_guard<std::mutex> g(R->kflag_mu);  // (Replica::owned is shared with index_for)
                R->owned.push_back(d);
            }
            ok = ok && HIP_CHECK(hipMemcpy(d, T.off.data(), sizeof(uint64_t) * (nk + 1), hipMemcpyHostToDevice));
            T.d_off.push_back(d);
        }
        if (dev >= 0) (void)hipSetDevice(dev);
        T.ok = ok;
    });
    return T.ok ? &T : nullptr;
}

// searchU8 / scoreU8 and the U8 batch calls (counts null: one query). The answers are the W
// call's on the decoded units; the result strings are the UTF-8 key table's. Up to kSmallBatch
// queries are decoded on the host and take the wide latency path; a larger batch goes up as UTF-8
// and is decoded on the device (queue_host_chunk), answered by the first replica.
uint32_t u8_query(uint32_t handle, const char* const* queries, uint32_t nq, float thr, uint32_t limit,
                  uint32_t* counts, char*** results, float** scores) {
    const bool single = counts == nullptr;
    if (counts) std::fill(counts, counts + nq, 0u);
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed || !queries || (single && !queries[0]) || L->host.csize != sizeof(uint32_t)) return 0;
    const Library::U8Keys* T = u8_keys(*L);
    if (!T) return 0;
    BatchGuard bg(batch_mark(L, nq));
    std::vector<uint32_t> cnt, keys;
    std::vector<float> sc;
    HostTimer ht;
    if (nq <= kSmallBatch) {
        DecodedStrings D;
        decode_strings(queries, nq, D);
        if (!host_search(*L, D.ptr.data(), nq, thr, limit, cnt, keys, sc)) return 0;
    } else {
        const uint32_t Lm = effective_limit(*L, limit);
        if (Lm && (uint64_t)nq * Lm <= kDirectMax)
            return direct_batch(*L, queries, nq, thr, Lm, counts, results, scores, ht, T);
        bool ok = host_search_chunks(*L, *L->reps.front(), queries, nq, thr, Lm, cnt,
                                     [&](const void* recs, const float* s, uint32_t n, bool, uint32_t) {
            const uint32_t* k = static_cast<const uint32_t*>(recs);
            keys.insert(keys.end(), k, k + n);
            sc.insert(sc.end(), s, s + n);
        }, 0, T, 0);
        if (!ok) return 0;
        g_host_phase[kHpCalls].fetch_add(1, std::memory_order_relaxed);
    }
    if (counts) std::copy(cnt.begin(), cnt.end(), counts);
    const uint32_t n = marshal(*L, keys, sc, results, scores, T);
    ht.mark(kHpCall, "search + marshal (UTF-8)");
    return n;
}

}  // namespace
}  // namespace ngs

using namespace ngs;

namespace ngs {
namespace {
// dllmain.cpp:37-59 for every index flavour: smallest free handle, build, upload.
template <class Build>
uint32_t new_library(Build&& build) {
    std::unique_lock<std::shared_mutex> lk(g_lock);  // dllmain.cpp:39
    uint32_t handle = 1;                             // dllmain.cpp:41-46
    const uint32_t maxVal = std::numeric_limits<uint32_t>::max();
    while (g_libs.count(handle) && handle < maxVal) ++handle;
    if (handle == maxVal) return 0;
    auto L = std::make_unique<Library>();
    L->serial = g_next_serial++;
    set_valid(*L, kDefaultValid, (int)std::strlen(kDefaultValid));
    std::vector<int> devs = t_devices;
    if (devs.empty()) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        devs.push_back(dev);
    }
    (void)hipSetDevice(devs.front());  // the build's device kernels run on the first replica's device
    PhaseTimer pt;
    build(L->host);
    pt.mark("build (intern + layout)");
    if (L->host.indexed && !upload(*L, devs)) {
        std::fprintf(stderr, "ngram_search: indexN could not place the index on a GPU\n");
        return 0;
    }
    if (!L->host.indexed) L->device = devs.front();
    g_libs.emplace(handle, std::move(L));
    return handle;
}

// A search that answered kRetryQcap (k_prep flagged a batch that does not fit the context's
// normalised-query buffer) runs again with the batch's byte count, read back on s; a second retry
// is -5. Every other rc passes through.
int rerun_outgrown(int rc, Library& L, Replica& R, Context& c, const uint8_t* d_raw, const uint64_t* d_off, uint32_t B,
                   float thr, uint32_t Lm, uint32_t stride, uint32_t* d_n, uint32_t* d_k, float* d_s, hipStream_t s) {
    if (rc != kRetryQcap) return rc;
    uint64_t qbytes = 0;
    rc = HIP_CHECK(hipMemcpyAsync(&qbytes, d_off + B, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) &&
                 HIP_CHECK(hipStreamSynchronize(s))
             ? device_search(L, R, c, d_raw, d_off, B, qbytes, thr, Lm, stride, d_n, d_k, d_s, s)
             : -4;
    if (rc == kRetryQcap) {
        rc = -5;
        t_last_error = kErrQueryBuffer;
    }
    return rc;
}

// ngsSearchDevice on replica R (the caller holds the shared lock and a BatchGuard, and R's device
// is current): a context from R's pool, the search, the rerun when the batch outgrew the context's
// normalised-query buffer.
int search_on_replica(Library& L, Replica& R, const uint8_t* d_raw, const uint64_t* d_off, uint32_t B, float thr,
                      uint32_t Lm, uint32_t stride, uint32_t* d_n, uint32_t* d_k, float* d_s, hipStream_t s) {
    if (Lm == 0) {
        return HIP_CHECK(hipMemsetAsync(d_n, 0, sizeof(uint32_t) * B, s)) && HIP_CHECK(hipStreamSynchronize(s)) ? 0 : -4;
    }
    std::unique_ptr<Context> c = R.acquire();
    if (!c) return -4;
    // The batch's byte count sizes the normalised-query buffer. A context that has one already
    // launches without reading it back (a sync before any kernel); k_prep flags a batch that
    // does not fit and the call reruns after the read-back (rerun_outgrown).
    int rc = 0;
    uint64_t qbytes = 0;
    if (B && !c->qcap &&
        !(HIP_CHECK(hipMemcpyAsync(&qbytes, d_off + B, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) &&
          HIP_CHECK(hipStreamSynchronize(s))))
        rc = -4;
    if (!rc) rc = device_search(L, R, *c, d_raw, d_off, B, qbytes, thr, Lm, stride, d_n, d_k, d_s, s);
    rc = rerun_outgrown(rc, L, R, *c, d_raw, d_off, B, thr, Lm, stride, d_n, d_k, d_s, s);
    R.give_back(std::move(c));
    return rc;
}

// ---- the similarity stage (ngsSimilarityDevice / ngsRerankDevice / scoreBatchSim*) ----

// The key -> term map of replica R for the similarity kernels: null with ok == true when the index
// has kt_off / kt_term (they list every key's terms). Otherwise every key has one pair and nothing
// maps it back: the first call builds key_term[n_keys] from the device's own tk arrays (the host's
// are released after the upload), synchronously on the null stream like a validChar set's key
// flags, so that a call on any stream may use it as soon as it is published. Kept until dispose
// (Replica::owned). R's device is current.
const uint32_t* sim_key_term(Replica& R, bool& ok) {
    ok = true;
    if (R.dev.kt_off) return nullptr;
    std::lock_guard<std::mutex> g(R.sim_mu);
    if (R.key_term) return R.key_term;
    uint32_t* kt = nullptr;
    ok = dev_alloc(&kt, R.dev.n_keys);
    if (!ok) return nullptr;
    {
        std::lock_guard<std::mutex> o(R.kflag_mu);  // (Replica::owned is shared with index_for)
        R.owned.push_back(kt);
    }
    ok = HIP_CHECK(build_key_term(R.dev, kt, nullptr)) && HIP_CHECK(hipStreamSynchronize(nullptr));
    if (!ok) return nullptr;
    R.key_term = kt;
    return kt;
}

// The token-sorted terms of replica R for a flagged similarity call: ts_off[n_terms
// + 1] and ts_bytes, in term_off / term_bytes' layout (character offsets; two dwords of padding
// behind the last term, which myers_narrow reads ahead into). The first flagged call builds them
// from the device's own term arrays: pass 1 the lengths and their scan, pass 2 the characters;
// synchronously on the null stream, published once and kept until dispose, as key_term is.
// R's device is current. False on a HIP failure.
bool sim_sorted_terms(Replica& R, DevIndex& X) {
    std::lock_guard<std::mutex> g(R.sim_mu);
    if (!R.ts_off) {
        const uint64_t cs = R.dev.csize;
        uint64_t* off = nullptr;
        uint8_t* bytes = nullptr;
        uint64_t chars = 0;
        auto own = [&](void* p) {
            std::lock_guard<std::mutex> o(R.kflag_mu);  // (Replica::owned is shared with index_for)
            R.owned.push_back(p);
        };
        if (!dev_alloc(&off, (size_t)R.dev.n_terms + 1)) return false;
        own(off);
        if (!HIP_CHECK(sorted_term_offsets(R.dev, off, nullptr)) ||
            !HIP_CHECK(hipMemcpy(&chars, off + R.dev.n_terms, sizeof chars, hipMemcpyDeviceToHost)) ||
            !dev_alloc(&bytes, (size_t)(chars * cs) + 8))
            return false;
        own(bytes);
        if (!HIP_CHECK(hipMemsetAsync(bytes + chars * cs, 0, 8, nullptr)) ||
            !HIP_CHECK(launch_sorted_terms(R.dev, off, bytes, nullptr)) || !HIP_CHECK(hipStreamSynchronize(nullptr)))
            return false;
        R.ts_bytes = bytes;
        R.ts_off = off;
    }
    X.term_off = R.ts_off;
    X.term_bytes = R.ts_bytes;
    return true;
}

// the argument checks of the two device entry points, before any handle or device is touched
bool sim_args_ok(const uint64_t* d_off, uint32_t n, uint32_t stride, const uint32_t* d_n, const uint32_t* d_k,
                 const float* d_v) {
    return d_off && d_n && !(n && stride && (!d_k || !d_v));
}

// What the similarity runs over: one index on a replica, or the members of an index set on the set's
// device (sim_view, here and behind KeySet). A member's replica is null where it has none there.
struct SimView {
    struct Member {
        Library* L;
        Replica* R;
        uint32_t base;
    };
    Member m[kSetMaxParts];
    uint32_t P, csize;
    bool set;  // launch_similarity_set, whatever P is
};
SimView sim_view(Library& L, Replica& R) { return {{{&L, &R, 0u}}, 1u, R.dev.csize, false}; }

// Queues the similarity kernel by `metric` (and, with `rerank`, the re-rank behind it) on s; nothing
// waits: -3 a member without a replica on the device, -4 a HIP failure. Every member's key_term map
// (and with kSimTokenSort its token-sorted terms, which the kernel then reads) is built where
// missing; the query is normalised under the first member's validChar set. d_t: the matched terms,
// or null. With kSimTokenSort and d_sort (= d_raw, writable: the host calls' own scratch) the
// queries are token-sorted in place in front of the kernel, under the same snapshot of the
// validChar set; without d_sort they are taken as given (the device entry points). The view's
// device is current.
int queue_similarity(const SimView& V, const uint8_t* d_raw, const uint64_t* d_off, uint32_t n, uint32_t stride,
                     uint32_t* d_n, uint32_t* d_k, float* d_s, float* d_v, uint32_t* d_t, uint32_t metric, bool rerank,
                     float min_sim, hipStream_t s, uint8_t* d_sort = nullptr) {
    if (n == 0) return 0;
    const bool sorted = (metric & kSimTokenSort) != 0;
    DevIndex X{};  // (a handle's: its one member's)
    SimMembers T{};
    for (uint32_t p = 0; p < V.P; ++p) {
        Replica* R = V.m[p].R;
        if (!R) return -3;
        bool ok = true;
        const uint32_t* key_term = sim_key_term(*R, ok);
        if (!ok) return -4;
        X = R->dev;
        if (sorted && !sim_sorted_terms(*R, X)) return -4;
        T.m[p] = SimMember{X.kt_off, X.kt_term, key_term, X.term_off, X.term_bytes, X.n_keys, X.n_terms, V.m[p].base, 0u};
    }
    uint32_t valid[8];
    {
        std::lock_guard<std::mutex> g(V.m[0].L->valid_mu);
        std::memcpy(valid, V.m[0].L->valid, sizeof valid);
    }
    if (sorted && d_sort && !HIP_CHECK(launch_token_sort(valid, V.csize, d_raw, d_off, n, d_sort, s))) return -4;
    const uint32_t base = sim_metric_base(metric);
    if (!HIP_CHECK(V.set ? launch_similarity_set(T, V.P, V.csize, valid, d_raw, d_off, n, stride, d_n, d_k, base, d_v, d_t, s)
                         : launch_similarity(X, valid, T.m[0].key_term, d_raw, d_off, n, stride, d_n, d_k, base, d_v, d_t, s)))
        return -4;
    if (rerank && !HIP_CHECK(launch_rerank(n, stride, d_n, d_k, d_s, d_v, d_t, min_sim, s))) return -4;
    return 0;
}

// ngsSimilarityDeviceM / ngsRerankDeviceM and their set forms behind the fronts that resolve the view
// (the lock and the guards held): without and with the re-rank
int similarity_entry(const SimView& V, const uint8_t* d_raw, const uint64_t* d_off, uint32_t n, uint32_t stride,
                     const uint32_t* d_n, const uint32_t* d_k, uint32_t metric, float* d_v, uint32_t* d_t, void* stream) {
    return queue_similarity(V, d_raw, d_off, n, stride, const_cast<uint32_t*>(d_n), const_cast<uint32_t*>(d_k), nullptr,
                            d_v, d_t, metric, false, 0.0f, (hipStream_t)stream);
}
// the argument checks of the re-rank entry points, in front of their fronts
bool rerank_args_ok(const uint64_t* d_off, uint32_t n, uint32_t stride, const uint32_t* d_n, const uint32_t* d_k,
                    const float* d_s, const float* d_v, uint32_t metric, float min_sim) {
    return sim_args_ok(d_off, n, stride, d_n, d_k, d_v) && !(n && stride && !d_s) && stride <= kRerankMaxStride &&
           min_sim == min_sim && sim_metric_ok(metric);
}

// The device entry points' front, in two halves (the caller holds the lock; each entry point puts
// its own checks before, between and behind them). The library of `handle`: -1 none, -2 not built.
int entry_library(uint32_t handle, Library*& L) {
    L = find_lib(handle);
    if (!L) return -1;
    return L->host.indexed ? 0 : -2;
}
// The replica on the caller's current device: -4 no device, -3 no replica there (the caller's
// buffers and stream belong to that device).
int entry_replica(Library& L, Replica*& R) {
    int cur = L.device;
    if (!HIP_CHECK(hipGetDevice(&cur))) return -4;
    R = L.replica_at(cur);
    return R ? 0 : -3;
}
// the search calls' pointer and stride check, at the effective limit Lm
bool search_args_ok(const uint64_t* d_off, uint32_t n, uint32_t Lm, uint32_t stride, const uint32_t* d_n,
                    const uint32_t* d_k, const float* d_s) {
    return d_off && d_n && !(n && Lm && (!d_k || !d_s || stride < Lm));
}

// The stream and the device blocks of one host call of the later stages (scoreBatchSim*, selfJoin,
// dedupKeys*, ngsSelfJoinDevice's gathered queries), freed when it returns.
struct CallScratch {
    std::vector<void*> mem;
    hipStream_t stream = nullptr;
    // the arrays every stage works on (begin); a stage's further ones are alloc calls of its own
    uint8_t* d_raw = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t *d_n = nullptr, *d_k = nullptr;
    float* d_s = nullptr;
    template <class T>
    bool alloc(T** p, size_t n) {
        if (!dev_alloc(p, n)) return false;
        mem.push_back(*p);
        return true;
    }
    // the call's stream, and for batches of up to `rows` queries of `stride` records and
    // `raw_bytes` query bytes: the bytes (with 16 bytes of slack behind them), the offsets, counts,
    // key ids and scores
    bool begin(size_t rows, size_t stride, size_t raw_bytes) {
        return HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) && alloc(&d_raw, raw_bytes + 16) &&
               alloc(&d_off, rows + 1) && alloc(&d_n, rows) && alloc(&d_k, rows * stride) && alloc(&d_s, rows * stride);
    }
    ~CallScratch() {
        if (stream) (void)hipStreamDestroy(stream);
        for (void* p : mem) (void)hipFree(p);
    }
};
constexpr size_t kSimChunkRecords = size_t(1) << 22;  // records (query x limit) per chunk of a scoreBatchSim* call

// The queries of a host call as they go up, `chunk` at a time: every query's bytes and their number,
// and the bytes of the largest chunk (raw_cap), so that the device buffers are made once.
struct QueryChunks {
    uint32_t chunk;
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> bytes;
    size_t raw_cap = 0;
    std::vector<uint64_t> h_off;
    std::vector<uint8_t> h_raw;
    // bytes_of(i, n): query i's bytes, n their number
    template <class F>
    QueryChunks(uint32_t nq, uint32_t chunk_, F&& bytes_of) : chunk(chunk_), ptr(nq), bytes(nq), h_off((size_t)chunk_ + 1) {
        for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
            size_t sum = 0;
            for (uint32_t i = q0; i < q0 + std::min(chunk, nq - q0); ++i) {
                ptr[i] = static_cast<const uint8_t*>(bytes_of(i, bytes[i]));
                sum += bytes[i];
            }
            raw_cap = std::max(raw_cap, sum);
        }
    }
    // queries [q0, q0 + B) packed behind one another, their B + 1 byte offsets and their bytes queued
    // for d_off / d_raw on s (the host copies stay valid until the next chunk is packed)
    bool upload(uint32_t q0, uint32_t B, uint64_t* d_off, uint8_t* d_raw, hipStream_t s) {
        h_raw.clear();
        h_off[0] = 0;
        for (uint32_t i = 0; i < B; ++i) {
            if (bytes[q0 + i]) h_raw.insert(h_raw.end(), ptr[q0 + i], ptr[q0 + i] + bytes[q0 + i]);
            h_off[i + 1] = h_raw.size();
        }
        return HIP_CHECK(hipMemcpyAsync(d_off, h_off.data(), sizeof(uint64_t) * (B + 1), hipMemcpyHostToDevice, s)) &&
               (h_raw.empty() || HIP_CHECK(hipMemcpyAsync(d_raw, h_raw.data(), h_raw.size(), hipMemcpyHostToDevice, s)));
    }
};

// scoreBatchSim / scoreBatchSimW / scoreBatchSimU8, plainly on top of the device stages: the
// queries packed and uploaded, the search as ngsSearchDevice runs it, ngsRerankDevice's kernels
// behind it on the same stream, then counts, key ids, scores and sims read back and the result
// pointers built as marshal() builds every other call's. u8: UTF-8 queries on a wide index
// (decoded on the host), the strings of the UTF-8 key table. The first replica answers.
// The similarity is by `metric`; with terms != null the matched term ids come back as a fourth flat
// array (ngsReleaseTerms).
template <typename CharT>
uint32_t sim_batch(uint32_t handle, const CharT* const* queries, uint32_t nq, float thr, uint32_t limit, float min_sim,
                   uint32_t* counts, CharT*** results, float** scores, float** sims, bool u8, uint32_t metric,
                   uint32_t** terms) {
    if (counts) std::fill(counts, counts + nq, 0u);
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    const uint32_t cs = u8 ? (uint32_t)sizeof(uint32_t) : (uint32_t)sizeof(CharT);
    if (!L || !L->host.indexed || !queries || !counts || !results || !scores || !sims || L->host.csize != cs) return 0;
    if (min_sim != min_sim || !sim_metric_ok(metric)) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    const uint32_t Lm = effective_limit(*L, limit);
    if (Lm > kRerankMaxStride) {
        t_last_error = kErrRerankLimit;
        return 0;
    }
    const Library::U8Keys* T = u8 ? u8_keys(*L) : nullptr;
    if (u8 && !T) return 0;
    if (Lm == 0 || nq == 0) return 0;
    BatchGuard bg(L);
    Replica& R = *L->reps.front();
    if (!HIP_CHECK(hipSetDevice(R.device))) return 0;
    // 1. the queries as the device entry points take them: characters of cs bytes, byte offsets
    DecodedStrings D;
    if (u8) decode_strings(reinterpret_cast<const char* const*>(queries), nq, D);
    const uint32_t chunk = (uint32_t)std::min<size_t>(nq, std::max<size_t>(1, kSimChunkRecords / Lm));
    QueryChunks Q(nq, chunk, [&](uint32_t i, size_t& bytes) -> const void* {
        if (u8) {
            bytes = D.ptr[i] ? str_len(D.ptr[i]) * cs : 0;
            return D.ptr[i];
        }
        bytes = queries[i] ? str_len(queries[i]) * cs : 0;
        return queries[i];
    });
    CallScratch M;
    uint32_t* d_t = nullptr;
    float* d_v = nullptr;
    const size_t recs = (size_t)chunk * Lm;
    if (!M.begin(chunk, Lm, Q.raw_cap) || !M.alloc(&d_v, recs) || (terms && !M.alloc(&d_t, recs))) return 0;
    std::vector<uint32_t> cnt(nq, 0), keys, h_n(chunk), h_k(recs);  // (counts stay zero unless the whole call succeeds)
    std::vector<uint32_t> tv, h_t(terms ? recs : 0);
    std::vector<float> sc, sv, h_s(recs), h_v(recs);
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t B = std::min(chunk, nq - q0);
        if (!Q.upload(q0, B, M.d_off, M.d_raw, M.stream)) return 0;
        // 2. the search, 3. the re-rank behind it
        if (search_on_replica(*L, R, M.d_raw, M.d_off, B, thr, Lm, Lm, M.d_n, M.d_k, M.d_s, M.stream) != 0) {
            if (!t_last_error) t_last_error = kErrInternal;
            return 0;
        }
        if (queue_similarity(sim_view(*L, R), M.d_raw, M.d_off, B, Lm, M.d_n, M.d_k, M.d_s, d_v, d_t, metric, true, min_sim,
                             M.stream, M.d_raw) != 0)
            return 0;
        // 4. everything back
        const size_t rb = (size_t)B * Lm;
        if (!HIP_CHECK(hipMemcpyAsync(h_n.data(), M.d_n, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_k.data(), M.d_k, sizeof(uint32_t) * rb, hipMemcpyDeviceToHost, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_s.data(), M.d_s, sizeof(float) * rb, hipMemcpyDeviceToHost, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_v.data(), d_v, sizeof(float) * rb, hipMemcpyDeviceToHost, M.stream)) ||
            (terms &&
             !HIP_CHECK(hipMemcpyAsync(h_t.data(), d_t, sizeof(uint32_t) * rb, hipMemcpyDeviceToHost, M.stream))) ||
            !HIP_CHECK(hipStreamSynchronize(M.stream)))
            return 0;
        for (uint32_t i = 0; i < B; ++i) {
            const uint32_t c = std::min(h_n[i], Lm);
            const size_t at = (size_t)i * Lm;
            cnt[q0 + i] = c;
            keys.insert(keys.end(), h_k.begin() + at, h_k.begin() + at + c);
            sc.insert(sc.end(), h_s.begin() + at, h_s.begin() + at + c);
            sv.insert(sv.end(), h_v.begin() + at, h_v.begin() + at + c);
            if (terms) tv.insert(tv.end(), h_t.begin() + at, h_t.begin() + at + c);
        }
    }
    // 5. the result pointers, and the third flat array
    std::copy(cnt.begin(), cnt.end(), counts);
    const uint32_t total = marshal(*L, keys, sc, results, scores, T);
    *sims = new float[std::max<size_t>(sv.size(), 1)];
    std::copy(sv.begin(), sv.end(), *sims);
    if (terms) {
        *terms = new uint32_t[std::max<size_t>(tv.size(), 1)];
        std::copy(tv.begin(), tv.end(), *terms);
    }
    return total;
}

// ---- the self-join (ngsKeyQueriesDevice .. dedupKeys) ----

// keys [first, first + n) lie in the index
bool join_range_ok(const Library& L, uint32_t first, uint32_t n) {
    return (uint64_t)first + n <= L.host.n_keys;
}
uint64_t join_query_bytes(const Library& L, uint32_t first, uint32_t n) {
    return join_query_off(L.host.key_off.data(), first, n, L.host.csize);
}
// the most query bytes a batch takes when keys [first, first + nk) are gathered B at a time
uint64_t join_max_query_bytes(const Library& L, uint32_t first, uint32_t nk, uint32_t B) {
    uint64_t most = 0;
    for (uint32_t k0 = first; k0 < first + nk; k0 += B)
        most = std::max(most, join_query_bytes(L, k0, std::min(B, first + nk - k0)));
    return most;
}
// the limit the join's search runs with: one more than the caller's, for the record that is found
// and removed (limit 0: every key)
uint32_t join_search_limit(const Library& L, uint32_t limit) {
    const uint64_t want = (uint64_t)(limit ? limit : kInt32Max) + 1u;
    return (uint32_t)std::min<uint64_t>(want, L.host.n_keys);
}

// One batch of the join on replica R (its device current, lock and BatchGuard held by the caller):
// the keys gathered into d_raw / d_off, the search with one record more, the key's own record
// dropped. The results are complete on return when `wait`; else drop-self is queued on s.
int join_batch(Library& L, Replica& R, uint32_t first, uint32_t n, float thr, uint32_t limit, uint32_t stride,
               uint8_t* d_raw, uint64_t* d_off, uint32_t* d_n, uint32_t* d_k, float* d_s, hipStream_t s, bool wait) {
    if (!HIP_CHECK(launch_key_queries(R.dev, first, n, join_query_bytes(L, first, n), d_raw, d_off, s))) return -4;
    if (const int rc = search_on_replica(L, R, d_raw, d_off, n, thr, join_search_limit(L, limit), stride, d_n, d_k, d_s, s))
        return rc;
    if (!HIP_CHECK(launch_drop_self(d_n, d_k, d_s, n, stride, first, limit, s))) return -4;
    return !wait || HIP_CHECK(hipStreamSynchronize(s)) ? 0 : -4;
}

// keys per batch of a host join: at most `want` (0: kJoinBatchKeys), and a result block within kOutBudget
uint32_t join_batch_keys(uint32_t want, uint32_t nk, uint32_t Ls) {
    const size_t fit = std::max<size_t>(1, kOutBudget / (sizeof(uint32_t) + sizeof(float)) / std::max(Ls, 1u));
    return (uint32_t)std::min<size_t>({want ? want : kJoinBatchKeys, std::max(nk, 1u), fit});
}

// What a host join runs over: one index on its first replica (OneJoin), or an index set (SetJoin,
// further down). Key ids are the source's own: an index's, or a set's global ones. The caller holds
// the lock and the guards, and the source's device is current.
struct OneJoin {
    Library& L;
    Replica& R;
    uint32_t n_keys() const { return L.host.n_keys; }
    uint32_t search_limit(uint32_t limit) const { return join_search_limit(L, limit); }
    uint64_t max_query_bytes(uint32_t first, uint32_t nk, uint32_t B) const {
        return join_max_query_bytes(L, first, nk, B);
    }
    bool blocks(CallScratch&, size_t, uint32_t) { return true; }  // (a set's members' blocks)
    // one batch into M's arrays, queued on M.stream
    int batch(CallScratch& M, uint32_t first, uint32_t n, float thr, uint32_t limit, uint32_t stride) {
        return join_batch(L, R, first, n, thr, limit, stride, M.d_raw, M.d_off, M.d_n, M.d_k, M.d_s, M.stream, false);
    }
    // the batch's similarities into d_v (the gathered queries token-sorted in place when flagged)
    int similarity(CallScratch& M, uint32_t n, uint32_t stride, float* d_v, uint32_t metric) {
        return queue_similarity(sim_view(L, R), M.d_raw, M.d_off, n, stride, M.d_n, M.d_k, M.d_s, d_v, nullptr, metric, false,
                                0.0f, M.stream, M.d_raw);
    }
};

// selfJoin / selfJoinSet behind their fronts: keys [first, first + nk) of J a batch at a time.
template <class J, class Fail>
uint32_t self_join_run(J& j, uint32_t first, uint32_t nk, float thr, uint32_t limit, uint32_t stride, uint32_t* counts,
                       uint32_t* key_ids, float* scores, Fail&& fail) {
    const uint32_t Ls = j.search_limit(limit);
    const uint32_t B = join_batch_keys(0, nk, Ls);
    // a batch's records come back packed ({key id, score bits} in row order behind the rows' offsets,
    // as ngsPackResults writes them): the bytes read back follow the records, not keys x stride
    CallScratch M;
    uint8_t* d_tmp = nullptr;
    uint32_t *d_pos = nullptr, *d_rec = nullptr;
    const size_t tmp_bytes = std::max<size_t>(pack_pairs_temp_bytes(B), 1 << 16);
    if (!M.begin(B, Ls, j.max_query_bytes(first, nk, B)) || !j.blocks(M, B, limit) || !M.alloc(&d_pos, (size_t)B + 1) ||
        !M.alloc(&d_rec, 2 * (size_t)B * Ls) || !M.alloc(&d_tmp, tmp_bytes))
        return fail(0);
    std::vector<uint32_t> h_pos((size_t)B + 1), h_rec;
    uint64_t total = 0;
    for (uint32_t done = 0; done < nk; done += B) {
        const uint32_t n = std::min(B, nk - done);
        if (j.batch(M, first + done, n, thr, limit, Ls) != 0) return fail(kErrInternal);
        if (!HIP_CHECK(launch_pack_pairs(M.d_n, M.d_k, M.d_s, n, Ls, d_pos, d_rec, d_tmp, tmp_bytes, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_pos.data(), d_pos, sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost,
                                      M.stream)) ||
            !HIP_CHECK(hipStreamSynchronize(M.stream)))
            return fail(0);
        const uint32_t recs = h_pos[n];
        h_rec.resize(2 * (size_t)recs);
        if (recs && (!HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, sizeof(uint32_t) * 2 * recs, hipMemcpyDeviceToHost,
                                               M.stream)) ||
                     !HIP_CHECK(hipStreamSynchronize(M.stream))))
            return fail(0);
        for (uint32_t i = 0; i < n; ++i) {  // (a row keeps at most min(limit, keys) <= stride records)
            const uint32_t c = h_pos[i + 1] - h_pos[i];
            const uint32_t* rec = h_rec.data() + 2 * (size_t)h_pos[i];
            uint32_t* k = key_ids + (size_t)(done + i) * stride;
            float* sc = scores + (size_t)(done + i) * stride;
            for (uint32_t r = 0; r < c; ++r) {
                k[r] = rec[2 * r];
                std::memcpy(sc + r, rec + 2 * r + 1, sizeof(float));
            }
            counts[done + i] = c;
        }
        total += recs;
    }
    if (total > 0xFFFFFFFFull) return fail((int)hipErrorInvalidValue);  // (the return value is 32-bit)
    return (uint32_t)total;
}

uint32_t self_join_host(uint32_t handle, uint32_t first, uint32_t nk, float thr, uint32_t limit, uint32_t stride,
                        uint32_t* counts, uint32_t* key_ids, float* scores) {
    if (counts) std::fill(counts, counts + nk, 0u);
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    auto fail = [&](int err) -> uint32_t {  // (counts may hold finished batches by then)
        if (err && !t_last_error) t_last_error = err;
        if (counts) std::fill(counts, counts + nk, 0u);
        return 0;
    };
    if (!L || !L->host.indexed || !counts || !join_range_ok(*L, first, nk)) return fail((int)hipErrorInvalidValue);
    const uint32_t Lm = effective_limit(*L, limit);
    if (stride < Lm || (nk && Lm && (!key_ids || !scores))) return fail((int)hipErrorInvalidValue);
    if (nk == 0 || Lm == 0) return 0;
    BatchGuard bg(L);
    Replica& R = *L->reps.front();
    if (!HIP_CHECK(hipSetDevice(R.device))) return fail(0);
    OneJoin j{*L, R};
    return self_join_run(j, first, nk, thr, limit, stride, counts, key_ids, scores, fail);
}

// the checks dedupKeys* and dedupKeysSet make before any handle is looked at
bool dedup_args_ok(uint32_t limit, uint32_t metric, float min_sim, const uint32_t* labels) {
    if (labels && limit != 0 && limit <= kRerankMaxStride && min_sim == min_sim && sim_metric_ok(metric)) return true;
    t_last_error = labels && limit > kRerankMaxStride ? kErrRerankLimit : (int)hipErrorInvalidValue;
    return false;
}

// dedupKeys* / dedupKeysSet behind their fronts: every key of J joined a batch at a time, the batches'
// records merged into one label array on the device.
template <class J>
uint32_t dedup_run(J& j, float thr, uint32_t limit, uint32_t metric, float min_sim, uint32_t batch_keys,
                   uint32_t* labels) {
    const uint32_t nk = j.n_keys();
    if (nk == 0) return 0;
    const uint32_t Ls = j.search_limit(limit);
    const uint32_t B = join_batch_keys(batch_keys, nk, Ls);
    const bool verify = min_sim > -1.0f;  // every similarity is >= -1: nothing to filter at or below it
    CallScratch M;
    uint32_t* d_lab = nullptr;
    float* d_v = nullptr;
    if (!M.begin(B, Ls, j.max_query_bytes(0, nk, B)) || !j.blocks(M, B, limit) || !M.alloc(&d_lab, nk) ||
        (verify && !M.alloc(&d_v, (size_t)B * Ls)))
        return 0;
    // the label array stays on the device across the batches: finished and read back once
    for (uint32_t done = 0; done < nk; done += B) {
        const uint32_t n = std::min(B, nk - done);
        if (j.batch(M, done, n, thr, limit, Ls) != 0) {
            if (!t_last_error) t_last_error = kErrInternal;
            return 0;
        }
        if (verify && (j.similarity(M, n, Ls, d_v, metric) != 0 ||
                       !HIP_CHECK(launch_keep_similar(M.d_n, M.d_k, M.d_s, d_v, n, Ls, min_sim, M.stream))))
            return 0;
        const uint32_t flags = (done == 0 ? kClusterInit : 0u) | (done + n == nk ? kClusterFinish : 0u);
        if (!HIP_CHECK(launch_cluster(M.d_n, M.d_k, n, Ls, done, d_lab, nk, flags, M.stream))) return 0;
    }
    if (!HIP_CHECK(hipMemcpyAsync(labels, d_lab, sizeof(uint32_t) * nk, hipMemcpyDeviceToHost, M.stream)) ||
        !HIP_CHECK(hipStreamSynchronize(M.stream)))
        return 0;
    uint32_t clusters = 0;
    for (uint32_t k = 0; k < nk; ++k) clusters += labels[k] == k;
    return clusters;
}

uint32_t dedup_host(uint32_t handle, float thr, uint32_t limit, uint32_t metric, float min_sim, uint32_t batch_keys,
                    uint32_t* labels) {
    if (!dedup_args_ok(limit, metric, min_sim, labels)) return 0;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    if (L->host.n_keys == 0) return 0;
    BatchGuard bg(L);
    Replica& R = *L->reps.front();
    if (!HIP_CHECK(hipSetDevice(R.device))) return 0;
    OneJoin j{*L, R};
    return dedup_run(j, thr, limit, metric, min_sim, batch_keys, labels);
}

// ---- linking two indexes (linkKeys) ----
constexpr uint32_t kLinkRoundsPerRead = 4;  // rounds queued between two reads of the pair count

// linkKeys: the keys of S searched in T a batch at a time (gathered on S's replica, searched and
// measured on T's first one, both on one device), then per source key the best target (kLinkBest, a
// batch's block at a time) or the greedy one-to-one matching over the whole block kept on the device
// (kLinkOneToOne, in rounds). The match, the chosen records' scores and similarities are read back once.
uint32_t link_host(uint32_t h_from, uint32_t h_to, float thr, uint32_t limit, uint32_t metric, float min_sim,
                   uint32_t mode, uint32_t batch_keys, uint32_t* match, float* scores, float* sims) {
    if (!match || limit == 0 || limit > kRerankMaxStride || min_sim != min_sim || !sim_metric_ok(metric) ||
        mode >= kLinkModes) {
        t_last_error = match && limit > kRerankMaxStride ? kErrRerankLimit : (int)hipErrorInvalidValue;
        return 0;
    }
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* S = find_lib(h_from);
    Library* T = find_lib(h_to);
    if (!S || !T || !S->host.indexed || !T->host.indexed || S->host.csize != T->host.csize) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    Replica& R = *T->reps.front();
    Replica* RS = S->replica_at(R.device);
    if (!RS) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    const uint32_t nS = S->host.n_keys, nT = T->host.n_keys;
    if (nS == 0) return 0;
    BatchGuard bg_to(T), bg_from(S == T ? nullptr : S);
    if (!HIP_CHECK(hipSetDevice(R.device))) return 0;
    const uint32_t Ls = std::max(effective_limit(*T, limit), 1u);  // (a target without keys: empty rows of one cell)
    const uint32_t B = join_batch_keys(batch_keys, nS, Ls);
    const bool verify = min_sim > -1.0f;  // every similarity is >= -1: nothing to filter at or below it
    const bool whole = mode == kLinkOneToOne;
    const uint32_t rows = whole ? nS : B;  // the block kept: every batch's, or one batch's
    CallScratch M;
    uint32_t *d_match = nullptr, *d_match_b = nullptr, *d_matched = nullptr;
    uint64_t* d_bids = nullptr;
    float *d_v = nullptr, *d_os = nullptr, *d_ov = nullptr;
    if (!M.begin(rows, Ls, join_max_query_bytes(*S, 0, nS, B)) || !M.alloc(&d_match, nS) || !M.alloc(&d_matched, 1) ||
        !M.alloc(&d_os, nS) || !M.alloc(&d_ov, nS) || (verify && !M.alloc(&d_v, (size_t)rows * Ls)) ||
        (whole && (!M.alloc(&d_match_b, nT) || !M.alloc(&d_bids, nT))))
        return 0;
    if (!whole && !HIP_CHECK(hipMemsetAsync(d_matched, 0, sizeof(uint32_t), M.stream))) return 0;
    for (uint32_t done = 0; done < nS; done += B) {
        const uint32_t n = std::min(B, nS - done);
        const size_t at = whole ? (size_t)done : 0;
        uint32_t *d_n = M.d_n + at, *d_k = M.d_k + at * Ls;
        float *d_s = M.d_s + at * Ls, *d_sim = verify ? d_v + at * Ls : nullptr;
        if (!HIP_CHECK(launch_key_queries(RS->dev, done, n, join_query_bytes(*S, done, n), M.d_raw, M.d_off, M.stream)))
            return 0;
        if (search_on_replica(*T, R, M.d_raw, M.d_off, n, thr, effective_limit(*T, limit), Ls, d_n, d_k, d_s,
                              M.stream) != 0) {
            if (!t_last_error) t_last_error = kErrInternal;
            return 0;
        }
        if (verify && (queue_similarity(sim_view(*T, R), M.d_raw, M.d_off, n, Ls, d_n, d_k, d_s, d_sim, nullptr, metric, false,
                                        0.0f, M.stream, M.d_raw) != 0 ||
                       !HIP_CHECK(launch_keep_similar(d_n, d_k, d_s, d_sim, n, Ls, min_sim, M.stream, d_sim))))
            return 0;
        if (!whole && (!HIP_CHECK(launch_match_best(d_n, d_k, verify ? d_sim : d_s, n, Ls, done, d_match, nS, nT,
                                                    d_matched, M.stream)) ||
                       !HIP_CHECK(launch_match_gather(d_n, d_k, d_s, d_sim, n, Ls, done, d_match, nS, d_os, d_ov,
                                                      M.stream))))
            return 0;
    }
    uint32_t matched = 0;
    auto read_matched = [&](uint32_t& out) {
        return HIP_CHECK(hipMemcpyAsync(&out, d_matched, sizeof(uint32_t), hipMemcpyDeviceToHost, M.stream)) &&
               HIP_CHECK(hipStreamSynchronize(M.stream));
    };
    if (whole) {
        // rounds until one adds nothing: a round on a complete matching changes nothing, so a few are
        // queued per read of the count
        const float* d_val = verify ? d_v : M.d_s;
        uint32_t flags = kMatchFlags;  // INIT with the first round
        for (uint32_t before = kNoMatch; matched != before;) {
            before = matched;
            for (uint32_t r = 0; r < kLinkRoundsPerRead; ++r, flags &= ~kMatchInit)
                if (!HIP_CHECK(launch_match(M.d_n, M.d_k, d_val, nS, Ls, 0, d_match, nS, d_match_b, nT, d_bids,
                                            d_matched, flags, M.stream)))
                    return 0;
            if (!read_matched(matched)) return 0;
        }
        if (!HIP_CHECK(launch_match_gather(M.d_n, M.d_k, M.d_s, d_v, nS, Ls, 0, d_match, nS, d_os, d_ov, M.stream)))
            return 0;
    }
    std::vector<uint32_t> h_match(nS);
    std::vector<float> h_os(scores ? nS : 0), h_ov(sims ? nS : 0);
    if (!HIP_CHECK(hipMemcpyAsync(h_match.data(), d_match, sizeof(uint32_t) * nS, hipMemcpyDeviceToHost, M.stream)) ||
        (scores && !HIP_CHECK(hipMemcpyAsync(h_os.data(), d_os, sizeof(float) * nS, hipMemcpyDeviceToHost, M.stream))) ||
        (sims && !HIP_CHECK(hipMemcpyAsync(h_ov.data(), d_ov, sizeof(float) * nS, hipMemcpyDeviceToHost, M.stream))) ||
        !read_matched(matched))
        return 0;
    std::copy(h_match.begin(), h_match.end(), match);
    if (scores) std::copy(h_os.begin(), h_os.end(), scores);
    if (sims) std::copy(h_ov.begin(), h_ov.end(), sims);
    return matched;
}

// ---- index sets (ngsSet* / scoreBatchSet*) ----

// A set names its members and owns their key-length tables on its device; the members stay their
// own (Library::serial tells a member from a later index under the same handle id).
struct KeySet {
    struct Member {
        uint32_t handle = 0;
        uint64_t serial = 0;
        uint32_t base = 0, n_keys = 0;
        uint32_t* d_len = nullptr;  // [n_keys] on `device`
        // the dead mask (§9.9), one bit a key: made by the member's first ngsSetRemove, the device's
        // copy equal to the host's whenever the exclusive lock is released
        std::vector<uint32_t> dead;
        uint32_t* d_dead = nullptr;
        uint32_t n_dead = 0;
    };
    std::vector<Member> parts;
    int device = 0;
    uint32_t csize = 0, gsz = 0;
    uint64_t n_keys = 0, n_dead = 0;
    // ngsSetDeadStats: searches count under the shared lock
    mutable std::atomic<uint64_t> drop_launches{0}, re_searches{0}, max_fetch{0};
    ~KeySet() {
        for (Member& m : parts) {
            if (m.d_len) (void)hipFree(m.d_len);
            if (m.d_dead) (void)hipFree(m.d_dead);
        }
    }
};
std::unordered_map<uint32_t, std::unique_ptr<KeySet>> g_sets;  // a namespace of its own (under g_lock)

// The set and its members' libraries (the caller holds the lock): -1 for an unknown set or a member
// that has been disposed, whoever holds its handle id now.
int entry_set(uint32_t set, KeySet*& S, Library** libs) {
    auto it = g_sets.find(set);
    if (it == g_sets.end()) return -1;
    S = it->second.get();
    for (size_t p = 0; p < S->parts.size(); ++p) {
        Library* L = find_lib(S->parts[p].handle);
        if (!L || L->serial != S->parts[p].serial) return -1;
        libs[p] = L;
    }
    return 0;
}

// `handle` appended to S under the exclusive lock: 0, -3 a condition fails, -4 HIP error. The
// member's key lengths are computed on the set's device before this returns.
int set_join(KeySet& S, uint32_t handle) {
    Library* L = find_lib(handle);
    if (S.parts.size() >= kSetMaxParts || !L || !L->host.indexed || L->reps.empty()) return -3;
    const bool first = S.parts.empty();
    const int device = first ? L->reps.front()->device : S.device;
    Replica* R = L->replica_at(device);
    if (!R || (!first && (L->host.csize != S.csize || L->host.gsz != S.gsz)) ||
        S.n_keys + L->host.n_keys > 0xFFFFFFFFull)
        return -3;
    int cur = -1;
    (void)hipGetDevice(&cur);
    KeySet::Member m;
    m.handle = handle;
    m.serial = L->serial;
    m.base = (uint32_t)S.n_keys;
    m.n_keys = L->host.n_keys;
    const bool ok = HIP_CHECK(hipSetDevice(device)) && dev_alloc(&m.d_len, m.n_keys) &&
                    HIP_CHECK(launch_key_len(R->dev.key_off, 0, m.n_keys, m.d_len, nullptr)) &&
                    HIP_CHECK(hipStreamSynchronize(nullptr));
    if (cur >= 0) (void)hipSetDevice(cur);
    if (!ok) {
        if (m.d_len) (void)hipFree(m.d_len);
        return -4;
    }
    if (first) {
        S.device = device;
        S.csize = L->host.csize;
        S.gsz = L->host.gsz;
    }
    S.n_keys += m.n_keys;
    S.parts.push_back(m);
    return 0;
}

uint32_t set_effective_limit(const KeySet& S, uint32_t limit) {
    return (uint32_t)std::min<uint64_t>(set_limit(limit), S.n_keys);
}

// The members' blocks of a set search of up to `rows` queries at `limit`, in M: member p's has the
// stride min(L, nKeys_p); a member with dead keys (§9.9) the stride of its first over-fetch (0 when
// all its keys are dead), and the set then has the members' short-row counters too (a set without
// dead keys allocates what it did before).
struct SetBlocks {
    MergeParts parts{};
    uint64_t records = 0;  // per query, all members
    size_t rows = 0;
    uint32_t cap[kSetMaxParts] = {};  // the records a row of member p's block has room for
    uint32_t* d_short = nullptr;      // [kSetMaxParts]
};
// the stride member p's block starts with: min(L, nKeys_p), or that of its first over-fetch
uint32_t set_first_stride(const KeySet& S, Library* const* libs, size_t p, uint32_t limit) {
    const uint32_t d = S.parts[p].n_dead, L = set_limit(limit);
    if (d && d == S.parts[p].n_keys) return 0;  // wholly dead: never searched, no records
    return d ? dead_fetch_stride(L, dead_first_fetch(d, L), S.parts[p].n_keys) : effective_limit(*libs[p], limit);
}
bool set_blocks(CallScratch& M, const KeySet& S, Library* const* libs, size_t rows, uint32_t limit, SetBlocks& K) {
    K.rows = rows;
    for (size_t p = 0; p < S.parts.size(); ++p) {
        MergePart& B = K.parts.p[p];
        B.stride = set_first_stride(S, libs, p, limit);
        B.base = S.parts[p].base;
        B.n_keys = S.parts[p].n_keys;
        B.len = S.parts[p].d_len;
        K.cap[p] = B.stride;
        K.records += B.stride;
    }
    if (!S.n_dead) {  // (as before dead keys existed: three allocations a member)
        for (size_t p = 0; p < S.parts.size(); ++p) {
            MergePart& B = K.parts.p[p];
            uint32_t *d_n = nullptr, *d_k = nullptr;
            float* d_s = nullptr;
            if (!M.alloc(&d_n, rows) || !M.alloc(&d_k, rows * B.stride) || !M.alloc(&d_s, rows * B.stride)) return false;
            B.counts = d_n;
            B.keys = d_k;
            B.scores = d_s;
        }
        return true;
    }
    // With dead keys the blocks are wider, and an allocation of 2 MiB and more was measured at some
    // 0.18 ms each (§9.9): all blocks and the short counters are cut from one allocation, every
    // array starting at a multiple of 256 bytes.
    auto pad = [](size_t words) { return (words + 63u) & ~size_t(63); };
    size_t words = pad(kSetMaxParts);
    for (size_t p = 0; p < S.parts.size(); ++p) words += pad(rows) + 2 * pad(rows * K.parts.p[p].stride);
    uint32_t* slab = nullptr;
    if (!M.alloc(&slab, words)) return false;
    K.d_short = slab;
    slab += pad(kSetMaxParts);
    for (size_t p = 0; p < S.parts.size(); ++p) {
        MergePart& B = K.parts.p[p];
        const size_t recs = pad(rows * B.stride);
        B.counts = slab;
        B.keys = slab + pad(rows);
        B.scores = reinterpret_cast<float*>(slab + pad(rows) + recs);
        slab += pad(rows) + 2 * recs;
    }
    return true;
}

// Every member's BatchGuard, held from before the first member's search until the merge has run: no
// member's server kernel is relaunched in between, so neither a later member's kernels nor the merge
// queue behind one on a shared hardware queue.
struct SetGuards {
    std::unique_ptr<BatchGuard> g[kSetMaxParts];
    SetGuards(const KeySet& S, Library* const* libs) {
        for (size_t p = 0; p < S.parts.size(); ++p) g[p] = std::make_unique<BatchGuard>(libs[p]);
    }
};

// ngsSetSearchDevice's work (the shared lock and the members' SetGuards held, the set's device
// current): every member searched into its block, one after another, then the merge queued on s.
// Nothing waits for the merge.
// With dead keys (§9.9) a member that has some is searched at L + E_p into a block of stride
// min(L + E_p, nKeys_p), and one k_drop_dead launch over those members cuts their rows to L before
// the merge. The members' short-row counters are read back once a round (the one extra wait, taken
// only when the set has dead keys): a member with short rows whose stride was below both L + d_p and
// nKeys_p is searched again with a larger E_p, into a larger block from M where it needs one.
int set_search(const KeySet& S, Library* const* libs, CallScratch& M, SetBlocks& K, const uint8_t* d_raw,
               const uint64_t* d_off, uint32_t n, float thr, uint32_t limit, uint32_t out_stride, uint32_t* d_n,
               uint32_t* d_k, float* d_s, hipStream_t s) {
    const uint32_t P = (uint32_t)S.parts.size(), L = set_limit(limit);
    auto search = [&](uint32_t p) {
        Replica* R = libs[p]->replica_at(S.device);
        if (!R) return -3;
        const MergePart& B = K.parts.p[p];
        return search_on_replica(*libs[p], *R, d_raw, d_off, n, thr, B.stride, B.stride, const_cast<uint32_t*>(B.counts),
                                 const_cast<uint32_t*>(B.keys), const_cast<float*>(B.scores), s);
    };
    auto fetched = [&](uint32_t E) {  // ngsSetDeadStats: the largest over-fetch used
        uint64_t seen = S.max_fetch.load(std::memory_order_relaxed);
        while (seen < E && !S.max_fetch.compare_exchange_weak(seen, E, std::memory_order_relaxed)) {
        }
    };
    uint32_t E[kSetMaxParts] = {}, todo = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t d = S.parts[p].n_dead;
        if (d && d == S.parts[p].n_keys) {  // wholly dead: it can give no record, so it is not searched
            if (!HIP_CHECK(hipMemsetAsync(const_cast<uint32_t*>(K.parts.p[p].counts), 0, sizeof(uint32_t) * n, s))) return -4;
            continue;
        }
        if (d) {
            E[p] = dead_first_fetch(d, L);
            K.parts.p[p].stride = dead_fetch_stride(L, E[p], S.parts[p].n_keys);  // (<= K.cap[p]: set_blocks)
            fetched(E[p]);
            todo |= 1u << p;
        }
        if (const int rc = search(p)) return rc;
    }
    while (todo) {
        DropBlocks D{};
        uint32_t nb = 0, h_short[kSetMaxParts] = {};
        for (uint32_t p = 0; p < P; ++p) {
            if (!(todo >> p & 1u)) continue;
            const MergePart& B = K.parts.p[p];
            D.b[nb++] = DropBlock{const_cast<uint32_t*>(B.counts), const_cast<uint32_t*>(B.keys),
                                  const_cast<float*>(B.scores), S.parts[p].d_dead, K.d_short + p, B.stride, B.n_keys};
        }
        if (!HIP_CHECK(hipMemsetAsync(K.d_short, 0, sizeof h_short, s)) || !HIP_CHECK(launch_drop_dead(D, nb, n, limit, s)) ||
            !HIP_CHECK(hipMemcpyAsync(h_short, K.d_short, sizeof h_short, hipMemcpyDeviceToHost, s)) ||
            !HIP_CHECK(hipStreamSynchronize(s)))
            return -4;
        S.drop_launches.fetch_add(1, std::memory_order_relaxed);
        uint32_t again = 0;
        for (uint32_t p = 0; p < P; ++p) {
            if (!(todo >> p & 1u)) continue;
            MergePart& B = K.parts.p[p];
            const uint32_t d = S.parts[p].n_dead;
            if (!h_short[p] || B.stride >= dead_fetch_stride(L, d, B.n_keys)) continue;
            E[p] = dead_next_fetch(d, E[p]);
            B.stride = dead_fetch_stride(L, E[p], B.n_keys);
            if (B.stride > K.cap[p]) {
                uint32_t* keys = nullptr;
                float* scores = nullptr;
                if (!M.alloc(&keys, K.rows * B.stride) || !M.alloc(&scores, K.rows * B.stride)) return -4;
                B.keys = keys;
                B.scores = scores;
                K.cap[p] = B.stride;
            }
            fetched(E[p]);
            S.re_searches.fetch_add(1, std::memory_order_relaxed);
            if (const int rc = search(p)) return rc;
            again |= 1u << p;
        }
        todo = again;
    }
    return HIP_CHECK(launch_merge_parts(K.parts, P, n, limit, out_stride, d_n, d_k, d_s, s)) ? 0 : -4;
}

static_assert(kSetDeadFastLimit == kWaveMaxLimit, "the first over-fetch fills tier 1's limit");

// The rows of a join over keys [first, first + n) whose own key is dead emptied (§9.9), queued on s;
// nothing is launched for a set without dead keys.
bool set_zero_dead_rows(const KeySet& S, uint32_t* d_n, uint32_t n, uint32_t first, hipStream_t s) {
    if (!S.n_dead) return true;
    DeadMasks D{};
    for (size_t p = 0; p < S.parts.size(); ++p) {
        D.dead[p] = S.parts[p].n_dead ? S.parts[p].d_dead : nullptr;
        D.base[p] = S.parts[p].base;
        D.n_keys[p] = S.parts[p].n_keys;
    }
    return HIP_CHECK(launch_zero_dead_rows(D, (uint32_t)S.parts.size(), d_n, n, first, s));
}

// ngsSetRemove (dead = true) / ngsSetRestore under the exclusive lock: every id checked before
// anything changes, the bits flipped in copies of the touched members' masks, the copies uploaded,
// and only then kept. No search is in flight (each holds the shared lock until its results are
// complete), so the device's masks change between two searches.
int set_mark(uint32_t set, const uint32_t* ids, uint32_t n, bool dead) {
    std::unique_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (n && !ids) return -3;
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= S->n_keys) return -3;
    const size_t P = S->parts.size();
    std::vector<std::vector<uint32_t>> next(P);
    std::vector<uint32_t> changed(P, 0);
    for (uint32_t i = 0; i < n; ++i) {
        size_t p = P - 1;  // (as ngsSetLocate)
        while (S->parts[p].base > ids[i]) --p;
        KeySet::Member& m = S->parts[p];
        if (next[p].empty()) {
            next[p] = m.dead;
            next[p].resize(((size_t)m.n_keys + 31u) / 32u, 0u);
        }
        const uint32_t k = ids[i] - m.base, bit = 1u << (k & 31u);
        if (((next[p][k >> 5] & bit) != 0u) == dead) continue;
        next[p][k >> 5] ^= bit;
        ++changed[p];
    }
    int cur = -1;
    (void)hipGetDevice(&cur);
    bool ok = HIP_CHECK(hipSetDevice(S->device));
    size_t done = 0;
    for (; ok && done < P; ++done) {
        KeySet::Member& m = S->parts[done];
        if (!changed[done]) continue;
        ok = (m.d_dead || dev_alloc(&m.d_dead, next[done].size())) &&
             HIP_CHECK(hipMemcpy(m.d_dead, next[done].data(), sizeof(uint32_t) * next[done].size(), hipMemcpyHostToDevice));
    }
    if (!ok)  // the masks already uploaded go back to what the host keeps
        for (size_t p = 0; p < done; ++p)
            if (changed[p] && S->parts[p].d_dead && !S->parts[p].dead.empty())
                (void)hipMemcpy(S->parts[p].d_dead, S->parts[p].dead.data(), sizeof(uint32_t) * S->parts[p].dead.size(),
                                hipMemcpyHostToDevice);
    if (cur >= 0) (void)hipSetDevice(cur);
    if (!ok) return -4;
    uint32_t total = 0;
    for (size_t p = 0; p < P; ++p) {
        if (!changed[p]) continue;
        KeySet::Member& m = S->parts[p];
        m.dead.swap(next[p]);
        m.n_dead = dead ? m.n_dead + changed[p] : m.n_dead - changed[p];
        total += changed[p];
    }
    S->n_dead = dead ? S->n_dead + total : S->n_dead - total;
    return (int)std::min<uint32_t>(total, kInt32Max);
}

// ---- the later stages over a set (ngsSetSimilarityDeviceM .. dedupKeysSet) ----

// The current device is the set's: -4 no device, -3 another one (the caller's buffers and stream
// belong to the current one).
int set_device_current(const KeySet& S) {
    int cur = -1;
    if (!HIP_CHECK(hipGetDevice(&cur))) return -4;
    return cur == S.device ? 0 : -3;
}

// the similarity's view of a set: its members on the set's device, one launch of k_sim_set for a block
SimView sim_view(const KeySet& S, Library* const* libs) {
    SimView V{{}, (uint32_t)S.parts.size(), S.csize, true};
    for (uint32_t p = 0; p < V.P; ++p) V.m[p] = {libs[p], libs[p]->replica_at(S.device), S.parts[p].base};
    return V;
}

// f(p, local first key, keys, position in the range) for every member holding keys of the global
// range [first, first + n), in order
template <class F>
void set_segments(const KeySet& S, uint32_t first, uint32_t n, F&& f) {
    const uint64_t end = (uint64_t)first + n;
    for (size_t p = 0; p < S.parts.size(); ++p) {
        const uint64_t base = S.parts[p].base;
        const uint64_t a = std::max<uint64_t>(first, base), b = std::min<uint64_t>(end, base + S.parts[p].n_keys);
        if (a < b) f(p, (uint32_t)(a - base), (uint32_t)(b - a), (uint32_t)(a - first));
    }
}
bool set_range_ok(const KeySet& S, uint32_t first, uint32_t n) { return (uint64_t)first + n <= S.n_keys; }
uint64_t set_query_bytes(const KeySet& S, Library* const* libs, uint32_t first, uint32_t n) {
    uint64_t bytes = 0;
    set_segments(S, first, n, [&](size_t p, uint32_t k0, uint32_t nk, uint32_t) {
        bytes += join_query_bytes(*libs[p], k0, nk);
    });
    return bytes;
}
uint64_t set_max_query_bytes(const KeySet& S, Library* const* libs, uint32_t first, uint32_t nk, uint32_t B) {
    uint64_t most = 0;
    for (uint32_t k0 = first; k0 < first + nk; k0 += B)
        most = std::max(most, set_query_bytes(S, libs, k0, std::min(B, first + nk - k0)));
    return most;
}
// join_search_limit over the set's keys
uint32_t set_join_limit(const KeySet& S, uint32_t limit) {
    return (uint32_t)std::min<uint64_t>((uint64_t)(limit ? limit : kInt32Max) + 1u, S.n_keys);
}

// The keys of the global range as one query batch in ngsKeyQueriesDevice's layout: each member's
// keys gathered behind the earlier members' bytes, its offsets (written from 0) moved up by them.
// A member's first offset is its predecessor's last; the stream orders the two writes.
bool set_key_queries(const KeySet& S, Library* const* libs, uint32_t first, uint32_t n, uint8_t* d_raw,
                     uint64_t* d_off, hipStream_t s) {
    if (n == 0) return HIP_CHECK(hipMemsetAsync(d_off, 0, sizeof(uint64_t), s));
    uint64_t at = 0;
    bool ok = true;
    set_segments(S, first, n, [&](size_t p, uint32_t k0, uint32_t nk, uint32_t i0) {
        Replica* R = libs[p]->replica_at(S.device);
        if (!ok || !R) {
            ok = false;
            return;
        }
        const uint64_t bytes = join_query_bytes(*libs[p], k0, nk);
        ok = HIP_CHECK(launch_key_queries(R->dev, k0, nk, bytes, d_raw + at, d_off + i0, s)) &&
             HIP_CHECK(launch_shift_offsets(d_off + i0, (uint64_t)nk + 1u, at, s));
        at += bytes;
    });
    return ok;
}

// join_batch over a set (its device current, the lock and the members' guards held): the gather, the
// set search with one record more, the key's own record dropped by its global id.
int set_join_batch(const KeySet& S, Library* const* libs, CallScratch& M, SetBlocks& K, uint32_t first, uint32_t n, float thr,
                   uint32_t limit, uint32_t stride, uint8_t* d_raw, uint64_t* d_off, uint32_t* d_n, uint32_t* d_k,
                   float* d_s, hipStream_t s, bool wait) {
    if (!set_key_queries(S, libs, first, n, d_raw, d_off, s)) return -4;
    if (const int rc = set_search(S, libs, M, K, d_raw, d_off, n, thr, set_join_limit(S, limit), stride, d_n, d_k, d_s, s))
        return rc;
    if (!HIP_CHECK(launch_drop_self(d_n, d_k, d_s, n, stride, first, limit, s)) || !set_zero_dead_rows(S, d_n, n, first, s))
        return -4;
    return !wait || HIP_CHECK(hipStreamSynchronize(s)) ? 0 : -4;
}

// OneJoin's counterpart: key ids are the set's global ones, a batch may span members.
struct SetJoin {
    const KeySet& S;
    Library* const* libs;
    SetBlocks K{};
    uint32_t n_keys() const { return (uint32_t)S.n_keys; }
    uint32_t search_limit(uint32_t limit) const { return set_join_limit(S, limit); }
    uint64_t max_query_bytes(uint32_t first, uint32_t nk, uint32_t B) const {
        return set_max_query_bytes(S, libs, first, nk, B);
    }
    bool blocks(CallScratch& M, size_t rows, uint32_t limit) { return set_blocks(M, S, libs, rows, search_limit(limit), K); }
    int batch(CallScratch& M, uint32_t first, uint32_t n, float thr, uint32_t limit, uint32_t stride) {
        return set_join_batch(S, libs, M, K, first, n, thr, limit, stride, M.d_raw, M.d_off, M.d_n, M.d_k, M.d_s, M.stream,
                              false);
    }
    int similarity(CallScratch& M, uint32_t n, uint32_t stride, float* d_v, uint32_t metric) {
        return queue_similarity(sim_view(S, libs), M.d_raw, M.d_off, n, stride, M.d_n, M.d_k, M.d_s, d_v, nullptr, metric, false,
                                    0.0f, M.stream, M.d_raw);
    }
};

// scoreBatchSetSimM*'s part of set_batch: the re-rank by `metric` behind the set search, the
// similarities and (terms != null) the members' matched term ids read back in the records' layout
struct SetSim {
    uint32_t metric;
    float min_sim;
    float* sims;
    uint32_t* terms;
};

// scoreBatchSet / scoreBatchSetW / scoreBatchSetU8: the queries packed and uploaded a chunk at a time
// (u8: as UTF-8, decoded on the device like a large scoreBatchU8 batch), the set search, the merged
// block read back into the caller's arrays. With `sim` (scoreBatchSetSimM*) the similarity and the
// re-rank run between the two, on the call's own copy of the queries.
template <typename CharT>
uint32_t set_batch(uint32_t set, const CharT* const* queries, uint32_t nq, float thr, uint32_t limit, uint32_t stride,
                   uint32_t* counts, uint32_t* key_ids, float* scores, bool u8, const SetSim* sim = nullptr) {
    if (counts) std::fill(counts, counts + nq, 0u);
    auto fail = [&](int err) -> uint32_t {  // (counts may hold finished chunks by then)
        if (err && !t_last_error) t_last_error = err;
        if (counts) std::fill(counts, counts + nq, 0u);
        return 0;
    };
    if (!counts || (nq && !queries)) return fail((int)hipErrorInvalidValue);
    if (sim && (sim->min_sim != sim->min_sim || !sim_metric_ok(sim->metric))) return fail((int)hipErrorInvalidValue);
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (entry_set(set, S, libs) != 0) return fail((int)hipErrorInvalidValue);
    const uint32_t cs = u8 ? (uint32_t)sizeof(uint32_t) : (uint32_t)sizeof(CharT);
    const uint32_t Lm = set_effective_limit(*S, limit);
    if (S->csize != cs || stride < Lm || (nq && Lm && (!key_ids || !scores || (sim && !sim->sims))))
        return fail((int)hipErrorInvalidValue);
    if (sim && Lm > kRerankMaxStride) return fail(kErrRerankLimit);
    if (nq == 0 || Lm == 0) return 0;
    if (!HIP_CHECK(hipSetDevice(S->device))) return fail(0);
    SetGuards guards(*S, libs);
    uint64_t per_query = 0;
    for (size_t p = 0; p < S->parts.size(); ++p) per_query += set_first_stride(*S, libs, p, limit);  // (the blocks' strides)
    const uint32_t chunk =
        (uint32_t)std::min<uint64_t>(nq, std::max<uint64_t>(1, kSimChunkRecords / std::max<uint64_t>(per_query, 1)));
    // every query's bytes as they go up (u8: the UTF-8 bytes), and the bytes of the largest chunk
    const uint32_t up = u8 ? 1u : cs;  // bytes per unit of what is uploaded
    QueryChunks Q(nq, chunk, [&](uint32_t i, size_t& bytes) -> const void* {
        bytes = queries[i] ? str_len(queries[i]) * up : 0;
        return queries[i];
    });
    const size_t raw_cap = Q.raw_cap;
    CallScratch M;
    SetBlocks K;
    uint8_t *d_u8 = nullptr, *d_u8temp = nullptr;
    uint64_t* d_u8off = nullptr;
    const size_t u8temp = u8 ? utf8_temp_bytes(chunk) : 0;
    const size_t recs = (size_t)chunk * Lm;
    float* d_v = nullptr;
    uint32_t* d_t = nullptr;
    if (!M.begin(chunk, Lm, u8 ? 4 * raw_cap : raw_cap) || !set_blocks(M, *S, libs, chunk, limit, K) ||
        (u8 && (!M.alloc(&d_u8, raw_cap + 16) || !M.alloc(&d_u8off, (size_t)chunk + 1) || !M.alloc(&d_u8temp, u8temp))) ||
        (sim && (!M.alloc(&d_v, recs) || (sim->terms && !M.alloc(&d_t, recs)))))
        return fail(0);
    std::vector<uint32_t> h_n(chunk), h_k(recs), h_t(d_t ? recs : 0);
    std::vector<float> h_s(recs), h_v(sim ? recs : 0);
    uint64_t total = 0;
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t B = std::min(chunk, nq - q0);
        if (!Q.upload(q0, B, u8 ? d_u8off : M.d_off, u8 ? d_u8 : M.d_raw, M.stream) ||
            (u8 && !HIP_CHECK(launch_utf8_decode(d_u8, d_u8off, B, reinterpret_cast<uint32_t*>(M.d_raw), raw_cap,
                                                 M.d_off, d_u8temp, u8temp, M.stream))))
            return fail(0);
        if (set_search(*S, libs, M, K, M.d_raw, M.d_off, B, thr, limit, Lm, M.d_n, M.d_k, M.d_s, M.stream) != 0)
            return fail(kErrInternal);
        if (sim && queue_similarity(sim_view(*S, libs), M.d_raw, M.d_off, B, Lm, M.d_n, M.d_k, M.d_s, d_v, d_t, sim->metric, true,
                                        sim->min_sim, M.stream, M.d_raw) != 0)
            return fail(kErrInternal);
        const size_t rb = (size_t)B * Lm;
        if (!HIP_CHECK(hipMemcpyAsync(h_n.data(), M.d_n, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_k.data(), M.d_k, sizeof(uint32_t) * rb, hipMemcpyDeviceToHost, M.stream)) ||
            !HIP_CHECK(hipMemcpyAsync(h_s.data(), M.d_s, sizeof(float) * rb, hipMemcpyDeviceToHost, M.stream)) ||
            (sim && !HIP_CHECK(hipMemcpyAsync(h_v.data(), d_v, sizeof(float) * rb, hipMemcpyDeviceToHost, M.stream))) ||
            (d_t && !HIP_CHECK(hipMemcpyAsync(h_t.data(), d_t, sizeof(uint32_t) * rb, hipMemcpyDeviceToHost, M.stream))) ||
            !HIP_CHECK(hipStreamSynchronize(M.stream)))
            return fail(0);
        for (uint32_t i = 0; i < B; ++i) {
            const uint32_t c = std::min(h_n[i], Lm);
            std::copy_n(h_k.begin() + (size_t)i * Lm, c, key_ids + (size_t)(q0 + i) * stride);
            std::copy_n(h_s.begin() + (size_t)i * Lm, c, scores + (size_t)(q0 + i) * stride);
            if (sim) std::copy_n(h_v.begin() + (size_t)i * Lm, c, sim->sims + (size_t)(q0 + i) * stride);
            if (d_t) std::copy_n(h_t.begin() + (size_t)i * Lm, c, sim->terms + (size_t)(q0 + i) * stride);
            counts[q0 + i] = c;
            total += c;
        }
    }
    if (total > 0xFFFFFFFFull) return fail((int)hipErrorInvalidValue);  // (the return value is 32-bit)
    return (uint32_t)total;
}

// A scan's scratch: one grow-only buffer per (device, stream), 64 KiB at first, so that calls on
// different streams never share one while their scans run; a buffer is replaced only after its
// stream's earlier work has finished with it. The caller holds mu from get() until its kernels are
// queued (the mutex orders the host-side bookkeeping only). Each user keeps an instance of its
// own: two users' kernels may be queued on one stream at once.
struct StreamScratch {
    std::mutex mu;
    std::map<std::pair<int, hipStream_t>, std::pair<void*, size_t>> temp;
    // {buffer, its bytes >= need}; {null, 0} after a HIP error
    std::pair<void*, size_t> get(int dev, hipStream_t s, size_t need) {
        auto& t = temp[{dev, s}];
        if (need > t.second) {
            if (t.first && !HIP_CHECK(hipStreamSynchronize(s))) return {nullptr, 0};
            if (t.first) (void)hipFree(t.first);
            t = {nullptr, 0};
            if (!HIP_CHECK(hipMalloc(&t.first, std::max<size_t>(need, 1 << 16)))) return {nullptr, 0};
            t.second = std::max<size_t>(need, 1 << 16);
        }
        return t;
    }
};
}  // namespace
}  // namespace ngs

extern "C" {

NGS_API uint32_t indexN(char** words, uint64_t size, uint16_t rowSize, float* weight) {
    return new_library([&](HostIndex& H) { build_index(H, words, size, rowSize, weight); });
}

NGS_API uint32_t indexG(char** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize) {
    if (gSize < 1 || gSize > kMaxGramSize) return 0;
    return new_library([&](HostIndex& H) { build_index_g(H, words, size, rowSize, weight, gSize); });
}

NGS_API uint32_t indexW(wchar_t** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize) {
    static_assert(sizeof(wchar_t) == 4, "wide strings are UTF-32");
    if (gSize < 1 || gSize > kMaxGramSize) return 0;
    return new_library([&](HostIndex& H) {
        build_index_w(H, reinterpret_cast<const uint32_t* const*>(words), size, rowSize, weight, gSize);
    });
}

NGS_API uint32_t search(uint32_t handle, const char* query, char*** results, float threshold, uint32_t limit) {
    return one_query(handle, query, results, nullptr, threshold, limit);
}

NGS_API uint32_t score(uint32_t handle, const char* query, char*** results, float** scores, float threshold,
                       uint32_t limit) {
    return one_query(handle, query, results, scores, threshold, limit);
}

NGS_API void release(uint32_t handle, char** results, float* scores) {
    std::shared_lock<std::shared_mutex> lk(g_lock);  // dllmain.cpp:100-103
    if (!find_lib(handle)) return;
    delete[] results;
    delete[] scores;
}

NGS_API void dispose(uint32_t handle) {
    std::unique_lock<std::shared_mutex> lk(g_lock);  // dllmain.cpp:112-113
    g_libs.erase(handle);
}

NGS_API uint64_t getSize(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? L->host.n_terms : 0;
}

NGS_API uint64_t getLibSize(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? L->host.n_grams : 0;
}

NGS_API void setValidChar(uint32_t handle, char* characters, int n) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (L && (characters || n == 0)) set_valid(*L, characters, n);
}

NGS_API uint32_t scoreBatch(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                            uint32_t limit, uint32_t* counts, char*** results, float** scores) {
    return batch_query(handle, queries, nQueries, threshold, limit, counts, results, scores);
}

NGS_API uint32_t searchBatch(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                             uint32_t limit, uint32_t* counts, char*** results) {
    return batch_query(handle, queries, nQueries, threshold, limit, counts, results, nullptr);
}

// ---- wide (UTF-32 wchar_t) API: Readme.md:91,135,170,190,208,226, keyed by handle like the
// narrow exports (dllmain.cpp). Valid only on indexW handles; narrow calls on a wide handle
// and wide calls on a narrow handle return 0 / nothing.

NGS_API uint32_t searchW(uint32_t handle, const wchar_t* query, wchar_t*** results, float threshold,
                         uint32_t limit) {
    return one_query(handle, query, results, nullptr, threshold, limit);
}

NGS_API uint32_t scoreW(uint32_t handle, const wchar_t* query, wchar_t*** results, float** scores,
                        float threshold, uint32_t limit) {
    return one_query(handle, query, results, scores, threshold, limit);
}

NGS_API uint32_t scoreBatchW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                             uint32_t limit, uint32_t* counts, wchar_t*** results, float** scores) {
    return batch_query(handle, queries, nQueries, threshold, limit, counts, results, scores);
}

NGS_API uint32_t searchBatchW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                              uint32_t limit, uint32_t* counts, wchar_t*** results) {
    return batch_query(handle, queries, nQueries, threshold, limit, counts, results, nullptr);
}

NGS_API void releaseW(uint32_t handle, wchar_t** results, float* scores) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    if (!find_lib(handle)) return;
    delete[] results;
    delete[] scores;
}

NGS_API void disposeW(uint32_t handle) { dispose(handle); }

NGS_API uint64_t getSizeW(uint32_t handle) { return getSize(handle); }

NGS_API uint64_t getLibSizeW(uint32_t handle) { return getLibSize(handle); }

// ---- UTF-8 API on wide indexes (include/ngram_search.h): strings in and out are UTF-8, the
// index and the search are the wide ones.

NGS_API uint32_t indexU8(char** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize) {
    if (gSize < 1 || gSize > kMaxGramSize) return 0;
    DecodedStrings D;
    if (words) decode_strings(words, size, D);
    return new_library([&](HostIndex& H) {
        build_index_w(H, words ? D.ptr.data() : nullptr, size, rowSize, weight, gSize);
    });
}

NGS_API uint32_t searchU8(uint32_t handle, const char* query, char*** results, float threshold, uint32_t limit) {
    return u8_query(handle, &query, 1, threshold, limit, nullptr, results, nullptr);
}

NGS_API uint32_t scoreU8(uint32_t handle, const char* query, char*** results, float** scores, float threshold,
                         uint32_t limit) {
    return u8_query(handle, &query, 1, threshold, limit, nullptr, results, scores);
}

NGS_API uint32_t scoreBatchU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                              uint32_t limit, uint32_t* counts, char*** results, float** scores) {
    if (!counts) return 0;
    return u8_query(handle, queries, nQueries, threshold, limit, counts, results, scores);
}

NGS_API uint32_t searchBatchU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, uint32_t* counts, char*** results) {
    if (!counts) return 0;
    return u8_query(handle, queries, nQueries, threshold, limit, counts, results, nullptr);
}

NGS_API const char* ngsKeyU8(uint32_t handle, uint32_t keyId) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed || keyId >= L->host.n_keys || L->host.csize != sizeof(uint32_t)) return nullptr;
    const Library::U8Keys* T = u8_keys(*L);
    return T ? T->bytes.data() + T->off[keyId] : nullptr;
}

NGS_API int ngsUtf8Decode(const uint8_t* dBytes, const uint64_t* dOffsets, uint32_t n, uint8_t* dOut,
                          uint64_t outCapBytes, uint64_t* dOutOffsets, void* stream) {
    if (!dOffsets || !dOutOffsets || (n && !dBytes) || (outCapBytes >= 4 && !dOut) || ((uintptr_t)dOut & 3u))
        return -3;
    static StreamScratch scratch;  // the scan's, kept as ngsPackResults keeps its own
    int dev = 0;
    if (!HIP_CHECK(hipGetDevice(&dev))) return -4;
    std::lock_guard<std::mutex> g(scratch.mu);
    const auto t = scratch.get(dev, (hipStream_t)stream, utf8_temp_bytes(n));
    if (!t.first) return -4;
    return HIP_CHECK(launch_utf8_decode(dBytes, dOffsets, n, reinterpret_cast<uint32_t*>(dOut), outCapBytes / 4,
                                        dOutOffsets, t.first, t.second, (hipStream_t)stream))
               ? 0
               : -4;
}

NGS_API int ngsTokenSortDevice(uint32_t handle, const uint8_t* dBytes, const uint64_t* dOffsets, uint32_t n,
                               uint8_t* dOut, void* stream) {
    if (!dOffsets || (n && (!dBytes || !dOut))) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    BatchGuard bg(L);
    uint32_t valid[8];
    {
        std::lock_guard<std::mutex> g(L->valid_mu);
        std::memcpy(valid, L->valid, sizeof valid);
    }
    return HIP_CHECK(launch_token_sort(valid, L->host.csize, dBytes, dOffsets, n, dOut, (hipStream_t)stream)) ? 0 : -4;
}

NGS_API int ngsSearchDeviceU8(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                              uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                              uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* Rp = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (L->host.csize != sizeof(uint32_t)) return -3;
    const uint32_t Lm = effective_limit(*L, limit);
    if (!search_args_ok(dQueryOffsets, nQueries, Lm, outStride, dCounts, dKeys, dScores)) return -3;
    if (const int rc = entry_replica(*L, Rp)) return rc;
    Replica& R = *Rp;
    hipStream_t s = (hipStream_t)stream;
    BatchGuard bg(L);
    if (Lm == 0 || nQueries == 0) {
        return HIP_CHECK(hipMemsetAsync(dCounts, 0, sizeof(uint32_t) * nQueries, s)) &&
                       HIP_CHECK(hipStreamSynchronize(s))
                   ? 0
                   : -4;
    }
    // the batch's UTF-8 byte count bounds its units: the context's query buffer takes 4 bytes each
    uint64_t ends[2] = {0, 0};
    if (!HIP_CHECK(hipMemcpyAsync(&ends[0], dQueryOffsets, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) ||
        !HIP_CHECK(hipMemcpyAsync(&ends[1], dQueryOffsets + nQueries, sizeof(uint64_t), hipMemcpyDeviceToHost, s)) ||
        !HIP_CHECK(hipStreamSynchronize(s)))
        return -4;
    if (ends[1] < ends[0]) return -3;
    const uint64_t qbytes = 4 * (ends[1] - ends[0]);
    std::unique_ptr<Context> c = R.acquire();
    if (!c) return -4;
    int rc = -4;
    if (ensure_queries(*c, nQueries, qbytes) && ensure_u8(*c, nQueries, 0) &&
        HIP_CHECK(launch_utf8_decode(dQueryBytes, dQueryOffsets, nQueries, reinterpret_cast<uint32_t*>(c->d_raw),
                                     c->qcap / 4, c->d_off, c->d_u8temp, c->u8temp_bytes, s)))
        rc = device_search(*L, R, *c, c->d_raw, c->d_off, nQueries, qbytes, threshold, Lm, outStride, dCounts, dKeys,
                           dScores, s);
    // (cannot happen: the buffer was sized for the batch)
    rc = rerun_outgrown(rc, *L, R, *c, c->d_raw, c->d_off, nQueries, threshold, Lm, outStride, dCounts, dKeys, dScores,
                        s);
    R.give_back(std::move(c));
    return rc;
}

NGS_API int ngsSetDevices(const int* devices, int n) {
    if (n < 0 || (n > 0 && !devices)) return -(int)hipErrorInvalidValue;
    int nd = 0;
    hipError_t e = hipGetDeviceCount(&nd);
    if (e != hipSuccess) return -(int)e;
    for (int i = 0; i < n; ++i)
        if (devices[i] < 0 || devices[i] >= nd) return -(int)hipErrorInvalidDevice;
    t_devices.assign(devices, devices + n);
    return 0;
}

NGS_API int ngsSetDevice(int device) { return ngsSetDevices(&device, 1); }

NGS_API int ngsReplicaCount(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? (int)L->reps.size() : -1;
}

NGS_API int ngsDeviceCount(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

NGS_API uint32_t ngsNumKeys(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? L->host.n_keys : 0;
}

NGS_API const char* ngsKey(uint32_t handle, uint32_t keyId) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || keyId >= L->host.n_keys || L->host.csize != 1) return nullptr;
    return L->host.key_bytes.data() + L->host.key_off[keyId];
}

NGS_API const wchar_t* ngsKeyW(uint32_t handle, uint32_t keyId) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || keyId >= L->host.n_keys || L->host.csize != sizeof(wchar_t)) return nullptr;
    return reinterpret_cast<const wchar_t*>(L->host.key_bytes.data() + L->host.key_off[keyId] * sizeof(wchar_t));
}

NGS_API uint32_t ngsCharSize(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? L->host.csize : 0;
}

NGS_API uint32_t ngsGramSize(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    return L ? L->host.gsz : 0;
}

NGS_API int ngsSearchDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                            uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride, uint32_t* dCounts,
                            uint32_t* dKeys, float* dScores, void* stream) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    const uint32_t Lm = effective_limit(*L, limit);
    if (!search_args_ok(dQueryOffsets, nQueries, Lm, outStride, dCounts, dKeys, dScores)) return -3;
    if (const int rc = entry_replica(*L, R)) return rc;
    hipStream_t s = (hipStream_t)stream;
    BatchGuard bg(L);
    return search_on_replica(*L, *R, dQueryBytes, dQueryOffsets, nQueries, threshold, Lm, outStride, dCounts, dKeys,
                             dScores, s);
}

// Asynchronous form (bench.py's pipeline; a server's batches): queue the search on a pooled
// context's own streams, ordered after the work already queued on `stream`, and return. Two
// calls in flight overlap on the GPU: one batch's tail (the last tier-1a waves, k_emit, tier 1b)
// runs beside the next batch's counting.
NGS_API int ngsSearchDeviceAsync(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                 uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                                 uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream, uint64_t* ticket) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* Rp = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    const uint32_t Lm = effective_limit(*L, limit);
    if (!ticket || !search_args_ok(dQueryOffsets, nQueries, Lm, outStride, dCounts, dKeys, dScores)) return -3;
    if (const int rc = entry_replica(*L, Rp)) return rc;
    hipStream_t s = (hipStream_t)stream;
    BatchGuard bg(L);  // the server stops here; the pending call keeps it stopped until its Wait
    // the batch mark the pending call holds until its Wait; released here on any early return
    struct Mark {
        Library* L;
        bool armed = true;
        explicit Mark(Library* l) : L(l) { L->batches.fetch_add(1, std::memory_order_acq_rel); }
        ~Mark() {
            if (armed) L->batches.fetch_sub(1, std::memory_order_acq_rel);
        }
    } mark(L);
    Library::Pending pd;
    pd.R = Rp;
    pd.dq = dQueryBytes;
    pd.doff = dQueryOffsets;
    pd.B = nQueries;
    pd.Lm = Lm;
    pd.stride = outStride;
    pd.thr = threshold;
    pd.dn = dCounts;
    pd.dk = dKeys;
    pd.ds = dScores;
    if (Lm == 0 || nQueries == 0) {
        if (!HIP_CHECK(hipMemsetAsync(dCounts, 0, sizeof(uint32_t) * nQueries, s))) return -4;
    } else {
        pd.c = Rp->acquire();
        if (!pd.c) return -4;
        Context& c = *pd.c;
        uint64_t qbytes = 0;
        if (!c.qcap && !(HIP_CHECK(hipMemcpyAsync(&qbytes, dQueryOffsets + nQueries, sizeof(uint64_t),
                                                 hipMemcpyDeviceToHost, s)) &&
                         HIP_CHECK(hipStreamSynchronize(s)))) {
            Rp->give_back(std::move(pd.c));
            return -4;
        }
        if (!HIP_CHECK(hipEventRecord(c.in_ev, s)) || !HIP_CHECK(hipStreamWaitEvent(c.stream, c.in_ev, 0))) {
            Rp->give_back(std::move(pd.c));
            return -4;
        }
        pd.rc = queue_search(*L, *Rp, c, dQueryBytes, dQueryOffsets, nQueries, qbytes, threshold, Lm, outStride,
                             dCounts, dKeys, dScores, c.stream, pd.P, false);
    }
    std::lock_guard<std::mutex> g(L->pend_mu);
    *ticket = L->next_ticket++;
    L->pending.emplace(*ticket, std::move(pd));
    mark.armed = false;  // ngsSearchDeviceWait releases it
    return 0;
}

// Completes an ngsSearchDeviceAsync call: waits for its kernels, runs the general path for the
// queries that need it, records the statistics (ngsLastStats). The results are then in place.
// Same return codes as ngsSearchDevice; -3 for an unknown ticket.
NGS_API int ngsSearchDeviceWait(uint32_t handle, uint64_t ticket) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L) return -1;
    Library::Pending pd;
    {
        std::lock_guard<std::mutex> g(L->pend_mu);
        auto it = L->pending.find(ticket);
        if (it == L->pending.end()) return -3;
        pd = std::move(it->second);
        L->pending.erase(it);
    }
    struct Done {  // the Async call's batch mark ends with its Wait
        Library* L;
        ~Done() { L->batches.fetch_sub(1, std::memory_order_acq_rel); }
    } done{L};
    if (!pd.c) return 0;  // nothing was queued (limit 0 or no queries): the counts were cleared
    Replica& R = *pd.R;
    Context& c = *pd.c;
    if (!HIP_CHECK(hipSetDevice(R.device))) {
        R.give_back(std::move(pd.c));
        return -4;
    }
    int rc = pd.rc ? pd.rc : finish_search(*L, R, c, pd.B, pd.P, pd.doff, pd.dn, pd.dk, pd.ds, c.stream);
    rc = rerun_outgrown(rc, *L, R, c, pd.dq, pd.doff, pd.B, pd.thr, pd.Lm, pd.stride, pd.dn, pd.dk, pd.ds, c.stream);
    R.give_back(std::move(pd.c));
    return rc;
}

NGS_API int ngsServe(uint32_t handle, int enable) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L) return -1;
    if (!L->host.indexed || L->reps.empty()) return -2;
    if (L->host.csize != 1) return -3;
    std::lock_guard<std::shared_mutex> g(L->server_mu);
    if (!enable) {
        L->serve_pref.store(-1);  // off, and no automatic start either
        L->serving.store(false, std::memory_order_release);
        L->server.reset();
        return 0;
    }
    L->serve_pref.store(1);
    if (L->server) return 0;
    auto sv = std::make_unique<Server>();
    if (!sv->init(L->reps.front()->device)) return -4;
    L->server = std::move(sv);
    L->serving.store(true, std::memory_order_release);
    return 0;
}

NGS_API int ngsPackResults(const uint32_t* dCounts, const uint32_t* dKeys, const float* dScores, uint32_t n,
                           uint32_t stride, uint32_t* dOffsets, uint32_t* dRecords, void* stream) {
    if (!dCounts || !dOffsets || (n && (!dKeys || !dScores || !dRecords || !stride))) return -3;
    if ((uint64_t)n * stride > 0xFFFFFFFFull) return -3;  // the offsets are 32-bit
    static StreamScratch scratch;  // the scan's
    int dev = 0;
    if (!HIP_CHECK(hipGetDevice(&dev))) return -4;
    std::lock_guard<std::mutex> g(scratch.mu);
    const auto t = scratch.get(dev, (hipStream_t)stream, pack_pairs_temp_bytes(n));
    if (!t.first) return -4;
    return HIP_CHECK(launch_pack_pairs(dCounts, dKeys, dScores, n, stride, dOffsets, dRecords, t.first, t.second,
                                       (hipStream_t)stream))
               ? 0
               : -4;
}

// The entry points without a metric are the M forms at kSimLevenshtein without terms.
NGS_API int ngsSimilarityDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                uint32_t nQueries, uint32_t stride, const uint32_t* dCounts, const uint32_t* dKeys,
                                float* dSim, void* stream) {
    return ngsSimilarityDeviceM(handle, dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, kSimLevenshtein,
                                dSim, nullptr, stream);
}

NGS_API int ngsRerankDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                            uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                            float* dSim, float minSimilarity, void* stream) {
    return ngsRerankDeviceM(handle, dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, dScores, dSim,
                            nullptr, kSimLevenshtein, minSimilarity, stream);
}

NGS_API uint32_t scoreBatchSim(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, float minSimilarity, uint32_t* counts, char*** results, float** scores,
                               float** sims) {
    return scoreBatchSimM(handle, queries, nQueries, threshold, limit, kSimLevenshtein, minSimilarity, counts, results,
                          scores, sims, nullptr);
}

NGS_API uint32_t scoreBatchSimW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, float minSimilarity, uint32_t* counts, wchar_t*** results,
                                float** scores, float** sims) {
    return scoreBatchSimMW(handle, queries, nQueries, threshold, limit, kSimLevenshtein, minSimilarity, counts, results,
                           scores, sims, nullptr);
}

NGS_API uint32_t scoreBatchSimU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, float minSimilarity, uint32_t* counts, char*** results, float** scores,
                                 float** sims) {
    return scoreBatchSimMU8(handle, queries, nQueries, threshold, limit, kSimLevenshtein, minSimilarity, counts,
                            results, scores, sims, nullptr);
}

NGS_API int ngsSimilarityDeviceM(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                 uint32_t nQueries, uint32_t stride, const uint32_t* dCounts, const uint32_t* dKeys,
                                 uint32_t metric, float* dSim, uint32_t* dTerms, void* stream) {
    if (!sim_args_ok(dQueryOffsets, nQueries, stride, dCounts, dKeys, dSim) || !sim_metric_ok(metric)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (const int rc = entry_replica(*L, R)) return rc;
    BatchGuard bg(L);
    return similarity_entry(sim_view(*L, *R), dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, metric, dSim,
                            dTerms, stream);
}

NGS_API int ngsRerankDeviceM(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                             uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                             float* dSim, uint32_t* dTerms, uint32_t metric, float minSimilarity, void* stream) {
    if (!rerank_args_ok(dQueryOffsets, nQueries, stride, dCounts, dKeys, dScores, dSim, metric, minSimilarity)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (const int rc = entry_replica(*L, R)) return rc;
    BatchGuard bg(L);
    return queue_similarity(sim_view(*L, *R), dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, dScores, dSim,
                            dTerms, metric, true, minSimilarity, (hipStream_t)stream);
}

NGS_API uint32_t scoreBatchSimM(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts, char*** results,
                                float** scores, float** sims, uint32_t** terms) {
    return sim_batch(handle, queries, nQueries, threshold, limit, minSimilarity, counts, results, scores, sims, false,
                     metric, terms);
}

NGS_API uint32_t scoreBatchSimMW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts,
                                 wchar_t*** results, float** scores, float** sims, uint32_t** terms) {
    return sim_batch(handle, queries, nQueries, threshold, limit, minSimilarity, counts, results, scores, sims, false,
                     metric, terms);
}

NGS_API uint32_t scoreBatchSimMU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                  uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts,
                                  char*** results, float** scores, float** sims, uint32_t** terms) {
    return sim_batch(handle, queries, nQueries, threshold, limit, minSimilarity, counts, results, scores, sims, true,
                     metric, terms);
}

NGS_API void ngsReleaseTerms(uint32_t* terms) { delete[] terms; }

NGS_API int64_t ngsTerm(uint32_t handle, uint32_t termId, void* buf, uint64_t capBytes) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (termId >= L->host.n_terms) return -3;
    BatchGuard bg(L);
    Replica& R = *L->reps.front();
    int cur = 0;
    if (!HIP_CHECK(hipGetDevice(&cur))) return -4;
    struct Back {  // the caller's device is current again on return
        int dev;
        ~Back() { (void)hipSetDevice(dev); }
    } back{cur};
    if (!HIP_CHECK(hipSetDevice(R.device))) return -4;
    uint64_t span[2] = {0, 0};  // term_off holds character offsets
    if (!HIP_CHECK(hipMemcpy(span, R.dev.term_off + termId, sizeof span, hipMemcpyDeviceToHost))) return -4;
    const uint64_t len = span[1] - span[0], cs = L->host.csize;
    const uint64_t take = std::min(capBytes / cs, len);
    if (take && !buf) return -3;
    if (take && !HIP_CHECK(hipMemcpy(buf, R.dev.term_bytes + span[0] * cs, take * cs, hipMemcpyDeviceToHost))) return -4;
    return (int64_t)len;
}

NGS_API uint64_t ngsKeyQueryBytes(uint32_t handle, uint32_t firstKey, uint32_t nKeys) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !L->host.indexed || !join_range_ok(*L, firstKey, nKeys)) return 0;
    return join_query_bytes(*L, firstKey, nKeys);
}

NGS_API int ngsKeyQueriesDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, uint8_t* dBytes, uint64_t capBytes,
                                uint64_t* dOffsets, void* stream) {
    if (!dOffsets || (capBytes && !dBytes)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (!join_range_ok(*L, firstKey, nKeys)) return -3;
    const uint64_t total = join_query_bytes(*L, firstKey, nKeys);
    if (capBytes < total || (L->host.csize == 4 && (reinterpret_cast<uintptr_t>(dBytes) & 3u))) return -3;
    if (const int rc = entry_replica(*L, R)) return rc;
    BatchGuard bg(L);
    return HIP_CHECK(launch_key_queries(R->dev, firstKey, nKeys, total, dBytes, dOffsets, (hipStream_t)stream)) ? 0 : -4;
}

NGS_API int ngsDropSelfDevice(uint32_t* dCounts, uint32_t* dKeys, float* dScores, uint32_t n, uint32_t stride,
                              uint32_t firstKey, uint32_t limit, void* stream) {
    if (!dCounts || (n && stride && (!dKeys || !dScores))) return -3;
    return HIP_CHECK(launch_drop_self(dCounts, dKeys, dScores, n, stride, firstKey, limit, (hipStream_t)stream)) ? 0 : -4;
}

NGS_API int ngsSelfJoinDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                              uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream) {
    if (!dCounts || (nKeys && (!dKeys || !dScores))) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (!join_range_ok(*L, firstKey, nKeys) || outStride < join_search_limit(*L, limit)) return -3;
    if (const int rc = entry_replica(*L, R)) return rc;
    if (nKeys == 0) return 0;
    BatchGuard bg(L);
    // the call's own scratch: the gathered queries, released once the search has read them (the
    // results and the stream are the caller's)
    CallScratch M;
    if (!M.alloc(&M.d_raw, join_max_query_bytes(*L, firstKey, nKeys, nKeys) + 16) ||
        !M.alloc(&M.d_off, (size_t)nKeys + 1))
        return -4;
    return join_batch(*L, *R, firstKey, nKeys, threshold, limit, outStride, M.d_raw, M.d_off, dCounts, dKeys, dScores,
                      (hipStream_t)stream, true);
}

NGS_API int ngsClusterDevice(const uint32_t* dCounts, const uint32_t* dKeys, uint32_t n, uint32_t stride,
                             uint32_t firstKey, uint32_t* dLabels, uint32_t nLabels, uint32_t flags, void* stream) {
    if ((flags & ~(kClusterInit | kClusterFinish)) || (nLabels && !dLabels) || (n && stride && (!dCounts || !dKeys)))
        return -3;
    return HIP_CHECK(launch_cluster(dCounts, dKeys, n, stride, firstKey, dLabels, nLabels, flags, (hipStream_t)stream))
               ? 0
               : -4;
}

NGS_API uint32_t selfJoin(uint32_t handle, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                          uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores) {
    return self_join_host(handle, firstKey, nKeys, threshold, limit, stride, counts, keyIds, scores);
}

NGS_API uint32_t dedupKeys(uint32_t handle, float threshold, uint32_t limit, float minSimilarity, uint32_t batchKeys,
                           uint32_t* labels) {
    return dedupKeysM(handle, threshold, limit, kSimLevenshtein, minSimilarity, batchKeys, labels);
}

NGS_API uint32_t dedupKeysM(uint32_t handle, float threshold, uint32_t limit, uint32_t metric, float minSimilarity,
                            uint32_t batchKeys, uint32_t* labels) {
    return dedup_host(handle, threshold, limit, metric, minSimilarity, batchKeys, labels);
}

NGS_API int ngsMatchDevice(const uint32_t* dCounts, const uint32_t* dKeys, const float* dValues, uint32_t n,
                           uint32_t stride, uint32_t firstKey, uint32_t* dMatchA, uint32_t nA, uint32_t* dMatchB,
                           uint32_t nB, uint64_t* dBids, uint32_t* dMatched, uint32_t flags, void* stream) {
    if ((flags & ~kMatchFlags) || !dMatched || (nA && !dMatchA) || (nB && (!dMatchB || !dBids)) ||
        (n && stride && (flags & (kMatchBid | kMatchAccept)) && (!dCounts || !dKeys || !dValues)))
        return -3;
    return HIP_CHECK(launch_match(dCounts, dKeys, dValues, n, stride, firstKey, dMatchA, nA, dMatchB, nB, dBids,
                                  dMatched, flags, (hipStream_t)stream))
               ? 0
               : -4;
}

NGS_API uint32_t linkKeys(uint32_t hFrom, uint32_t hTo, float threshold, uint32_t limit, uint32_t metric,
                          float minSimilarity, uint32_t mode, uint32_t batchKeys, uint32_t* match, float* scores,
                          float* sims) {
    return link_host(hFrom, hTo, threshold, limit, metric, minSimilarity, mode, batchKeys, match, scores, sims);
}

NGS_API int ngsKeyLengthsDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, uint32_t* dLen, void* stream) {
    if (nKeys && !dLen) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = nullptr;
    Replica* R = nullptr;
    if (const int rc = entry_library(handle, L)) return rc;
    if (!join_range_ok(*L, firstKey, nKeys)) return -3;
    if (const int rc = entry_replica(*L, R)) return rc;
    BatchGuard bg(L);
    return HIP_CHECK(launch_key_len(R->dev.key_off, firstKey, nKeys, dLen, (hipStream_t)stream)) ? 0 : -4;
}

NGS_API int ngsMergeResultsDevice(const ngs_merge_part* parts, uint32_t nParts, uint32_t nQueries, uint32_t limit,
                                  uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                                  void* stream) {
    if (!parts || nParts == 0 || nParts > kSetMaxParts || nQueries > kInt32Max ||
        (nQueries && (!dCounts || !dKeys || !dScores)))
        return -3;
    MergeParts M{};
    for (uint32_t p = 0; p < nParts; ++p) {
        const ngs_merge_part& a = parts[p];
        if (!a.dCounts || (a.stride && (!a.dKeys || !a.dScores)) || (a.nKeys && !a.dKeyLen)) return -3;
        M.p[p] = MergePart{a.dCounts, a.dKeys, a.dScores, a.dKeyLen, a.stride, a.keyBase, a.nKeys, 0u};
    }
    if (outStride < merge_min_stride(M.p, nParts, limit)) return -3;
    return HIP_CHECK(launch_merge_parts(M, nParts, nQueries, limit, outStride, dCounts, dKeys, dScores,
                                        (hipStream_t)stream))
               ? 0
               : -4;
}

NGS_API uint32_t ngsSetCreate(const uint32_t* handles, uint32_t n) {
    if (!handles || n == 0 || n > kSetMaxParts) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    std::unique_lock<std::shared_mutex> lk(g_lock);
    auto S = std::make_unique<KeySet>();
    for (uint32_t p = 0; p < n; ++p)
        if (const int rc = set_join(*S, handles[p])) {
            if (rc == -3 || !t_last_error) t_last_error = (int)hipErrorInvalidValue;
            return 0;
        }
    uint32_t id = 1;
    while (g_sets.count(id) && id < std::numeric_limits<uint32_t>::max()) ++id;
    if (id == std::numeric_limits<uint32_t>::max()) return 0;
    g_sets.emplace(id, std::move(S));
    return id;
}

NGS_API int ngsSetAdd(uint32_t set, uint32_t handle) {
    std::unique_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    return set_join(*S, handle);
}

NGS_API void ngsSetDispose(uint32_t set) {
    std::unique_lock<std::shared_mutex> lk(g_lock);
    g_sets.erase(set);
}

NGS_API int ngsSetParts(uint32_t set) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    return (int)S->parts.size();
}

NGS_API uint32_t ngsSetNumKeys(uint32_t set) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    return entry_set(set, S, libs) ? 0u : (uint32_t)S->n_keys;
}

NGS_API int ngsSetLocate(uint32_t set, uint32_t keyId, uint32_t* handle, uint32_t* localKey) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (keyId >= S->n_keys) return -3;
    size_t p = S->parts.size() - 1;  // the last member whose base is at or below the id (a member may be empty)
    while (S->parts[p].base > keyId) --p;
    if (handle) *handle = S->parts[p].handle;
    if (localKey) *localKey = keyId - S->parts[p].base;
    return 0;
}

NGS_API int ngsDropDeadDevice(uint32_t* dCounts, uint32_t* dKeys, float* dScores, uint32_t n, uint32_t stride,
                              const uint32_t* dDead, uint32_t nKeys, uint32_t limit, uint32_t* dShort, void* stream) {
    if (!dCounts || (n && stride && (!dKeys || !dScores)) || (nKeys && !dDead) || n > kInt32Max) return -3;
    DropBlocks D{};
    D.b[0] = DropBlock{dCounts, dKeys, dScores, dDead, dShort, stride, nKeys};
    return HIP_CHECK(launch_drop_dead(D, 1, n, limit, (hipStream_t)stream)) ? 0 : -4;
}

NGS_API int ngsSetRemove(uint32_t set, const uint32_t* keyIds, uint32_t n) { return set_mark(set, keyIds, n, true); }
NGS_API int ngsSetRestore(uint32_t set, const uint32_t* keyIds, uint32_t n) { return set_mark(set, keyIds, n, false); }

NGS_API uint32_t ngsSetLiveKeys(uint32_t set) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    return entry_set(set, S, libs) ? 0u : (uint32_t)(S->n_keys - S->n_dead);
}

NGS_API uint32_t ngsSetDeadKeys(uint32_t set, uint32_t* out, uint32_t cap) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (entry_set(set, S, libs) != 0) return 0;
    uint32_t at = 0;
    for (const KeySet::Member& m : S->parts)
        for (size_t w = 0; out && at < cap && w < m.dead.size(); ++w)
            for (uint32_t bits = m.dead[w]; bits && at < cap; bits &= bits - 1u)
                out[at++] = m.base + (uint32_t)w * 32u + (uint32_t)__builtin_ctz(bits);
    return (uint32_t)S->n_dead;
}

NGS_API int ngsSetIsLive(uint32_t set, uint32_t keyId) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (keyId >= S->n_keys) return -3;
    size_t p = S->parts.size() - 1;
    while (S->parts[p].base > keyId) --p;
    const KeySet::Member& m = S->parts[p];
    return m.dead.empty() || !dead_bit(m.dead.data(), m.n_keys, keyId - m.base) ? 1 : 0;
}

NGS_API int ngsSetDeadStats(uint32_t set, uint64_t* out, int n) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (n < 0 || (n && !out)) return -3;
    const uint64_t v[NGS_SET_DEAD_STATS] = {S->drop_launches.load(), S->re_searches.load(), S->max_fetch.load()};
    for (int i = 0; i < n && i < (int)NGS_SET_DEAD_STATS; ++i) out[i] = v[i];
    return (int)NGS_SET_DEAD_STATS;
}

NGS_API int ngsSetSearchDevice(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                               uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                               uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    const uint32_t Lm = set_effective_limit(*S, limit);
    if (!search_args_ok(dQueryOffsets, nQueries, Lm, outStride, dCounts, dKeys, dScores)) return -3;
    int cur = -1;
    if (!HIP_CHECK(hipGetDevice(&cur))) return -4;
    if (cur != S->device) return -3;
    hipStream_t s = (hipStream_t)stream;
    if (Lm == 0 || nQueries == 0)
        return HIP_CHECK(hipMemsetAsync(dCounts, 0, sizeof(uint32_t) * nQueries, s)) && HIP_CHECK(hipStreamSynchronize(s))
                   ? 0
                   : -4;
    // the call's own scratch: the members' blocks, released once the merge has read them
    CallScratch M;
    SetBlocks K;
    if (!set_blocks(M, *S, libs, nQueries, limit, K)) return -4;
    SetGuards guards(*S, libs);  // (until the final synchronise)
    if (const int rc = set_search(*S, libs, M, K, dQueryBytes, dQueryOffsets, nQueries, threshold, limit, outStride, dCounts,
                                  dKeys, dScores, s))
        return rc;
    return HIP_CHECK(hipStreamSynchronize(s)) ? 0 : -4;
}

NGS_API uint32_t scoreBatchSet(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores) {
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, false);
}

NGS_API uint32_t scoreBatchSetW(uint32_t set, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores) {
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, false);
}

NGS_API uint32_t scoreBatchSetU8(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores) {
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, true);
}

NGS_API int ngsSetSimilarityDeviceM(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                    uint32_t nQueries, uint32_t stride, const uint32_t* dCounts, const uint32_t* dKeys,
                                    uint32_t metric, float* dSim, uint32_t* dTerms, void* stream) {
    if (!sim_args_ok(dQueryOffsets, nQueries, stride, dCounts, dKeys, dSim) || !sim_metric_ok(metric)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (const int rc = set_device_current(*S)) return rc;
    SetGuards guards(*S, libs);
    return similarity_entry(sim_view(*S, libs), dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, metric, dSim,
                            dTerms, stream);
}

NGS_API int ngsSetRerankDeviceM(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                                float* dSim, uint32_t* dTerms, uint32_t metric, float minSimilarity, void* stream) {
    if (!rerank_args_ok(dQueryOffsets, nQueries, stride, dCounts, dKeys, dScores, dSim, metric, minSimilarity)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (const int rc = set_device_current(*S)) return rc;
    SetGuards guards(*S, libs);
    return queue_similarity(sim_view(*S, libs), dQueryBytes, dQueryOffsets, nQueries, stride, dCounts, dKeys, dScores, dSim,
                            dTerms, metric, true, minSimilarity, (hipStream_t)stream);
}

NGS_API uint64_t ngsSetKeyQueryBytes(uint32_t set, uint32_t firstKey, uint32_t nKeys) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (entry_set(set, S, libs) != 0 || !set_range_ok(*S, firstKey, nKeys)) return 0;
    return set_query_bytes(*S, libs, firstKey, nKeys);
}

NGS_API int ngsSetKeyQueriesDevice(uint32_t set, uint32_t firstKey, uint32_t nKeys, uint8_t* dBytes, uint64_t capBytes,
                                   uint64_t* dOffsets, void* stream) {
    if (!dOffsets || (capBytes && !dBytes)) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    if (!set_range_ok(*S, firstKey, nKeys)) return -3;
    const uint64_t total = set_query_bytes(*S, libs, firstKey, nKeys);
    if (capBytes < total || (S->csize == 4 && (reinterpret_cast<uintptr_t>(dBytes) & 3u))) return -3;
    if (const int rc = set_device_current(*S)) return rc;
    SetGuards guards(*S, libs);
    return set_key_queries(*S, libs, firstKey, nKeys, dBytes, dOffsets, (hipStream_t)stream) ? 0 : -4;
}

NGS_API int ngsSetSelfJoinDevice(uint32_t set, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                                 uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream) {
    if (!dCounts || (nKeys && (!dKeys || !dScores))) return -3;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (const int rc = entry_set(set, S, libs)) return rc;
    const uint32_t Ls = set_join_limit(*S, limit);
    if (!set_range_ok(*S, firstKey, nKeys) || outStride < Ls) return -3;
    if (const int rc = set_device_current(*S)) return rc;
    if (nKeys == 0) return 0;
    SetGuards guards(*S, libs);  // (until the final synchronise)
    // the call's own scratch: the gathered queries and the members' blocks, released once the merge
    // has read them (the results and the stream are the caller's)
    CallScratch M;
    SetBlocks K;
    if (!M.alloc(&M.d_raw, set_query_bytes(*S, libs, firstKey, nKeys) + 16) || !M.alloc(&M.d_off, (size_t)nKeys + 1) ||
        !set_blocks(M, *S, libs, nKeys, Ls, K))
        return -4;
    return set_join_batch(*S, libs, M, K, firstKey, nKeys, threshold, limit, outStride, M.d_raw, M.d_off, dCounts, dKeys,
                          dScores, (hipStream_t)stream, true);
}

NGS_API uint32_t scoreBatchSetSimM(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                   uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                   uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms) {
    const SetSim sim{metric, minSimilarity, sims, terms};
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, false, &sim);
}

NGS_API uint32_t scoreBatchSetSimMW(uint32_t set, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                    uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                    uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms) {
    const SetSim sim{metric, minSimilarity, sims, terms};
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, false, &sim);
}

NGS_API uint32_t scoreBatchSetSimMU8(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                     uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                     uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms) {
    const SetSim sim{metric, minSimilarity, sims, terms};
    return set_batch(set, queries, nQueries, threshold, limit, stride, counts, keyIds, scores, true, &sim);
}

NGS_API uint32_t selfJoinSet(uint32_t set, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                             uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores) {
    if (counts) std::fill(counts, counts + nKeys, 0u);
    auto fail = [&](int err) -> uint32_t {  // (counts may hold finished batches by then)
        if (err && !t_last_error) t_last_error = err;
        if (counts) std::fill(counts, counts + nKeys, 0u);
        return 0;
    };
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (!counts || entry_set(set, S, libs) != 0 || !set_range_ok(*S, firstKey, nKeys))
        return fail((int)hipErrorInvalidValue);
    const uint32_t Lm = set_effective_limit(*S, limit);
    if (stride < Lm || (nKeys && Lm && (!keyIds || !scores))) return fail((int)hipErrorInvalidValue);
    if (nKeys == 0 || Lm == 0) return 0;
    if (!HIP_CHECK(hipSetDevice(S->device))) return fail(0);
    SetGuards guards(*S, libs);
    SetJoin j{*S, libs};
    return self_join_run(j, firstKey, nKeys, threshold, limit, stride, counts, keyIds, scores, fail);
}

NGS_API uint32_t dedupKeysSet(uint32_t set, float threshold, uint32_t limit, uint32_t metric, float minSimilarity,
                              uint32_t batchKeys, uint32_t* labels) {
    if (!dedup_args_ok(limit, metric, minSimilarity, labels)) return 0;
    std::shared_lock<std::shared_mutex> lk(g_lock);
    KeySet* S = nullptr;
    Library* libs[kSetMaxParts] = {};
    if (entry_set(set, S, libs) != 0) {
        t_last_error = (int)hipErrorInvalidValue;
        return 0;
    }
    if (S->n_keys == 0 || !HIP_CHECK(hipSetDevice(S->device))) return 0;
    SetGuards guards(*S, libs);
    SetJoin j{*S, libs};
    // a dead key is alone under its own label (§9.9): the clusters of the live keys are counted
    const uint32_t clusters = dedup_run(j, threshold, limit, metric, minSimilarity, batchKeys, labels);
    return clusters > S->n_dead ? clusters - (uint32_t)S->n_dead : 0u;
}

NGS_API int ngsServeState(uint32_t handle) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L) return -1;
    std::shared_lock<std::shared_mutex> g(L->server_mu);
    if (!L->server) return 0;
    return L->server->stopped() ? 1 : 2;
}

NGS_API int ngsLastError(int clear) {
    const int e = t_last_error;
    if (clear) t_last_error = 0;
    return e;
}

NGS_API int ngsSetTiming(uint32_t handle, int enable) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L) return -1;
    L->timing.store(enable != 0);
    return 0;
}

NGS_API int ngsLastStats(uint32_t handle, ngs_stats* out) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L || !out) return -1;
    std::lock_guard<std::mutex> g(L->stats_mu);
    *out = L->last;
    return 0;
}

#ifndef NGS_SRC_HASH
#define NGS_SRC_HASH "unknown"
#endif
NGS_API const char* ngsVersion(void) { return "ngram_search 0.2 gfx950 src=" NGS_SRC_HASH; }

NGS_API int ngsIndexDigest(uint32_t handle, uint64_t* out, int n) { return ngsReplicaDigest(handle, 0, out, n); }

NGS_API int ngsReplicaDigest(uint32_t handle, int replica, uint64_t* out, int n) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    auto it = g_libs.find(handle);
    if (it == g_libs.end() || replica < 0 || (size_t)replica >= it->second->reps.size() || !out) return -1;
    Library& L = *it->second;
    const Replica& R = *L.reps[replica];
    const DevIndex& X = R.dev;
    if (!HIP_CHECK(hipSetDevice(R.device))) return -4;
    // (bytes, FNV-1a) of gram_off, post, gram_row, skip as the kernels read them
    auto digest = [](const void* d, size_t bytes, uint64_t& h) -> bool {
        std::vector<uint8_t> v(bytes);
        if (bytes && !HIP_CHECK(hipMemcpy(v.data(), d, bytes, hipMemcpyDeviceToHost))) return false;
        h = 1469598103934665603ull;
        for (uint8_t c : v) h = (h ^ c) * 1099511628211ull;
        return true;
    };
    uint64_t vals[20] = {};
    {  // the gram CSR: direct-indexed (kGramSpace codes) or over the dictionary's gram ids
        uint64_t n_post = 0;
        const size_t nspace = X.gram_mode == 0 ? (size_t)kGramSpace : (size_t)R.n_gram_ids;
        if (!HIP_CHECK(hipMemcpy(&n_post, X.gram_off + nspace, sizeof(uint64_t), hipMemcpyDeviceToHost))) return -4;
        const size_t rows = L.host.n_grams;
        const size_t sizes[4] = {sizeof(uint64_t) * (nspace + 1), sizeof(uint32_t) * n_post, sizeof(uint32_t) * nspace,
                                 sizeof(uint32_t) * rows * (X.n_buckets + 1)};
        const void* ptrs[4] = {X.gram_off, X.post, X.gram_row, X.skip};
        vals[0] = n_post;
        vals[1] = rows;
        vals[2] = X.n_buckets;
        for (int i = 0; i < 4; ++i)
            if (!digest(ptrs[i], sizes[i], vals[3 + i])) return -4;
        vals[7] = X.bucket_span;
    }
    // the interned library (ngs_intern.hip or the host build): terms, pairs, keys, wildcard answer
    uint64_t tchars = 0;
    uint32_t npairs = 0;
    if (!HIP_CHECK(hipMemcpy(&tchars, X.term_off + X.n_terms, sizeof(uint64_t), hipMemcpyDeviceToHost)) ||
        !HIP_CHECK(hipMemcpy(&npairs, X.tk_off + X.n_terms, sizeof(uint32_t), hipMemcpyDeviceToHost)))
        return -4;
    const uint64_t kchars = L.host.key_off[X.n_keys];
    const size_t tsizes[8] = {sizeof(uint64_t) * (X.n_terms + 1), tchars * X.csize,
                              sizeof(uint32_t) * (X.n_terms + 1), sizeof(uint2) * npairs,
                              sizeof(uint64_t) * (X.n_keys + 1), kchars * X.csize,
                              sizeof(uint32_t) * X.n_keys, sizeof(float) * X.n_keys};
    const void* tptrs[8] = {X.term_off, X.term_bytes, X.tk_off, X.tk, X.key_off, X.key_bytes, X.wild_key, X.wild_score};
    for (int i = 0; i < 8; ++i)
        if (!digest(tptrs[i], tsizes[i], vals[8 + i])) return -4;
    // the shape flags the kernels branch on
    const uint64_t flags = (X.keys_unique ? 1u : 0u) | (X.tk_identity ? 2u : 0u) | (X.tk_monotone ? 4u : 0u) |
                           (X.rank_post ? 8u : 0u);
    vals[16] = flags;
    // the gram dictionary's lookup table as uploaded (direct-indexed indexes: zeros)
    if (X.gram_mode == 1) {
        if (!digest(X.ghash_key, sizeof(uint64_t) * R.ghash_slots, vals[17]) ||
            !digest(X.ghash_val, sizeof(uint32_t) * R.ghash_slots, vals[18]))
            return -4;
        vals[19] = X.ghash_bits;
    }
    const int m = std::max(0, std::min(n, 20));
    for (int i = 0; i < m; ++i) out[i] = vals[i];
    return m;
}

// ---- index files: the interned library, the part the build spends its
// time on; the gram CSR and skip table are rebuilt from it on load (GPU, or host for gram
// dictionaries), the keys' wildcard answer too. Little-endian, native widths:
//   "NGSIDX01" | u32 csize, gsz, gram_mode, short_term_len, short_query_len, full_scan_len,
//   n_terms, n_short, n_keys, valid[8] | arrays (u64 element count, then the elements):
//   term_off u64, term_bytes u8, tk_off u32, tk {u32 key, u32 weight bits}, key_off u64,
//   key_bytes u8, wild_w f32
extern "C++" {
namespace ngs {
namespace {
constexpr char kIndexMagic[8] = {'N', 'G', 'S', 'I', 'D', 'X', '0', '1'};

template <class T>
bool put_array(std::FILE* f, const T* p, uint64_t n) {
    return std::fwrite(&n, sizeof n, 1, f) == 1 && (n == 0 || std::fwrite(p, sizeof(T), n, f) == n);
}
// `file_size`: the whole file's; a count whose elements the rest of the file cannot hold is
// refused before anything is allocated for it
template <class T>
bool get_array(std::FILE* f, std::vector<T>& v, uint64_t max_n, uint64_t file_size) {
    uint64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n > max_n) return false;
    const long pos = std::ftell(f);
    if (pos < 0 || (uint64_t)pos > file_size || n > (file_size - (uint64_t)pos) / sizeof(T)) return false;
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
bool download_vec(std::vector<T>& v, const T* d, uint64_t n) {
    v.resize(n);
    return n == 0 || HIP_CHECK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
}
}  // namespace
}  // namespace ngs
}  // extern "C++"

NGS_API int ngsSaveIndex(uint32_t handle, const char* path) {
    std::shared_lock<std::shared_mutex> lk(g_lock);
    Library* L = find_lib(handle);
    if (!L) return -1;
    if (!L->host.indexed || L->reps.empty()) return -2;
    if (!path) return -3;
    const HostIndex& H = L->host;
    const Replica& R = *L->reps.front();
    if (!HIP_CHECK(hipSetDevice(R.device))) return -4;
    const DevIndex& X = R.dev;
    std::vector<uint64_t> term_off;
    std::vector<uint8_t> term_bytes;
    std::vector<uint32_t> tk_off;
    std::vector<uint2> tk;
    std::vector<float> wild_w;
    if (!download_vec(term_off, X.term_off, (uint64_t)H.n_terms + 1) ||
        !download_vec(term_bytes, X.term_bytes, term_off.back() * H.csize) ||
        !download_vec(tk_off, X.tk_off, (uint64_t)H.n_terms + 1) || !download_vec(tk, X.tk, tk_off.back()) ||
        !download_vec(wild_w, R.wild_w, H.n_keys))
        return -4;
    uint32_t valid[8];
    {
        std::lock_guard<std::mutex> g(L->valid_mu);
        std::memcpy(valid, L->valid, sizeof valid);
    }
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return -3;
    const uint32_t sc[9] = {H.csize,          H.gsz,         H.gram_mode, H.short_term_len, H.short_query_len,
                            H.full_scan_len,  H.n_terms,     H.n_short,   H.n_keys};
    bool ok = std::fwrite(kIndexMagic, 1, 8, f) == 8 && std::fwrite(sc, sizeof sc, 1, f) == 1 &&
              std::fwrite(valid, sizeof valid, 1, f) == 1 && put_array(f, term_off.data(), term_off.size()) &&
              put_array(f, term_bytes.data(), term_bytes.size()) && put_array(f, tk_off.data(), tk_off.size()) &&
              put_array(f, tk.data(), tk.size()) && put_array(f, H.key_off.data(), H.key_off.size()) &&
              put_array(f, H.key_bytes.data(), H.key_bytes.size()) && put_array(f, wild_w.data(), wild_w.size());
    ok = (std::fclose(f) == 0) && ok;
    return ok ? 0 : -3;
}

NGS_API uint32_t ngsLoadIndex(const char* path) {
    if (!path) return 0;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 0;
    HostIndex H;
    char magic[8];
    uint32_t sc[9], valid[8];
    constexpr uint64_t kMax = uint64_t(1) << 40;
    uint64_t fsz = 0;
    {
        const long end = std::fseek(f, 0, SEEK_END) == 0 ? std::ftell(f) : -1;
        if (end < 0 || std::fseek(f, 0, SEEK_SET) != 0) {
            std::fclose(f);
            return 0;
        }
        fsz = (uint64_t)end;
    }
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, kIndexMagic, 8) == 0 &&
              std::fread(sc, sizeof sc, 1, f) == 1 && std::fread(valid, sizeof valid, 1, f) == 1 &&
              get_array(f, H.term_off, kMax, fsz) && get_array(f, H.term_bytes, kMax, fsz) &&
              get_array(f, H.tk_off, kMax, fsz) && get_array(f, H.tk, kMax, fsz) &&
              get_array(f, H.key_off, kMax, fsz) && get_array(f, H.key_bytes, kMax, fsz) &&
              get_array(f, H.wild_w, kMax, fsz);
    std::fclose(f);
    if (!ok) return 0;
    H.csize = sc[0];
    H.gsz = sc[1];
    H.gram_mode = sc[2];
    H.short_term_len = sc[3];
    H.short_query_len = sc[4];
    H.full_scan_len = sc[5];
    H.n_terms = sc[6];
    H.n_short = sc[7];
    H.n_keys = sc[8];
    // the arrays must describe the counts (a truncated or foreign file is refused)
    if ((H.csize != 1 && H.csize != 4) || H.gsz < 1 || H.gsz > kMaxGramSize || H.gram_mode > 1 ||
        H.n_short > H.n_terms || H.term_off.size() != (size_t)H.n_terms + 1 ||
        H.tk_off.size() != (size_t)H.n_terms + 1 || H.key_off.size() != (size_t)H.n_keys + 1 ||
        H.wild_w.size() != H.n_keys || H.term_bytes.size() != H.term_off.back() * H.csize ||
        H.tk.size() != H.tk_off.back() || H.key_bytes.size() != H.key_off.back() * H.csize)
        return 0;
    for (const uint2& kw : H.tk)
        if (kw.x >= H.n_keys) return 0;
    // every offset array ascends from 0 to its array's end (a crafted file must not send the
    // kernels or marshal() out of bounds), every key ends in a NUL, the length parameters are the
    // gram size's, and the short / long term split matches the term lengths
    auto ascending = [](const auto& off) {
        if (off.empty() || off.front() != 0) return false;
        for (size_t i = 1; i < off.size(); ++i)
            if (off[i] < off[i - 1]) return false;
        return true;
    };
    if (!ascending(H.term_off) || !ascending(H.tk_off) || !ascending(H.key_off)) return 0;
    if (H.short_term_len != 2 * H.gsz || H.short_query_len != 3 * H.gsz || H.full_scan_len != H.gsz ||
        H.gram_mode != ((H.csize == 1 && H.gsz == 3) ? 0u : 1u))
        return 0;
    for (uint32_t k = 0; k < H.n_keys; ++k) {
        if (H.key_off[k + 1] == H.key_off[k]) return 0;  // not even the NUL
        const uint64_t last = (H.key_off[k + 1] - 1) * H.csize;
        for (uint32_t b = 0; b < H.csize; ++b)
            if (H.key_bytes[last + b] != 0) return 0;
    }
    for (uint32_t t = 0; t < H.n_terms; ++t) {
        const bool is_short = H.term_off[t + 1] - H.term_off[t] < H.short_term_len;
        if (is_short != (t < H.n_short)) return 0;
    }
    H.indexed = true;
    H.grams_built = false;
    const uint32_t handle = new_library([&](HostIndex& dst) {
        dst = std::move(H);  // the gram CSR (and a dictionary index's gram table) built at upload
    });
    if (handle) {
        std::shared_lock<std::shared_mutex> lk(g_lock);
        if (Library* L = find_lib(handle)) {
            std::lock_guard<std::mutex> g(L->valid_mu);
            std::memcpy(L->valid, valid, sizeof valid);
        }
    }
    return handle;
}

NGS_API int ngsHostPhases(uint64_t* out, int n, int reset) {
    const int k = std::min<int>(n, kHpN);
    for (int i = 0; i < k; ++i) out[i] = reset ? g_host_phase[i].exchange(0) : g_host_phase[i].load();
    for (int i = k; reset && i < kHpN; ++i) g_host_phase[i].store(0);
    return kHpN;
}

NGS_API int ngsPhaseStats(uint64_t* out, int n, int reset) {
    return phase_stats((unsigned long long*)out, n, reset != 0);
}

}  // extern "C"
