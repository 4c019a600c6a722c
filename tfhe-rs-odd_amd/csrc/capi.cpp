// capi.cpp -- C ABI implementation (include/tfhe_mi355.h).  Host-side runtime of the engine:
// context = device + parameter set + key material + FFT tables, guarded by a mutex so that
// concurrent callers (the reference's rayon workers, shortint/engine/mod.rs:23-25) can share one
// key.  Error convention: 0/1 return + thread-local message (tfhe/src/c_api/utils.rs:3-73).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is opened at run time, when keys are replicated

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <atomic>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tfhe_mi355.h"
#include "engine.h"
#include "errors.h"

using namespace tfhe_mi355;

namespace {

struct Failure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Failure(buf);
}

void check(hipError_t e, const char *what) {
    if (e != hipSuccess) fail("%s: %s", what, hipGetErrorString(e));
}

// The calling thread's current HIP device is the caller's (a Rust or C caller may use HIP itself):
// every entry point that selects another device puts the caller's back before it returns, success
// or failure.  A thread without a device (no GPU, or HIP not initialised) keeps none.
struct CallerDevice {
    int d = -1;
    CallerDevice() {
        if (hipGetDevice(&d) != hipSuccess) d = -1;
    }
    ~CallerDevice() {
        int now = -1;
        if (d >= 0 && (hipGetDevice(&now) != hipSuccess || now != d)) (void)hipSetDevice(d);
    }
    CallerDevice(const CallerDevice &) = delete;
    CallerDevice &operator=(const CallerDevice &) = delete;
};

template <class F>
int guarded(F &&f) {
    CallerDevice keep;
    try {
        f();
        last_error_text().clear();
        return TFHE_MI355_OK;
    } catch (const std::exception &ex) {
        last_error_text() = ex.what();
        return TFHE_MI355_ERROR;
    } catch (...) {
        last_error_text() = "unknown failure";
        return TFHE_MI355_ERROR;
    }
}

struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }
    void reserve(size_t b) {
        if (b <= bytes) return;
        if (ptr) check(hipFree(ptr), "hipFree");
        ptr = nullptr;
        bytes = 0;
        check(hipMalloc(&ptr, b), "hipMalloc");
        bytes = b;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

// page-locked host staging of the host-pointer entry points (hipHostMalloc), one per pipeline lane
struct PinnedBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { release(); }
    void reserve(size_t b) {
        if (b <= bytes) return;
        release();
        check(hipHostMalloc(&ptr, b, hipHostMallocDefault), "hipHostMalloc");
        bytes = b;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

// an environment switch is on when set to a non-empty value other than "0"
bool env_flag(const char *name) {
    const char *e = std::getenv(name);
    return e && *e && std::strcmp(e, "0") != 0;
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

bool is_pow2(uint32_t x) { return x && !(x & (x - 1)); }
}  // namespace

// one small host-pointer call waiting to be coalesced into a batch (see "request coalescing")
enum CoalescedOp { CO_PBS = 0, CO_KS_PBS, CO_PBS_KS, CO_KS, CO_OPS };
struct CoalescedReq {
    const uint64_t *in;
    uint64_t *out;
    const uint64_t *luts;
    size_t lut_count;
    const uint32_t *idx;
    size_t count;
    bool sync = false;  // a blocking caller (coalesced_call), not a submitted request
    // blocking callers copy their own rows out of the slot's pinned staging once woken (in parallel
    // instead of one after the other on the dispatcher), then release the slot (pending)
    const uint64_t *src = nullptr;
    size_t src_bytes = 0;
    std::atomic<int> *pending = nullptr;
    // completion: set by the dispatcher, waited on by the caller alone (no shared mutex, so a
    // finished batch wakes its callers without a thundering herd on the queue lock)
    std::mutex m;
    std::condition_variable cv;
    bool done = false;
    std::string err;
};

struct RcclComms;  // communicator over a multi-device context's distinct devices (key replication)

// Worker threads of a multi-device context, one per shard after the first, started with the context
// and joined by its destroy: a batched host-pointer call hands each of them its shard's row share
// (split_rows) instead of starting threads per call.  Each worker runs its queue in
// order; concurrent calls queue behind each other per shard, as they would on the shard's lock.
struct ShardWorker {
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    bool stop = false;
    std::thread t;
    void post(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(m);
            q.push_back(std::move(f));
        }
        cv.notify_one();
    }
    void loop() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return stop || !q.empty(); });
                if (q.empty()) return;  // stop with nothing queued
                f = std::move(q.front());
                q.pop_front();
            }
            f();
        }
    }
    ~ShardWorker() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_one();
        if (t.joinable()) t.join();
    }
};

struct TfheMi355Context {
    TfheMi355Parameters p{};
    int device = 0;
    int cus = 256;  // compute units of the device (the latency kernels run one ciphertext per CU)
    std::mutex mu;
    // Key material vs the coalescer's batches: every key upload holds it exclusively, every
    // dispatcher batch shared, so a re-upload waits for the batches in flight and no batch starts
    // on a half-written key (the large host-pointer calls are ordered with uploads by `mu`).
    // Uploads go through KeyWrite, batches through KeyRead.
    std::shared_mutex keys_mu;
    // key writers waiting or running: a batch does not take keys_mu while one is pending, so an
    // upload is never starved by back-to-back batches (libstdc++'s shared_mutex lets new readers
    // in ahead of a waiting writer)
    std::atomic<int> key_writers{0};
    // Multi-device context (tfhe_mi355_context_create_devices): one single-device context per
    // listed device (a device may repeat), owned by this one; empty for a single-device context.
    // Every entry point of a multi-device context dispatches to them (see "multi-device").
    std::vector<TfheMi355Context *> shards;
    std::atomic<size_t> next_shard{0};  // round robin of coalesced calls and submits
    std::vector<std::unique_ptr<ShardWorker>> workers;  // shards 1.. (split_rows)
    int replication = 0;  // how the last key replication ran (tfhe_mi355_context_replication)
    RcclComms *rccl = nullptr;
    std::string replicate_note;  // why the last replication did not use RCCL in auto mode (empty: it did, or no need)
    TfheMi355Context *owner = nullptr;  // a shard: its multi-device context (destroyed with it)
    bool multi() const { return !shards.empty(); }
    hipStream_t stream = nullptr;
    FftTables tables;
    DeviceBuffer fbsk, ksk, std_staging;
    DeviceBuffer io_luts, io_tmp;
    DeviceBuffer ksk_planes;   // int8 byte planes of the KSK for the MFMA keyswitch
    // Host-pointer entry points: kernels run in chunk order on `stream`; each of two lanes has a
    // copy stream, page-locked staging and device in/out buffers, so that chunk i's copies (and
    // the host-side copies into and out of the staging) overlap chunk i+-1's kernels.  Only the
    // synchronous entry points use these, under `mu`; the _async entry points take all their
    // scratch from the caller (no shared mutable state, capturable into a hipGraph).
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t h2d = nullptr, kern = nullptr, done = nullptr;
        PinnedBuffer h_in, h_out, h_idx;
        DeviceBuffer d_in, d_out, d_idx;
        bool pending = false;
        bool direct_out = false;  // this chunk's D2H went straight into the caller's pinned buffer
        size_t first = 0, count = 0;
    } lanes[2];
    bool ksk_planes_ready = false;
    bool fbsk_ready = false, ksk_ready = false;
    // LWE -> GLWE packing keyswitching key of the gadget layer (big LWE key -> GLWE key)
    DeviceBuffer pksk, pksk_planes;
    uint32_t pks_base_log = 0, pks_level = 0;
    bool pksk_ready = false, pksk_planes_ready = false;
    // private functional packing keyswitching keys of the circuit bootstrap (big LWE key -> GLWE key,
    // one key per GGSW row), in the reference's order; byte planes for the int8-MFMA form
    DeviceBuffer pfpksk, pfpksk_planes;
    uint32_t pfks_base_log = 0, pfks_level = 0;
    bool pfpksk_ready = false, pfpksk_planes_ready = false;
    // GLWE relinearisation key of the gadget layer's lwe_mult (glwe_mult.hip), the reference's order
    DeviceBuffer rlk;
    uint32_t rlk_base_log = 0, rlk_level = 0;
    bool rlk_ready = false;
    // 32-bit torus keys (the boolean module's; "32-bit torus" section below).  The Fourier key of a u32
    // bootstrapping key lives in `fbsk` (same format); a context holds keys of one width only.
    DeviceBuffer ksk32, ksk32_planes;  // u32 keyswitching key and its four int8 byte planes
    DeviceBuffer lut_true32;           // the gates' accumulator: trivial GLWE, body all 1 << 29
    bool fbsk32_ready = false, ksk32_ready = false, ksk32_planes_ready = false;
    bool has_u32_keys() const { return fbsk32_ready || ksk32_ready; }
    // 128-bit torus ("128-bit torus" section below): the Fourier key as four f64 planes per polynomial and
    // the double-double tables of the context's N.  for_u128: created by tfhe_mi355_context_create_u128, whose
    // shape the u64 and u32 kernels need not take -- such a context serves u128 calls only.
    DeviceBuffer fbsk128, tables128;
    bool fbsk128_ready = false, for_u128 = false;
    bool has_u128_keys() const { return fbsk128_ready; }
    bool has_u64_keys() const { return fbsk_ready || ksk_ready || pksk_ready || pfpksk_ready || rlk_ready; }
    KernelTimer timer;  // per-kernel durations (tfhe_mi355_kernel_timing_*), off by default
    // one u32 the quad CMUX sets when a flag wait timed out (check_quad_fail); allocated zeroed at
    // creation for the contexts that can take the quad path (quad_max > 0)
    DeviceBuffer quad_fail;
    // Request coalescing of small host-pointer calls (the reference calls the PBS one ciphertext
    // at a time from rayon workers: shortint/server_key/mod.rs:783-857, radix_parallel/mul.rs:
    // 347-407).  Concurrent calls are queued per op; dispatcher threads (one per batch slot,
    // started with the first coalesced call) each gather a queue into a batch (after a short
    // window or when the batch is full) and run it on their slot's stream, staging and scratch;
    // every caller gets its rows back bit-identical to a call of its own.
    struct Coalescer {
        std::mutex m;
        std::condition_variable cv;  // dispatchers: work queued / stop
        std::vector<CoalescedReq *> queue[CO_OPS];
        size_t queued[CO_OPS] = {};
        size_t queued_sync[CO_OPS] = {};  // of queued[]: rows from blocking callers
        size_t last_sync_rows[CO_OPS] = {};  // rows of the op's previous batch if all were blocking calls
        std::chrono::steady_clock::time_point last_arrival[CO_OPS];
        bool stop = false;
        std::vector<std::thread> workers;
        struct Slot {
            hipStream_t stream = nullptr;
            PinnedBuffer h_in, h_out;            // h_in / d_in: [LUT sets | input rows | LUT indexes]
            DeviceBuffer d_in, d_out, d_scratch;
            std::atomic<int> copies{0};          // callers of the last batch still copying out of h_out
        } slots[9];  // 0-7: dispatchers; 8: direct calls (coalesced_call)
        bool direct_busy = false;  // slot 8 in use, under m
        // statistics (tfhe_mi355_coalesce_stats), under m
        uint64_t batches = 0, rows = 0, in_flight = 0, max_in_flight = 0;
        double batch_seconds = 0;
    } co;
    KernelTimer *timer_or_null() { return timer.every > 0 ? &timer : nullptr; }

    size_t n() const { return p.lwe_dimension; }
    size_t k() const { return p.glwe_dimension; }
    size_t N() const { return p.polynomial_size; }
    size_t big_dim() const { return k() * N(); }
    size_t glwe_len() const { return (k() + 1) * N(); }
    // GGSWs in the key: n (classic) or (n/g) 2^g (multi-bit, lwe_multi_bit_bootstrap_key.rs:40-55)
    size_t ggsw_count() const {
        return p.grouping_factor ? (n() / p.grouping_factor) << p.grouping_factor : n();
    }
    size_t std_bsk_len() const {
        return ggsw_count() * p.pbs_level * (k() + 1) * (k() + 1) * N();
    }
    size_t fourier_bsk_bytes() const {
        return ggsw_count() * p.pbs_level * (k() + 1) * (k() + 1) * (N() / 2) * sizeof(double2);
    }
    size_t ksk_len() const { return big_dim() * p.ks_level * (n() + 1); }
    size_t pksk_len(uint32_t level) const { return big_dim() * level * glwe_len(); }
    size_t pfpksk_len(uint32_t level) const { return (k() + 1) * (big_dim() + 1) * level * glwe_len(); }
    size_t rlk_len(uint32_t level) const { return k() * (k() + 1) / 2 * level * glwe_len(); }
};

// A keyswitching key of its own dimensions and decomposition (tfhe_mi355_lwe_keyswitch_key_create): one
// copy per distinct device of its context, read-only after creation.
struct TfheMi355KeyswitchKey {
    TfheMi355Context *ctx = nullptr;
    size_t in_dim = 0, out_dim = 0;
    uint32_t base_log = 0, level = 0;
    bool mfma = false;  // int8 byte planes built: the MFMA form runs
    struct Part {
        int device = 0;
        DeviceBuffer ksk, planes;
    };
    std::vector<std::unique_ptr<Part>> parts;
    const Part *on(int device) const {
        for (auto &p : parts)
            if (p->device == device) return p.get();
        return nullptr;
    }
};

namespace {

// ---- key transactions ------------------------------------------------------------------------
// A key write holds the context's mutex and keys_mu exclusively.  It is re-entrant per thread: a
// transaction (tfhe_mi355::begin_key_transaction, e.g. the serialized-key upload, which uploads the
// KSK, fills the Fourier buffer and marks it ready through three ABI calls) keeps both locks for its
// whole duration, and the nested calls on the same context from the same thread skip the locking.
thread_local std::vector<const TfheMi355Context *> tl_key_writes;

struct KeyWrite {
    TfheMi355Context *c = nullptr;
    std::unique_lock<std::mutex> g;
    std::unique_lock<std::shared_mutex> k;
    explicit KeyWrite(TfheMi355Context *c_) {
        if (std::find(tl_key_writes.begin(), tl_key_writes.end(), c_) != tl_key_writes.end()) return;
        c = c_;
        c->key_writers.fetch_add(1, std::memory_order_acq_rel);
        g = std::unique_lock<std::mutex>(c->mu);
        k = std::unique_lock<std::shared_mutex>(c->keys_mu);
        tl_key_writes.push_back(c);
    }
    KeyWrite(const KeyWrite &) = delete;
    KeyWrite &operator=(const KeyWrite &) = delete;
    ~KeyWrite() {
        if (!c) return;
        tl_key_writes.erase(std::find(tl_key_writes.begin(), tl_key_writes.end(), c));
        k.unlock();
        g.unlock();
        c->key_writers.fetch_sub(1, std::memory_order_acq_rel);
    }
};

// a coalesced batch reads the keys: it waits while an upload is pending (writer preference), then
// holds keys_mu shared for the batch
struct KeyRead {
    std::shared_lock<std::shared_mutex> k;
    explicit KeyRead(TfheMi355Context *c) {
        if (std::find(tl_key_writes.begin(), tl_key_writes.end(), c) != tl_key_writes.end()) return;
        while (c->key_writers.load(std::memory_order_acquire) > 0)
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        k = std::shared_lock<std::shared_mutex>(c->keys_mu);
    }
};

// cos and sin called separately through opaque pointers (no compiler fusion into sincos, whose
// last bits can differ): the same tables as the oracle's fft_init, bit for bit.
double (*volatile host_cos)(double) = static_cast<double (*)(double)>(std::cos);
double (*volatile host_sin)(double) = static_cast<double (*)(double)>(std::sin);

void build_tables(TfheMi355Context *c) {
    const int N = c->p.polynomial_size, M = N / 2;
    // W[t] = exp(-2 pi i t / M); twist w_j = exp(i pi j / N) as fft/mod.rs:58-69
    std::vector<double2> W(M), tw(M);
    for (int t = 0; t < M; t++) {
        double ang = 2.0 * M_PI * (double)t / (double)M;
        W[t] = make_double2(host_cos(ang), -host_sin(ang));
    }
    double unit = M_PI / (2.0 * (double)M);
    for (int j = 0; j < M; j++) {
        double a = (double)j * unit;
        tw[j] = make_double2(host_cos(a), host_sin(a));
    }
    size_t bytes = sizeof(double2) * M;
    check(hipMalloc(&c->tables.W, bytes), "hipMalloc(W)");
    check(hipMalloc(&c->tables.twist, bytes), "hipMalloc(twist)");
    check(hipMemcpy(c->tables.W, W.data(), bytes, hipMemcpyHostToDevice), "upload W");
    check(hipMemcpy(c->tables.twist, tw.data(), bytes, hipMemcpyHostToDevice), "upload twist");
    if (N >= 4096) {
        // the split CMUX's top radix-R stage (R = M / 1024) reads W[a c] for a < 1024: laid out
        // [c-1][a] so that a wave's 64 consecutive butterflies read 1 KiB contiguously instead of
        // 64 scattered lines
        const int A = 1024, R = M / A;
        std::vector<double2> top((size_t)(R - 1) * A);
        for (int c = 1; c < R; c++)
            for (int a = 0; a < A; a++) top[(size_t)(c - 1) * A + a] = W[(size_t)a * c];
        const size_t tb = sizeof(double2) * top.size();
        check(hipMalloc(&c->tables.wtop, tb), "hipMalloc(wtop)");
        check(hipMemcpy(c->tables.wtop, top.data(), tb, hipMemcpyHostToDevice), "upload wtop");
    }
    c->tables.N = N;
}

// one torus width per context: u64 uploads and compute calls refuse a context that holds u32 keys
void require_not_width128(const TfheMi355Context *c) {
    if (c->for_u128) fail("the context was created for the 128-bit torus: it serves the _u128 calls only");
    if (c->has_u128_keys()) fail("the context holds 128-bit-torus keys: other widths need a context of their own");
}
void require_width64(const TfheMi355Context *c) {
    if (c->has_u32_keys()) fail("the context holds 32-bit-torus keys: 64-bit calls need a context of their own");
    require_not_width128(c);
}
void require_width32(const TfheMi355Context *c) {
    if (c->has_u64_keys()) fail("the context holds 64-bit-torus keys: 32-bit calls need a context of their own");
    require_not_width128(c);
}
void require_fbsk(TfheMi355Context *c) {
    require_width64(c);
    if (!c->fbsk_ready) fail("bootstrapping key not uploaded");
}
void require_ksk(TfheMi355Context *c) {
    require_width64(c);
    if (!c->ksk_ready) fail("keyswitching key not uploaded");
}

hipError_t convert_bsk(TfheMi355Context *c, const uint64_t *d_std, size_t npoly, hipStream_t s) {
    if (large_pbs_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level))
        return launch_large_bsk_to_fourier(d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
    return launch_bsk_to_fourier((int)c->N(), d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
}

// ---- scratch sizes -----------------------------------------------------------------------------
// Every launcher takes its device scratch explicitly: the _async entry points pass the caller's
// d_scratch (sized by the *_scratch queries), the host-pointer entry points a lane's own buffer.

// the split CMUX of N >= 4096 (classic, or multi-bit at the N = 8192 sets): accumulators in scratch
bool is_large(const TfheMi355Context *c) {
    if (c->p.grouping_factor)
        return large_multibit_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level, (int)c->p.grouping_factor);
    return large_pbs_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level);
}

// N >= 4096: ciphertexts per pass of the split CMUX.  The chunk's accumulators + spectra should
// stay resident in the 256 MiB Infinity Cache: 128 at N = 32768 (1.5 MiB per ciphertext at 4_4,
// best of 64..1024 measured), otherwise ~200 MiB of scratch in multiples of 64 (64..1024) --
// round 4 sweeps (profiles/r04_chunk_sweep.log): 3_3 384 / 512 / 768 -> 5.94k / 6.17k / 5.55k,
// 2_5 192 / 256 -> 2268 / 2307, 1_4 832 / 1024 -> 13.5k / 14.3k KS+PBS/s (160 MiB gave 384 / 192 / 832);
// multi-bit mb3_3g3 (512 here) 384 / 512 / 768 / 1024 -> 9.11k / 9.30k / 8.59k / 8.19k (r04_mbchunk_*.log).
// Round 5, after the paired multi-bit kernel (large_mb_pair2_kernel) and the fused top_inv/top_fwd
// made the chunk's spectra traffic the smaller share: 512 / 768 / 1024 / 1280 / 2048 ->
// mb3_3g3 12.04k / 12.24k / 12.18k / 11.52k / 11.54k, mb3_3g2 10.21k / 10.44k / 10.63k / 9.65k /
// 9.65k (profiles/r05_mbchunk_*.json), so multi-bit takes 1024 (400 MiB of scratch).
size_t large_chunk(const TfheMi355Context *c) {
    static const size_t forced = [] {
        const char *e = std::getenv("TFHE_MI355_LARGE_CHUNK");
        const long x = e ? std::atol(e) : 0;
        return x > 0 ? (size_t)x : (size_t)0;
    }();
    if (forced) return forced;
    if (c->N() >= 32768) return 128;
    if (c->p.grouping_factor) return 1024;
    const size_t per = large_pbs_scratch_per_ct((int)c->N(), (int)c->k(), (int)c->p.pbs_level);
    return std::min<size_t>(1024, std::max<size_t>(64, ((size_t)200 << 20) / per / 64 * 64));
}

size_t pbs_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (count == 0 || (c->p.grouping_factor && !is_large(c))) return 0;
    if (!is_large(c)) return classic_pbs_ticket_bytes((int)c->N(), (int)c->k(), (int)c->p.pbs_level);
    const size_t per_ct = large_pbs_scratch_per_ct((int)c->N(), (int)c->k(), (int)c->p.pbs_level);
    return per_ct * std::min(count, large_chunk(c));
}

// The on-chip CMUX (the whole blind rotation in one workgroup: one ciphertext per CU at N = 8192,
// two per CU at N = 4096) against the split CMUX (a ciphertext's sub-blocks over several CUs, in several
// launches per CMUX): at 3_3 the split path takes 16.3 / 18.8 / 23.2 / 25.4 ms for 1 / 64 / 96 / 128
// ciphertexts, the on-chip one 22.9-25.1 ms for any count up to one per CU
// (profiles/r05_sweep33_onchip{0,1}.json); at 1_4 (N = 4096) split 11.0 / 13.3 / 14.0 / 19.3 ms for
// 1 / 96 / 128 / 192, on-chip 18.6-18.9 ms up to two per CU (r05_sweep14_onchip{0,1}.json).  So the
// on-chip kernel from 3/8 (N = 8192) / 5/8 (N = 4096) of the CU count on: 96 / 160 on MI355X.
// TFHE_MI355_ONCHIP_MIN overrides.
size_t onchip_min(const TfheMi355Context *c) {
    static const long env = [] {
        const char *e = std::getenv("TFHE_MI355_ONCHIP_MIN");
        return e && *e ? std::strtol(e, nullptr, 10) : -1L;
    }();
    if (env >= 0) return (size_t)env;
    return c->N() == 4096 ? (size_t)c->cus * 5 / 8 : (size_t)c->cus * 3 / 8;
}

// The quad CMUX (N = 8192, L = 1 or 2 classic, four CUs per ciphertext, pbs_large.hip; N = 4096: two CUs,
// the "duo") for batches of at most this many ciphertexts: one pass of CUs / R by default (R = N / 2048
// sub-blocks); TFHE_MI355_QUAD_MAX overrides (0 = never)
size_t quad_sub_blocks(const TfheMi355Context *c) { return c->N() / 2048; }
size_t quad_max(const TfheMi355Context *c) {
    if ((c->N() != 8192 && c->N() != 4096) || (c->p.pbs_level != 2 && c->p.pbs_level != 1) || c->p.grouping_factor ||
        c->k() != 1)
        return 0;
    static const long env = [] {
        const char *e = std::getenv("TFHE_MI355_QUAD_MAX");
        return e && *e ? std::strtol(e, nullptr, 10) : -1L;
    }();
    return env >= 0 ? (size_t)env : (size_t)c->cus / quad_sub_blocks(c);
}

// Batches of at most this many ciphertexts run the latency kernels (one ciphertext per CU) at the
// shapes they support.  Chosen by predicted time: the latency kernel takes one pass per CU-full of
// ciphertexts, the throughput kernel a time that steps with its ciphertexts per CU (<= 1024 rows:
// small batches spread over the CUs), so latency wins while passes x T_latency < T_throughput.
// Measured at 2_2 (profiles/r05_lat_sweep_{lat,thr}.json, 1..1024 rows): latency 2.54-2.60 ms per
// pass; throughput 5.6 / 6.0 / 8.6 / 8.8 ms at 1 / 2 / 3 / 4 ciphertexts per CU -> the latency
// kernel up to 3 passes (768 rows on 256 CUs: 7.7-8.0 vs 8.6 ms), the throughput kernel from the
// 4th (10.3 vs 8.8 ms).  Multi-bit (profiles/r05_lat_sweep_mb{3,2}_{lat,thr}.json): latency kernel
// 1.8-2.1 ms per pass (g = 3; 2.0 at g = 2), the slot-split throughput kernel 4.7-5.2 ms (g = 3;
// 5.0 at g = 2) for any batch up to 1024 rows -> two passes (512 rows: 4.25 vs 4.72 ms), not three
// (6.0 vs 4.7 ms).  TFHE_MI355_LATENCY_MAX overrides the row count for every shape (0 = never).
constexpr size_t kLatPassesClassic = 3, kLatPassesMb = 2;
size_t latency_max(const TfheMi355Context *c) {
    static const long forced = [] {
        const char *e = std::getenv("TFHE_MI355_LATENCY_MAX");
        return e && *e ? std::max(0L, std::atol(e)) : -1L;
    }();
    if (forced >= 0) return (size_t)forced;
    return (c->p.grouping_factor ? kLatPassesMb : kLatPassesClassic) * (size_t)c->cus;
}

bool ks_use_mfma(const TfheMi355Context *c) {
    static const bool disabled = env_flag("TFHE_MI355_KS_NO_MFMA");
    return !disabled && ks_mfma_supported((int)c->big_dim(), (int)c->p.ks_level, (int)c->p.ks_base_log);
}

size_t ks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (!c->ksk_planes_ready && !ks_use_mfma(c)) return 0;
    return count ? ks_mfma_scratch_bytes((int)c->big_dim(), (int)c->p.ks_level, (int)count) : 0;
}

// The packing key's decomposition (base, level) is part of the key, not of the parameter set, so
// this size is defined from the key's upload on (the scratch query fails before it); it follows
// from the decomposition and the MFMA eligibility alone, not from the repack having run.
bool pks_use_mfma(const TfheMi355Context *c) {
    static const bool disabled = env_flag("TFHE_MI355_KS_NO_MFMA");
    return !disabled && c->pks_level &&
           ks_mfma_supported((int)c->big_dim(), (int)c->pks_level, (int)c->pks_base_log);
}
size_t pks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (!pks_use_mfma(c) || count == 0) return 0;
    return ks_mfma_scratch_bytes((int)c->big_dim(), (int)c->pks_level, (int)count);
}

// KS -> PBS: the small-LWE intermediate, then (reused in stream order) the KS digits or the PBS
// chunk scratch
size_t ks_pbs_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return align256(count * (c->n() + 1) * 8) + std::max(ks_scratch_bytes(c, count), pbs_scratch_bytes(c, count));
}
// PBS -> KS: the big-LWE intermediate, then the PBS or KS scratch
size_t pbs_ks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return align256(count * (c->big_dim() + 1) * 8) + std::max(ks_scratch_bytes(c, count), pbs_scratch_bytes(c, count));
}

void require_scratch(size_t have, size_t need) {
    if (have < need) fail("device scratch too small: %zu bytes given, %zu needed (see the *_scratch queries)", have, need);
}

// ---- launchers ---------------------------------------------------------------------------------

void launch_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                    size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                    hipStream_t s, bool glwe_out = false) {
    require_fbsk(c);
    if (lut_count == 0) fail("lut_count must be >= 1");
    if (lut_count > 0xffffffffu) fail("lut_count too large");
    if (count > 0x7fffffff) fail("batch too large");
    if (count == 0) return;
    if (c->p.grouping_factor && !is_large(c)) {
        MultiBitPbsLaunch a;
        a.lwe_in = d_in;
        a.lwe_out = d_out;
        a.luts = d_luts;
        a.lut_indexes = d_idx;
        a.lut_count = (uint32_t)lut_count;
        a.fbsk = reinterpret_cast<const double2 *>(c->fbsk.ptr);
        a.W = c->tables.W;
        a.twist = c->tables.twist;
        a.n = (int)c->n();
        a.base_log = (int)c->p.pbs_base_log;
        a.count = (int)count;
        a.glwe_out = glwe_out;
        if (count <= latency_max(c) && latency_multibit_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level,
                                                                 (int)c->p.grouping_factor)) {
            TimedLaunch tl(c->timer_or_null(), "pbs_mb_latency_kernel", s);
            check(launch_latency_multibit_pbs((int)c->p.grouping_factor, a, s), "launch multi-bit latency pbs");
            return;
        }
        TimedLaunch tl(c->timer_or_null(), "pbs_multibit", s);
        check(launch_multibit_pbs((int)c->N(), (int)c->k(), (int)c->p.pbs_level, (int)c->p.grouping_factor, a, s),
              "launch multi-bit pbs");
        return;
    }
    if (is_large(c)) {
        if (glwe_out) fail("blind rotation without sample extraction is not available at N = %zu", c->N());
        const size_t per_ct = large_pbs_scratch_per_ct((int)c->N(), (int)c->k(), (int)c->p.pbs_level);
        if (!scratch || scratch_bytes < per_ct)
            fail("N = %zu PBS needs >= %zu bytes of device scratch per chunk ciphertext (%zu given)", c->N(), per_ct,
                 scratch_bytes);
        LargePbsLaunch a{};
        a.lwe_in = d_in;
        a.lwe_out = d_out;
        a.luts = d_luts;
        a.lut_indexes = d_idx;
        a.lut_count = (uint32_t)lut_count;
        a.fbsk = reinterpret_cast<const double2 *>(c->fbsk.ptr);
        a.W = c->tables.W;
        a.twist = c->tables.twist;
        a.wtop = c->tables.wtop;
        a.n = (int)c->n();
        a.base_log = (int)c->p.pbs_base_log;
        a.count = (int)count;
        a.scratch = scratch;
        a.scratch_bytes = std::min(scratch_bytes, per_ct * large_chunk(c));
        a.timer = c->timer_or_null();
        a.grouping = (int)c->p.grouping_factor;
        a.onchip_min_count = (int)onchip_min(c);
        a.quad_pass = (int)(c->cus / quad_sub_blocks(c));
        a.quad_max_count = (int)quad_max(c);
        if (a.quad_max_count > 0 && count <= (size_t)a.quad_max_count)
            a.quad_fail = static_cast<uint32_t *>(c->quad_fail.ptr);  // allocated with the context
        check(launch_large_pbs((int)c->N(), (int)c->k(), (int)c->p.pbs_level, a, s), "launch large pbs");
        return;
    }
    ClassicPbsLaunch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.luts = d_luts;
    a.lut_indexes = d_idx;
    a.lut_count = (uint32_t)lut_count;
    a.fbsk = reinterpret_cast<const double2 *>(c->fbsk.ptr);
    a.W = c->tables.W;
    a.twist = c->tables.twist;
    a.n = (int)c->n();
    a.base_log = (int)c->p.pbs_base_log;
    a.count = (int)count;
    a.glwe_out = glwe_out;
    // small batches: the latency kernel (one ciphertext per CU, all 8 waves on it; same outputs)
    if (count <= latency_max(c) && latency_pbs_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level)) {
#if LAT_STAMPS
        a.ticket = reinterpret_cast<uint32_t *>(scratch);  // diagnostic builds: the stamp buffer
#endif
        TimedLaunch tl(c->timer_or_null(), "pbs_latency_kernel", s);
        check(launch_latency_pbs(a, s), "launch latency pbs");
        return;
    }
    // persistent grid: a zeroed ticket word from the caller's scratch (none given: one pass)
    if (classic_pbs_ticket_bytes((int)c->N(), (int)c->k(), (int)c->p.pbs_level) && scratch && scratch_bytes >= 4) {
        a.ticket = reinterpret_cast<uint32_t *>(scratch);
        check(hipMemsetAsync(a.ticket, 0, sizeof(uint32_t), s), "zero pbs ticket");
    }
    TimedLaunch tl(c->timer_or_null(), "pbs_classic_kernel", s);
    check(launch_classic_pbs((int)c->N(), (int)c->k(), (int)c->p.pbs_level, a, s), "launch pbs");
}

// KSK -> int8 byte planes (once per key, after the u64 KSK is on the device)
void repack_ksk(TfheMi355Context *c, hipStream_t s) {
    c->ksk_planes_ready = false;
    if (!ks_use_mfma(c)) return;
    const size_t bytes = 8 * ks_mfma_rows((int)c->big_dim(), (int)c->p.ks_level) * ks_mfma_cols((int)c->n());
    c->ksk_planes.reserve(bytes);
    check(launch_ksk_repack((const uint64_t *)c->ksk.ptr, (int8_t *)c->ksk_planes.ptr, (int)c->big_dim(),
                            (int)c->p.ks_level, (int)c->n(), s),
          "ksk repack");
    c->ksk_planes_ready = true;
}

void launch_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, size_t count, void *scratch,
                   size_t scratch_bytes, hipStream_t s) {
    require_ksk(c);
    if (count == 0) return;
    if (count > 0x7fffffffu) fail("count too large");
    KeyswitchLaunch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.ksk = reinterpret_cast<const uint64_t *>(c->ksk.ptr);
    a.in_dim = (int)c->big_dim();
    a.out_dim = (int)c->n();
    a.base_log = (int)c->p.ks_base_log;
    a.level = (int)c->p.ks_level;
    a.count = (int)count;
    TimedLaunch tl(c->timer_or_null(), "keyswitch", s);
    if (c->ksk_planes_ready) {
        require_scratch(scratch ? scratch_bytes : 0, ks_scratch_bytes(c, count));
        check(launch_keyswitch_mfma(a, (const int8_t *)c->ksk_planes.ptr, scratch, s), "launch mfma keyswitch");
        return;
    }
    check(launch_keyswitch(a, s), "launch keyswitch");
}

// keyswitch under a key object, on shard (or single-device context) c
size_t ks_key_scratch_bytes(const TfheMi355KeyswitchKey *key, size_t count) {
    return key->mfma && count ? ks_mfma_scratch_bytes((int)key->in_dim, (int)key->level, (int)count) : 0;
}
void launch_ks_key_dev(TfheMi355Context *c, const TfheMi355KeyswitchKey *key, const uint64_t *d_in, uint64_t *d_out,
                       size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    const TfheMi355KeyswitchKey::Part *part = key->on(c->device);
    if (!part) fail("keyswitching key has no copy on device %d", c->device);
    if (count == 0) return;
    if (count > 0x7fffffffu) fail("count too large");
    KeyswitchLaunch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.ksk = reinterpret_cast<const uint64_t *>(part->ksk.ptr);
    a.in_dim = (int)key->in_dim;
    a.out_dim = (int)key->out_dim;
    a.base_log = (int)key->base_log;
    a.level = (int)key->level;
    a.count = (int)count;
    TimedLaunch tl(c->timer_or_null(), "keyswitch", s);
    if (key->mfma) {
        require_scratch(scratch ? scratch_bytes : 0, ks_key_scratch_bytes(key, count));
        check(launch_keyswitch_mfma(a, (const int8_t *)part->planes.ptr, scratch, s), "launch mfma keyswitch");
        return;
    }
    check(key->base_log > 7 ? launch_keyswitch_wide(a, s) : launch_keyswitch(a, s), "launch keyswitch");
}

// LWE -> GLWE packing keyswitch (lwe_packing_keyswitch.rs:102-186): the LWE keyswitch GEMM with
// (k+1)N-word GLWE rows and the input body landing on the GLWE body's constant term
KeyswitchLaunch packing_ks_args(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, size_t count) {
    KeyswitchLaunch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.ksk = reinterpret_cast<const uint64_t *>(c->pksk.ptr);
    a.in_dim = (int)c->big_dim();
    a.out_dim = (int)c->glwe_len() - 1;
    a.body_col = (int)c->big_dim();
    a.base_log = (int)c->pks_base_log;
    a.level = (int)c->pks_level;
    a.count = (int)count;
    return a;
}

void launch_packing_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, size_t count, void *scratch,
                           size_t scratch_bytes, hipStream_t s) {
    if (!c->pksk_ready) fail("packing keyswitching key not uploaded");
    if (count == 0) return;
    if (count > 0x7fffffffu) fail("count too large");
    KeyswitchLaunch a = packing_ks_args(c, d_in, d_out, count);
    if (c->pksk_planes_ready) {
        require_scratch(scratch ? scratch_bytes : 0, pks_scratch_bytes(c, count));
        check(launch_keyswitch_mfma(a, (const int8_t *)c->pksk_planes.ptr, scratch, s),
              "launch mfma packing keyswitch");
    } else {
        check(launch_keyswitch(a, s), "launch packing keyswitch");
    }
}

// shortint KS -> PBS on device: scratch = [small LWE intermediate | KS digits or PBS chunk scratch]
void launch_ks_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s) {
    require_fbsk(c);
    require_ksk(c);
    if (count == 0) return;
    require_scratch(scratch ? scratch_bytes : 0, ks_pbs_scratch_bytes(c, count));
    const size_t head = align256(count * (c->n() + 1) * 8);
    uint64_t *small = reinterpret_cast<uint64_t *>(scratch);
    void *rest = reinterpret_cast<char *>(scratch) + head;
    launch_ks_dev(c, d_in, small, count, rest, scratch_bytes - head, s);
    launch_pbs_dev(c, small, d_out, d_luts, lut_count, d_idx, count, rest, scratch_bytes - head, s);
}

// shortint PBS -> KS on device: scratch = [big LWE intermediate | PBS or KS scratch]
void launch_pbs_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s) {
    require_fbsk(c);
    require_ksk(c);
    if (count == 0) return;
    require_scratch(scratch ? scratch_bytes : 0, pbs_ks_scratch_bytes(c, count));
    const size_t head = align256(count * (c->big_dim() + 1) * 8);
    uint64_t *big = reinterpret_cast<uint64_t *>(scratch);
    void *rest = reinterpret_cast<char *>(scratch) + head;
    launch_pbs_dev(c, d_in, big, d_luts, lut_count, d_idx, count, rest, scratch_bytes - head, s);
    launch_ks_dev(c, big, d_out, count, rest, scratch_bytes - head, s);
}

void launch_glwe_poly_mul_dev(TfheMi355Context *c, const uint64_t *d_glwe, size_t glwe_per_item,
                              const uint64_t *d_polys, size_t npoly, size_t count, bool extract, uint64_t *d_out,
                              hipStream_t s) {
    if (glwe_per_item == 0 || glwe_per_item > 0xffff) fail("glwe_per_item out of range");
    if (npoly > 0x7fffffffu) fail("npoly too large");
    GlwePolyMulLaunch a;
    a.glwe_in = d_glwe;
    a.polys = d_polys;
    a.out = d_out;
    a.k = (int)c->k();
    a.N = (int)c->N();
    a.J = (int)glwe_per_item;
    a.npoly = (int)npoly;
    a.count = count;
    a.extract = extract;
    check(launch_glwe_poly_mul(a, s), "launch glwe poly mul");
}

// ---- GGSW operations (ggsw_ops.hip): per-item GGSW ciphertexts, decomposition chosen per call ----
// ---- GLWE x GLWE product with relinearisation (glwe_mult.hip) -----------------------------------
void require_rlk(const TfheMi355Context *c) {
    if (!c->rlk_ready) fail("relinearization key not uploaded");
}

void require_glwe_mult_shape(const TfheMi355Context *c) {
    if (!glwe_mult_supported((int)c->N(), (int)c->k()))
        fail("glwe_mult: N must be a power of two in [256, 2048], 1 <= k <= 5 and (k+1)*N <= 4096 (got N=%zu k=%zu)",
             c->N(), c->k());
}

void validate_log_p(uint32_t log_p) {
    if (log_p > 64) fail("glwe_mult: log_p %u > 64", log_p);
    if (log_p & 1) fail("glwe_mult: log_p %u is odd (the reference asserts an even one)", log_p);
}

// [a, a + an) and [b, b + bn) (u64 words) share a word
bool words_overlap(const uint64_t *a, size_t an, const uint64_t *b, size_t bn) {
    return an && bn && a < b + bn && b < a + an;
}

size_t glwe_mult_scratch(const TfheMi355Context *c, size_t count) {
    return align256(glwe_mult_scratch_bytes((int)c->N(), (int)c->k(), count));
}

void launch_glwe_mult_dev(TfheMi355Context *c, const uint64_t *d_lhs, const uint64_t *d_rhs, uint32_t log_p,
                          bool extract, uint64_t *d_out, size_t count, void *scratch, size_t scratch_bytes,
                          hipStream_t s) {
    require_glwe_mult_shape(c);
    validate_log_p(log_p);
    require_rlk(c);
    if (count == 0) return;
    if (count > 0x7fffffffu) fail("count too large");
    const size_t out_words = extract ? c->big_dim() + 1 : c->glwe_len();
    if (words_overlap(d_out, count * out_words, d_lhs, count * c->glwe_len()) ||
        words_overlap(d_out, count * out_words, d_rhs, count * c->glwe_len()))
        fail("glwe_mult: out overlaps an input");
    require_scratch(scratch ? scratch_bytes : 0, glwe_mult_scratch(c, count));
    GlweMultLaunch a;
    a.lhs = d_lhs;
    a.rhs = d_rhs;
    a.out = d_out;
    a.tr = reinterpret_cast<uint64_t *>(scratch);
    a.rlk = reinterpret_cast<const uint64_t *>(c->rlk.ptr);
    a.k = (int)c->k();
    a.N = (int)c->N();
    a.log_p = (int)log_p;
    a.base_log = (int)c->rlk_base_log;
    a.level = (int)c->rlk_level;
    a.extract = extract ? 1 : 0;
    a.count = count;
    a.timer = c->timer_or_null();
    check(launch_glwe_mult(a, s), "launch glwe_mult");
}

// lwe_mult: scratch = [2 count LWE rows, lhs then rhs | their packed GLWEs | packing-KS digits, then
// (reused in stream order) the product's T/R polynomials]
size_t lwe_mult_scratch(const TfheMi355Context *c, size_t count) {
    return align256(2 * count * (c->big_dim() + 1) * 8) + align256(2 * count * c->glwe_len() * 8) +
           std::max(align256(pks_scratch_bytes(c, 2 * count)), glwe_mult_scratch(c, count));
}

void launch_lwe_mult_dev(TfheMi355Context *c, const uint64_t *d_lhs, const uint64_t *d_rhs, uint32_t log_p,
                         uint64_t *d_out, size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_glwe_mult_shape(c);
    validate_log_p(log_p);
    require_rlk(c);
    if (!c->pksk_ready) fail("packing keyswitching key not uploaded");
    if (count == 0) return;
    if (count > 0x3fffffffu) fail("count too large");
    const size_t lwe = c->big_dim() + 1, glwe = c->glwe_len();
    if (words_overlap(d_out, count * lwe, d_lhs, count * lwe) || words_overlap(d_out, count * lwe, d_rhs, count * lwe))
        fail("lwe_mult: out overlaps an input");
    require_scratch(scratch ? scratch_bytes : 0, lwe_mult_scratch(c, count));
    char *p = reinterpret_cast<char *>(scratch);
    uint64_t *rows = reinterpret_cast<uint64_t *>(p);
    p += align256(2 * count * lwe * 8);
    uint64_t *packed = reinterpret_cast<uint64_t *>(p);
    p += align256(2 * count * glwe * 8);
    const size_t rest = scratch_bytes - (size_t)(p - reinterpret_cast<char *>(scratch));
    check(hipMemcpyAsync(rows, d_lhs, count * lwe * 8, hipMemcpyDeviceToDevice, s), "gather lhs");
    check(hipMemcpyAsync(rows + count * lwe, d_rhs, count * lwe * 8, hipMemcpyDeviceToDevice, s), "gather rhs");
    {
        TimedLaunch tl(c->timer_or_null(), "packing_keyswitch", s);
        launch_packing_ks_dev(c, rows, packed, 2 * count, p, rest, s);
    }
    launch_glwe_mult_dev(c, packed, packed + count * glwe, log_p, true, d_out, count, p, rest, s);
}

// host-pointer form of a two-input product: pairs in chunks through device buffers of the call's own,
// on the context's stream; f(d_lhs, d_rhs, d_out, n, d_scratch, scratch_bytes, stream) launches one chunk
template <class Scratch, class F>
void host_pair_call(TfheMi355Context *ctx, const uint64_t *lhs, const uint64_t *rhs, size_t in_words, uint64_t *out,
                    size_t out_words, size_t count, Scratch &&scratch_bytes, F &&f) {
    if (count == 0) return;
    const size_t chunk = std::min<size_t>(count, 4096);
    DeviceBuffer d_lhs, d_rhs, d_out, d_scr;
    d_lhs.reserve(chunk * in_words * 8);
    d_rhs.reserve(chunk * in_words * 8);
    d_out.reserve(chunk * out_words * 8);
    d_scr.reserve(std::max<size_t>(scratch_bytes(chunk), 256));
    hipStream_t s = ctx->stream;
    for (size_t a = 0; a < count; a += chunk) {
        const size_t n = std::min(chunk, count - a);
        check(hipMemcpyAsync(d_lhs.ptr, lhs + a * in_words, n * in_words * 8, hipMemcpyHostToDevice, s), "H2D lhs");
        check(hipMemcpyAsync(d_rhs.ptr, rhs + a * in_words, n * in_words * 8, hipMemcpyHostToDevice, s), "H2D rhs");
        f((const uint64_t *)d_lhs.ptr, (const uint64_t *)d_rhs.ptr, (uint64_t *)d_out.ptr, n, d_scr.ptr, d_scr.bytes, s);
        check(hipMemcpyAsync(out + a * out_words, d_out.ptr, n * out_words * 8, hipMemcpyDeviceToHost, s), "D2H out");
        check(hipStreamSynchronize(s), "product sync");
    }
}
size_t ggsw_polys(const TfheMi355Context *c, uint32_t level) { return (size_t)level * (c->k() + 1) * (c->k() + 1); }
size_t ggsw_std_words(const TfheMi355Context *c, uint32_t level) { return ggsw_polys(c, level) * c->N(); }
size_t ggsw_fourier_bytes(const TfheMi355Context *c, uint32_t level) {
    return ggsw_polys(c, level) * (c->N() / 2) * sizeof(double2);
}

void require_ggsw_shape(const TfheMi355Context *c, uint32_t base_log, uint32_t level) {
    if (!ggsw_ops_supported((int)c->N(), (int)c->k()))
        fail("GGSW operations support N in {256, 512, 1024, 2048} and 1 <= k <= 5, not N = %zu, k = %zu", c->N(), c->k());
    if (base_log == 0 || level == 0 || base_log > 32 || level > 32 || base_log * level > 32)
        fail("GGSW decomposition base_log %u x level %u outside the 32-bit decomposer (base_log * level <= 32)",
             base_log, level);
}

void validate_ggsw_indexes(const uint32_t *idx, size_t count, size_t ggsw_count) {
    if (!idx) {
        if (ggsw_count < count) fail("GGSW list has %zu ciphertexts for %zu items (no ggsw_indexes)", ggsw_count, count);
        return;
    }
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= ggsw_count) fail("ggsw_indexes[%zu] = %u out of range (ggsw_count %zu)", i, idx[i], ggsw_count);
}

void ggsw_list_to_fourier_dev(TfheMi355Context *c, const uint64_t *d_std, double2 *d_fourier, size_t ggsw_count,
                              uint32_t level, hipStream_t s) {
    TimedLaunch tl(c->timer_or_null(), "ggsw_to_fourier", s);
    check(launch_bsk_to_fourier((int)c->N(), d_std, d_fourier, ggsw_count * ggsw_polys(c, level), c->tables, s),
          "launch GGSW list conversion");
}

GgswCmuxLaunch ggsw_launch_args(TfheMi355Context *c, const double2 *d_fggsw, size_t ggsw_blocks, const uint32_t *d_idx,
                                uint32_t base_log, uint32_t level) {
    GgswCmuxLaunch a{};
    a.fggsw = d_fggsw;
    a.ggsw_indexes = d_idx;
    a.ggsw_blocks = ggsw_blocks;
    a.ggsw_per_item = 1;
    a.nodes_per_item = 1;
    a.in_stride = c->glwe_len();
    a.base_log = (int)base_log;
    a.level = (int)level;
    a.W = c->tables.W;
    a.twist = c->tables.twist;
    return a;
}

// external product (mode GGSW_EP: in1 = glwe_in, out accumulated) or CMUX (GGSW_CMUX) of `count` items
void launch_ggsw_node_dev(TfheMi355Context *c, int mode, const double2 *d_fggsw, size_t ggsw_count,
                          const uint32_t *d_idx, uint32_t base_log, uint32_t level, const uint64_t *d_in0,
                          const uint64_t *d_in1, uint64_t *d_out, size_t count, hipStream_t s) {
    require_ggsw_shape(c, base_log, level);
    if (count == 0) return;
    if (ggsw_count == 0) fail("empty GGSW list");
    if (!d_idx && ggsw_count < count) fail("GGSW list has %zu ciphertexts for %zu items (no ggsw_indexes)", ggsw_count, count);
    GgswCmuxLaunch a = ggsw_launch_args(c, d_fggsw, ggsw_count, d_idx, base_log, level);
    a.mode = mode;
    a.in0 = d_in0;
    a.in1 = d_in1;
    a.out = d_out;
    a.nodes = count;
    TimedLaunch tl(c->timer_or_null(), mode == GGSW_EP ? "ggsw_external_product" : "ggsw_cmux", s);
    check(launch_ggsw_cmux((int)c->N(), (int)c->k(), a, s), "launch GGSW node");
}

// vertical packing: log2(npoly) tree bits, then nbits - log2(npoly) rotation bits
struct VpShape {
    uint32_t nt, nr;
};
VpShape vp_shape(const TfheMi355Context *c, uint32_t nbits, size_t npoly) {
    if (npoly == 0 || npoly > 0x40000000u || !is_pow2((uint32_t)npoly))
        fail("vertical packing: the LUT has %zu polynomials, not a power of two", npoly);
    uint32_t nt = 0;
    while (((size_t)1 << nt) < npoly) nt++;
    if (nbits == 0) fail("vertical packing: no GGSW ciphertext");
    if (nt > nbits) fail("vertical packing: %zu LUT polynomials need %u tree bits, only %u GGSWs given", npoly, nt, nbits);
    uint32_t log2n = 0;
    while (((size_t)1 << log2n) < c->N()) log2n++;
    if (nbits - nt > log2n)
        fail("vertical packing: %u rotation bits exceed log2(N) = %u", nbits - nt, log2n);
    return {nt, nbits - nt};
}

// two ping-pong GLWE buffers per (item, output): the tree's first level leaves npoly/2 nodes, the next
// npoly/4; without a tree the first holds the rotation steps' accumulator
size_t vp_scratch_bytes(const TfheMi355Context *c, size_t npoly, size_t nout, size_t count) {
    const size_t a = std::max<size_t>(npoly / 2, 1), b = std::max<size_t>(npoly / 4, 1);
    return align256(count * nout * a * c->glwe_len() * 8) + align256(count * nout * b * c->glwe_len() * 8);
}

// TFHE_MI355_VP_STEPWISE=1: one launch per rotation step instead of the chain launch (A/B arm); read at
// every call, so that one process can run both arms
bool vp_stepwise() { return env_flag("TFHE_MI355_VP_STEPWISE"); }

// luts [lut_count][nout][npoly][N], d_lwe_out [count][nout][kN+1]: every launch covers the nout outputs
// of every item (GgswCmuxLaunch::nout), so a tree level is one launch over count nout (npoly >> (j+1))
// nodes and the rotation steps are one chain launch over count nout nodes
void launch_vertical_packing_dev(TfheMi355Context *c, const double2 *d_fggsw, uint32_t base_log, uint32_t level,
                                 uint32_t nbits, const uint64_t *d_luts, size_t lut_count, size_t nout, size_t npoly,
                                 const uint32_t *d_lut_idx, size_t count, uint64_t *d_lwe_out, void *scratch,
                                 size_t scratch_bytes, hipStream_t s) {
    require_ggsw_shape(c, base_log, level);
    const VpShape sh = vp_shape(c, nbits, npoly);
    if (lut_count == 0 || lut_count > 0xffffffffu) fail("lut_count out of range");
    if (nout == 0 || nout > 0xffffu) fail("vertical packing: nout %zu out of range", nout);
    if (count == 0) return;
    if (count > 0x7fffffffu / (nout * std::max<size_t>(npoly / 2, 1))) fail("count too large");
    require_scratch(scratch ? scratch_bytes : 0, vp_scratch_bytes(c, npoly, nout, count));
    const size_t glwe = c->glwe_len();
    uint64_t *buf[2] = {
        reinterpret_cast<uint64_t *>(scratch),
        reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(scratch) +
                                     align256(count * nout * std::max<size_t>(npoly / 2, 1) * glwe * 8))};
    GgswCmuxLaunch a = ggsw_launch_args(c, d_fggsw, count, nullptr, base_log, level);
    a.ggsw_per_item = (int)nbits;
    a.lut_indexes = d_lut_idx;
    a.lut_count = (uint32_t)lut_count;
    a.npoly = (int)npoly;
    a.nout = (int)nout;
    const uint64_t *cur = nullptr;  // the accumulators so far (null: still the LUT itself)
    // CMUX tree, level by level: layer j pairs the nodes (2i, 2i+1) of the layer before under GGSW
    // nt-1-j (the list is most significant bit first; cmux_tree_memory_optimized walks it reversed)
    for (uint32_t j = 0; j < sh.nt; j++) {
        const bool last = j + 1 == sh.nt && sh.nr == 0;
        a.mode = GGSW_CMUX;
        a.leaf = cur == nullptr;
        a.ggsw_sel = (int)(sh.nt - 1 - j);
        a.nodes_per_item = npoly >> (j + 1);
        a.nodes = count * nout * a.nodes_per_item;
        a.in0 = cur ? cur : d_luts;
        a.in1 = cur ? cur + glwe : nullptr;
        a.in_stride = 2 * glwe;
        a.extract = last;
        a.out = last ? d_lwe_out : buf[j & 1];
        TimedLaunch tl(c->timer_or_null(), "ggsw_cmux_tree", s);
        check(launch_ggsw_cmux((int)c->N(), (int)c->k(), a, s), "launch CMUX tree level");
        cur = a.out;
    }
    // blind rotation by the remaining GGSWs, last first, monomial degrees 1, 2, 4, ... (in place): one
    // chain launch runs every step and the sample extraction
    if (sh.nr && !vp_stepwise()) {
        a.mode = GGSW_ROT;
        a.leaf = cur == nullptr;
        a.ggsw_sel = (int)(nbits - 1);
        a.rot = 1;
        a.chain = (int)sh.nr;
        a.nodes_per_item = 1;
        a.nodes = count * nout;
        a.in0 = cur ? cur : d_luts;
        a.in1 = nullptr;
        a.in_stride = glwe;
        a.acc = cur ? const_cast<uint64_t *>(cur) : buf[0];
        a.extract = 1;
        a.out = d_lwe_out;
        TimedLaunch tl(c->timer_or_null(), "ggsw_rotate_chain", s);
        check(launch_ggsw_cmux((int)c->N(), (int)c->k(), a, s), "launch rotation chain");
        return;
    }
    for (uint32_t i = 0; i < sh.nr; i++) {
        const bool last = i + 1 == sh.nr;
        a.mode = GGSW_ROT;
        a.leaf = cur == nullptr;
        a.ggsw_sel = (int)(nbits - 1 - i);
        a.rot = 1 << i;
        a.nodes_per_item = 1;
        a.nodes = count * nout;
        a.in0 = cur ? cur : d_luts;
        a.in1 = nullptr;
        a.in_stride = glwe;
        a.extract = last;
        a.out = last ? d_lwe_out : (cur ? const_cast<uint64_t *>(cur) : buf[0]);
        TimedLaunch tl(c->timer_or_null(), "ggsw_rotate", s);
        check(launch_ggsw_cmux((int)c->N(), (int)c->k(), a, s), "launch rotation step");
        cur = a.out;
    }
}

// ---- WoP-PBS, the bootstrapped half: pfpks, bit extraction, circuit bootstrap -----------------------
// The pfpksk list's decomposition belongs to the key (as the packing key's): the scratch sizes are
// defined from its upload on.
bool pfpks_use_mfma(const TfheMi355Context *c) {
    static const bool disabled = env_flag("TFHE_MI355_PFPKS_NO_MFMA");
    return !disabled && c->pfks_level &&
           pfpks_mfma_supported((int)c->big_dim() + 1, (int)c->pfks_level, (int)c->pfks_base_log);
}
size_t pfpks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (!pfpks_use_mfma(c) || count == 0) return 0;
    return pfpks_mfma_scratch_bytes((int)c->big_dim() + 1, (int)c->pfks_level, (int)count);
}
void require_pfpksk(const TfheMi355Context *c) {
    if (!c->pfpksk_ready) fail("private functional packing keyswitching keys not uploaded");
}

// rows of one pfpks launch: 64-row tiles in grid.y
constexpr size_t kPfpksMaxRows = (size_t)65535 * 64;

void launch_pfpks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, size_t count, void *scratch,
                      size_t scratch_bytes, hipStream_t s) {
    require_pfpksk(c);
    if (count == 0) return;
    if (count > kPfpksMaxRows) fail("count too large");
    PfpksLaunch a;
    a.lwe_in = d_in;
    a.glwe_out = d_out;
    a.key = reinterpret_cast<const uint64_t *>(c->pfpksk.ptr);
    a.in_rows = (int)c->big_dim() + 1;
    a.glwe = (int)c->glwe_len();
    a.ncols = (int)((c->k() + 1) * c->glwe_len());
    a.base_log = (int)c->pfks_base_log;
    a.level = (int)c->pfks_level;
    a.count = (int)count;
    if (c->pfpksk_planes_ready) {
        require_scratch(scratch ? scratch_bytes : 0, pfpks_scratch_bytes(c, count));
        TimedLaunch tl(c->timer_or_null(), "pfpks_mfma", s);
        check(launch_pfpks_mfma(a, (const int8_t *)c->pfpksk_planes.ptr, scratch, s), "launch mfma pfpks");
    } else {
        TimedLaunch tl(c->timer_or_null(), "pfpks_generic", s);
        check(launch_pfpks(a, s), "launch pfpks");
    }
}

// the circuit bootstrap and the bit extraction run the classic PBS and the GGSW kernels' shapes
void require_wop_shape(const TfheMi355Context *c) {
    if (c->p.grouping_factor || is_large(c) || !ggsw_ops_supported((int)c->N(), (int)c->k()))
        fail("WoP-PBS needs a classic PBS shape with N in {256, 512, 1024, 2048} and 1 <= k <= 5, not N = %zu, k = %zu, "
             "grouping_factor = %u",
             c->N(), c->k(), c->p.grouping_factor);
}

// bit extraction (wop_pbs/mod.rs:66-225): scratch = [running input | shifted input | keyswitch output |
// LUT | PBS output | keyswitch digits or PBS scratch]
void validate_extract_bits(uint32_t delta_log, uint32_t nbits) {
    if (nbits == 0) fail("extract_bits: no bit to extract");
    if (delta_log > 64 || nbits > 64 || delta_log + nbits > 64)
        fail("extract_bits: delta_log %u + nbits %u exceeds the 64 bits of a ciphertext word", delta_log, nbits);
    if (delta_log == 0 && nbits > 1)
        fail("extract_bits: delta_log 0 with %u bits (the LUT of the lowest bit would be 2^-1)", nbits);
}
size_t extract_bits_scratch_bytes(const TfheMi355Context *c, size_t count) {
    const size_t big = align256(count * (c->big_dim() + 1) * 8), small = align256(count * (c->n() + 1) * 8);
    return 3 * big + small + align256(c->glwe_len() * 8) +
           std::max<size_t>(std::max(ks_scratch_bytes(c, count), pbs_scratch_bytes(c, count)), 256);
}
void launch_extract_bits_dev(TfheMi355Context *c, const uint64_t *d_in, uint32_t delta_log, uint32_t nbits,
                             uint64_t *d_out, size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_wop_shape(c);
    require_fbsk(c);
    require_ksk(c);
    validate_extract_bits(delta_log, nbits);
    if (count == 0) return;
    if (count > 0x7fffffffu / nbits) fail("count too large");
    require_scratch(scratch ? scratch_bytes : 0, extract_bits_scratch_bytes(c, count));
    const size_t bw = c->big_dim() + 1, sw = c->n() + 1;
    const size_t big = align256(count * bw * 8), small = align256(count * sw * 8), lut_b = align256(c->glwe_len() * 8);
    char *p = reinterpret_cast<char *>(scratch);
    uint64_t *cur = reinterpret_cast<uint64_t *>(p);
    uint64_t *shifted = reinterpret_cast<uint64_t *>(p + big);
    uint64_t *pbs_out = reinterpret_cast<uint64_t *>(p + 2 * big);
    uint64_t *ks_out = reinterpret_cast<uint64_t *>(p + 3 * big);
    uint64_t *lut = reinterpret_cast<uint64_t *>(p + 3 * big + small);
    void *rest = p + 3 * big + small + lut_b;
    const size_t rest_bytes = scratch_bytes - (3 * big + small + lut_b);
    check(hipMemcpyAsync(cur, d_in, count * bw * 8, hipMemcpyDeviceToDevice, s), "extract_bits: copy input");
    for (uint32_t b = 0; b < nbits; b++) {
        {
            TimedLaunch tl(c->timer_or_null(), "wop_glue", s);
            check(launch_wop_shift_rows(shifted, cur, count, bw, bw, 1, (int)(64 - delta_log - b - 1), 0, s),
                  "extract_bits: shift");
        }
        launch_ks_dev(c, shifted, ks_out, count, rest, rest_bytes, s);
        const bool last = b + 1 == nbits;
        {
            TimedLaunch tl(c->timer_or_null(), "wop_glue", s);
            // slot nbits-1-b of the item's output list; then q/4 on the keyswitch output's body
            check(launch_wop_shift_rows(d_out + (size_t)(nbits - 1 - b) * sw, ks_out, count, sw, (size_t)nbits * sw, 1, 0, 0, s),
                  "extract_bits: store");
            if (last) break;
            check(launch_wop_add_body(ks_out, count, sw, 62, 0, 1, s), "extract_bits: q/4");
            check(launch_wop_fill_luts(lut, 1, c->glwe_len(), c->big_dim(), (int)(delta_log - 1 + b), 0, nullptr, 0, s),
                  "extract_bits: LUT");
        }
        launch_pbs_dev(c, ks_out, pbs_out, lut, 1, nullptr, count, rest, rest_bytes, s);
        TimedLaunch tl(c->timer_or_null(), "wop_glue", s);
        check(launch_wop_sub_rows(cur, pbs_out, count, bw, (uint64_t)1 << (delta_log + b - 1), s), "extract_bits: subtract");
    }
}

// circuit bootstrap (wop_pbs/mod.rs:243-444): one PBS launch over count * Lc rows (level l of an item
// under LUT l), one pfpks launch over the same rows writing the GGSW list [count][Lc][k+1][(k+1)N].
// scratch = [shifted rows | LUTs | LUT indexes | PBS output | PBS ticket or pfpks digits]
void validate_cbs(const TfheMi355Context *c, uint32_t delta_log, uint32_t base_log, uint32_t level) {
    require_ggsw_shape(c, base_log, level);
    if (delta_log > 63) fail("circuit bootstrap: delta_log %u out of range (at most 63)", delta_log);
}
size_t cbs_scratch_bytes(const TfheMi355Context *c, uint32_t level, size_t count) {
    const size_t rows = count * level;
    return align256(rows * (c->n() + 1) * 8) + align256((size_t)level * c->glwe_len() * 8) + align256(rows * 4) +
           align256(rows * (c->big_dim() + 1) * 8) +
           std::max<size_t>(std::max(pbs_scratch_bytes(c, rows), pfpks_scratch_bytes(c, rows)), 256);
}
void launch_cbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint32_t delta_log, uint32_t base_log, uint32_t level,
                    uint64_t *d_ggsw_out, size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_wop_shape(c);
    validate_cbs(c, delta_log, base_log, level);
    require_fbsk(c);
    require_pfpksk(c);
    if (count == 0) return;
    if (count > kPfpksMaxRows / level) fail("count too large");
    require_scratch(scratch ? scratch_bytes : 0, cbs_scratch_bytes(c, level, count));
    const size_t rows = count * level, sw = c->n() + 1, bw = c->big_dim() + 1;
    const size_t o1 = align256(rows * sw * 8), o2 = o1 + align256((size_t)level * c->glwe_len() * 8),
                 o3 = o2 + align256(rows * 4), o4 = o3 + align256(rows * bw * 8);
    char *p = reinterpret_cast<char *>(scratch);
    uint64_t *shifted = reinterpret_cast<uint64_t *>(p);
    uint64_t *luts = reinterpret_cast<uint64_t *>(p + o1);
    uint32_t *idx = reinterpret_cast<uint32_t *>(p + o2);
    uint64_t *pbs_out = reinterpret_cast<uint64_t *>(p + o3);
    void *rest = p + o4;
    const size_t rest_bytes = scratch_bytes - o4;
    {
        TimedLaunch tl(c->timer_or_null(), "wop_glue", s);
        check(launch_wop_shift_rows(shifted, d_in, rows, sw, sw, level, (int)(63 - delta_log), (uint64_t)1 << 62, s),
              "circuit bootstrap: shift");
        check(launch_wop_fill_luts(luts, level, c->glwe_len(), c->big_dim(), (int)(63 - base_log), (int)base_log, idx,
                                   rows, s),
              "circuit bootstrap: LUTs");
    }
    launch_pbs_dev(c, shifted, pbs_out, luts, level, idx, rows, rest, rest_bytes, s);
    {
        TimedLaunch tl(c->timer_or_null(), "wop_glue", s);
        check(launch_wop_add_body(pbs_out, rows, bw, (int)(63 - base_log), (int)base_log, level, s),
              "circuit bootstrap: add alpha");
    }
    launch_pfpks_dev(c, pbs_out, d_ggsw_out, rows, rest, rest_bytes, s);
}

// circuit_bootstrap_boolean_vertical_packing (wop_pbs/mod.rs:647-746): lwe_in [count][nbits] bits at
// q/2, luts [lut_count][nout][npoly][N]; output o of an item is the vertical packing of polynomials
// [o npoly, (o+1) npoly) of its LUT, under the same GGSWs: one vertical packing over (item, output).
// scratch = [standard GGSWs | Fourier GGSWs | circuit bootstrap or vertical packing scratch]
struct CbvpLayout {
    size_t std_b, four_b, rest_b;
    size_t total() const { return std_b + four_b + rest_b; }
};
CbvpLayout cbvp_layout(const TfheMi355Context *c, uint32_t nbits, uint32_t level, size_t nout, size_t npoly,
                       size_t lut_count, size_t count) {
    CbvpLayout l;
    l.std_b = align256(count * nbits * ggsw_std_words(c, level) * 8);
    l.four_b = align256(count * nbits * ggsw_fourier_bytes(c, level));
    l.rest_b = std::max(cbs_scratch_bytes(c, level, count * nbits),
                        std::max<size_t>(vp_scratch_bytes(c, npoly, nout, count), 256));
    return l;
}
void launch_cbvp_dev(TfheMi355Context *c, const uint64_t *d_in, uint32_t nbits, uint32_t base_log, uint32_t level,
                     const uint64_t *d_luts, size_t lut_count, size_t nout, size_t npoly, const uint32_t *d_lut_idx,
                     size_t count, uint64_t *d_out, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_wop_shape(c);
    validate_cbs(c, 63, base_log, level);
    vp_shape(c, nbits, npoly);
    if (nout == 0 || nout > 0xffffu) fail("circuit bootstrap + vertical packing: nout %zu out of range", nout);
    if (lut_count == 0 || lut_count > 0xffffffffu) fail("lut_count out of range");
    if (count == 0) return;
    if (count > kPfpksMaxRows / ((size_t)nbits * level)) fail("count too large");
    const CbvpLayout l = cbvp_layout(c, nbits, level, nout, npoly, lut_count, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    char *p = reinterpret_cast<char *>(scratch);
    uint64_t *ggsw_std = reinterpret_cast<uint64_t *>(p);
    double2 *ggsw_f = reinterpret_cast<double2 *>(p + l.std_b);
    void *rest = p + l.std_b + l.four_b;
    launch_cbs_dev(c, d_in, 63, base_log, level, ggsw_std, count * nbits, rest, l.rest_b, s);
    ggsw_list_to_fourier_dev(c, ggsw_std, ggsw_f, count * nbits, level, s);
    launch_vertical_packing_dev(c, ggsw_f, base_log, level, nbits, d_luts, lut_count, nout, npoly, d_lut_idx, count,
                                d_out, rest, l.rest_b, s);
}

void validate_lut_indexes(const uint32_t *idx, size_t count, size_t lut_count) {
    if (!idx) return;
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= lut_count) fail("lut_indexes[%zu] = %u out of range (lut_count %zu)", i, idx[i], lut_count);
}

// ---- host-pointer pipeline ------------------------------------------------------------------------
// The synchronous entry points (host buffers in and out, the form the Rust binding calls) run the
// batch in chunks: per chunk, the host input slice is copied into a lane's page-locked buffer and
// DMA'd up on the lane's copy stream, the kernels run on ctx->stream (chunks in order, so the GPU
// stays busy), and the output is DMA'd back on the copy stream and copied into the caller's
// buffer while the next chunk's kernels run.  The LUTs go up once per call.  Callers are
// serialised by ctx->mu.

using ChunkLaunch = void (*)(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                             size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch,
                             size_t scratch_bytes, hipStream_t s);
using ScratchSize = size_t (*)(const TfheMi355Context *c, size_t count);

size_t host_chunk(const TfheMi355Context *c, size_t count) {
    static const size_t forced = [] {
        const char *e = std::getenv("TFHE_MI355_HOST_CHUNK");
        const long x = e ? std::atol(e) : 0;
        return x > 0 ? (size_t)x : (size_t)0;
    }();
    if (forced) return forced;
    if (is_large(c)) return large_chunk(c);
    // >= 4 chunks so that copies hide behind kernels (also with pinned caller buffers: 2 chunks
    // measured 93.5k vs 112.9k PBS/s at 4096); >= one full wave of PBS slots (256 CUs x 4
    // ciphertexts) and <= 4 waves per launch
    const size_t slots = 1024;
    const size_t quarter = (count + 3) / 4;
    return std::min<size_t>(4 * slots, std::max(slots, (quarter + slots - 1) / slots * slots));
}

// true when [p, p + bytes) is page-locked host memory (tfhe_mi355_host_alloc, hipHostMalloc or
// hipHostRegister): the pipeline then DMAs straight from / into the caller's buffer
bool is_pinned(const void *p, size_t bytes) {
    if (!p || !bytes) return false;
    for (const void *q : {p, (const void *)((const char *)p + bytes - 1)}) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();  // pageable memory: clear the non-sticky error
            return false;
        }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

void lane_finish(TfheMi355Context::Lane &L, void *out, size_t out_words) {
    if (!L.pending) return;
    L.pending = false;
    check(hipEventSynchronize(L.done), "chunk sync");
    if (!L.direct_out)
        std::memcpy(static_cast<uint64_t *>(out) + L.first * out_words, L.h_out.ptr, L.count * out_words * 8);
}

// after a synchronous call's device work: a quad CMUX launch of this context whose flag wait timed
// out (its partner workgroups never became resident -- e.g. another process's quad grid held the
// CUs) left invalid outputs; fail the call loudly instead of returning them
void check_quad_fail(TfheMi355Context *c) {
    if (!c->quad_fail.ptr) return;
    uint32_t v = 0;
    check(hipMemcpy(&v, c->quad_fail.ptr, 4, hipMemcpyDeviceToHost), "quad fail word");
    if (v) {
        (void)hipMemset(c->quad_fail.ptr, 0, 4);
        fail("quad CMUX: a workgroup waited in vain for its partners (is another process running quad CMUX "
             "kernels on this GPU?); the outputs are invalid -- TFHE_MI355_QUAD=0 disables the quad CMUX");
    }
}

void run_host_pipeline(TfheMi355Context *c, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                       const uint64_t *luts, size_t lut_words, size_t lut_count, const uint32_t *idx, size_t count,
                       ChunkLaunch launch, ScratchSize scratch_size) {
    if (count == 0) return;
    hipStream_t cs = c->stream;
    const uint64_t *d_luts = nullptr;
    if (luts) {  // on the kernel stream: ordered before every chunk's kernels
        c->io_luts.reserve(lut_count * lut_words * 8);
        check(hipMemcpyAsync(c->io_luts.ptr, luts, lut_count * lut_words * 8, hipMemcpyHostToDevice, cs),
              "H2D luts");
        d_luts = (const uint64_t *)c->io_luts.ptr;
    }
    // page-locked caller buffers are DMA'd directly (no staging copies on the host)
    const bool pin_in = is_pinned(in, count * in_words * 8), pin_out = is_pinned(out, count * out_words * 8);
    const size_t chunk = std::min(count, host_chunk(c, count));
    // kernels of consecutive chunks are ordered on cs: one scratch serves them all
    const size_t need_scratch = scratch_size ? scratch_size(c, chunk) : 0;
    if (need_scratch) c->io_tmp.reserve(need_scratch);
    try {
        size_t next = 0;
        for (int q = 0; next < count; q ^= 1) {
            TfheMi355Context::Lane &L = c->lanes[q];
            lane_finish(L, out, out_words);  // this lane's previous chunk: all its device work is done
            const size_t cnt = std::min(chunk, count - next);
            if (!pin_in) L.h_in.reserve(chunk * in_words * 8);
            if (!pin_out) L.h_out.reserve(chunk * out_words * 8);
            L.d_in.reserve(chunk * in_words * 8);
            L.d_out.reserve(chunk * out_words * 8);
            const uint64_t *src = in + next * in_words;
            if (!pin_in) {
                std::memcpy(L.h_in.ptr, src, cnt * in_words * 8);
                src = (const uint64_t *)L.h_in.ptr;
            }
            check(hipMemcpyAsync(L.d_in.ptr, src, cnt * in_words * 8, hipMemcpyHostToDevice, L.stream), "H2D in");
            const uint32_t *d_idx = nullptr;
            if (idx) {
                L.h_idx.reserve(chunk * 4);
                L.d_idx.reserve(chunk * 4);
                std::memcpy(L.h_idx.ptr, idx + next, cnt * 4);
                check(hipMemcpyAsync(L.d_idx.ptr, L.h_idx.ptr, cnt * 4, hipMemcpyHostToDevice, L.stream), "H2D idx");
                d_idx = (const uint32_t *)L.d_idx.ptr;
            }
            check(hipEventRecord(L.h2d, L.stream), "h2d event");
            check(hipStreamWaitEvent(cs, L.h2d, 0), "wait h2d");
            launch(c, (const uint64_t *)L.d_in.ptr, (uint64_t *)L.d_out.ptr, d_luts, lut_count, d_idx, cnt,
                   need_scratch ? c->io_tmp.ptr : nullptr, need_scratch ? c->io_tmp.bytes : 0, cs);
            check(hipEventRecord(L.kern, cs), "kernel event");
            check(hipStreamWaitEvent(L.stream, L.kern, 0), "wait kernels");
            L.direct_out = pin_out;
            check(hipMemcpyAsync(pin_out ? (void *)(out + next * out_words) : L.h_out.ptr, L.d_out.ptr,
                                 cnt * out_words * 8, hipMemcpyDeviceToHost, L.stream),
                  "D2H out");
            check(hipEventRecord(L.done, L.stream), "chunk event");
            L.pending = true;
            L.first = next;
            L.count = cnt;
            next += cnt;
        }
        // retire in chunk order: the lane holding the older chunk first
        TfheMi355Context::Lane &a = c->lanes[0], &b = c->lanes[1];
        if (a.pending && b.pending && b.first < a.first) {
            lane_finish(b, out, out_words);
            lane_finish(a, out, out_words);
        } else {
            lane_finish(a, out, out_words);
            lane_finish(b, out, out_words);
        }
        check_quad_fail(c);
    } catch (...) {
        (void)hipStreamSynchronize(cs);
        for (auto &L : c->lanes) {
            (void)hipStreamSynchronize(L.stream);
            L.pending = false;
        }
        throw;
    }
}

// adapters of the launchers to ChunkLaunch
void chunk_pbs(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *l, size_t lc, const uint32_t *x,
               size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_pbs_dev(c, i, o, l, lc, x, n, sc, sb, s);
}
void chunk_blind_rotate(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *l, size_t lc,
                        const uint32_t *x, size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_pbs_dev(c, i, o, l, lc, x, n, sc, sb, s, true);
}
void chunk_ks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
              size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_ks_dev(c, i, o, n, sc, sb, s);
}
void chunk_pks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
               size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_packing_ks_dev(c, i, o, n, sc, sb, s);
}

// ---- request coalescing ---------------------------------------------------------------------------
// Calls of at most coalesce_max_count() ciphertexts (default 64; TFHE_MI355_COALESCE_MAX_COUNT,
// 0 = off) are coalesced: up to coalesce_batch() ciphertexts (default 1024, one ciphertext per PBS
// slot of the chip at 2_2) gathered until no call has arrived for coalesce_gap() (default 50 us),
// for at most coalesce_window() (default 1000 us) from the first queued call.  Both are small next
// to a PBS (milliseconds), and a full batch leaves at once.
size_t env_size(const char *name, size_t dflt) {
    const char *e = std::getenv(name);
    if (!e || !*e) return dflt;
    const long x = std::atol(e);
    return x >= 0 ? (size_t)x : dflt;
}
size_t coalesce_batch() {
    static const size_t v = std::max<size_t>(env_size("TFHE_MI355_COALESCE_BATCH", 1024), 1);
    return v;
}
// never above the batch size: a dispatcher always takes its queue's first request whole, and the
// slot staging is sized for one batch
size_t coalesce_max_count() {
    static const size_t v = std::min(env_size("TFHE_MI355_COALESCE_MAX_COUNT", 64), coalesce_batch());
    return v;
}
// batch slots (dispatcher threads, up to 8): batches in flight at once, each on its own stream.
// A PBS batch takes about one CMUX chain (6-9 ms at 2_2) whatever its size up to a chip-full, so
// by Little's law T callers get at most T / (chain + window) calls/s; a second slot that starts
// whenever work is queued only splits the callers into half batches that the device does not
// overlap (measured at 64 / 256 synchronous callers: 1 slot 10.4k / 37.5k calls/s, 2 slots
// 10.3k / 30.4k, 3 slots 7.6k / 26.7k).  So a slot other than the first starts only when
// coalesce_overflow() rows are queued (coalesce_dispatcher): synchronous callers see one slot,
// while submit/wait callers with thousands of requests in flight overlap host staging with the
// device (64 threads x 64 in flight: 92k calls/s with 1 slot, 108-113k with 2).  Default 2.
size_t coalesce_slots() {
    static const size_t v = std::min<size_t>(std::max<size_t>(env_size("TFHE_MI355_COALESCE_SLOTS", 2), 1), 8);
    return v;
}
// queued ciphertexts of one op that start a batch on a second slot while another runs (default
// half a batch: 16 threads x 64 submitted requests 62.6k calls/s at a full batch, 67.5k at half;
// 256 synchronous callers never queue that many, so they keep one slot)
size_t coalesce_overflow() {
    static const size_t v = std::max<size_t>(env_size("TFHE_MI355_COALESCE_OVERFLOW", coalesce_batch() / 2), 1);
    return v;
}
std::chrono::microseconds coalesce_window() {
    static const size_t v = env_size("TFHE_MI355_COALESCE_WINDOW_US", 1000);
    return std::chrono::microseconds(v);
}
// the batch also closes once no request of its op has arrived for this long: callers woken one by
// one after a batch (or a thread submitting a burst) re-queue within microseconds of each other
std::chrono::microseconds coalesce_gap() {
    static const size_t v = env_size("TFHE_MI355_COALESCE_GAP_US", 50);
    return std::chrono::microseconds(v);
}

struct CoalescedOpDesc {
    size_t in_words, out_words;
    bool lut;
    ChunkLaunch launch;
    ScratchSize scratch;
};
CoalescedOpDesc coalesced_op(const TfheMi355Context *c, CoalescedOp op) {
    const size_t small = c->n() + 1, big = c->big_dim() + 1;
    switch (op) {
        case CO_PBS: return {small, big, true, chunk_pbs, pbs_scratch_bytes};
        case CO_KS_PBS: return {big, big, true, launch_ks_pbs_dev, ks_pbs_scratch_bytes};
        case CO_PBS_KS: return {small, small, true, launch_pbs_ks_dev, pbs_ks_scratch_bytes};
        default: return {big, small, false, chunk_ks, ks_scratch_bytes};
    }
}

// one batch on one slot: concatenated inputs, LUT sets deduplicated by pointer with per-row LUT
// indexes shifted to the set's offset, one launch of the _async path on the slot's stream
void run_coalesced_batch(TfheMi355Context *c, TfheMi355Context::Coalescer::Slot &sl, CoalescedOp op,
                         const std::vector<CoalescedReq *> &batch) {
    check(hipSetDevice(c->device), "hipSetDevice");
    const CoalescedOpDesc d = coalesced_op(c, op);
    if (!sl.stream) check(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking), "hipStreamCreate(slot)");
    // the previous batch's blocking callers copy their rows out of h_out themselves (a few us each)
    while (sl.copies.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    size_t total = 0;
    for (auto *r : batch) total += r->count;
    // sized for a full batch once (no hipFree between batches: it would wait for the device); a
    // batch is at most `cap` rows (coalesce_max_count() <= cap, submit counts <= cap), the max()
    // keeps the copies below in bounds whatever the settings
    const size_t cap = std::max(coalesce_batch(), total), glwe = c->glwe_len();
    sl.h_out.reserve(cap * d.out_words * 8);
    sl.d_out.reserve(cap * d.out_words * 8);
    const size_t scratch = d.scratch(c, cap);
    if (scratch) sl.d_scratch.reserve(scratch);
    size_t rows = 0, sets = 0;
    std::vector<std::pair<const uint64_t *, size_t>> seen;  // LUT pointer -> first set index
    std::vector<size_t> seen_count;                           // its lut_count
    std::vector<size_t> base(batch.size(), 0);
    if (d.lut) {  // distinct LUT sets (by pointer) and their offsets
        for (size_t b = 0; b < batch.size(); b++) {
            const CoalescedReq *r = batch[b];
            base[b] = (size_t)-1;
            for (size_t q = 0; q < seen.size(); q++)  // same buffer, same number of tables
                if (seen[q].first == r->luts && seen_count[q] == r->lut_count) base[b] = seen[q].second;
            if (base[b] == (size_t)-1) {
                base[b] = sets;
                seen.push_back({r->luts, sets});
                seen_count.push_back(r->lut_count);
                sets += r->lut_count;
            }
        }
    }
    // ONE host->device copy per batch: [LUT sets | input rows | per-row LUT indexes (> 1 set)] packed
    // in the slot's pinned staging and its device twin (each copy is a DMA with its own ~10 us of
    // setup: a one-ciphertext call paid three of them).  Capacity: a full batch of rows plus the
    // sets seen so far, grown (rarely) on demand.
    const size_t lut_bytes = d.lut ? sets * glwe * 8 : 0;
    const size_t in_off = align256(lut_bytes), in_bytes = total * d.in_words * 8;
    const bool with_idx = d.lut && sets > 1;
    const size_t idx_off = align256(in_off + in_bytes), span = idx_off + (with_idx ? total * 4 : 0);
    const size_t room = align256(lut_bytes) + align256(cap * d.in_words * 8) + cap * 4;
    sl.h_in.reserve(std::max(span, room));
    sl.d_in.reserve(std::max(span, room));
    char *hs = static_cast<char *>(sl.h_in.ptr);
    for (size_t q = 0; q < seen.size(); q++)
        std::memcpy(hs + seen[q].second * glwe * 8, seen[q].first, seen_count[q] * glwe * 8);
    uint32_t *hidx = reinterpret_cast<uint32_t *>(hs + idx_off);
    for (size_t b = 0; b < batch.size(); b++) {
        const CoalescedReq *r = batch[b];
        std::memcpy(hs + in_off + rows * d.in_words * 8, r->in, r->count * d.in_words * 8);
        if (with_idx)
            for (size_t i = 0; i < r->count; i++) hidx[rows + i] = (uint32_t)(base[b] + (r->idx ? r->idx[i] : 0));
        rows += r->count;
    }
    const hipStream_t s = sl.stream;
    check(hipMemcpyAsync(sl.d_in.ptr, sl.h_in.ptr, span, hipMemcpyHostToDevice, s), "H2D batch");
    char *ds = static_cast<char *>(sl.d_in.ptr);
    d.launch(c, (const uint64_t *)(ds + in_off), (uint64_t *)sl.d_out.ptr, (const uint64_t *)ds,
             d.lut ? sets : 0, with_idx ? (const uint32_t *)(ds + idx_off) : nullptr, total,
             scratch ? sl.d_scratch.ptr : nullptr, scratch ? sl.d_scratch.bytes : 0, s);
    check(hipMemcpyAsync(sl.h_out.ptr, sl.d_out.ptr, total * d.out_words * 8, hipMemcpyDeviceToHost, s), "D2H batch");
    check(hipStreamSynchronize(s), "batch sync");
    check_quad_fail(c);
    rows = 0;
    int deferred = 0;
    for (auto *r : batch) {
        const uint64_t *src = static_cast<uint64_t *>(sl.h_out.ptr) + rows * d.out_words;
        if (r->sync) {  // copied by its caller after the wake-up (coalesce_wait)
            r->src = src;
            r->src_bytes = r->count * d.out_words * 8;
            r->pending = &sl.copies;
            deferred++;
        } else {
            std::memcpy(r->out, src, r->count * d.out_words * 8);
        }
        rows += r->count;
    }
    sl.copies.store(deferred, std::memory_order_release);  // before any caller is woken
}

// dispatcher of batch slot q: waits for queued work, lets the window fill the batch, takes the
// longest-waiting op's queue (up to a full batch) and runs it; callers are woken one by one
void coalesce_dispatcher(TfheMi355Context *c, size_t q) {
    auto &co = c->co;
    auto &sl = co.slots[q];
    const size_t cap = coalesce_batch();
    size_t rr = 0;  // round robin over the ops
    for (;;) {
        std::vector<CoalescedReq *> batch;
        CoalescedOp op = CO_PBS;
        size_t cts = 0;
        {
            std::unique_lock<std::mutex> lk(co.m);
            auto pending = [&] {
                for (int o = 0; o < CO_OPS; o++)
                    if (!co.queue[o].empty()) return true;
                return false;
            };
            auto full = [&] {
                for (int o = 0; o < CO_OPS; o++)
                    if (co.queued[o] >= coalesce_overflow()) return true;
                return false;
            };
            // a batch starts when no other slot is busy, or when a full batch is waiting (overflow:
            // callers with many requests in flight, e.g. through tfhe_mi355_submit)
            co.cv.wait(lk, [&] { return co.stop || (pending() && (co.in_flight == 0 || full())); });
            if (co.stop && !pending()) return;
            co.max_in_flight = std::max(co.max_in_flight, ++co.in_flight);  // claimed before the window
            for (int k = 0; k < CO_OPS; k++) {
                const int o = (int)((rr + k) % CO_OPS);
                if (!co.queue[o].empty()) {
                    op = (CoalescedOp)o;
                    break;
                }
            }
            rr = (size_t)op + 1;
            // the window also closes as soon as the blocking callers of the op's previous batch can
            // all be back (as many blocking rows queued as it had; each such caller has one call
            // outstanding).  Submitted requests keep the gap rule: a burst from one thread says
            // nothing about how many more are coming.
            const auto close = std::chrono::steady_clock::now() + coalesce_window();
            while (!co.stop && co.queued[op] < cap &&
                   !(co.last_sync_rows[op] && co.queued_sync[op] >= co.last_sync_rows[op])) {
                const auto t = std::min(close, co.last_arrival[op] + coalesce_gap());
                if (std::chrono::steady_clock::now() >= t) break;
                co.cv.wait_until(lk, t);
            }
            auto &qu = co.queue[op];
            size_t take = 0;
            size_t sync_rows = 0;
            while (take < qu.size() && (batch.empty() || cts + qu[take]->count <= cap)) {
                cts += qu[take]->count;
                if (qu[take]->sync) sync_rows += qu[take]->count;
                batch.push_back(qu[take++]);
            }
            qu.erase(qu.begin(), qu.begin() + take);
            co.queued[op] -= cts;
            co.queued_sync[op] -= sync_rows;
            if (batch.empty()) {  // another slot took the queue during the window
                co.in_flight--;
                continue;
            }
            co.last_sync_rows[op] = sync_rows == cts ? cts : 0;  // only a batch that ran says how many callers
            if (full()) co.cv.notify_one();  // another full batch: an idle slot can run it now
        }
        std::string err;
        const auto t0 = std::chrono::steady_clock::now();
        try {
            KeyRead keys(c);  // no key upload mid-batch
            run_coalesced_batch(c, sl, op, batch);
        } catch (const std::exception &ex) {
            err = ex.what();
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (auto *x : batch) {  // notified under its lock: the caller may free x as soon as it wakes
            std::lock_guard<std::mutex> g(x->m);
            x->err = err;
            x->done = true;
            x->cv.notify_one();
        }
        {  // the slot counts as busy until its callers are all woken, so the next batch's window
           // (on whichever slot) starts after they have had the chance to queue again
            std::lock_guard<std::mutex> g(co.m);
            co.in_flight--;
            co.batches++;
            co.rows += cts;
            co.batch_seconds += dt;
        }
        co.cv.notify_one();  // a slot waiting for this one to finish
    }
}

// a request joins its op's queue (the dispatchers start with the first one)
void coalesce_enqueue(TfheMi355Context *c, CoalescedOp op, CoalescedReq &r) {
    auto &co = c->co;
    {
        std::lock_guard<std::mutex> g(co.m);
        if (co.workers.empty())
            for (size_t q = 0; q < coalesce_slots(); q++) co.workers.emplace_back(coalesce_dispatcher, c, q);
        co.queue[op].push_back(&r);
        co.queued[op] += r.count;
        if (r.sync) co.queued_sync[op] += r.count;
        co.last_arrival[op] = std::chrono::steady_clock::now();
    }
    co.cv.notify_one();
}

void coalesce_wait(CoalescedReq &r) {
    {
        std::unique_lock<std::mutex> lk(r.m);
        r.cv.wait(lk, [&] { return r.done; });
    }
    if (r.pending) {  // this caller's rows are in the slot's staging: copy them, release the slot
        std::memcpy(r.out, r.src, r.src_bytes);
        r.pending->fetch_sub(1, std::memory_order_release);
    }
    if (!r.err.empty()) fail("%s", r.err.c_str());
}

// A synchronous call that finds the coalescer idle (nothing queued, no batch in flight) runs at once
// on the calling thread as a batch of its own, on slot 8 (TFHE_MI355_COALESCE_DIRECT=0: never):
// it skips the batching window and two thread hand-offs (~0.1 ms of a ~2.6 ms call).  It is not
// counted in in_flight, so calls arriving meanwhile are batched by the dispatchers on their own
// slots and run beside it (the latency kernel puts each ciphertext on its own CU).
bool coalesce_direct() {
    static const bool v = env_size("TFHE_MI355_COALESCE_DIRECT", 1) != 0;
    return v;
}

// the calling thread's request joins its op's queue and waits for its own completion
void coalesced_call(TfheMi355Context *c, CoalescedOp op, CoalescedReq &r) {
    auto &co = c->co;
    bool direct = false;
    if (coalesce_direct()) {
        std::lock_guard<std::mutex> g(co.m);
        // ... and only while this entry point's traffic is one blocking caller at a time (its last
        // dispatcher batch had at most one blocking row): with several callers a direct call would
        // split their batch in two
        bool idle = !co.stop && !co.direct_busy && co.in_flight == 0 && co.last_sync_rows[op] <= 1;
        for (int o = 0; o < CO_OPS && idle; o++) idle = co.queue[o].empty();
        if (idle) co.direct_busy = direct = true;
    }
    if (!direct) {
        r.sync = true;
        coalesce_enqueue(c, op, r);
        coalesce_wait(r);
        return;
    }
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    try {
        KeyRead keys(c);  // no key upload mid-batch
        const std::vector<CoalescedReq *> one{&r};
        run_coalesced_batch(c, co.slots[8], op, one);
    } catch (const std::exception &ex) {
        err = ex.what();
    }
    {
        std::lock_guard<std::mutex> g(co.m);
        co.direct_busy = false;
        co.batches++;
        co.rows += r.count;
        co.batch_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!err.empty()) fail("%s", err.c_str());
}

bool coalescible(size_t count) { return count > 0 && count <= coalesce_max_count(); }

// an ABI call made from inside another one: its failure text becomes ours
void abi(int rc) {
    if (rc != TFHE_MI355_OK) fail("%s", tfhe_mi355_last_error());
}

// ---- multi-device contexts ----------------------------------------------------------------------
// SURVEY.md 8b `ctx_create(params, device_mask)` / 8e: ONE process drives several GPUs through one
// context, the way the reference's one process drives its rayon pool (a thread-local ShortintEngine
// per worker, shortint/engine/mod.rs:23-25, and one KS+PBS per block from par_iter,
// integer/server_key/radix_parallel/mul.rs:347-407, through the ShortintBootstrappingKey arms,
// shortint/server_key/mod.rs:104-111,783-857).  A multi-device context owns one single-device context
// ("shard") per listed device; a device may be listed more than once (shards on one GPU then run
// side by side on their own streams).
//   keys: uploaded once, to the first shard, and replicated from its device memory: an RCCL
//     broadcast over xGMI among the distinct devices (librccl opened at run time; ncclCommInitAll
//     over the device list, one rank per distinct device), then device-to-device copies to further
//     shards on the same device.  TFHE_MI355_REPLICATE=copy uses peer copies instead of RCCL,
//     =rccl forces the broadcast even with one distinct device (a one-rank communicator copying
//     into the second shard of that device; a test hook);
//   batched host-pointer calls: split into contiguous shares, one per shard, each run by the shard's
//     own entry point on a thread of its own (its own stream, staging, lock) and joined before the
//     call returns;
//   small calls (the coalesced ones) and submitted requests: round-robin to the shards' coalescers;
//   device-pointer (_async) calls and their scratch queries: the first device's shard (a device
//     pointer belongs to one device; tfhe_mi355_context_device_context hands out each shard).
}  // namespace

struct RcclComms {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) init_all = nullptr;
    decltype(&ncclBroadcast) broadcast = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::vector<int> devices;  // rank -> device
    std::vector<ncclComm_t> comms;
    ~RcclComms() {
        for (size_t r = 0; r < comms.size(); r++)
            if (comms[r] && comm_destroy) {
                (void)hipSetDevice(devices[r]);
                (void)comm_destroy(comms[r]);
            }
        if (lib) dlclose(lib);
    }
};

namespace {

void check_nccl(const RcclComms &rc, ncclResult_t r, const char *what) {
    if (r != ncclSuccess) fail("%s: %s", what, rc.error_string ? rc.error_string(r) : "RCCL error");
}

// the communicator over `devices` (rank 0 = the source's device), created once per context
RcclComms &rccl_for(TfheMi355Context *m, const std::vector<int> &devices) {
    if (m->rccl && m->rccl->devices == devices) return *m->rccl;
    delete m->rccl;
    m->rccl = nullptr;
    auto rc = std::make_unique<RcclComms>();
    rc->lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!rc->lib) rc->lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!rc->lib) fail("RCCL is not available for key replication (%s); TFHE_MI355_REPLICATE=copy uses peer copies",
                       dlerror());
    auto sym = [&](const char *name) {
        void *f = dlsym(rc->lib, name);
        if (!f) fail("librccl lacks %s", name);
        return f;
    };
    rc->init_all = reinterpret_cast<decltype(rc->init_all)>(sym("ncclCommInitAll"));
    rc->broadcast = reinterpret_cast<decltype(rc->broadcast)>(sym("ncclBroadcast"));
    rc->group_start = reinterpret_cast<decltype(rc->group_start)>(sym("ncclGroupStart"));
    rc->group_end = reinterpret_cast<decltype(rc->group_end)>(sym("ncclGroupEnd"));
    rc->comm_destroy = reinterpret_cast<decltype(rc->comm_destroy)>(sym("ncclCommDestroy"));
    rc->error_string = reinterpret_cast<decltype(rc->error_string)>(sym("ncclGetErrorString"));
    rc->devices = devices;
    rc->comms.assign(devices.size(), nullptr);
    check_nccl(*rc, rc->init_all(rc->comms.data(), (int)devices.size(), devices.data()), "ncclCommInitAll");
    m->rccl = rc.release();
    return *m->rccl;
}

// TFHE_MI355_REPLICATE: "auto" (default), "rccl", "copy" ("fail": a replication failure, test hook)
std::string replicate_mode() {
    const char *e = std::getenv("TFHE_MI355_REPLICATE");
    return e && *e ? std::string(e) : std::string("auto");
}

enum class KeyPart { Fourier, Ksk };

// shard 0's key part -> every other shard (see above); the ready flags are the caller's business
void replicate(TfheMi355Context *m, KeyPart part) {
    auto &S = m->shards;
    TfheMi355Context *src = S[0];
    const size_t bytes = part == KeyPart::Fourier ? src->fourier_bsk_bytes() : src->ksk_len() * sizeof(uint64_t);
    auto buffer = [&](TfheMi355Context *s) -> DeviceBuffer & { return part == KeyPart::Fourier ? s->fbsk : s->ksk; };
    if (!buffer(src).ptr || buffer(src).bytes < bytes) fail("no key on the first device to replicate");
    // distinct devices in order of first appearance (rank 0: the source's) and the shards on each
    std::vector<int> devs;
    std::vector<std::vector<size_t>> on;
    for (size_t i = 0; i < S.size(); i++) {
        const auto it = std::find(devs.begin(), devs.end(), S[i]->device);
        if (it == devs.end()) {
            devs.push_back(S[i]->device);
            on.push_back({i});
        } else {
            on[it - devs.begin()].push_back(i);
        }
    }
    for (size_t i = 1; i < S.size(); i++) {
        check(hipSetDevice(S[i]->device), "hipSetDevice");
        buffer(S[i]).reserve(bytes);
    }
    // the shard of each device that receives the broadcast: the first one on it (on the source's
    // device: a second shard there, else the source itself, in place)
    std::vector<size_t> holder(devs.size());
    for (size_t r = 0; r < devs.size(); r++) holder[r] = r == 0 && on[0].size() > 1 ? on[0][1] : on[r][0];
    const std::string mode = replicate_mode();
    m->replicate_note.clear();
    if (mode == "fail") fail("key replication failed (TFHE_MI355_REPLICATE=fail test hook)");
    bool use_rccl = mode == "rccl" || (mode != "copy" && devs.size() > 1);
    RcclComms *rcp = nullptr;
    if (use_rccl) {
        try {
            rcp = &rccl_for(m, devs);
        } catch (const Failure &e) {
            if (mode == "rccl") throw;
            // auto: librccl missing or its communicator refused -> the peer-copy path
            m->replicate_note = std::string("RCCL unavailable, peer copies: ") + e.what();
            use_rccl = false;
        }
    }
    auto sync_all = [&] {
        for (auto *s : S) {
            check(hipSetDevice(s->device), "hipSetDevice");
            check(hipStreamSynchronize(s->stream), "key replication sync");
        }
    };
    check(hipSetDevice(src->device), "hipSetDevice");
    check(hipStreamSynchronize(src->stream), "key source sync");
    m->replication = use_rccl ? TFHE_MI355_REPLICATION_RCCL
                     : devs.size() > 1 ? TFHE_MI355_REPLICATION_PEER_COPY : TFHE_MI355_REPLICATION_DEVICE_COPY;
    if (use_rccl) {
        RcclComms &rc = *rcp;
        check_nccl(rc, rc.group_start(), "ncclGroupStart");
        for (size_t r = 0; r < devs.size(); r++) {
            check(hipSetDevice(devs[r]), "hipSetDevice");
            TfheMi355Context *h = S[holder[r]];
            const ncclResult_t e =
                rc.broadcast(buffer(src).ptr, buffer(h).ptr, bytes, ncclUint8, 0, rc.comms[r], h->stream);
            if (e != ncclSuccess) {
                (void)rc.group_end();
                check_nccl(rc, e, "ncclBroadcast");
            }
        }
        check_nccl(rc, rc.group_end(), "ncclGroupEnd");
    } else {
        for (size_t r = 0; r < devs.size(); r++) {
            if (holder[r] == 0) continue;
            TfheMi355Context *h = S[holder[r]];
            check(hipSetDevice(h->device), "hipSetDevice");
            check(h->device == src->device
                      ? hipMemcpyAsync(buffer(h).ptr, buffer(src).ptr, bytes, hipMemcpyDeviceToDevice, h->stream)
                      : hipMemcpyPeerAsync(buffer(h).ptr, h->device, buffer(src).ptr, src->device, bytes, h->stream),
                  "key peer copy");
        }
    }
    sync_all();
    for (size_t r = 0; r < devs.size(); r++)  // the other shards of each device: from its holder
        for (size_t i : on[r]) {
            if (i == 0 || i == holder[r]) continue;
            check(hipSetDevice(S[i]->device), "hipSetDevice");
            check(hipMemcpyAsync(buffer(S[i]).ptr, buffer(S[holder[r]]).ptr, bytes, hipMemcpyDeviceToDevice,
                                 S[i]->stream),
                  "key device copy");
        }
    if (part == KeyPart::Ksk)  // each shard repacks its own byte planes for the MFMA keyswitch
        for (size_t i = 1; i < S.size(); i++) {
            check(hipSetDevice(S[i]->device), "hipSetDevice");
            repack_ksk(S[i], S[i]->stream);
        }
    sync_all();
    check(hipSetDevice(src->device), "hipSetDevice");
}

// the context itself, or the first shard of a multi-device one (device-pointer calls)
TfheMi355Context *primary(TfheMi355Context *c) { return c && c->multi() ? c->shards[0] : c; }

// the shard that takes the next small call / submitted request
TfheMi355Context *pick_shard(TfheMi355Context *m) {
    return m->shards[m->next_shard.fetch_add(1, std::memory_order_relaxed) % m->shards.size()];
}

// key writes of a multi-device context: its own lock (uploads in turn), then every shard's (no
// coalesced batch on any device while the key changes)
std::vector<std::unique_ptr<KeyWrite>> key_write_all(TfheMi355Context *c) {
    std::vector<std::unique_ptr<KeyWrite>> w;
    w.emplace_back(new KeyWrite(c));
    for (auto *s : c->shards) w.emplace_back(new KeyWrite(s));
    return w;
}

void set_ready_all(TfheMi355Context *m, KeyPart part, bool ready) {
    for (auto *s : m->shards) {
        if (part == KeyPart::Fourier) s->fbsk_ready = ready;
        else s->ksk_ready = ready;
    }
}

// a batched host-pointer call of a multi-device context: shard i runs rows [count i / S, count (i+1)
// / S) through `f(shard, first, count)` (an entry point of the shard, 0 = ok), shard 0 on the calling
// thread and the others on threads of their own; joined, then the first failure is reported
// The whole call holds the multi-device context's key lock shared, so a concurrent key upload
// (key_write_all: this context exclusively first) lands before or after it, never between two
// shards' shares.
template <class F>
void split_rows(TfheMi355Context *m, size_t count, F &&f) {
    const size_t S = m->shards.size();
    KeyRead keys(m);
    std::vector<std::string> errs(S);
    auto run = [&](size_t i) {
        const size_t a = count * i / S, b = count * (i + 1) / S;
        if (a == b) return;
        try {
            if (f(m->shards[i], a, b - a) != TFHE_MI355_OK) errs[i] = tfhe_mi355_last_error();
        } catch (const std::exception &e) {
            errs[i] = e.what();
        }
    };
    std::mutex dm;
    std::condition_variable dcv;
    size_t left = 0;
    for (size_t i = 1; i < S; i++) {
        if (count * i / S == count * (i + 1) / S) continue;
        left++;
        m->workers[i - 1]->post([&, i] {
            run(i);
            std::lock_guard<std::mutex> g(dm);
            if (--left == 0) dcv.notify_one();
        });
    }
    run(0);
    {
        std::unique_lock<std::mutex> g(dm);
        dcv.wait(g, [&] { return left == 0; });
    }
    for (size_t i = 0; i < S; i++)
        if (!errs[i].empty()) fail("device %d (shard %zu): %s", m->shards[i]->device, i, errs[i].c_str());
}

// peer access between every two distinct devices of a multi-device context, so that the peer-copy
// replication (TFHE_MI355_REPLICATE=copy, or auto without RCCL) is a direct xGMI copy rather than
// a staged one; a pair the platform cannot map keeps the staged path (not an error)
void enable_peer_access(const std::vector<int> &devs) {
    std::vector<int> d = devs;
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    for (int a : d)
        for (int b : d) {
            if (a == b) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) continue;
            if (hipSetDevice(a) != hipSuccess) continue;
            (void)hipDeviceEnablePeerAccess(b, 0);  // hipErrorPeerAccessAlreadyEnabled is fine too
            (void)hipGetLastError();                 // ... and leaves its code behind
        }
}

// parameter checks shared by the single- and multi-device constructors
void validate_parameters(const TfheMi355Parameters &p) {
    if (!is_pow2(p.polynomial_size)) fail("polynomial_size must be a power of two");
    if (p.grouping_factor != 0) {
        if (!multibit_pbs_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level,
                                    (int)p.grouping_factor) &&
            !large_multibit_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level,
                                      (int)p.grouping_factor))
            fail("no multi-bit kernel for N=%u k=%u pbs_level=%u grouping_factor=%u", p.polynomial_size,
                 p.glwe_dimension, p.pbs_level, p.grouping_factor);
        if (p.lwe_dimension % p.grouping_factor)
            fail("lwe_dimension %u is not a multiple of grouping_factor %u", p.lwe_dimension, p.grouping_factor);
    } else if (!classic_pbs_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level) &&
               !large_pbs_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level)) {
        fail("no kernel for N=%u k=%u pbs_level=%u", p.polynomial_size, p.glwe_dimension, p.pbs_level);
    }
    // the N <= 2048 kernels (and the grouped N = 32768 CMUX) decompose in 32-bit registers;
    // the split CMUX of N >= 4096 in 64-bit ones (the shortint sets reach 11 x 3 = 33 bits)
    const bool split = !p.grouping_factor && p.polynomial_size >= 4096;
    const uint32_t max_bits = split ? 63 : 30;
    if (p.pbs_base_log < 2 || p.pbs_base_log * p.pbs_level > max_bits)
        fail("pbs decomposition base_log*level must be in [2, %u] (got %u x %u)", max_bits, p.pbs_base_log,
             p.pbs_level);
    // the split CMUX keeps the lower levels' digits as int16 between passes: a signed digit lies
    // in [-2^(beta-1), 2^(beta-1)], so beta <= 15 (beta = 16 would wrap +2^15 to -2^15); this
    // also keeps the grouped N = 32768, L = 2 path's 32-bit decomposition at beta * L <= 30
    if (split && p.pbs_level > 1 && p.pbs_base_log > 15)
        fail("pbs base_log %u > 15 with %u levels at N = %u (digits are packed as int16)", p.pbs_base_log,
             p.pbs_level, p.polynomial_size);
    // ... and returns every digit as int32 (decompose64): the one-level digit lies in
    // (-2^(beta-1), 2^(beta-1)], so beta <= 31 (beta = 32 would wrap +2^31 to -2^31)
    if (split && p.pbs_level == 1 && p.pbs_base_log > 31)
        fail("pbs base_log %u > 31 with one level at N = %u (digits are computed as int32)", p.pbs_base_log,
             p.polynomial_size);
    if (p.ks_level && (p.ks_base_log == 0 || p.ks_base_log * p.ks_level >= 64)) fail("invalid ks decomposition");
    if (p.lwe_dimension == 0) fail("lwe_dimension must be > 0");
}

TfheMi355Context *create_single(const TfheMi355Parameters &p, int device) {
    check(hipSetDevice(device), "hipSetDevice");
    auto *c = new TfheMi355Context();
    c->p = p;
    c->device = device;
    try {
        check(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->cus = cus;
        for (auto &L : c->lanes) {
            check(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking), "hipStreamCreate(lane)");
            for (hipEvent_t *e : {&L.h2d, &L.kern, &L.done})
                check(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate(lane)");
        }
        if (quad_max(c) > 0) {  // the quad CMUX's failure word (needs c->cus)
            c->quad_fail.reserve(4);
            check(hipMemset(c->quad_fail.ptr, 0, 4), "quad fail word");
        }
        build_tables(c);
    } catch (...) {
        tfhe_mi355_context_destroy(c);
        throw;
    }
    return c;
}
}  // namespace

// key transaction of serde.cpp's serialized-key uploads (engine.h)
std::shared_ptr<void> tfhe_mi355::begin_key_transaction(TfheMi355Context *ctx) {
    return std::make_shared<std::vector<std::unique_ptr<KeyWrite>>>(key_write_all(ctx));
}

extern "C" {

const char *tfhe_mi355_last_error(void) { return last_error_text().c_str(); }

int tfhe_mi355_device_count(int *out_count) {
    return guarded([&] {
        if (!out_count) fail("null out_count");
        *out_count = 0;
        int n = 0;
        check(hipGetDeviceCount(&n), "hipGetDeviceCount");
        *out_count = n;
    });
}

int tfhe_mi355_kernel_timing_enable(TfheMi355Context *ctx, int every) {
    return guarded([&] {
        if (!ctx) fail("null argument");
        if (every < 0) fail("sampling interval must be >= 0");
        if (ctx->multi()) {
            for (auto *s : ctx->shards) abi(tfhe_mi355_kernel_timing_enable(s, every));
            return;
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->timer.reset();
        ctx->timer.every = every;
    });
}

int tfhe_mi355_kernel_timing_entry(TfheMi355Context *ctx, size_t index, char *name, size_t name_len,
                                   double *total_ms, uint64_t *launches) {
    return guarded([&] {
        if (!ctx || !name || !name_len || !total_ms || !launches) fail("null argument");
        name[0] = 0;
        *total_ms = 0;
        *launches = 0;
        if (ctx->multi()) {  // summed over the devices, by kernel family
            std::map<std::string, std::pair<double, uint64_t>> all;
            char nm[256];
            for (auto *s : ctx->shards) {
                double ms = 0;
                uint64_t cnt = 0;
                for (size_t i = 0; tfhe_mi355_kernel_timing_entry(s, i, nm, sizeof nm, &ms, &cnt) == TFHE_MI355_OK; i++) {
                    all[nm].first += ms;
                    all[nm].second += cnt;
                }
            }
            if (index >= all.size()) fail("kernel timing index %zu out of range (%zu entries)", index, all.size());
            auto it = all.begin();
            std::advance(it, index);
            std::snprintf(name, name_len, "%s", it->first.c_str());
            *total_ms = it->second.first;
            *launches = it->second.second;
            return;
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->timer.collect();
        std::lock_guard<std::mutex> g(ctx->timer.mu);
        if (index >= ctx->timer.totals.size()) fail("kernel timing index %zu out of range (%zu entries)", index,
                                                    ctx->timer.totals.size());
        auto it = ctx->timer.totals.begin();
        std::advance(it, index);
        std::snprintf(name, name_len, "%s", it->first.c_str());
        *total_ms = it->second.first;
        *launches = it->second.second;
    });
}

struct TfheMi355Request {
    CoalescedReq req;
};

int tfhe_mi355_submit(TfheMi355Context *ctx, int op, const uint64_t *lwe_in, uint64_t *lwe_out, const uint64_t *luts,
                      size_t lut_count, const uint32_t *lut_indexes, size_t count, TfheMi355Request **out_req) {
    return guarded([&] {
        if (!out_req) fail("null argument");
        *out_req = nullptr;
        if (!ctx || !lwe_in || !lwe_out) fail("null argument");
        if (op < 0 || op >= CO_OPS) fail("unknown op %d (0 PBS, 1 KS->PBS, 2 PBS->KS, 3 KS)", op);
        if (ctx->multi()) {  // round robin over the devices' coalescers
            abi(tfhe_mi355_submit(pick_shard(ctx), op, lwe_in, lwe_out, luts, lut_count, lut_indexes, count, out_req));
            return;
        }
        if (count == 0 || count > coalesce_batch())
            fail("submit takes 1..%zu ciphertexts (larger batches: the batched entry points)", coalesce_batch());
        check(hipSetDevice(ctx->device), "hipSetDevice");
        const bool lut = op != CO_KS;
        if (lut) {
            require_fbsk(ctx);
            if (!luts || lut_count == 0) fail("lut_count must be >= 1");
            validate_lut_indexes(lut_indexes, count, lut_count);
        }
        if (op != CO_PBS) require_ksk(ctx);
        auto *h = new TfheMi355Request{{lwe_in, lwe_out, lut ? luts : nullptr, lut ? lut_count : 0,
                                        lut ? lut_indexes : nullptr, count}};
        coalesce_enqueue(ctx, (CoalescedOp)op, h->req);
        *out_req = h;
    });
}

int tfhe_mi355_wait(TfheMi355Request *req) {
    return guarded([&] {
        if (!req) fail("null request");
        std::unique_ptr<TfheMi355Request> own(req);
        coalesce_wait(own->req);
    });
}

int tfhe_mi355_coalesce_stats(TfheMi355Context *ctx, int reset, uint64_t *batches, uint64_t *rows,
                              uint64_t *max_in_flight, double *batch_seconds) {
    return guarded([&] {
        if (!ctx || !batches || !rows || !max_in_flight || !batch_seconds) fail("null argument");
        if (ctx->multi()) {  // summed over the devices (max_in_flight: the sum of the devices' maxima)
            *batches = *rows = *max_in_flight = 0;
            *batch_seconds = 0;
            for (auto *s : ctx->shards) {
                uint64_t b = 0, r = 0, m = 0;
                double t = 0;
                abi(tfhe_mi355_coalesce_stats(s, reset, &b, &r, &m, &t));
                *batches += b;
                *rows += r;
                *max_in_flight += m;
                *batch_seconds += t;
            }
            return;
        }
        auto &co = ctx->co;
        std::lock_guard<std::mutex> g(co.m);
        *batches = co.batches;
        *rows = co.rows;
        *max_in_flight = co.max_in_flight;
        *batch_seconds = co.batch_seconds;
        if (reset) {
            co.batches = co.rows = 0;
            co.max_in_flight = co.in_flight;
            co.batch_seconds = 0;
        }
    });
}

int tfhe_mi355_host_alloc(size_t bytes, void **out_ptr) {
    return guarded([&] {
        if (!out_ptr) fail("null out_ptr");
        *out_ptr = nullptr;
        if (!bytes) fail("zero-byte host allocation");
        void *p = nullptr;
        check(hipHostMalloc(&p, bytes, hipHostMallocPortable), "hipHostMalloc");
        *out_ptr = p;
    });
}

int tfhe_mi355_host_free(void *ptr) {
    return guarded([&] {
        if (ptr) check(hipHostFree(ptr), "hipHostFree");
    });
}

int tfhe_mi355_context_create(const TfheMi355Parameters *params, int device, TfheMi355Context **out_ctx) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!params) fail("null params");
        validate_parameters(*params);
        *out_ctx = create_single(*params, device);
    });
}

int tfhe_mi355_context_create_devices(const TfheMi355Parameters *params, const int *devices, size_t device_count,
                                      TfheMi355Context **out_ctx) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!params || (!devices && device_count)) fail("null argument");
        validate_parameters(*params);
        int visible = 0;
        check(hipGetDeviceCount(&visible), "hipGetDeviceCount");
        std::vector<int> devs(devices, devices + device_count);
        if (devs.empty())  // no list: every visible device
            for (int d = 0; d < visible; d++) devs.push_back(d);
        if (devs.empty()) fail("no GPU visible");
        if (devs.size() > 64) fail("at most 64 devices per context (%zu listed)", devs.size());
        for (int d : devs)
            if (d < 0 || d >= visible) fail("device %d is not visible (%d devices)", d, visible);
        if (devs.size() == 1) {
            *out_ctx = create_single(*params, devs[0]);
            return;
        }
        auto *m = new TfheMi355Context();
        m->p = *params;
        m->device = devs[0];
        try {
            for (int d : devs) {
                m->shards.push_back(create_single(*params, d));
                m->shards.back()->owner = m;
            }
            for (size_t i = 1; i < devs.size(); i++) {
                m->workers.emplace_back(new ShardWorker());
                ShardWorker *w = m->workers.back().get();
                w->t = std::thread([w] { w->loop(); });
            }
            enable_peer_access(devs);
        } catch (...) {
            tfhe_mi355_context_destroy(m);
            throw;
        }
        *out_ctx = m;
    });
}

int tfhe_mi355_context_devices(TfheMi355Context *ctx, size_t *count) {
    return guarded([&] {
        if (!ctx || !count) fail("null argument");
        *count = ctx->multi() ? ctx->shards.size() : 1;
    });
}

int tfhe_mi355_context_replication(TfheMi355Context *ctx, int *mode, const char **note) {
    return guarded([&] {
        if (!ctx || !mode) fail("null argument");
        *mode = ctx->multi() ? ctx->replication : TFHE_MI355_REPLICATION_NONE;
        if (note) *note = ctx->replicate_note.c_str();
    });
}

int tfhe_mi355_context_device_context(TfheMi355Context *ctx, size_t index, TfheMi355Context **out_ctx,
                                      int *device) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!ctx) fail("null ctx");
        const size_t n = ctx->multi() ? ctx->shards.size() : 1;
        if (index >= n) fail("device index %zu out of range (%zu devices)", index, n);
        TfheMi355Context *s = ctx->multi() ? ctx->shards[index] : ctx;
        if (device) *device = s->device;
        *out_ctx = s;
    });
}

int tfhe_mi355_context_destroy(TfheMi355Context *ctx) {
    return guarded([&] {
        if (!ctx) return;
        if (ctx->owner) fail("this context belongs to a multi-device context: destroy that one");
        if (ctx->multi()) {  // every shard (each reports its own queued requests), then the communicator
            ctx->workers.clear();  // joins the shard workers (a split call still running finishes first)
            std::string errs;
            for (auto *s : ctx->shards) {
                s->owner = nullptr;
                if (tfhe_mi355_context_destroy(s) != TFHE_MI355_OK)
                    errs += std::string(errs.empty() ? "" : "; ") + tfhe_mi355_last_error();
            }
            delete ctx->rccl;
            delete ctx;
            if (!errs.empty()) fail("%s", errs.c_str());
            return;
        }
        (void)hipSetDevice(ctx->device);
        // 1. The coalescer first: take every still-queued request out of the queues and stop the
        //    dispatchers (a batch already running completes; its callers get their rows), join
        //    them, then fail the taken requests with rc = 1 -- they never launch a kernel on the
        //    tables and streams freed below (c_api/utils.rs:3-11 error convention).
        std::vector<CoalescedReq *> orphans;
        {
            std::lock_guard<std::mutex> g(ctx->co.m);
            ctx->co.stop = true;
            for (int o = 0; o < CO_OPS; o++) {
                orphans.insert(orphans.end(), ctx->co.queue[o].begin(), ctx->co.queue[o].end());
                ctx->co.queue[o].clear();
                ctx->co.queued[o] = 0;
                ctx->co.queued_sync[o] = 0;
            }
        }
        ctx->co.cv.notify_all();
        for (auto &t : ctx->co.workers) t.join();
        ctx->co.workers.clear();
        // a direct call (coalesced_call on an idle coalescer) still running on another thread
        // finishes on slot 8 before the slots' streams and the tables go (none starts after stop)
        for (;;) {
            {
                std::lock_guard<std::mutex> g(ctx->co.m);
                if (!ctx->co.direct_busy) break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        for (auto *x : orphans) {
            std::lock_guard<std::mutex> g(x->m);
            x->err = "the context was destroyed before this request ran (wait on every request first)";
            x->done = true;
            x->cv.notify_one();
        }
        for (auto &sl : ctx->co.slots)  // woken callers still copying their rows out of the staging
            while (sl.copies.load(std::memory_order_acquire) != 0) std::this_thread::yield();
        for (auto &sl : ctx->co.slots)
            if (sl.stream) {
                (void)hipStreamSynchronize(sl.stream);
                (void)hipStreamDestroy(sl.stream);
                sl.stream = nullptr;
            }
        // 2. then the device work of the synchronous paths, the tables and the streams
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (auto &L : ctx->lanes)
            if (L.stream) (void)hipStreamSynchronize(L.stream);
        if (ctx->tables.W) (void)hipFree(ctx->tables.W);
        if (ctx->tables.twist) (void)hipFree(ctx->tables.twist);
        if (ctx->tables.wtop) (void)hipFree(ctx->tables.wtop);
        for (auto &L : ctx->lanes) {
            for (hipEvent_t e : {L.h2d, L.kern, L.done})
                if (e) (void)hipEventDestroy(e);
            if (L.stream) (void)hipStreamDestroy(L.stream);
        }
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;  // device and pinned buffers free themselves
        if (!orphans.empty())
            fail("context destroyed with %zu request(s) still queued: they were not run and their wait returns 1",
                 orphans.size());
    });
}

}  // extern "C"

namespace {
// a key upload of a multi-device context: `first` (the same entry point) on the first device's
// shard, then the key part replicated to the other shards (RCCL broadcast / device copies)
template <class F>
void multi_key_upload(TfheMi355Context *m, KeyPart part, F &&first) {
    auto w = key_write_all(m);
    set_ready_all(m, part, false);
    try {
        abi(first(m->shards[0]));
        replicate(m, part);
    } catch (...) {  // the first shard may hold the new key already: no shard serves a half-replicated one
        set_ready_all(m, part, false);
        throw;
    }
    set_ready_all(m, part, true);
}
}  // namespace

extern "C" {

int tfhe_mi355_bootstrap_key_upload(TfheMi355Context *ctx, const uint64_t *bsk, size_t len) {
    return guarded([&] {
        if (!ctx || !bsk) fail("null argument");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Fourier, [&](TfheMi355Context *s) {
                return tfhe_mi355_bootstrap_key_upload(s, bsk, len);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->std_bsk_len()) fail("bootstrapping key has %zu words, expected %zu", len, ctx->std_bsk_len());
        ctx->fbsk_ready = false;
        ctx->std_staging.reserve(len * sizeof(uint64_t));
        check(hipMemcpyAsync(ctx->std_staging.ptr, bsk, len * sizeof(uint64_t), hipMemcpyHostToDevice,
                             ctx->stream), "upload bsk");
        ctx->fbsk.reserve(ctx->fourier_bsk_bytes());
        check(convert_bsk(ctx, (const uint64_t *)ctx->std_staging.ptr, len / ctx->N(), ctx->stream),
              "bsk conversion");
        check(hipStreamSynchronize(ctx->stream), "bsk conversion sync");
        ctx->std_staging.release();
        ctx->fbsk_ready = true;
    });
}

namespace {
// AES tables of a compression seed on the device (a few KiB, one per call)
void upload_aes_tables(TfheMi355Context *c, uint64_t seed_lo, uint64_t seed_hi, DeviceBuffer &d) {
    std::vector<unsigned char> host(aes_tables_bytes());
    aes_tables_build(seed_lo, seed_hi, host.data());
    d.reserve(host.size());
    check(hipMemcpyAsync(d.ptr, host.data(), host.size(), hipMemcpyHostToDevice, c->stream), "upload aes tables");
    check(hipStreamSynchronize(c->stream), "aes tables sync");
}
}  // namespace

int tfhe_mi355_bootstrap_key_upload_seeded(TfheMi355Context *ctx, const uint64_t *bodies, size_t len,
                                           uint64_t seed_lo, uint64_t seed_hi) {
    return guarded([&] {
        if (!ctx || !bodies) fail("null argument");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Fourier, [&](TfheMi355Context *s) {
                return tfhe_mi355_bootstrap_key_upload_seeded(s, bodies, len, seed_lo, seed_hi);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        const size_t rows = ctx->ggsw_count() * ctx->p.pbs_level * (ctx->k() + 1);
        if (len != rows * ctx->N()) fail("seeded bootstrapping key has %zu body words, expected %zu", len, rows * ctx->N());
        ctx->fbsk_ready = false;
        DeviceBuffer tab;
        upload_aes_tables(ctx, seed_lo, seed_hi, tab);
        DeviceBuffer d_bodies;
        d_bodies.reserve(len * sizeof(uint64_t));
        check(hipMemcpyAsync(d_bodies.ptr, bodies, len * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream),
              "upload bodies");
        ctx->std_staging.reserve(ctx->std_bsk_len() * sizeof(uint64_t));
        check(launch_seeded_decompress(tab.ptr, (const uint64_t *)d_bodies.ptr, rows, ctx->k() * ctx->N(), ctx->N(),
                                       (uint64_t *)ctx->std_staging.ptr, ctx->stream),
              "seeded bsk decompression");
        ctx->fbsk.reserve(ctx->fourier_bsk_bytes());
        check(convert_bsk(ctx, (const uint64_t *)ctx->std_staging.ptr, ctx->std_bsk_len() / ctx->N(), ctx->stream),
              "bsk conversion");
        check(hipStreamSynchronize(ctx->stream), "seeded bsk sync");
        ctx->std_staging.release();
        d_bodies.release();
        tab.release();
        ctx->fbsk_ready = true;
    });
}

int tfhe_mi355_keyswitch_key_upload_seeded(TfheMi355Context *ctx, const uint64_t *bodies, size_t len,
                                           uint64_t seed_lo, uint64_t seed_hi) {
    return guarded([&] {
        if (!ctx || !bodies) fail("null argument");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Ksk, [&](TfheMi355Context *s) {
                return tfhe_mi355_keyswitch_key_upload_seeded(s, bodies, len, seed_lo, seed_hi);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        const size_t rows = ctx->big_dim() * ctx->p.ks_level;
        if (len != rows) fail("seeded keyswitching key has %zu body words, expected %zu", len, rows);
        DeviceBuffer tab;
        upload_aes_tables(ctx, seed_lo, seed_hi, tab);
        DeviceBuffer d_bodies;
        d_bodies.reserve(len * sizeof(uint64_t));
        check(hipMemcpyAsync(d_bodies.ptr, bodies, len * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream),
              "upload bodies");
        ctx->ksk_ready = false;
        ctx->ksk.reserve(ctx->ksk_len() * sizeof(uint64_t));
        check(launch_seeded_decompress(tab.ptr, (const uint64_t *)d_bodies.ptr, rows, ctx->n(), 1,
                                       (uint64_t *)ctx->ksk.ptr, ctx->stream),
              "seeded ksk decompression");
        repack_ksk(ctx, ctx->stream);
        check(hipStreamSynchronize(ctx->stream), "seeded ksk sync");
        d_bodies.release();
        tab.release();
        ctx->ksk_ready = true;
    });
}

int tfhe_mi355_csprng_mask_words(TfheMi355Context *ctx, uint64_t seed_lo, uint64_t seed_hi, uint64_t *out,
                                 size_t words) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!out && words)) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (words == 0) return;
        DeviceBuffer tab;
        upload_aes_tables(ctx, seed_lo, seed_hi, tab);
        DeviceBuffer d_words;
        d_words.reserve(words * sizeof(uint64_t));
        check(launch_seeded_decompress(tab.ptr, nullptr, 1, words, 0, (uint64_t *)d_words.ptr, ctx->stream),
              "csprng");
        check(hipMemcpyAsync(out, d_words.ptr, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream),
              "D2H words");
        check(hipStreamSynchronize(ctx->stream), "csprng sync");
        tab.release();
    });
}

int tfhe_mi355_bootstrap_key_convert_async(TfheMi355Context *ctx, const uint64_t *d_bsk, size_t len,
                                           void *stream) {
    return guarded([&] {
        if (!ctx || !d_bsk) fail("null argument");
        if (ctx->multi())  // d_bsk on the first device
            return multi_key_upload(ctx, KeyPart::Fourier, [&](TfheMi355Context *s) {
                return tfhe_mi355_bootstrap_key_convert_async(s, d_bsk, len, stream);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->std_bsk_len()) fail("bootstrapping key has %zu words, expected %zu", len, ctx->std_bsk_len());
        ctx->fbsk_ready = false;
        ctx->fbsk.reserve(ctx->fourier_bsk_bytes());
        check(convert_bsk(ctx, d_bsk, len / ctx->N(), (hipStream_t)stream), "bsk conversion");
        // the key counts as ready only once the conversion has run: every later call (on any
        // stream, including ctx->stream, which is not ordered after the caller's) sees it whole
        check(hipStreamSynchronize((hipStream_t)stream), "bsk conversion sync");
        ctx->fbsk_ready = true;
    });
}

int tfhe_mi355_context_parameters(TfheMi355Context *ctx, TfheMi355Parameters *out) {
    return guarded([&] {
        if (!ctx || !out) fail("null argument");
        *out = ctx->p;
    });
}

int tfhe_mi355_bootstrap_key_fourier(TfheMi355Context *ctx, void **d_ptr, size_t *bytes) {
    return guarded([&] {
        if (!ctx || !d_ptr || !bytes) fail("null argument");
        *d_ptr = nullptr;
        *bytes = 0;
        if (ctx->multi()) {  // the first device's buffer; _set_ready replicates it to the others
            auto w = key_write_all(ctx);
            abi(tfhe_mi355_bootstrap_key_fourier(ctx->shards[0], d_ptr, bytes));
            // the caller now rewrites shard 0's copy: no device serves this key part until _set_ready
            // (batches fail cleanly instead of mixing a half-written key with the old replicas)
            set_ready_all(ctx, KeyPart::Fourier, false);
            return;
        }
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        // (either width: the Fourier form of a u32 key has the same layout and lives in the same buffer)
        check(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->fbsk.reserve(ctx->fourier_bsk_bytes());
        *d_ptr = ctx->fbsk.ptr;
        *bytes = ctx->fourier_bsk_bytes();
    });
}

int tfhe_mi355_bootstrap_key_fourier_set_ready(TfheMi355Context *ctx) {
    return guarded([&] {
        if (!ctx) fail("null ctx");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Fourier, [&](TfheMi355Context *s) {
                return tfhe_mi355_bootstrap_key_fourier_set_ready(s);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        if (!ctx->fbsk.ptr) fail("no Fourier key buffer");
        ctx->fbsk_ready = true;
    });
}

int tfhe_mi355_keyswitch_key_upload(TfheMi355Context *ctx, const uint64_t *ksk, size_t len) {
    return guarded([&] {
        if (!ctx || !ksk) fail("null argument");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Ksk, [&](TfheMi355Context *s) {
                return tfhe_mi355_keyswitch_key_upload(s, ksk, len);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->ksk_len()) fail("keyswitching key has %zu words, expected %zu", len, ctx->ksk_len());
        ctx->ksk_ready = false;
        ctx->ksk.reserve(len * sizeof(uint64_t));
        check(hipMemcpy(ctx->ksk.ptr, ksk, len * sizeof(uint64_t), hipMemcpyHostToDevice), "upload ksk");
        repack_ksk(ctx, ctx->stream);
        check(hipStreamSynchronize(ctx->stream), "ksk repack sync");
        ctx->ksk_ready = true;
    });
}

int tfhe_mi355_keyswitch_key_upload_async(TfheMi355Context *ctx, const uint64_t *d_ksk, size_t len,
                                          void *stream) {
    return guarded([&] {
        if (!ctx || !d_ksk) fail("null argument");
        if (ctx->multi())  // d_ksk on the first device
            return multi_key_upload(ctx, KeyPart::Ksk, [&](TfheMi355Context *s) {
                return tfhe_mi355_keyswitch_key_upload_async(s, d_ksk, len, stream);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->ksk_len()) fail("keyswitching key has %zu words, expected %zu", len, ctx->ksk_len());
        ctx->ksk.reserve(len * sizeof(uint64_t));
        ctx->ksk_ready = false;
        check(hipMemcpyAsync(ctx->ksk.ptr, d_ksk, len * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                             (hipStream_t)stream), "copy ksk");
        repack_ksk(ctx, (hipStream_t)stream);
        check(hipStreamSynchronize((hipStream_t)stream), "ksk upload sync");  // see bootstrap_key_convert_async
        ctx->ksk_ready = true;
    });
}

int tfhe_mi355_keyswitch_key_device(TfheMi355Context *ctx, void **d_ptr, size_t *bytes) {
    return guarded([&] {
        if (!ctx || !d_ptr || !bytes) fail("null argument");
        *d_ptr = nullptr;
        *bytes = 0;
        if (ctx->multi()) {  // the first device's buffer; _set_ready replicates it to the others
            auto w = key_write_all(ctx);
            abi(tfhe_mi355_keyswitch_key_device(ctx->shards[0], d_ptr, bytes));
            // the caller now rewrites shard 0's copy: no device serves this key part until _set_ready
            // (batches fail cleanly instead of mixing a half-written key with the old replicas)
            set_ready_all(ctx, KeyPart::Ksk, false);
            return;
        }
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->ksk.reserve(ctx->ksk_len() * sizeof(uint64_t));
        *d_ptr = ctx->ksk.ptr;
        *bytes = ctx->ksk_len() * sizeof(uint64_t);
    });
}

int tfhe_mi355_keyswitch_key_set_ready(TfheMi355Context *ctx) {
    return guarded([&] {
        if (!ctx) fail("null ctx");
        if (ctx->multi())
            return multi_key_upload(ctx, KeyPart::Ksk, [&](TfheMi355Context *s) {
                return tfhe_mi355_keyswitch_key_set_ready(s);
            });
        KeyWrite kw(ctx);  // no coalesced batch in flight, none starts until done
        require_width64(ctx);
        if (!ctx->ksk.ptr) fail("no keyswitching key buffer");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        repack_ksk(ctx, ctx->stream);
        check(hipStreamSynchronize(ctx->stream), "ksk repack sync");
        ctx->ksk_ready = true;
    });
}

int tfhe_mi355_programmable_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out,
                                      const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes,
                                      size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!lwe_out && count) || !luts) fail("null argument");
        if (ctx->multi()) {
            const size_t wi = ctx->n() + 1, wo = ctx->big_dim() + 1;
            if (coalescible(count))
                return abi(tfhe_mi355_programmable_bootstrap(pick_shard(ctx), lwe_in, lwe_out, luts, lut_count,
                                                             lut_indexes, count));
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_programmable_bootstrap(s, lwe_in + a * wi, lwe_out + a * wo, luts, lut_count,
                                                         lut_indexes ? lut_indexes + a : nullptr, n);
            });
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_fbsk(ctx);
        if (lut_count == 0) fail("lut_count must be >= 1");
        validate_lut_indexes(lut_indexes, count, lut_count);
        if (coalescible(count)) {
            CoalescedReq r{lwe_in, lwe_out, luts, lut_count, lut_indexes, count};
            return coalesced_call(ctx, CO_PBS, r);
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        run_host_pipeline(ctx, lwe_in, ctx->n() + 1, lwe_out, ctx->big_dim() + 1, luts, ctx->glwe_len(), lut_count,
                          lut_indexes, count, chunk_pbs, pbs_scratch_bytes);
    });
}

int tfhe_mi355_programmable_bootstrap_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        *bytes = pbs_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_programmable_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_in, uint64_t *d_out,
                                            const uint64_t *d_luts, size_t lut_count, const uint32_t *d_idx,
                                            size_t count, void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_in && count) || (!d_out && count) || !d_luts) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        // the scratch query is the contract: the persistent grid's ticket word at the classic
        // shapes that use one (a NULL scratch there would silently run the slower one-pass grid);
        // at N >= 4096 at least one ciphertext's worth (smaller passes below the query's size)
        if (count && !is_large(ctx)) require_scratch(d_scratch ? scratch_bytes : 0, pbs_scratch_bytes(ctx, count));
        launch_pbs_dev(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, d_scratch, scratch_bytes,
                       (hipStream_t)stream);
    });
}

int tfhe_mi355_blind_rotate(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out, const uint64_t *luts,
                            size_t lut_count, const uint32_t *lut_indexes, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!glwe_out && count) || !luts) fail("null argument");
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_blind_rotate(s, lwe_in + a * (ctx->n() + 1), glwe_out + a * ctx->glwe_len(), luts,
                                               lut_count, lut_indexes ? lut_indexes + a : nullptr, n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_fbsk(ctx);
        if (lut_count == 0) fail("lut_count must be >= 1");
        if (is_large(ctx)) fail("blind rotation without sample extraction is not available at N = %zu", ctx->N());
        validate_lut_indexes(lut_indexes, count, lut_count);
        run_host_pipeline(ctx, lwe_in, ctx->n() + 1, glwe_out, ctx->glwe_len(), luts, ctx->glwe_len(), lut_count,
                          lut_indexes, count, chunk_blind_rotate, pbs_scratch_bytes);
    });
}

int tfhe_mi355_blind_rotate_async(TfheMi355Context *ctx, const uint64_t *d_in, uint64_t *d_glwe_out,
                                  const uint64_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes,
                                  size_t count, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_in && count) || (!d_glwe_out && count) || !d_luts) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_pbs_dev(ctx, d_in, d_glwe_out, d_luts, lut_count, d_lut_indexes, count, nullptr, 0,
                       (hipStream_t)stream, true);
    });
}

int tfhe_mi355_packing_keyswitch_key_upload(TfheMi355Context *ctx, const uint64_t *pksk, size_t len,
                                            uint32_t base_log, uint32_t level) {
    return guarded([&] {
        if (!ctx || !pksk) fail("null argument");
        if (level == 0 || base_log == 0 || base_log * level >= 64) fail("invalid packing ks decomposition");
        if (ctx->multi()) {  // a gadget-layer key: uploaded to every device from the host
            auto w = key_write_all(ctx);
            for (auto *s : ctx->shards) abi(tfhe_mi355_packing_keyswitch_key_upload(s, pksk, len, base_log, level));
            return;
        }
        KeyWrite kw(ctx);
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->pksk_len(level))
            fail("packing keyswitching key has %zu words, expected %zu", len, ctx->pksk_len(level));
        ctx->pksk_ready = ctx->pksk_planes_ready = false;
        ctx->pksk.reserve(len * sizeof(uint64_t));
        check(hipMemcpy(ctx->pksk.ptr, pksk, len * sizeof(uint64_t), hipMemcpyHostToDevice), "upload pksk");
        ctx->pks_base_log = base_log;
        ctx->pks_level = level;
        const int in_dim = (int)ctx->big_dim(), out_dim = (int)ctx->glwe_len() - 1;
        if (pks_use_mfma(ctx)) {
            ctx->pksk_planes.reserve(8 * ks_mfma_rows(in_dim, (int)level) * ks_mfma_cols(out_dim));
            check(launch_ksk_repack((const uint64_t *)ctx->pksk.ptr, (int8_t *)ctx->pksk_planes.ptr, in_dim,
                                    (int)level, out_dim, ctx->stream),
                  "pksk repack");
            ctx->pksk_planes_ready = true;
        }
        check(hipStreamSynchronize(ctx->stream), "pksk repack sync");
        ctx->pksk_ready = true;
    });
}

int tfhe_mi355_packing_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!glwe_out && count)) fail("null argument");
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_packing_keyswitch(s, lwe_in + a * (ctx->big_dim() + 1), glwe_out + a * ctx->glwe_len(), n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (!ctx->pksk_ready) fail("packing keyswitching key not uploaded");
        run_host_pipeline(ctx, lwe_in, ctx->big_dim() + 1, glwe_out, ctx->glwe_len(), nullptr, 0, 0, nullptr, count,
                          chunk_pks, pks_scratch_bytes);
    });
}

int tfhe_mi355_packing_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        if (!ctx->pksk_ready) fail("packing keyswitching key not uploaded: its decomposition sizes the scratch");
        *bytes = pks_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_packing_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint64_t *d_glwe_out,
                                       size_t count, void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_in && count) || (!d_glwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_packing_ks_dev(ctx, d_lwe_in, d_glwe_out, count, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_relinearization_key_upload(TfheMi355Context *ctx, const uint64_t *rlk, size_t len, uint32_t base_log,
                                          uint32_t level) {
    return guarded([&] {
        if (!ctx || !rlk) fail("null argument");
        if (level == 0 || base_log == 0 || base_log > 31 || (uint64_t)base_log * level > 63)
            fail("invalid relinearization decomposition %u x %u (1 <= base_log <= 31, base_log*level <= 63)", base_log,
                 level);
        if (ctx->multi()) {  // a gadget-layer key: uploaded to every device from the host
            auto w = key_write_all(ctx);
            for (auto *s : ctx->shards) abi(tfhe_mi355_relinearization_key_upload(s, rlk, len, base_log, level));
            return;
        }
        KeyWrite kw(ctx);
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_glwe_mult_shape(ctx);
        if (len != ctx->rlk_len(level))
            fail("relinearization key has %zu words, expected %zu ([k(k+1)/2][level][(k+1)N])", len, ctx->rlk_len(level));
        ctx->rlk_ready = false;
        ctx->rlk.reserve(len * sizeof(uint64_t));
        check(hipMemcpy(ctx->rlk.ptr, rlk, len * sizeof(uint64_t), hipMemcpyHostToDevice), "upload rlk");
        ctx->rlk_base_log = base_log;
        ctx->rlk_level = level;
        ctx->rlk_ready = true;
    });
}

int tfhe_mi355_glwe_mult(TfheMi355Context *ctx, const uint64_t *glwe_lhs, const uint64_t *glwe_rhs, uint32_t log_p,
                         int extract, uint64_t *out, size_t count) {
    return guarded([&] {
        if (!ctx || (!glwe_lhs && count) || (!glwe_rhs && count) || (!out && count)) fail("null argument");
        const size_t glwe = ctx->glwe_len(), out_words = extract ? ctx->big_dim() + 1 : glwe;
        if (words_overlap(out, count * out_words, glwe_lhs, count * glwe) ||
            words_overlap(out, count * out_words, glwe_rhs, count * glwe))
            fail("glwe_mult: out overlaps an input");
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_glwe_mult(s, glwe_lhs + a * glwe, glwe_rhs + a * glwe, log_p, extract,
                                            out + a * out_words, n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_glwe_mult_shape(ctx);
        validate_log_p(log_p);
        require_rlk(ctx);
        host_pair_call(
            ctx, glwe_lhs, glwe_rhs, glwe, out, out_words, count, [&](size_t n) { return glwe_mult_scratch(ctx, n); },
            [&](const uint64_t *l, const uint64_t *r, uint64_t *o, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_glwe_mult_dev(ctx, l, r, log_p, extract != 0, o, n, sc, sb, s);
            });
    });
}

int tfhe_mi355_glwe_mult_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        require_glwe_mult_shape(ctx);
        if (!ctx->rlk_ready) fail("relinearization key not uploaded: the scratch is defined from its upload on");
        *bytes = glwe_mult_scratch(ctx, count);
    });
}

int tfhe_mi355_glwe_mult_async(TfheMi355Context *ctx, const uint64_t *d_glwe_lhs, const uint64_t *d_glwe_rhs,
                               uint32_t log_p, int extract, uint64_t *d_out, size_t count, void *d_scratch,
                               size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_glwe_lhs && count) || (!d_glwe_rhs && count) || (!d_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_glwe_mult_dev(ctx, d_glwe_lhs, d_glwe_rhs, log_p, extract != 0, d_out, count, d_scratch, scratch_bytes,
                             (hipStream_t)stream);
    });
}

int tfhe_mi355_lwe_mult(TfheMi355Context *ctx, const uint64_t *lwe_lhs, const uint64_t *lwe_rhs, uint32_t log_p,
                        uint64_t *lwe_out, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_lhs && count) || (!lwe_rhs && count) || (!lwe_out && count)) fail("null argument");
        const size_t lwe = ctx->big_dim() + 1;
        if (words_overlap(lwe_out, count * lwe, lwe_lhs, count * lwe) ||
            words_overlap(lwe_out, count * lwe, lwe_rhs, count * lwe))
            fail("lwe_mult: out overlaps an input");
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_lwe_mult(s, lwe_lhs + a * lwe, lwe_rhs + a * lwe, log_p, lwe_out + a * lwe, n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_glwe_mult_shape(ctx);
        validate_log_p(log_p);
        require_rlk(ctx);
        if (!ctx->pksk_ready) fail("packing keyswitching key not uploaded");
        host_pair_call(
            ctx, lwe_lhs, lwe_rhs, lwe, lwe_out, lwe, count, [&](size_t n) { return lwe_mult_scratch(ctx, n); },
            [&](const uint64_t *l, const uint64_t *r, uint64_t *o, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_lwe_mult_dev(ctx, l, r, log_p, o, n, sc, sb, s);
            });
    });
}

int tfhe_mi355_lwe_mult_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        require_glwe_mult_shape(ctx);
        if (!ctx->rlk_ready) fail("relinearization key not uploaded: the scratch is defined from its upload on");
        if (!ctx->pksk_ready) fail("packing keyswitching key not uploaded: its decomposition sizes the scratch");
        *bytes = lwe_mult_scratch(ctx, count);
    });
}

int tfhe_mi355_lwe_mult_async(TfheMi355Context *ctx, const uint64_t *d_lwe_lhs, const uint64_t *d_lwe_rhs,
                              uint32_t log_p, uint64_t *d_lwe_out, size_t count, void *d_scratch,
                              size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_lhs && count) || (!d_lwe_rhs && count) || (!d_lwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_lwe_mult_dev(ctx, d_lwe_lhs, d_lwe_rhs, log_p, d_lwe_out, count, d_scratch, scratch_bytes,
                            (hipStream_t)stream);
    });
}

int tfhe_mi355_glwe_poly_mul(TfheMi355Context *ctx, const uint64_t *glwe_in, size_t glwe_per_item,
                             const uint64_t *polys, size_t npoly, size_t count, int extract, uint64_t *out) {
    return guarded([&] {
        if (!ctx || (!glwe_in && count) || (!polys && npoly) || (!out && count && npoly)) fail("null argument");
        if (ctx->multi()) {
            const size_t wo = npoly * (extract ? ctx->big_dim() + 1 : ctx->glwe_len());
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_glwe_poly_mul(s, glwe_in + a * glwe_per_item * ctx->glwe_len(), glwe_per_item, polys,
                                                npoly, n, extract, out + a * wo);
            });
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (count == 0 || npoly == 0) return;
        const size_t out_words = extract ? ctx->big_dim() + 1 : ctx->glwe_len();
        const size_t in_b = count * glwe_per_item * ctx->glwe_len() * 8;
        const size_t poly_b = npoly * glwe_per_item * ctx->N() * 8, out_b = count * npoly * out_words * 8;
        DeviceBuffer d_in, d_polys, d_out;
        d_in.reserve(in_b);
        d_polys.reserve(poly_b);
        d_out.reserve(out_b);
        hipStream_t s = ctx->stream;
        check(hipMemcpyAsync(d_in.ptr, glwe_in, in_b, hipMemcpyHostToDevice, s), "H2D glwe");
        check(hipMemcpyAsync(d_polys.ptr, polys, poly_b, hipMemcpyHostToDevice, s), "H2D polys");
        launch_glwe_poly_mul_dev(ctx, (const uint64_t *)d_in.ptr, glwe_per_item, (const uint64_t *)d_polys.ptr, npoly,
                                 count, extract != 0, (uint64_t *)d_out.ptr, s);
        check(hipMemcpyAsync(out, d_out.ptr, out_b, hipMemcpyDeviceToHost, s), "D2H out");
        check(hipStreamSynchronize(s), "glwe poly mul sync");
    });
}

int tfhe_mi355_glwe_poly_mul_async(TfheMi355Context *ctx, const uint64_t *d_glwe_in, size_t glwe_per_item,
                                   const uint64_t *d_polys, size_t npoly, size_t count, int extract,
                                   uint64_t *d_out, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_glwe_in && count) || (!d_polys && npoly) || (!d_out && count && npoly))
            fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (count == 0 || npoly == 0) return;
        launch_glwe_poly_mul_dev(ctx, d_glwe_in, glwe_per_item, d_polys, npoly, count, extract != 0, d_out,
                                 (hipStream_t)stream);
    });
}

// ---- GGSW external product, CMUX, vertical packing ---------------------------------------------
namespace {
// host form of the external product (ct0 == nullptr: glwe_inout accumulated) and of the CMUX
void ggsw_node_host(TfheMi355Context *ctx, int mode, const uint64_t *ggsw_list, size_t ggsw_count, uint32_t base_log,
                    uint32_t level, const uint32_t *ggsw_indexes, const uint64_t *in0, const uint64_t *in1,
                    uint64_t *out, size_t count) {
    std::lock_guard<std::mutex> g(ctx->mu);
    check(hipSetDevice(ctx->device), "hipSetDevice");
    require_ggsw_shape(ctx, base_log, level);
    if (count == 0) return;
    validate_ggsw_indexes(ggsw_indexes, count, ggsw_count);
    const size_t used = ggsw_indexes ? ggsw_count : count;  // without indexes item i reads GGSW i
    const size_t std_b = used * ggsw_std_words(ctx, level) * 8, f_b = used * ggsw_fourier_bytes(ctx, level);
    const size_t rows_b = count * ctx->glwe_len() * 8;
    DeviceBuffer d_std, d_f, d_a, d_b, d_idx;
    d_std.reserve(std_b);
    d_f.reserve(f_b);
    d_a.reserve(rows_b);
    d_b.reserve(rows_b);
    hipStream_t s = ctx->stream;
    check(hipMemcpyAsync(d_std.ptr, ggsw_list, std_b, hipMemcpyHostToDevice, s), "H2D GGSW list");
    if (ggsw_indexes) {
        d_idx.reserve(count * 4);
        check(hipMemcpyAsync(d_idx.ptr, ggsw_indexes, count * 4, hipMemcpyHostToDevice, s), "H2D GGSW indexes");
    }
    // d_a: ct0, or the accumulated glwe_inout; d_b: ct1, or glwe_in
    check(hipMemcpyAsync(d_a.ptr, mode == GGSW_EP ? out : in0, rows_b, hipMemcpyHostToDevice, s), "H2D glwe");
    check(hipMemcpyAsync(d_b.ptr, in1, rows_b, hipMemcpyHostToDevice, s), "H2D glwe");
    ggsw_list_to_fourier_dev(ctx, (const uint64_t *)d_std.ptr, (double2 *)d_f.ptr, used, level, s);
    launch_ggsw_node_dev(ctx, mode, (const double2 *)d_f.ptr, used, (const uint32_t *)d_idx.ptr, base_log, level,
                         mode == GGSW_EP ? nullptr : (const uint64_t *)d_a.ptr, (const uint64_t *)d_b.ptr,
                         (uint64_t *)d_a.ptr, count, s);
    check(hipMemcpyAsync(out, d_a.ptr, rows_b, hipMemcpyDeviceToHost, s), "D2H glwe");
    check(hipStreamSynchronize(s), "GGSW node sync");
}

// a multi-device context's share [a, a + n) of a GGSW list: the whole list when indexed
const uint64_t *ggsw_share(const TfheMi355Context *c, const uint64_t *list, const uint32_t *idx, uint32_t level,
                           size_t a) {
    return idx ? list : list + a * ggsw_std_words(c, level);
}
}  // namespace

int tfhe_mi355_ggsw_external_product(TfheMi355Context *ctx, const uint64_t *ggsw_list, size_t ggsw_count,
                                     uint32_t base_log, uint32_t level, const uint32_t *ggsw_indexes,
                                     const uint64_t *glwe_in, uint64_t *glwe_inout, size_t count) {
    return guarded([&] {
        if (!ctx || (!ggsw_list && count) || (!glwe_in && count) || (!glwe_inout && count)) fail("null argument");
        if (ctx->multi()) {
            require_ggsw_shape(ctx, base_log, level);
            validate_ggsw_indexes(ggsw_indexes, count, ggsw_count);
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_ggsw_external_product(
                    s, ggsw_share(ctx, ggsw_list, ggsw_indexes, level, a), ggsw_indexes ? ggsw_count : n, base_log,
                    level, ggsw_indexes ? ggsw_indexes + a : nullptr, glwe_in + a * ctx->glwe_len(),
                    glwe_inout + a * ctx->glwe_len(), n);
            });
        }
        ggsw_node_host(ctx, GGSW_EP, ggsw_list, ggsw_count, base_log, level, ggsw_indexes, nullptr, glwe_in,
                       glwe_inout, count);
    });
}

int tfhe_mi355_ggsw_external_product_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, size_t ggsw_count,
                                           uint32_t base_log, uint32_t level, const uint32_t *d_ggsw_indexes,
                                           const uint64_t *d_glwe_in, uint64_t *d_glwe_inout, size_t count,
                                           void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_fourier_ggsw && count) || (!d_glwe_in && count) || (!d_glwe_inout && count))
            fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ggsw_node_dev(ctx, GGSW_EP, (const double2 *)d_fourier_ggsw, ggsw_count, d_ggsw_indexes, base_log,
                             level, nullptr, d_glwe_in, d_glwe_inout, count, (hipStream_t)stream);
    });
}

int tfhe_mi355_ggsw_cmux(TfheMi355Context *ctx, const uint64_t *ggsw_list, size_t ggsw_count, uint32_t base_log,
                         uint32_t level, const uint32_t *ggsw_indexes, const uint64_t *ct0, const uint64_t *ct1,
                         uint64_t *out, size_t count) {
    return guarded([&] {
        if (!ctx || (!ggsw_list && count) || (!ct0 && count) || (!ct1 && count) || (!out && count))
            fail("null argument");
        if (ctx->multi()) {
            require_ggsw_shape(ctx, base_log, level);
            validate_ggsw_indexes(ggsw_indexes, count, ggsw_count);
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_ggsw_cmux(s, ggsw_share(ctx, ggsw_list, ggsw_indexes, level, a),
                                            ggsw_indexes ? ggsw_count : n, base_log, level,
                                            ggsw_indexes ? ggsw_indexes + a : nullptr, ct0 + a * ctx->glwe_len(),
                                            ct1 + a * ctx->glwe_len(), out + a * ctx->glwe_len(), n);
            });
        }
        ggsw_node_host(ctx, GGSW_CMUX, ggsw_list, ggsw_count, base_log, level, ggsw_indexes, ct0, ct1, out, count);
    });
}

int tfhe_mi355_ggsw_cmux_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, size_t ggsw_count,
                               uint32_t base_log, uint32_t level, const uint32_t *d_ggsw_indexes,
                               const uint64_t *d_ct0, const uint64_t *d_ct1, uint64_t *d_out, size_t count,
                               void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_fourier_ggsw && count) || (!d_ct0 && count) || (!d_ct1 && count) || (!d_out && count))
            fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ggsw_node_dev(ctx, GGSW_CMUX, (const double2 *)d_fourier_ggsw, ggsw_count, d_ggsw_indexes, base_log,
                             level, d_ct0, d_ct1, d_out, count, (hipStream_t)stream);
    });
}

int tfhe_mi355_ggsw_list_fourier_bytes(TfheMi355Context *ctx, size_t ggsw_count, uint32_t level, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);
        if (!ctx || !bytes) fail("null argument");
        if (level == 0 || level > 32) fail("GGSW level %u out of range", level);
        *bytes = ggsw_count * ggsw_fourier_bytes(ctx, level);
    });
}

int tfhe_mi355_ggsw_list_convert_async(TfheMi355Context *ctx, const uint64_t *d_ggsw_list, size_t ggsw_count,
                                       uint32_t level, void *d_fourier_ggsw, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_ggsw_list && ggsw_count) || (!d_fourier_ggsw && ggsw_count)) fail("null argument");
        require_ggsw_shape(ctx, 1, level);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        ggsw_list_to_fourier_dev(ctx, d_ggsw_list, (double2 *)d_fourier_ggsw, ggsw_count, level, (hipStream_t)stream);
    });
}

int tfhe_mi355_vertical_packing_scratch(TfheMi355Context *ctx, size_t npoly, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        if (npoly == 0 || npoly > 0x40000000u || !is_pow2((uint32_t)npoly))
            fail("vertical packing: the LUT has %zu polynomials, not a power of two", npoly);
        *bytes = vp_scratch_bytes(ctx, npoly, 1, count);
    });
}

int tfhe_mi355_vertical_packing_async(TfheMi355Context *ctx, const void *d_fourier_ggsw, uint32_t base_log,
                                      uint32_t level, uint32_t nbits, const uint64_t *d_luts, size_t lut_count,
                                      size_t npoly, const uint32_t *d_lut_indexes, size_t count, uint64_t *d_lwe_out,
                                      void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_fourier_ggsw && count) || !d_luts || (!d_lwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_vertical_packing_dev(ctx, (const double2 *)d_fourier_ggsw, base_log, level, nbits, d_luts, lut_count,
                                    1, npoly, d_lut_indexes, count, d_lwe_out, d_scratch, scratch_bytes,
                                    (hipStream_t)stream);
    });
}

int tfhe_mi355_vertical_packing(TfheMi355Context *ctx, const uint64_t *ggsw_list, uint32_t base_log, uint32_t level,
                                uint32_t nbits, const uint64_t *luts, size_t lut_count, size_t npoly,
                                const uint32_t *lut_indexes, size_t count, uint64_t *lwe_out) {
    return guarded([&] {
        if (!ctx || (!ggsw_list && count) || !luts || (!lwe_out && count)) fail("null argument");
        if (ctx->multi()) {
            const size_t per_item = (size_t)nbits * ggsw_std_words(ctx, level <= 32 ? level : 0);
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_vertical_packing(s, ggsw_list + a * per_item, base_log, level, nbits, luts, lut_count,
                                                   npoly, lut_indexes ? lut_indexes + a : nullptr, n,
                                                   lwe_out + a * (ctx->big_dim() + 1));
            });
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_ggsw_shape(ctx, base_log, level);
        vp_shape(ctx, nbits, npoly);
        if (lut_count == 0) fail("lut_count out of range");
        validate_lut_indexes(lut_indexes, count, lut_count);
        if (count == 0) return;
        // items in chunks of at most ~256 MiB of standard-domain GGSWs (each item brings nbits of them)
        const size_t item_std = (size_t)nbits * ggsw_std_words(ctx, level) * 8;
        const size_t item_f = (size_t)nbits * ggsw_fourier_bytes(ctx, level);
        const size_t chunk = std::min(count, std::max<size_t>(1, ((size_t)256 << 20) / item_std));
        const size_t lut_b = lut_count * npoly * ctx->N() * 8, out_w = ctx->big_dim() + 1;
        DeviceBuffer d_std, d_f, d_luts, d_idx, d_out, d_scr;
        d_std.reserve(chunk * item_std);
        d_f.reserve(chunk * item_f);
        d_luts.reserve(lut_b);
        d_out.reserve(chunk * out_w * 8);
        d_scr.reserve(std::max<size_t>(vp_scratch_bytes(ctx, npoly, 1, chunk), 256));
        if (lut_indexes) d_idx.reserve(chunk * 4);
        hipStream_t s = ctx->stream;
        check(hipMemcpyAsync(d_luts.ptr, luts, lut_b, hipMemcpyHostToDevice, s), "H2D luts");
        for (size_t a = 0; a < count; a += chunk) {
            const size_t n = std::min(chunk, count - a);
            check(hipMemcpyAsync(d_std.ptr, ggsw_list + a * (item_std / 8), n * item_std, hipMemcpyHostToDevice, s),
                  "H2D GGSW list");
            if (lut_indexes)
                check(hipMemcpyAsync(d_idx.ptr, lut_indexes + a, n * 4, hipMemcpyHostToDevice, s), "H2D lut indexes");
            ggsw_list_to_fourier_dev(ctx, (const uint64_t *)d_std.ptr, (double2 *)d_f.ptr, n * nbits, level, s);
            launch_vertical_packing_dev(ctx, (const double2 *)d_f.ptr, base_log, level, nbits,
                                        (const uint64_t *)d_luts.ptr, lut_count, 1, npoly, (const uint32_t *)d_idx.ptr, n,
                                        (uint64_t *)d_out.ptr, d_scr.ptr, d_scr.bytes, s);
            check(hipMemcpyAsync(lwe_out + a * out_w, d_out.ptr, n * out_w * 8, hipMemcpyDeviceToHost, s), "D2H out");
            check(hipStreamSynchronize(s), "vertical packing sync");
        }
    });
}

// ---- WoP-PBS, the bootstrapped half ------------------------------------------------------------------

int tfhe_mi355_pfpksk_list_upload(TfheMi355Context *ctx, const uint64_t *pfpksk, size_t len, uint32_t base_log,
                                  uint32_t level) {
    return guarded([&] {
        if (!ctx || !pfpksk) fail("null argument");
        if (base_log < 1 || base_log > 31 || level < 1 || level > 63 || base_log * level > 63)
            fail("invalid pfpks decomposition base_log %u x level %u (1 <= base_log <= 31, level >= 1, base_log * level "
                 "<= 63)",
                 base_log, level);
        if (ctx->multi()) {  // uploaded to every device from the host, as the packing key
            auto w = key_write_all(ctx);
            for (auto *s : ctx->shards) abi(tfhe_mi355_pfpksk_list_upload(s, pfpksk, len, base_log, level));
            return;
        }
        KeyWrite kw(ctx);
        require_width64(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (ctx->glwe_len() % 64) fail("pfpks needs (k+1) * N to be a multiple of 64");
        if (len != ctx->pfpksk_len(level))
            fail("pfpksk list has %zu words, expected %zu ([k+1][kN+1][level][(k+1)N])", len, ctx->pfpksk_len(level));
        ctx->pfpksk_ready = ctx->pfpksk_planes_ready = false;
        ctx->pfpksk.reserve(len * sizeof(uint64_t));
        check(hipMemcpy(ctx->pfpksk.ptr, pfpksk, len * sizeof(uint64_t), hipMemcpyHostToDevice), "upload pfpksk");
        ctx->pfks_base_log = base_log;
        ctx->pfks_level = level;
        if (pfpks_use_mfma(ctx)) {
            const int in_rows = (int)ctx->big_dim() + 1, keys = (int)ctx->k() + 1;
            ctx->pfpksk_planes.reserve(8 * pfpks_mfma_rows(in_rows, (int)level) *
                                       pfpks_mfma_cols(keys * (int)ctx->glwe_len()));
            check(launch_pfpksk_repack((const uint64_t *)ctx->pfpksk.ptr, (int8_t *)ctx->pfpksk_planes.ptr, keys, in_rows,
                                       (int)level, (int)ctx->glwe_len(), ctx->stream),
                  "pfpksk repack");
            ctx->pfpksk_planes_ready = true;
        }
        check(hipStreamSynchronize(ctx->stream), "pfpksk repack sync");
        ctx->pfpksk_ready = true;
    });
}

}  // extern "C"

namespace {
void chunk_pfpks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
                 size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_pfpks_dev(c, i, o, n, sc, sb, s);
}

// host-pointer form of a WoP-PBS call: items in chunks through device buffers of the call's own, on
// the context's stream; f(d_in, d_out, d_idx, n, d_scratch, scratch_bytes, stream) launches one chunk
template <class Scratch, class F>
void host_wop_call(TfheMi355Context *ctx, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                   const uint32_t *idx, size_t count, size_t chunk, Scratch &&scratch_bytes, F &&f) {
    if (count == 0) return;
    chunk = std::min(count, std::max<size_t>(chunk, 1));
    DeviceBuffer d_in, d_out, d_idx, d_scr;
    d_in.reserve(chunk * in_words * 8);
    d_out.reserve(chunk * out_words * 8);
    d_scr.reserve(std::max<size_t>(scratch_bytes(chunk), 256));
    if (idx) d_idx.reserve(chunk * 4);
    hipStream_t s = ctx->stream;
    for (size_t a = 0; a < count; a += chunk) {
        const size_t n = std::min(chunk, count - a);
        check(hipMemcpyAsync(d_in.ptr, in + a * in_words, n * in_words * 8, hipMemcpyHostToDevice, s), "H2D in");
        if (idx) check(hipMemcpyAsync(d_idx.ptr, idx + a, n * 4, hipMemcpyHostToDevice, s), "H2D lut indexes");
        f((const uint64_t *)d_in.ptr, (uint64_t *)d_out.ptr, (const uint32_t *)d_idx.ptr, n, d_scr.ptr, d_scr.bytes, s);
        check(hipMemcpyAsync(out + a * out_words, d_out.ptr, n * out_words * 8, hipMemcpyDeviceToHost, s), "D2H out");
        check(hipStreamSynchronize(s), "WoP-PBS sync");
    }
}
constexpr size_t kWopChunkRows = 4096;  // PBS rows per chunk of the host-pointer forms
}  // namespace

extern "C" {

int tfhe_mi355_private_functional_packing_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out,
                                                    size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!glwe_out && count)) fail("null argument");
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_private_functional_packing_keyswitch(s, lwe_in + a * (ctx->big_dim() + 1),
                                                                       glwe_out + a * (ctx->k() + 1) * ctx->glwe_len(), n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_pfpksk(ctx);
        run_host_pipeline(ctx, lwe_in, ctx->big_dim() + 1, glwe_out, (ctx->k() + 1) * ctx->glwe_len(), nullptr, 0, 0,
                          nullptr, count, chunk_pfpks, pfpks_scratch_bytes);
    });
}

int tfhe_mi355_private_functional_packing_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        if (!ctx->pfpksk_ready)
            fail("private functional packing keyswitching keys not uploaded: their decomposition sizes the scratch");
        *bytes = pfpks_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_private_functional_packing_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in,
                                                          uint64_t *d_glwe_out, size_t count, void *d_scratch,
                                                          size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_in && count) || (!d_glwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_pfpks_dev(ctx, d_lwe_in, d_glwe_out, count, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_extract_bits(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t delta_log, uint32_t nbits,
                            uint64_t *lwe_out, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!lwe_out && count)) fail("null argument");
        validate_extract_bits(delta_log, nbits);
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_extract_bits(s, lwe_in + a * (ctx->big_dim() + 1), delta_log, nbits,
                                               lwe_out + a * nbits * (ctx->n() + 1), n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        host_wop_call(
            ctx, lwe_in, ctx->big_dim() + 1, lwe_out, (size_t)nbits * (ctx->n() + 1), nullptr, count, kWopChunkRows,
            [&](size_t n) { return extract_bits_scratch_bytes(ctx, n); },
            [&](const uint64_t *i, uint64_t *o, const uint32_t *, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_extract_bits_dev(ctx, i, delta_log, nbits, o, n, sc, sb, s);
            });
    });
}

int tfhe_mi355_extract_bits_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        *bytes = extract_bits_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_extract_bits_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t delta_log, uint32_t nbits,
                                  uint64_t *d_lwe_out, size_t count, void *d_scratch, size_t scratch_bytes,
                                  void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_in && count) || (!d_lwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_extract_bits_dev(ctx, d_lwe_in, delta_log, nbits, d_lwe_out, count, d_scratch, scratch_bytes,
                                (hipStream_t)stream);
    });
}

int tfhe_mi355_circuit_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t delta_log,
                                 uint32_t cbs_base_log, uint32_t cbs_level, uint64_t *ggsw_out, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!ggsw_out && count)) fail("null argument");
        if (ctx->multi()) {
            validate_cbs(ctx, delta_log, cbs_base_log, cbs_level);
            const size_t per_item = ggsw_std_words(ctx, cbs_level);
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_circuit_bootstrap(s, lwe_in + a * (ctx->n() + 1), delta_log, cbs_base_log, cbs_level,
                                                    ggsw_out + a * per_item, n);
            });
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_wop_shape(ctx);
        validate_cbs(ctx, delta_log, cbs_base_log, cbs_level);
        require_pfpksk(ctx);
        host_wop_call(
            ctx, lwe_in, ctx->n() + 1, ggsw_out, ggsw_std_words(ctx, cbs_level), nullptr, count,
            kWopChunkRows / cbs_level, [&](size_t n) { return cbs_scratch_bytes(ctx, cbs_level, n); },
            [&](const uint64_t *i, uint64_t *o, const uint32_t *, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_cbs_dev(ctx, i, delta_log, cbs_base_log, cbs_level, o, n, sc, sb, s);
            });
    });
}

int tfhe_mi355_circuit_bootstrap_scratch(TfheMi355Context *ctx, uint32_t cbs_level, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        if (cbs_level == 0 || cbs_level > 32) fail("GGSW level %u out of range", cbs_level);
        std::lock_guard<std::mutex> g(ctx->mu);
        if (!ctx->pfpksk_ready)
            fail("private functional packing keyswitching keys not uploaded: their decomposition sizes the scratch");
        *bytes = cbs_scratch_bytes(ctx, cbs_level, count);
    });
}

int tfhe_mi355_circuit_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t delta_log,
                                       uint32_t cbs_base_log, uint32_t cbs_level, uint64_t *d_ggsw_out, size_t count,
                                       void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_in && count) || (!d_ggsw_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_cbs_dev(ctx, d_lwe_in, delta_log, cbs_base_log, cbs_level, d_ggsw_out, count, d_scratch, scratch_bytes,
                       (hipStream_t)stream);
    });
}

int tfhe_mi355_circuit_bootstrap_vertical_packing(TfheMi355Context *ctx, const uint64_t *lwe_in, uint32_t nbits,
                                                  uint32_t cbs_base_log, uint32_t cbs_level, const uint64_t *luts,
                                                  size_t lut_count, size_t nout, size_t npoly,
                                                  const uint32_t *lut_indexes, size_t count, uint64_t *lwe_out) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || !luts || (!lwe_out && count)) fail("null argument");
        if (nout == 0 || nout > 0xffffu) fail("circuit bootstrap + vertical packing: nout %zu out of range", nout);
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_circuit_bootstrap_vertical_packing(
                    s, lwe_in + a * nbits * (ctx->n() + 1), nbits, cbs_base_log, cbs_level, luts, lut_count, nout, npoly,
                    lut_indexes ? lut_indexes + a : nullptr, n, lwe_out + a * nout * (ctx->big_dim() + 1));
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_wop_shape(ctx);
        validate_cbs(ctx, 63, cbs_base_log, cbs_level);
        vp_shape(ctx, nbits, npoly);
        if (lut_count == 0 || lut_count > 0xffffffffu) fail("lut_count out of range");
        validate_lut_indexes(lut_indexes, count, lut_count);
        require_pfpksk(ctx);
        if (count == 0) return;
        DeviceBuffer d_luts;
        const size_t lut_b = lut_count * nout * npoly * ctx->N() * 8;
        d_luts.reserve(lut_b);
        check(hipMemcpyAsync(d_luts.ptr, luts, lut_b, hipMemcpyHostToDevice, ctx->stream), "H2D luts");
        host_wop_call(
            ctx, lwe_in, (size_t)nbits * (ctx->n() + 1), lwe_out, nout * (ctx->big_dim() + 1), lut_indexes, count,
            kWopChunkRows / ((size_t)nbits * cbs_level),
            [&](size_t n) { return cbvp_layout(ctx, nbits, cbs_level, nout, npoly, lut_count, n).total(); },
            [&](const uint64_t *i, uint64_t *o, const uint32_t *x, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_cbvp_dev(ctx, i, nbits, cbs_base_log, cbs_level, (const uint64_t *)d_luts.ptr, lut_count, nout,
                                npoly, x, n, o, sc, sb, s);
            });
    });
}

int tfhe_mi355_circuit_bootstrap_vertical_packing_scratch(TfheMi355Context *ctx, uint32_t nbits, uint32_t cbs_level,
                                                          size_t lut_count, size_t nout, size_t npoly, size_t count,
                                                          size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        if (cbs_level == 0 || cbs_level > 32) fail("GGSW level %u out of range", cbs_level);
        vp_shape(ctx, nbits, npoly);
        std::lock_guard<std::mutex> g(ctx->mu);
        if (!ctx->pfpksk_ready)
            fail("private functional packing keyswitching keys not uploaded: their decomposition sizes the scratch");
        *bytes = cbvp_layout(ctx, nbits, cbs_level, nout, npoly, lut_count, count).total();
    });
}

int tfhe_mi355_circuit_bootstrap_vertical_packing_async(TfheMi355Context *ctx, const uint64_t *d_lwe_in, uint32_t nbits,
                                                        uint32_t cbs_base_log, uint32_t cbs_level,
                                                        const uint64_t *d_luts, size_t lut_count, size_t nout,
                                                        size_t npoly, const uint32_t *d_lut_indexes, size_t count,
                                                        uint64_t *d_lwe_out, void *d_scratch, size_t scratch_bytes,
                                                        void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_in && count) || !d_luts || (!d_lwe_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_cbvp_dev(ctx, d_lwe_in, nbits, cbs_base_log, cbs_level, d_luts, lut_count, nout, npoly, d_lut_indexes,
                        count, d_lwe_out, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!lwe_out && count)) fail("null argument");
        if (ctx->multi()) {
            const size_t wi = ctx->big_dim() + 1, wo = ctx->n() + 1;
            if (coalescible(count)) return abi(tfhe_mi355_keyswitch(pick_shard(ctx), lwe_in, lwe_out, count));
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_keyswitch(s, lwe_in + a * wi, lwe_out + a * wo, n);
            });
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_ksk(ctx);
        if (coalescible(count)) {
            CoalescedReq r{lwe_in, lwe_out, nullptr, 0, nullptr, count};
            return coalesced_call(ctx, CO_KS, r);
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        run_host_pipeline(ctx, lwe_in, ctx->big_dim() + 1, lwe_out, ctx->n() + 1, nullptr, 0, 0, nullptr, count,
                          chunk_ks, ks_scratch_bytes);
    });
}

int tfhe_mi355_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        *bytes = ks_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_in, uint64_t *d_out, size_t count,
                               void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_in && count) || (!d_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ks_dev(ctx, d_in, d_out, count, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_lwe_keyswitch_key_create(TfheMi355Context *ctx, const uint64_t *ksk, size_t len, size_t in_dim,
                                        size_t out_dim, uint32_t base_log, uint32_t level,
                                        TfheMi355KeyswitchKey **key) {
    return guarded([&] {
        if (!ctx || !ksk || !key) fail("null argument");
        *key = nullptr;
        if (in_dim == 0 || out_dim == 0) fail("keyswitching key: zero dimension (in_dim %zu, out_dim %zu)", in_dim, out_dim);
        if (in_dim > 0x3fffffffu || out_dim > 0x3fffffffu) fail("keyswitching key: dimension too large");
        if (base_log == 0 || level == 0 || (uint64_t)base_log * level >= 64)
            fail("keyswitching key: decomposition base_log %u x level %u out of range (base_log * level < 64)", base_log,
                 level);
        if (len != in_dim * level * (out_dim + 1))
            fail("keyswitching key has %zu words, expected %zu", len, in_dim * level * (out_dim + 1));
        static const bool no_mfma = env_flag("TFHE_MI355_KS_NO_MFMA");
        const bool mfma = !no_mfma && ks_mfma_supported((int)in_dim, (int)level, (int)base_log);
        if (!mfma && !keyswitch_scalar_supported((int)base_log, (int)level))
            fail("keyswitching key: no kernel for base_log %u x level %u (base_log <= 15, level <= 16)", base_log, level);
        std::unique_ptr<TfheMi355KeyswitchKey> k(new TfheMi355KeyswitchKey);
        k->ctx = ctx;
        k->in_dim = in_dim;
        k->out_dim = out_dim;
        k->base_log = base_log;
        k->level = level;
        k->mfma = mfma;
        std::vector<TfheMi355Context *> where = ctx->multi() ? ctx->shards : std::vector<TfheMi355Context *>{ctx};
        for (TfheMi355Context *c : where) {
            if (k->on(c->device)) continue;
            check(hipSetDevice(c->device), "hipSetDevice");
            std::unique_ptr<TfheMi355KeyswitchKey::Part> part(new TfheMi355KeyswitchKey::Part);
            part->device = c->device;
            part->ksk.reserve(len * sizeof(uint64_t));
            check(hipMemcpy(part->ksk.ptr, ksk, len * sizeof(uint64_t), hipMemcpyHostToDevice), "upload ksk");
            if (mfma) {
                std::lock_guard<std::mutex> g(c->mu);  // the repack runs on the context's stream
                part->planes.reserve(8 * ks_mfma_rows((int)in_dim, (int)level) * ks_mfma_cols((int)out_dim));
                check(launch_ksk_repack((const uint64_t *)part->ksk.ptr, (int8_t *)part->planes.ptr, (int)in_dim,
                                        (int)level, (int)out_dim, c->stream),
                      "ksk repack");
                check(hipStreamSynchronize(c->stream), "ksk repack sync");
            }
            k->parts.push_back(std::move(part));
        }
        *key = k.release();
    });
}

int tfhe_mi355_lwe_keyswitch_key_destroy(TfheMi355KeyswitchKey *key) {
    return guarded([&] {
        if (!key) return;
        for (auto &p : key->parts) {
            (void)hipSetDevice(p->device);
            p->ksk.release();
            p->planes.release();
        }
        delete key;
    });
}

int tfhe_mi355_keyswitch_with_key(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key, const uint64_t *lwe_in,
                                  uint64_t *lwe_out, size_t count) {
    return guarded([&] {
        if (!ctx || !key || (!lwe_in && count) || (!lwe_out && count)) fail("null argument");
        if (key->ctx != ctx && key->ctx != ctx->owner) fail("keyswitching key belongs to another context");
        const size_t wi = key->in_dim + 1, wo = key->out_dim + 1;
        if (ctx->multi())
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_keyswitch_with_key(s, key, lwe_in + a * wi, lwe_out + a * wo, n);
            });
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        host_wop_call(
            ctx, lwe_in, wi, lwe_out, wo, nullptr, count, kWopChunkRows,
            [&](size_t n) { return ks_key_scratch_bytes(key, n); },
            [&](const uint64_t *i, uint64_t *o, const uint32_t *, size_t n, void *sc, size_t sb, hipStream_t s) {
                launch_ks_key_dev(ctx, key, i, o, n, sc, sb, s);
            });
    });
}

int tfhe_mi355_keyswitch_with_key_scratch(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key, size_t count,
                                          size_t *bytes) {
    return guarded([&] {
        if (!ctx || !key || !bytes) fail("null argument");
        *bytes = ks_key_scratch_bytes(key, count);
    });
}

int tfhe_mi355_keyswitch_with_key_async(TfheMi355Context *ctx, const TfheMi355KeyswitchKey *key,
                                        const uint64_t *d_lwe_in, uint64_t *d_lwe_out, size_t count, void *d_scratch,
                                        size_t scratch_bytes, void *stream) {
    return guarded([&] {
        if (!ctx || !key || (!d_lwe_in && count) || (!d_lwe_out && count)) fail("null argument");
        if (key->ctx != ctx && key->ctx != ctx->owner) fail("keyswitching key belongs to another context");
        ctx = primary(ctx);  // device pointers: the first device's shard
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ks_key_dev(ctx, key, d_lwe_in, d_lwe_out, count, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_keyswitch_programmable_bootstrap_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        *bytes = ks_pbs_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_keyswitch_programmable_bootstrap_async(TfheMi355Context *ctx, const uint64_t *d_in,
                                                      uint64_t *d_out, const uint64_t *d_luts, size_t lut_count,
                                                      const uint32_t *d_idx, size_t count, void *d_scratch,
                                                      size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_in && count) || (!d_out && count) || !d_luts || (!d_scratch && count))
            fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ks_pbs_dev(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, d_scratch, scratch_bytes,
                          (hipStream_t)stream);
    });
}

int tfhe_mi355_keyswitch_programmable_bootstrap(TfheMi355Context *ctx, const uint64_t *lwe_in,
                                                uint64_t *lwe_out, const uint64_t *luts, size_t lut_count,
                                                const uint32_t *lut_indexes, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!lwe_out && count) || !luts) fail("null argument");
        if (ctx->multi()) {
            const size_t wi = ctx->big_dim() + 1, wo = ctx->big_dim() + 1;
            if (coalescible(count))
                return abi(tfhe_mi355_keyswitch_programmable_bootstrap(pick_shard(ctx), lwe_in, lwe_out, luts, lut_count, lut_indexes, count));
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_keyswitch_programmable_bootstrap(s, lwe_in + a * wi, lwe_out + a * wo, luts, lut_count,
                            lut_indexes ? lut_indexes + a : nullptr, n);
            });
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_fbsk(ctx);
        require_ksk(ctx);
        if (lut_count == 0) fail("lut_count must be >= 1");
        validate_lut_indexes(lut_indexes, count, lut_count);
        if (coalescible(count)) {
            CoalescedReq r{lwe_in, lwe_out, luts, lut_count, lut_indexes, count};
            return coalesced_call(ctx, CO_KS_PBS, r);
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        run_host_pipeline(ctx, lwe_in, ctx->big_dim() + 1, lwe_out, ctx->big_dim() + 1, luts, ctx->glwe_len(),
                          lut_count, lut_indexes, count, launch_ks_pbs_dev, ks_pbs_scratch_bytes);
    });
}

int tfhe_mi355_programmable_bootstrap_keyswitch_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || !bytes) fail("null argument");
        std::lock_guard<std::mutex> g(ctx->mu);
        *bytes = pbs_ks_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_programmable_bootstrap_keyswitch_async(TfheMi355Context *ctx, const uint64_t *d_in,
                                                      uint64_t *d_out, const uint64_t *d_luts, size_t lut_count,
                                                      const uint32_t *d_idx, size_t count, void *d_scratch,
                                                      size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_in && count) || (!d_out && count) || !d_luts || (!d_scratch && count))
            fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_pbs_ks_dev(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, d_scratch, scratch_bytes,
                          (hipStream_t)stream);
    });
}

int tfhe_mi355_programmable_bootstrap_keyswitch(TfheMi355Context *ctx, const uint64_t *lwe_in,
                                                uint64_t *lwe_out, const uint64_t *luts, size_t lut_count,
                                                const uint32_t *lut_indexes, size_t count) {
    return guarded([&] {
        if (!ctx || (!lwe_in && count) || (!lwe_out && count) || !luts) fail("null argument");
        if (ctx->multi()) {
            const size_t wi = ctx->n() + 1, wo = ctx->n() + 1;
            if (coalescible(count))
                return abi(tfhe_mi355_programmable_bootstrap_keyswitch(pick_shard(ctx), lwe_in, lwe_out, luts, lut_count, lut_indexes, count));
            return split_rows(ctx, count, [&](TfheMi355Context *s, size_t a, size_t n) {
                return tfhe_mi355_programmable_bootstrap_keyswitch(s, lwe_in + a * wi, lwe_out + a * wo, luts, lut_count,
                            lut_indexes ? lut_indexes + a : nullptr, n);
            });
        }
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_fbsk(ctx);
        require_ksk(ctx);
        if (lut_count == 0) fail("lut_count must be >= 1");
        validate_lut_indexes(lut_indexes, count, lut_count);
        if (coalescible(count)) {
            CoalescedReq r{lwe_in, lwe_out, luts, lut_count, lut_indexes, count};
            return coalesced_call(ctx, CO_PBS_KS, r);
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        run_host_pipeline(ctx, lwe_in, ctx->n() + 1, lwe_out, ctx->n() + 1, luts, ctx->glwe_len(), lut_count,
                          lut_indexes, count, launch_pbs_ks_dev, pbs_ks_scratch_bytes);
    });
}

int tfhe_mi355_lwe_scalar_mul_add_async(TfheMi355Context *ctx, uint64_t *d_y, const uint64_t *d_x, uint64_t scalar,
                                        size_t rows, size_t words, size_t y_stride, size_t x_stride, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_y && rows * words)) fail("null argument");
        if (words > y_stride || (d_x && words > x_stride)) fail("row stride smaller than the row");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        check(launch_lwe_scalar_mul_add(d_y, d_x, scalar, rows, words, y_stride, x_stride, (hipStream_t)stream),
              "lwe scalar_mul_add");
    });
}

int tfhe_mi355_trivial_pbs_async(TfheMi355Context *ctx, uint64_t *d_body, size_t rows, size_t stride,
                                 const uint64_t *d_lut, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || ((!d_body || !d_lut) && rows)) fail("null argument");
        const uint64_t msup = (uint64_t)ctx->p.message_modulus * ctx->p.carry_modulus;
        if (msup == 0 || ctx->N() % msup) fail("message space does not divide the polynomial size");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        check(launch_trivial_pbs(d_body, rows, stride, d_lut + ctx->k() * ctx->N(), (1ULL << 63) / msup, msup,
                                 ctx->N() / msup, (hipStream_t)stream),
              "trivial pbs");
    });
}

int tfhe_mi355_debug_torus_from_fraction(int device, const double *fr, uint64_t *acc_inout, uint64_t *set_out,
                                         size_t n) {
    return guarded([&] {
        if ((!fr || !acc_inout || !set_out) && n) fail("null argument");
        if (n == 0) return;
        check(hipSetDevice(device), "hipSetDevice");
        DeviceBuffer d_fr, d_acc, d_set;
        struct Release {
            DeviceBuffer *b[3];
            ~Release() {
                for (DeviceBuffer *x : b) x->release();
            }
        } release{{&d_fr, &d_acc, &d_set}};
        d_fr.reserve(n * sizeof(double));
        d_acc.reserve(n * sizeof(uint64_t));
        d_set.reserve(n * sizeof(uint64_t));
        check(hipMemcpy(d_fr.ptr, fr, n * sizeof(double), hipMemcpyHostToDevice), "H2D fr");
        check(hipMemcpy(d_acc.ptr, acc_inout, n * sizeof(uint64_t), hipMemcpyHostToDevice), "H2D acc");
        check(launch_torus_from_fraction((const double *)d_fr.ptr, (uint64_t *)d_acc.ptr, (uint64_t *)d_set.ptr, n,
                                         nullptr),
              "torus conversion");
        check(hipMemcpy(acc_inout, d_acc.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "D2H acc");
        check(hipMemcpy(set_out, d_set.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "D2H set");
    });
}

int tfhe_mi355_fill_accumulator(const TfheMi355Parameters *params, const uint64_t *f_values, uint64_t *acc) {
    return guarded([&] {
        if (!params || !f_values || !acc) fail("null argument");
        const size_t N = params->polynomial_size, k = params->glwe_dimension;
        const size_t p = (size_t)params->message_modulus * params->carry_modulus;
        if (p == 0 || N % p) fail("polynomial_size must be a multiple of message_modulus*carry_modulus");
        const size_t box = N / p, half = box / 2;
        const uint64_t delta = (1ULL << 63) / p;
        std::vector<uint64_t> body(N);
        for (size_t i = 0; i < p; i++)
            for (size_t j = 0; j < box; j++) body[i * box + j] = f_values[i] * delta;
        for (size_t j = 0; j < half; j++) body[j] = 0 - body[j];
        std::memset(acc, 0, sizeof(uint64_t) * k * N);
        for (size_t j = 0; j < N; j++) acc[k * N + j] = body[(j + half) % N];
    });
}

}  // extern "C"

// ---- 32-bit torus (include/tfhe_mi355.h "32-bit torus") ------------------------------------------
namespace {

void require_single32(const TfheMi355Context *c) {
    if (!c) fail("null ctx");
    if (c->multi()) fail("32-bit-torus calls are not available on a multi-device context");
}

void require_shape32(const TfheMi355Context *c) {
    const TfheMi355Parameters &p = c->p;
    if (p.grouping_factor || !classic_pbs32_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level))
        fail("no 32-bit-torus PBS kernel for N=%u k=%u pbs_level=%u grouping_factor=%u", p.polynomial_size,
             p.glwe_dimension, p.pbs_level, p.grouping_factor);
    if (p.pbs_base_log < 2 || p.pbs_base_log * p.pbs_level > 30)
        fail("32-bit-torus pbs decomposition: base_log >= 2 and base_log*level <= 30 (got %u x %u)", p.pbs_base_log,
             p.pbs_level);
}

void require_ks_shape32(const TfheMi355Context *c) {
    if (!keyswitch32_scalar_supported((int)c->p.ks_base_log, (int)c->p.ks_level))
        fail("32-bit-torus ks decomposition: base_log*level <= 30, base_log <= 15, level <= 16 (got %u x %u)",
             c->p.ks_base_log, c->p.ks_level);
}

void require_fbsk32(const TfheMi355Context *c) {
    require_width32(c);
    if (!c->fbsk32_ready) fail("32-bit-torus bootstrapping key not uploaded");
}
void require_ksk32(const TfheMi355Context *c) {
    require_width32(c);
    if (!c->ksk32_ready) fail("32-bit-torus keyswitching key not uploaded");
}
void require_order(int pbs_order) {
    if (pbs_order != 0 && pbs_order != 1) fail("pbs_order must be 0 (KeyswitchBootstrap) or 1 (BootstrapKeyswitch)");
}

bool ks32_use_mfma(const TfheMi355Context *c) {
    static const bool disabled = env_flag("TFHE_MI355_KS_NO_MFMA");
    return !disabled && ks32_mfma_supported((int)c->big_dim(), (int)c->p.ks_level, (int)c->p.ks_base_log);
}
size_t ks32_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return ks32_use_mfma(c) && count ? ks32_mfma_scratch_bytes((int)c->big_dim(), (int)c->p.ks_level, (int)count) : 0;
}
// the u32 PBS kernel covers the batch in one pass: no ticket, no scratch
size_t pbs32_scratch_bytes(const TfheMi355Context *, size_t) { return 0; }

void launch_pbs32_dev(TfheMi355Context *c, const uint32_t *d_in, uint32_t *d_out, const uint32_t *d_luts,
                      size_t lut_count, const uint32_t *d_idx, size_t count, hipStream_t s, bool glwe_out) {
    if (count == 0) return;
    require_fbsk32(c);
    if (lut_count == 0) fail("lut_count must be >= 1");
    if (lut_count > 0xffffffffu) fail("lut_count too large");
    if (count > 0x7fffffff) fail("batch too large");
    ClassicPbs32Launch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.luts = d_luts;
    a.lut_indexes = d_idx;
    a.lut_count = (uint32_t)lut_count;
    a.fbsk = reinterpret_cast<const double2 *>(c->fbsk.ptr);
    a.W = c->tables.W;
    a.twist = c->tables.twist;
    a.n = (int)c->n();
    a.base_log = (int)c->p.pbs_base_log;
    a.count = (int)count;
    a.glwe_out = glwe_out;
    TimedLaunch tl(c->timer_or_null(), "pbs_classic32_kernel", s);
    check(launch_classic_pbs32((int)c->N(), (int)c->k(), (int)c->p.pbs_level, a, s), "launch u32 pbs");
}

void launch_ks32_dev(TfheMi355Context *c, const uint32_t *d_in, uint32_t *d_out, size_t count, void *scratch,
                     size_t scratch_bytes, hipStream_t s) {
    if (count == 0) return;
    require_ksk32(c);
    if (count > 0x7fffffffu) fail("count too large");
    Keyswitch32Launch a;
    a.lwe_in = d_in;
    a.lwe_out = d_out;
    a.ksk = reinterpret_cast<const uint32_t *>(c->ksk32.ptr);
    a.in_dim = (int)c->big_dim();
    a.out_dim = (int)c->n();
    a.base_log = (int)c->p.ks_base_log;
    a.level = (int)c->p.ks_level;
    a.count = (int)count;
    TimedLaunch tl(c->timer_or_null(), "keyswitch32", s);
    if (c->ksk32_planes_ready) {
        require_scratch(scratch ? scratch_bytes : 0, ks32_scratch_bytes(c, count));
        check(launch_keyswitch32_mfma(a, (const int8_t *)c->ksk32_planes.ptr, scratch, s), "launch u32 mfma keyswitch");
        return;
    }
    check(launch_keyswitch32(a, s), "launch u32 keyswitch");
}

// gates: [prologue rows | other-side rows | keyswitch scratch]
struct Gates32Layout {
    size_t in_words, mid_words, a_bytes, b_bytes, ks_bytes;
    size_t total() const { return a_bytes + b_bytes + ks_bytes; }
};
Gates32Layout gates32_layout(const TfheMi355Context *c, size_t count, int pbs_order) {
    Gates32Layout l;
    l.in_words = (pbs_order ? c->n() : c->big_dim()) + 1;
    l.mid_words = (pbs_order ? c->big_dim() : c->n()) + 1;
    l.a_bytes = align256(count * l.in_words * sizeof(uint32_t));
    l.b_bytes = align256(count * l.mid_words * sizeof(uint32_t));
    l.ks_bytes = ks32_scratch_bytes(c, count);
    return l;
}

void launch_gates32_dev(TfheMi355Context *c, const uint8_t *d_ops, const uint32_t *d_lhs, const uint32_t *d_rhs,
                        uint32_t *d_out, size_t count, int pbs_order, void *scratch, size_t scratch_bytes,
                        hipStream_t s) {
    if (count == 0) return;
    require_fbsk32(c);
    require_ksk32(c);
    if (count > 0x3fffffffu) fail("count too large");
    const Gates32Layout l = gates32_layout(c, count, pbs_order);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    uint32_t *a = reinterpret_cast<uint32_t *>(scratch);
    uint32_t *b = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(scratch) + l.a_bytes);
    void *ks = reinterpret_cast<char *>(scratch) + l.a_bytes + l.b_bytes;
    const uint32_t *lut = reinterpret_cast<const uint32_t *>(c->lut_true32.ptr);
    {
        TimedLaunch tl(c->timer_or_null(), "boolean_ops", s);
        check(launch_bool_gates_prologue(d_ops, d_lhs, d_rhs, a, count, l.in_words, s), "gate prologue");
    }
    if (pbs_order) {  // bootstrap_keyswitch (bootstrapping.rs:299-344)
        launch_pbs32_dev(c, a, b, lut, 1, nullptr, count, s, false);
        launch_ks32_dev(c, b, d_out, count, ks, l.ks_bytes, s);
    } else {  // keyswitch_bootstrap (bootstrapping.rs:346-391)
        launch_ks32_dev(c, a, b, count, ks, l.ks_bytes, s);
        launch_pbs32_dev(c, b, d_out, lut, 1, nullptr, count, s, false);
    }
}

// mux: [2 count rows | 2 count rows | count big rows | keyswitch scratch (2 count rows)]
struct Mux32Layout {
    size_t in_words, a_bytes, c_bytes, ks_bytes;
    size_t total() const { return 2 * a_bytes + c_bytes + ks_bytes; }
};
Mux32Layout mux32_layout(const TfheMi355Context *c, size_t count, int pbs_order) {
    Mux32Layout l;
    l.in_words = (pbs_order ? c->n() : c->big_dim()) + 1;
    l.a_bytes = align256(2 * count * (std::max(c->n(), c->big_dim()) + 1) * sizeof(uint32_t));
    l.c_bytes = align256(count * (c->big_dim() + 1) * sizeof(uint32_t));
    l.ks_bytes = ks32_scratch_bytes(c, 2 * count);
    return l;
}

void launch_mux32_dev(TfheMi355Context *c, const uint32_t *d_cond, const uint32_t *d_then, const uint32_t *d_else,
                      uint32_t *d_out, size_t count, int pbs_order, void *scratch, size_t scratch_bytes,
                      hipStream_t s) {
    if (count == 0) return;
    require_fbsk32(c);
    require_ksk32(c);
    if (count > 0x1fffffffu) fail("count too large");
    const Mux32Layout l = mux32_layout(c, count, pbs_order);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    char *base = reinterpret_cast<char *>(scratch);
    uint32_t *a = reinterpret_cast<uint32_t *>(base);
    uint32_t *b = reinterpret_cast<uint32_t *>(base + l.a_bytes);
    uint32_t *sum = reinterpret_cast<uint32_t *>(base + 2 * l.a_bytes);
    void *ks = base + 2 * l.a_bytes + l.c_bytes;
    const uint32_t *lut = reinterpret_cast<const uint32_t *>(c->lut_true32.ptr);
    const size_t big = c->big_dim() + 1;
    {
        TimedLaunch tl(c->timer_or_null(), "boolean_ops", s);
        check(launch_bool_mux_prologue(d_cond, d_then, d_else, a, count, l.in_words, s), "mux prologue");
    }
    if (pbs_order) {  // mod.rs:548-565: two bootstraps, the sum, then one keyswitch
        launch_pbs32_dev(c, a, b, lut, 1, nullptr, 2 * count, s, false);
        {
            TimedLaunch tl(c->timer_or_null(), "boolean_ops", s);
            check(launch_bool_mux_epilogue(b, sum, count, big, s), "mux epilogue");
        }
        launch_ks32_dev(c, sum, d_out, count, ks, l.ks_bytes, s);
    } else {  // mod.rs:530-547: keyswitch and bootstrap each row, then the sum
        launch_ks32_dev(c, a, b, 2 * count, ks, l.ks_bytes, s);
        launch_pbs32_dev(c, b, a, lut, 1, nullptr, 2 * count, s, false);
        TimedLaunch tl(c->timer_or_null(), "boolean_ops", s);
        check(launch_bool_mux_epilogue(a, d_out, count, big, s), "mux epilogue");
    }
}

// A host-pointer u32 call: under the context's mutex, inputs staged into lane 0's device buffer, the
// kernels on the context's stream, the output copied back after them.
struct HostCall32 {
    TfheMi355Context *c;
    std::lock_guard<std::mutex> g;
    size_t in_off = 0;
    HostCall32(TfheMi355Context *c_, size_t in_bytes, size_t out_bytes, size_t scratch_bytes) : c(c_), g(c_->mu) {
        check(hipSetDevice(c->device), "hipSetDevice");
        c->lanes[0].d_in.reserve(std::max<size_t>(in_bytes, 256));
        c->lanes[0].d_out.reserve(std::max<size_t>(out_bytes, 256));
        c->io_tmp.reserve(std::max<size_t>(scratch_bytes, 256));
    }
    template <class T>
    const T *up(const T *host, size_t n) {
        if (!host || n == 0) return nullptr;
        char *d = reinterpret_cast<char *>(c->lanes[0].d_in.ptr) + in_off;
        check(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream), "H2D");
        in_off += align256(n * sizeof(T));
        return reinterpret_cast<const T *>(d);
    }
    uint32_t *out() { return reinterpret_cast<uint32_t *>(c->lanes[0].d_out.ptr); }
    void *scratch() { return c->io_tmp.ptr; }
    void down(uint32_t *host, size_t n) {
        check(hipMemcpyAsync(host, out(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream), "D2H");
        check(hipStreamSynchronize(c->stream), "u32 call sync");
    }
};

void pbs32_host(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *out, const uint32_t *luts, size_t lut_count,
                const uint32_t *lut_indexes, size_t count, bool glwe_out) {
    require_single32(ctx);
    if ((!lwe_in && count) || (!out && count) || !luts) fail("null argument");
    if (count == 0) return;
    require_fbsk32(ctx);
    if (lut_count == 0) fail("lut_count must be >= 1");
    validate_lut_indexes(lut_indexes, count, lut_count);
    const size_t wi = ctx->n() + 1, wo = glwe_out ? ctx->glwe_len() : ctx->big_dim() + 1;
    HostCall32 h(ctx, align256(count * wi * 4) + align256(lut_count * ctx->glwe_len() * 4) + align256(count * 4),
                 count * wo * 4, 0);
    const uint32_t *d_in = h.up(lwe_in, count * wi);
    const uint32_t *d_luts = h.up(luts, lut_count * ctx->glwe_len());
    const uint32_t *d_idx = h.up(lut_indexes, lut_indexes ? count : 0);
    launch_pbs32_dev(ctx, d_in, h.out(), d_luts, lut_count, d_idx, count, ctx->stream, glwe_out);
    h.down(out, count * wo);
}

}  // namespace

extern "C" {

int tfhe_mi355_bootstrap_key_upload_u32(TfheMi355Context *ctx, const uint32_t *bsk, size_t len) {
    return guarded([&] {
        require_single32(ctx);
        if (!bsk) fail("null argument");
        KeyWrite kw(ctx);
        require_width32(ctx);
        require_shape32(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->std_bsk_len()) fail("bootstrapping key has %zu words, expected %zu", len, ctx->std_bsk_len());
        ctx->fbsk32_ready = false;
        // [u32 key | the same words widened to u64], converted by the u64 path's kernel
        const size_t wide_off = align256(len * sizeof(uint32_t));
        ctx->std_staging.reserve(wide_off + len * sizeof(uint64_t));
        const uint32_t *d32 = reinterpret_cast<const uint32_t *>(ctx->std_staging.ptr);
        uint64_t *d64 = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(ctx->std_staging.ptr) + wide_off);
        check(hipMemcpyAsync(ctx->std_staging.ptr, bsk, len * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream),
              "upload u32 bsk");
        check(launch_widen32(d32, d64, len, ctx->stream), "widen u32 bsk");
        ctx->fbsk.reserve(ctx->fourier_bsk_bytes());
        check(launch_bsk_to_fourier((int)ctx->N(), d64, (double2 *)ctx->fbsk.ptr, len / ctx->N(), ctx->tables,
                                    ctx->stream),
              "u32 bsk conversion");
        // the gates' accumulator (bootstrapping.rs:59-60): zero mask, body all PLAINTEXT_TRUE
        std::vector<uint32_t> lut(ctx->glwe_len(), 0u);
        for (size_t j = ctx->big_dim(); j < ctx->glwe_len(); j++) lut[j] = 1u << 29;
        ctx->lut_true32.reserve(lut.size() * sizeof(uint32_t));
        check(hipMemcpyAsync(ctx->lut_true32.ptr, lut.data(), lut.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                             ctx->stream),
              "upload gate accumulator");
        check(hipStreamSynchronize(ctx->stream), "u32 bsk conversion sync");
        ctx->std_staging.release();
        ctx->fbsk32_ready = true;
    });
}

int tfhe_mi355_keyswitch_key_upload_u32(TfheMi355Context *ctx, const uint32_t *ksk, size_t len) {
    return guarded([&] {
        require_single32(ctx);
        if (!ksk) fail("null argument");
        KeyWrite kw(ctx);
        require_width32(ctx);
        require_ks_shape32(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->ksk_len()) fail("keyswitching key has %zu words, expected %zu", len, ctx->ksk_len());
        ctx->ksk32_ready = ctx->ksk32_planes_ready = false;
        ctx->ksk32.reserve(len * sizeof(uint32_t));
        check(hipMemcpyAsync(ctx->ksk32.ptr, ksk, len * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream),
              "upload u32 ksk");
        if (ks32_use_mfma(ctx)) {  // four int8 byte planes, once per key
            ctx->ksk32_planes.reserve(4 * ks_mfma_rows((int)ctx->big_dim(), (int)ctx->p.ks_level) *
                                      ks_mfma_cols((int)ctx->n()));
            check(launch_ksk32_repack((const uint32_t *)ctx->ksk32.ptr, (int8_t *)ctx->ksk32_planes.ptr,
                                      (int)ctx->big_dim(), (int)ctx->p.ks_level, (int)ctx->n(), ctx->stream),
                  "u32 ksk repack");
        }
        check(hipStreamSynchronize(ctx->stream), "u32 ksk upload sync");
        ctx->ksk32_planes_ready = ks32_use_mfma(ctx);
        ctx->ksk32_ready = true;
    });
}

int tfhe_mi355_programmable_bootstrap_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *lwe_out,
                                          const uint32_t *luts, size_t lut_count, const uint32_t *lut_indexes,
                                          size_t count) {
    return guarded([&] { pbs32_host(ctx, lwe_in, lwe_out, luts, lut_count, lut_indexes, count, false); });
}

int tfhe_mi355_blind_rotate_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *glwe_out,
                                const uint32_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count) {
    return guarded([&] { pbs32_host(ctx, lwe_in, glwe_out, luts, lut_count, lut_indexes, count, true); });
}

int tfhe_mi355_programmable_bootstrap_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        require_single32(ctx);
        if (!bytes) fail("null argument");
        *bytes = pbs32_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_blind_rotate_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return tfhe_mi355_programmable_bootstrap_u32_scratch(ctx, count, bytes);
}

int tfhe_mi355_programmable_bootstrap_u32_async(TfheMi355Context *ctx, const uint32_t *d_in, uint32_t *d_out,
                                                const uint32_t *d_luts, size_t lut_count, const uint32_t *d_idx,
                                                size_t count, void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        require_single32(ctx);
        if ((!d_in && count) || (!d_out && count) || !d_luts) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_scratch(d_scratch ? scratch_bytes : 0, pbs32_scratch_bytes(ctx, count));
        launch_pbs32_dev(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, (hipStream_t)stream, false);
    });
}

int tfhe_mi355_blind_rotate_u32_async(TfheMi355Context *ctx, const uint32_t *d_in, uint32_t *d_glwe_out,
                                      const uint32_t *d_luts, size_t lut_count, const uint32_t *d_idx, size_t count,
                                      void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        require_single32(ctx);
        if ((!d_in && count) || (!d_glwe_out && count) || !d_luts) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        require_scratch(d_scratch ? scratch_bytes : 0, pbs32_scratch_bytes(ctx, count));
        launch_pbs32_dev(ctx, d_in, d_glwe_out, d_luts, lut_count, d_idx, count, (hipStream_t)stream, true);
    });
}

int tfhe_mi355_keyswitch_u32(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *lwe_out, size_t count) {
    return guarded([&] {
        require_single32(ctx);
        if ((!lwe_in && count) || (!lwe_out && count)) fail("null argument");
        if (count == 0) return;
        require_ksk32(ctx);
        const size_t wi = ctx->big_dim() + 1, wo = ctx->n() + 1;
        const size_t sb = ks32_scratch_bytes(ctx, count);
        HostCall32 h(ctx, align256(count * wi * 4), count * wo * 4, sb);
        const uint32_t *d_in = h.up(lwe_in, count * wi);
        launch_ks32_dev(ctx, d_in, h.out(), count, h.scratch(), sb, ctx->stream);
        h.down(lwe_out, count * wo);
    });
}

int tfhe_mi355_keyswitch_u32_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        require_single32(ctx);
        if (!bytes) fail("null argument");
        *bytes = ks32_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_keyswitch_u32_async(TfheMi355Context *ctx, const uint32_t *d_in, uint32_t *d_out, size_t count,
                                   void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        require_single32(ctx);
        if ((!d_in && count) || (!d_out && count)) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_ks32_dev(ctx, d_in, d_out, count, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_boolean_gates(TfheMi355Context *ctx, const uint8_t *ops, const uint32_t *lhs, const uint32_t *rhs,
                             uint32_t *out, size_t count, int pbs_order) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if ((!ops || !lhs || !rhs || !out) && count) fail("null argument");
        if (count == 0) return;
        for (size_t i = 0; i < count; i++)
            if (ops[i] > TFHE_MI355_GATE_XNOR) fail("ops[%zu] = %u is not a gate opcode (0..5)", i, (unsigned)ops[i]);
        require_fbsk32(ctx);
        require_ksk32(ctx);
        const Gates32Layout l = gates32_layout(ctx, count, pbs_order);
        const size_t words = count * l.in_words;
        HostCall32 h(ctx, 2 * align256(words * 4) + align256(count), words * 4, l.total());
        const uint32_t *d_lhs = h.up(lhs, words);
        const uint32_t *d_rhs = h.up(rhs, words);
        const uint8_t *d_ops = h.up(ops, count);
        launch_gates32_dev(ctx, d_ops, d_lhs, d_rhs, h.out(), count, pbs_order, h.scratch(), l.total(), ctx->stream);
        h.down(out, words);
    });
}

int tfhe_mi355_boolean_gates_scratch(TfheMi355Context *ctx, size_t count, int pbs_order, size_t *bytes) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if (!bytes) fail("null argument");
        *bytes = count ? gates32_layout(ctx, count, pbs_order).total() : 0;
    });
}

int tfhe_mi355_boolean_gates_async(TfheMi355Context *ctx, const uint8_t *d_ops, const uint32_t *d_lhs,
                                   const uint32_t *d_rhs, uint32_t *d_out, size_t count, int pbs_order,
                                   void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if ((!d_ops || !d_lhs || !d_rhs || !d_out) && count) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_gates32_dev(ctx, d_ops, d_lhs, d_rhs, d_out, count, pbs_order, d_scratch, scratch_bytes,
                           (hipStream_t)stream);
    });
}

int tfhe_mi355_boolean_mux(TfheMi355Context *ctx, const uint32_t *cond, const uint32_t *then_ct,
                           const uint32_t *else_ct, uint32_t *out, size_t count, int pbs_order) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if ((!cond || !then_ct || !else_ct || !out) && count) fail("null argument");
        if (count == 0) return;
        require_fbsk32(ctx);
        require_ksk32(ctx);
        const Mux32Layout l = mux32_layout(ctx, count, pbs_order);
        const size_t words = count * l.in_words;
        HostCall32 h(ctx, 3 * align256(words * 4), words * 4, l.total());
        const uint32_t *d_c = h.up(cond, words);
        const uint32_t *d_t = h.up(then_ct, words);
        const uint32_t *d_e = h.up(else_ct, words);
        launch_mux32_dev(ctx, d_c, d_t, d_e, h.out(), count, pbs_order, h.scratch(), l.total(), ctx->stream);
        h.down(out, words);
    });
}

int tfhe_mi355_boolean_mux_scratch(TfheMi355Context *ctx, size_t count, int pbs_order, size_t *bytes) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if (!bytes) fail("null argument");
        *bytes = count ? mux32_layout(ctx, count, pbs_order).total() : 0;
    });
}

int tfhe_mi355_boolean_mux_async(TfheMi355Context *ctx, const uint32_t *d_cond, const uint32_t *d_then,
                                 const uint32_t *d_else, uint32_t *d_out, size_t count, int pbs_order,
                                 void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        require_single32(ctx);
        require_order(pbs_order);
        if ((!d_cond || !d_then || !d_else || !d_out) && count) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_mux32_dev(ctx, d_cond, d_then, d_else, d_out, count, pbs_order, d_scratch, scratch_bytes,
                         (hipStream_t)stream);
    });
}

int tfhe_mi355_boolean_not_async(TfheMi355Context *ctx, const uint32_t *d_in, uint32_t *d_out, size_t words,
                                 void *stream) {
    return guarded([&] {
        require_single32(ctx);
        if ((!d_in || !d_out) && words) fail("null argument");
        check(hipSetDevice(ctx->device), "hipSetDevice");
        TimedLaunch tl(ctx->timer_or_null(), "boolean_ops", (hipStream_t)stream);
        check(launch_bool_negate(d_in, d_out, words, (hipStream_t)stream), "boolean not");
    });
}

int tfhe_mi355_debug_torus32_from_fraction(int device, const double *fr, uint32_t *acc_inout, uint32_t *set_out,
                                           size_t n) {
    return guarded([&] {
        if ((!fr || !acc_inout || !set_out) && n) fail("null argument");
        if (n == 0) return;
        check(hipSetDevice(device), "hipSetDevice");
        DeviceBuffer d_fr, d_acc, d_set;
        d_fr.reserve(n * sizeof(double));
        d_acc.reserve(n * sizeof(uint32_t));
        d_set.reserve(n * sizeof(uint32_t));
        check(hipMemcpy(d_fr.ptr, fr, n * sizeof(double), hipMemcpyHostToDevice), "H2D fr");
        check(hipMemcpy(d_acc.ptr, acc_inout, n * sizeof(uint32_t), hipMemcpyHostToDevice), "H2D acc");
        check(launch_torus32_from_fraction((const double *)d_fr.ptr, (uint32_t *)d_acc.ptr, (uint32_t *)d_set.ptr, n,
                                           nullptr),
              "torus32 conversion");
        check(hipMemcpy(acc_inout, d_acc.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H acc");
        check(hipMemcpy(set_out, d_set.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H set");
    });
}

int tfhe_mi355_debug_keyswitch_u32(TfheMi355Context *ctx, const uint32_t *ksk, size_t in_dim, size_t out_dim,
                                   uint32_t base_log, uint32_t level, int arm, const uint32_t *lwe_in,
                                   uint32_t *lwe_out, size_t count) {
    return guarded([&] {
        require_single32(ctx);
        if (!ksk || ((!lwe_in || !lwe_out) && count)) fail("null argument");
        if (in_dim == 0 || out_dim == 0 || in_dim > (1u << 20) || out_dim > (1u << 20)) fail("dimension out of range");
        if (count > (1u << 20)) fail("count too large");
        if (base_log == 0 || level == 0 || base_log * level > 30) fail("ks decomposition: base_log*level <= 30");
        const bool can_mfma = ks32_mfma_supported((int)in_dim, (int)level, (int)base_log);
        const bool can_scalar = keyswitch32_scalar_supported((int)base_log, (int)level);
        if (arm < 0 || arm > 2) fail("arm must be 0 (the engine's choice), 1 (integer) or 2 (int8 MFMA)");
        if (arm == 2 && !can_mfma) fail("the int8-MFMA keyswitch does not take this shape");
        if (arm == 1 && !can_scalar) fail("the integer keyswitch does not take this decomposition");
        if (!can_mfma && !can_scalar) fail("no 32-bit keyswitch kernel for this decomposition");
        const bool mfma = arm == 2 || (arm == 0 && can_mfma);
        if (count == 0) return;
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        const size_t klen = in_dim * level * (out_dim + 1);
        DeviceBuffer d_ksk, d_planes, d_in, d_out, d_scratch;
        d_ksk.reserve(klen * 4);
        d_in.reserve(count * (in_dim + 1) * 4);
        d_out.reserve(count * (out_dim + 1) * 4);
        check(hipMemcpyAsync(d_ksk.ptr, ksk, klen * 4, hipMemcpyHostToDevice, ctx->stream), "H2D ksk");
        check(hipMemcpyAsync(d_in.ptr, lwe_in, count * (in_dim + 1) * 4, hipMemcpyHostToDevice, ctx->stream), "H2D");
        Keyswitch32Launch a;
        a.lwe_in = (const uint32_t *)d_in.ptr;
        a.lwe_out = (uint32_t *)d_out.ptr;
        a.ksk = (const uint32_t *)d_ksk.ptr;
        a.in_dim = (int)in_dim;
        a.out_dim = (int)out_dim;
        a.base_log = (int)base_log;
        a.level = (int)level;
        a.count = (int)count;
        if (mfma) {
            d_planes.reserve(4 * ks_mfma_rows((int)in_dim, (int)level) * ks_mfma_cols((int)out_dim));
            d_scratch.reserve(ks32_mfma_scratch_bytes((int)in_dim, (int)level, (int)count));
            check(launch_ksk32_repack(a.ksk, (int8_t *)d_planes.ptr, a.in_dim, a.level, a.out_dim, ctx->stream),
                  "u32 ksk repack");
            TimedLaunch tl(ctx->timer_or_null(), "keyswitch32_mfma", ctx->stream);
            check(launch_keyswitch32_mfma(a, (const int8_t *)d_planes.ptr, d_scratch.ptr, ctx->stream),
                  "launch u32 mfma keyswitch");
        } else {
            TimedLaunch tl(ctx->timer_or_null(), "keyswitch32_integer", ctx->stream);
            check(launch_keyswitch32(a, ctx->stream), "launch u32 keyswitch");
        }
        check(hipMemcpyAsync(lwe_out, d_out.ptr, count * (out_dim + 1) * 4, hipMemcpyDeviceToHost, ctx->stream), "D2H");
        check(hipStreamSynchronize(ctx->stream), "u32 keyswitch sync");
    });
}

int tfhe_mi355_debug_pbs_u32_resident(TfheMi355Context *ctx, size_t *count) {
    return guarded([&] {
        require_single32(ctx);
        if (!count) fail("null argument");
        require_shape32(ctx);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        *count = (size_t)classic_pbs32_resident_blocks((int)ctx->N(), (int)ctx->k(), (int)ctx->p.pbs_level);
    });
}


}  // extern "C"

// ---- 128-bit torus (pbs_f128.hip; the reference's fft128 path) ----------------------------------------
namespace {

typedef unsigned __int128 u128w;

void require_single128(const TfheMi355Context *c) {
    if (!c) fail("null ctx");
    if (c->multi()) fail("128-bit-torus calls are not available on a multi-device context");
}
void require_width128(const TfheMi355Context *c) {
    if (c->has_u64_keys()) fail("the context holds 64-bit-torus keys: 128-bit calls need a context of their own");
    if (c->has_u32_keys()) fail("the context holds 32-bit-torus keys: 128-bit calls need a context of their own");
}
// every limit of the f128 kernel, named
void validate_shape128(const TfheMi355Parameters &p) {
    const uint32_t N = p.polynomial_size, k = p.glwe_dimension;
    if (N != 256 && N != 512 && N != 1024 && N != 2048)
        fail("128-bit-torus PBS: polynomial_size must be 256, 512, 1024 or 2048 (got %u)", N);
    if (k < 1 || k > 3) fail("128-bit-torus PBS: glwe_dimension must be 1, 2 or 3 (got %u)", k);
    if ((k + 1) * N > 4096) fail("128-bit-torus PBS: (k+1)*N must be <= 4096 (got %u)", (k + 1) * N);
    if (p.pbs_level < 1 || p.pbs_level > 4) fail("128-bit-torus PBS: pbs_level must be in [1, 4] (got %u)", p.pbs_level);
    if (p.pbs_base_log < 2 || p.pbs_base_log > 31)
        fail("128-bit-torus PBS: pbs_base_log must be in [2, 31] (got %u)", p.pbs_base_log);
    if (p.pbs_base_log * p.pbs_level >= 128)
        fail("128-bit-torus PBS: pbs_base_log*pbs_level must be < 128 (got %u x %u)", p.pbs_base_log, p.pbs_level);
    if (p.grouping_factor) fail("128-bit-torus PBS: no multi-bit variant (grouping_factor %u)", p.grouping_factor);
    if (p.lwe_dimension == 0) fail("lwe_dimension must be > 0");
    if (!pbs_f128_supported((int)N, (int)k)) fail("no 128-bit-torus PBS kernel for N=%u k=%u", N, k);
}
void require_modulus128(uint32_t m) {
    if (m < 65 || m > 128) fail("128-bit-torus PBS: ciphertext_modulus_log must be in [65, 128] (got %u)", m);
}
void require_fbsk128(const TfheMi355Context *c) {
    require_width128(c);
    if (!c->fbsk128_ready) fail("128-bit-torus bootstrapping key not uploaded");
}
const double *twist128(const TfheMi355Context *c) { return reinterpret_cast<const double *>(c->tables128.ptr); }
const double *tw128(const TfheMi355Context *c) { return twist128(c) + 2 * c->N(); }

// the monomial degrees of the batch (one uint32_t per input word); everything else stays on chip
size_t pbs128_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return count ? align256(count * (c->n() + 1) * sizeof(uint32_t)) : 0;
}

void launch_pbs128_dev(TfheMi355Context *c, const void *d_in, void *d_out, const void *d_luts, size_t lut_count,
                       const uint32_t *d_idx, size_t count, uint32_t modulus_log, void *scratch, size_t scratch_bytes,
                       hipStream_t s, bool glwe_out) {
    require_modulus128(modulus_log);
    if (count == 0) return;
    require_fbsk128(c);
    require_scratch(scratch ? scratch_bytes : 0, pbs128_scratch_bytes(c, count));
    if (lut_count == 0) fail("lut_count must be >= 1");
    if (lut_count > 0xffffffffu) fail("lut_count too large");
    if (count > 0x7fffffff) fail("batch too large");
    PbsF128Launch a;
    a.lwe_in = reinterpret_cast<const u128w *>(d_in);
    a.lwe_out = reinterpret_cast<u128w *>(d_out);
    a.luts = reinterpret_cast<const u128w *>(d_luts);
    a.lut_indexes = d_idx;
    a.lut_count = (uint32_t)lut_count;
    a.fbsk = reinterpret_cast<const double *>(c->fbsk128.ptr);
    a.twist = twist128(c);
    a.tw = tw128(c);
    a.degrees = reinterpret_cast<uint32_t *>(scratch);
    a.n = (int)c->n();
    a.base_log = (int)c->p.pbs_base_log;
    a.level = (int)c->p.pbs_level;
    a.modulus_log = (int)modulus_log;
    a.count = (int)count;
    a.glwe_out = glwe_out;
    TimedLaunch tl(c->timer_or_null(), "pbs_f128_kernel", s);
    check(launch_pbs_f128((int)c->N(), (int)c->k(), a, s), "launch u128 pbs");
}

void pbs128_host(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *out, const uint64_t *luts, size_t lut_count,
                 const uint32_t *lut_indexes, size_t count, uint32_t modulus_log, bool glwe_out) {
    require_single128(ctx);
    require_modulus128(modulus_log);
    if ((!lwe_in && count) || (!out && count) || !luts) fail("null argument");
    if (count == 0) return;
    require_fbsk128(ctx);
    if (lut_count == 0) fail("lut_count must be >= 1");
    validate_lut_indexes(lut_indexes, count, lut_count);
    const size_t wi = ctx->n() + 1, wo = glwe_out ? ctx->glwe_len() : ctx->big_dim() + 1;
    const size_t in_b = align256(count * wi * 16), lut_b = align256(lut_count * ctx->glwe_len() * 16);
    std::lock_guard<std::mutex> g(ctx->mu);
    check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->lanes[0].d_in.reserve(in_b + lut_b + align256(count * 4));
    ctx->lanes[0].d_out.reserve(std::max<size_t>(count * wo * 16, 256));
    const size_t sb = pbs128_scratch_bytes(ctx, count);
    ctx->io_tmp.reserve(sb);
    char *d = reinterpret_cast<char *>(ctx->lanes[0].d_in.ptr);
    check(hipMemcpyAsync(d, lwe_in, count * wi * 16, hipMemcpyHostToDevice, ctx->stream), "H2D");
    check(hipMemcpyAsync(d + in_b, luts, lut_count * ctx->glwe_len() * 16, hipMemcpyHostToDevice, ctx->stream), "H2D");
    const uint32_t *d_idx = nullptr;
    if (lut_indexes) {
        check(hipMemcpyAsync(d + in_b + lut_b, lut_indexes, count * 4, hipMemcpyHostToDevice, ctx->stream), "H2D");
        d_idx = reinterpret_cast<const uint32_t *>(d + in_b + lut_b);
    }
    launch_pbs128_dev(ctx, d, ctx->lanes[0].d_out.ptr, d + in_b, lut_count, d_idx, count, modulus_log,
                      ctx->io_tmp.ptr, sb, ctx->stream, glwe_out);
    check(hipMemcpyAsync(out, ctx->lanes[0].d_out.ptr, count * wo * 16, hipMemcpyDeviceToHost, ctx->stream), "D2H");
    check(hipStreamSynchronize(ctx->stream), "u128 call sync");
}

void pbs128_async(TfheMi355Context *ctx, const void *d_in, void *d_out, const void *d_luts, size_t lut_count,
                  const uint32_t *d_idx, size_t count, uint32_t modulus_log, void *d_scratch, size_t scratch_bytes,
                  void *stream, bool glwe_out) {
    require_single128(ctx);
    if ((!d_in && count) || (!d_out && count) || !d_luts) fail("null argument");
    check(hipSetDevice(ctx->device), "hipSetDevice");
    launch_pbs128_dev(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, modulus_log, d_scratch, scratch_bytes,
                      (hipStream_t)stream, glwe_out);
}

}  // namespace

extern "C" {

int tfhe_mi355_context_create_u128(const TfheMi355Parameters *params, int device, TfheMi355Context **out_ctx) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!params) fail("null params");
        validate_shape128(*params);
        *out_ctx = create_single(*params, device);
        (*out_ctx)->for_u128 = true;
    });
}

int tfhe_mi355_bootstrap_key_upload_u128(TfheMi355Context *ctx, const uint64_t *bsk, size_t len) {
    return guarded([&] {
        require_single128(ctx);
        if (!bsk) fail("null argument");
        KeyWrite kw(ctx);
        require_width128(ctx);
        validate_shape128(ctx->p);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        if (len != ctx->std_bsk_len())
            fail("bootstrapping key has %zu u128 words, expected %zu", len, ctx->std_bsk_len());
        ctx->fbsk128_ready = false;
        const size_t N = ctx->N(), M = N / 2;
        std::vector<double> tab(4 * M + 4 * (M / 2));
        fft128_host_tables((int)N, tab.data(), tab.data() + 4 * M);
        ctx->tables128.reserve(tab.size() * sizeof(double));
        check(hipMemcpyAsync(ctx->tables128.ptr, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice,
                             ctx->stream),
              "upload f128 tables");
        ctx->std_staging.reserve(len * 16);
        check(hipMemcpyAsync(ctx->std_staging.ptr, bsk, len * 16, hipMemcpyHostToDevice, ctx->stream),
              "upload u128 bsk");
        ctx->fbsk128.reserve(len / N * 4 * M * sizeof(double));
        check(launch_bsk128_to_fourier((int)N, ctx->std_staging.ptr, (double *)ctx->fbsk128.ptr, len / N,
                                       twist128(ctx), tw128(ctx), ctx->stream),
              "u128 bsk conversion");
        check(hipStreamSynchronize(ctx->stream), "u128 bsk conversion sync");
        ctx->std_staging.release();
        ctx->fbsk128_ready = true;
    });
}

int tfhe_mi355_programmable_bootstrap_u128(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *lwe_out,
                                           const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes,
                                           size_t count, uint32_t ciphertext_modulus_log) {
    return guarded(
        [&] { pbs128_host(ctx, lwe_in, lwe_out, luts, lut_count, lut_indexes, count, ciphertext_modulus_log, false); });
}

int tfhe_mi355_blind_rotate_u128(TfheMi355Context *ctx, const uint64_t *lwe_in, uint64_t *glwe_out,
                                 const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count,
                                 uint32_t ciphertext_modulus_log) {
    return guarded(
        [&] { pbs128_host(ctx, lwe_in, glwe_out, luts, lut_count, lut_indexes, count, ciphertext_modulus_log, true); });
}

int tfhe_mi355_programmable_bootstrap_u128_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return guarded([&] {
        require_single128(ctx);
        if (!bytes) fail("null argument");
        *bytes = pbs128_scratch_bytes(ctx, count);
    });
}

int tfhe_mi355_blind_rotate_u128_scratch(TfheMi355Context *ctx, size_t count, size_t *bytes) {
    return tfhe_mi355_programmable_bootstrap_u128_scratch(ctx, count, bytes);
}

int tfhe_mi355_programmable_bootstrap_u128_async(TfheMi355Context *ctx, const uint64_t *d_in, uint64_t *d_out,
                                                 const uint64_t *d_luts, size_t lut_count, const uint32_t *d_idx,
                                                 size_t count, uint32_t ciphertext_modulus_log, void *d_scratch,
                                                 size_t scratch_bytes, void *stream) {
    return guarded([&] {
        pbs128_async(ctx, d_in, d_out, d_luts, lut_count, d_idx, count, ciphertext_modulus_log, d_scratch,
                     scratch_bytes, stream, false);
    });
}

int tfhe_mi355_blind_rotate_u128_async(TfheMi355Context *ctx, const uint64_t *d_in, uint64_t *d_glwe_out,
                                       const uint64_t *d_luts, size_t lut_count, const uint32_t *d_idx, size_t count,
                                       uint32_t ciphertext_modulus_log, void *d_scratch, size_t scratch_bytes,
                                       void *stream) {
    return guarded([&] {
        pbs128_async(ctx, d_in, d_glwe_out, d_luts, lut_count, d_idx, count, ciphertext_modulus_log, d_scratch,
                     scratch_bytes, stream, true);
    });
}

int tfhe_mi355_debug_fft128_tables(uint32_t polynomial_size, double *twist, double *twiddles) {
    return guarded([&] {
        if (!twist || !twiddles) fail("null argument");
        const uint32_t N = polynomial_size;
        if (N != 256 && N != 512 && N != 1024 && N != 2048)
            fail("128-bit-torus PBS: polynomial_size must be 256, 512, 1024 or 2048 (got %u)", N);
        fft128_host_tables((int)N, twist, twiddles);
    });
}

int tfhe_mi355_debug_torus128_from_f128(int device, const double *hi, const double *lo, const uint64_t *acc,
                                        uint64_t *out, size_t count) {
    return guarded([&] {
        if ((!hi || !lo || !out) && count) fail("null argument");
        if (count == 0) return;
        check(hipSetDevice(device), "hipSetDevice");
        DeviceBuffer d_hi, d_lo, d_acc, d_out;
        d_hi.reserve(count * sizeof(double));
        d_lo.reserve(count * sizeof(double));
        d_out.reserve(count * 16);
        check(hipMemcpy(d_hi.ptr, hi, count * sizeof(double), hipMemcpyHostToDevice), "H2D hi");
        check(hipMemcpy(d_lo.ptr, lo, count * sizeof(double), hipMemcpyHostToDevice), "H2D lo");
        if (acc) {
            d_acc.reserve(count * 16);
            check(hipMemcpy(d_acc.ptr, acc, count * 16, hipMemcpyHostToDevice), "H2D acc");
        }
        check(launch_torus128_from_f128((const double *)d_hi.ptr, (const double *)d_lo.ptr, acc ? d_acc.ptr : nullptr,
                                        d_out.ptr, count, nullptr),
              "torus128 conversion");
        check(hipMemcpy(out, d_out.ptr, count * 16, hipMemcpyDeviceToHost), "D2H out");
    });
}

int tfhe_mi355_debug_pbs_u128_resident(TfheMi355Context *ctx, size_t *count) {
    return guarded([&] {
        require_single128(ctx);
        if (!count) fail("null argument");
        validate_shape128(ctx->p);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        *count = (size_t)pbs_f128_resident_blocks((int)ctx->N(), (int)ctx->k());
    });
}

}  // extern "C"
