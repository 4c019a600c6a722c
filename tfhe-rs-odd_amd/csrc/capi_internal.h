// capi_internal.h -- what the capi*.cpp files share: the host-side runtime behind include/tfhe_mi355.h is
// split by subsystem (capi.cpp: errors, contexts, key transactions and key uploads; capi_pbs.cpp: the kernel-form
// policy, scratch sizes, launchers and entry points of the u64 PBS and keyswitch family; capi_pipeline.cpp: the
// host-pointer pipeline and the request coalescer; capi_gadget.cpp: packing keyswitch, products, GGSW nodes and
// vertical packing; capi_wopbs.cpp: the bootstrapped half of WoP-PBS; capi_multi.cpp: multi-device contexts;
// capi_u32.cpp, capi_u128.cpp: the other torus widths; capi_ingress.cpp: compressed ciphertext sources).  What
// crosses a subsystem's boundary is declared here, in namespace tfhe_mi355::capi; what one file alone uses stays
// in its anonymous namespace.
// Included by those files only, never by a .hip file or by engine.h.
#pragma once

#include <hip/hip_runtime.h>

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

struct RcclComms;  // communicator over a multi-device context's distinct devices (capi_multi.cpp)

namespace tfhe_mi355 {
namespace capi {

struct Failure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(const char *fmt, ...);
void check(hipError_t e, const char *what);

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
bool env_flag(const char *name);

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

inline bool is_pow2(uint32_t x) { return x && !(x & (x - 1)); }

// one small host-pointer call waiting to be coalesced into a batch (capi_pipeline.cpp, "request coalescing")
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

}  // namespace capi
}  // namespace tfhe_mi355

// The ABI's opaque types are declared at global scope by include/tfhe_mi355.h; their members are the engine's
// (engine.h) and the types above, which every capi*.cpp file names unqualified as well.
using namespace tfhe_mi355;
using namespace tfhe_mi355::capi;

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
    // Every entry point of a multi-device context dispatches to them (capi_multi.cpp).
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
    // compressed ciphertext ingress (capi_ingress.cpp): what a host-pointer call sends up once (a compact
    // container, the AES tables of a list's seed), and AES tables whose Te0 and S-box the kernels read
    DeviceBuffer io_src, aes_base;
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
        DeviceBuffer d_src;  // a chunk's slice of a compressed source (capi_ingress.cpp)
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
    // 32-bit torus keys (the boolean module's; capi_u32.cpp).  The Fourier key of a u32
    // bootstrapping key lives in `fbsk` (same format); a context holds keys of one width only.
    DeviceBuffer ksk32, ksk32_planes;  // u32 keyswitching key and its four int8 byte planes
    DeviceBuffer lut_true32;           // the gates' accumulator: trivial GLWE, body all 1 << 29
    bool fbsk32_ready = false, ksk32_ready = false, ksk32_planes_ready = false;
    bool has_u32_keys() const { return fbsk32_ready || ksk32_ready; }
    // 128-bit torus (capi_u128.cpp): the Fourier key as four f64 planes per polynomial and
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

namespace tfhe_mi355 {
namespace capi {

// ---- key transactions (capi.cpp) ---------------------------------------------------------------
// A key write holds the context's mutex and keys_mu exclusively.  It is re-entrant per thread: a
// transaction (tfhe_mi355::begin_key_transaction, e.g. the serialized-key upload, which uploads the
// KSK, fills the Fourier buffer and marks it ready through three ABI calls) keeps both locks for its
// whole duration, and the nested calls on the same context from the same thread skip the locking.
// The thread's list of contexts under a write is one object of capi.cpp: the members are out of line.
struct KeyWrite {
    TfheMi355Context *c = nullptr;
    std::unique_lock<std::mutex> g;
    std::unique_lock<std::shared_mutex> k;
    explicit KeyWrite(TfheMi355Context *c_);
    KeyWrite(const KeyWrite &) = delete;
    KeyWrite &operator=(const KeyWrite &) = delete;
    ~KeyWrite();
};

// a coalesced batch reads the keys: it waits while an upload is pending (writer preference), then
// holds keys_mu shared for the batch
struct KeyRead {
    std::shared_lock<std::shared_mutex> k;
    explicit KeyRead(TfheMi355Context *c);
};

// ---- scratch layouts ---------------------------------------------------------------------------
// Every op whose device scratch has more than one region builds one layout struct from (context, shape, count):
// the *_scratch query returns its total(), the launcher takes its pointers from the same offsets.  A layout
// function walks a cursor over the regions, each rounded up to 256 bytes.
struct ScratchCursor {
    size_t off = 0;
    // the offset of the next region, of `bytes`
    size_t take(size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    }
};
// the named regions in front, then the last one at `rest`: where nested launchers share it (reused in stream
// order), they get `scratch_bytes - rest` of the caller's buffer
struct TailLayout {
    size_t rest = 0, rest_bytes = 0;
    size_t total() const { return rest + rest_bytes; }
};
template <class T = void>
T *scratch_at(void *scratch, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(scratch) + off);
}

// ---- host-pointer call through lane 0 (capi_u32.cpp, capi_u128.cpp) ---------------------------
// Under the context's mutex, inputs staged one after the other (256-byte aligned) into lane 0's device buffer,
// the kernels on the context's stream, the output copied back after them.  The caller says how much of each
// buffer to reserve (each at least `floor` bytes) and names its final synchronisation for the error text.
struct HostCall {
    TfheMi355Context *c;
    std::lock_guard<std::mutex> g;
    const char *sync_what;
    size_t in_off = 0;
    HostCall(TfheMi355Context *c_, size_t in_bytes, size_t out_bytes, size_t scratch_bytes, size_t floor,
             const char *sync_what_)
        : c(c_), g(c_->mu), sync_what(sync_what_) {
        check(hipSetDevice(c->device), "hipSetDevice");
        c->lanes[0].d_in.reserve(std::max(in_bytes, floor));
        c->lanes[0].d_out.reserve(std::max(out_bytes, floor));
        c->io_tmp.reserve(std::max(scratch_bytes, floor));
    }
    template <class T>
    const T *up(const T *host, size_t n) {
        if (!host || n == 0) return nullptr;
        char *d = reinterpret_cast<char *>(c->lanes[0].d_in.ptr) + in_off;
        check(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream), "H2D");
        in_off += align256(n * sizeof(T));
        return reinterpret_cast<const T *>(d);
    }
    template <class T = void>
    T *out() {
        return reinterpret_cast<T *>(c->lanes[0].d_out.ptr);
    }
    void *scratch() { return c->io_tmp.ptr; }
    void down(void *host, size_t bytes) {
        check(hipMemcpyAsync(host, out(), bytes, hipMemcpyDeviceToHost, c->stream), "D2H");
        check(hipStreamSynchronize(c->stream), sync_what);
    }
};

// ---- functions that cross files ------------------------------------------------------------------
// capi.cpp
void require_width64(const TfheMi355Context *c);
void require_width32(const TfheMi355Context *c);
void require_fbsk(TfheMi355Context *c);
void require_ksk(TfheMi355Context *c);
void validate_parameters(const TfheMi355Parameters &p);
TfheMi355Context *create_single(const TfheMi355Parameters &p, int device);
void abi(int rc);

// capi_pbs.cpp: the u64 PBS and keyswitch family
bool ks_mfma_disabled();  // TFHE_MI355_KS_NO_MFMA, read once
void require_scratch(size_t have, size_t need);
void validate_lut_indexes(const uint32_t *idx, size_t count, size_t lut_count);
bool is_large(const TfheMi355Context *c);
size_t large_chunk(const TfheMi355Context *c);
size_t quad_max(const TfheMi355Context *c);
size_t pbs_scratch_bytes(const TfheMi355Context *c, size_t count);
size_t ks_scratch_bytes(const TfheMi355Context *c, size_t count);
size_t ks_pbs_scratch_bytes(const TfheMi355Context *c, size_t count);
size_t pbs_ks_scratch_bytes(const TfheMi355Context *c, size_t count);
void repack_ksk(TfheMi355Context *c, hipStream_t s);
void launch_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                    size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                    hipStream_t s, bool glwe_out = false);
void launch_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, size_t count, void *scratch,
                   size_t scratch_bytes, hipStream_t s);
void launch_ks_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s);
void launch_pbs_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s);
// adapters of launch_pbs_dev and launch_ks_dev to ChunkLaunch (below)
void chunk_pbs(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *l, size_t lc, const uint32_t *x,
               size_t n, void *sc, size_t sb, hipStream_t s);
void chunk_ks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
              size_t n, void *sc, size_t sb, hipStream_t s);

// capi_pipeline.cpp: the host-pointer pipeline and the request coalescer
using ChunkLaunch = void (*)(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                             size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch,
                             size_t scratch_bytes, hipStream_t s);
using ScratchSize = size_t (*)(const TfheMi355Context *c, size_t count);
// a chunk's input rows written on the device instead of copied up: stage() enqueues what rows [first,
// first + count) need on the lane's copy stream, expand() the kernels that fill L.d_in on the kernel stream
// (after the lane's copies, before the chunk's launch)
struct ChunkSource {
    std::function<void(TfheMi355Context::Lane &L, size_t first, size_t count)> stage;
    std::function<void(TfheMi355Context::Lane &L, size_t first, size_t count, hipStream_t s)> expand;
};
void run_host_pipeline(TfheMi355Context *c, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                       const uint64_t *luts, size_t lut_words, size_t lut_count, const uint32_t *idx, size_t count,
                       ChunkLaunch launch, ScratchSize scratch_size, const ChunkSource *from = nullptr);
bool coalescible(size_t count);
void coalesced_call(TfheMi355Context *c, CoalescedOp op, CoalescedReq &r);

// capi_multi.cpp
enum class KeyPart { Fourier, Ksk };
TfheMi355Context *primary(TfheMi355Context *c);
TfheMi355Context *pick_shard(TfheMi355Context *m);
std::vector<std::unique_ptr<KeyWrite>> key_write_all(TfheMi355Context *c);
void set_ready_all(TfheMi355Context *m, KeyPart part, bool ready);
void split_rows(TfheMi355Context *m, size_t count, const std::function<int(TfheMi355Context *, size_t, size_t)> &f);
void multi_key_upload(TfheMi355Context *m, KeyPart part, const std::function<int(TfheMi355Context *)> &first);
void destroy_multi(TfheMi355Context *m);

// capi_gadget.cpp: the gadget layer
struct VpShape {
    uint32_t nt, nr;
};
VpShape vp_shape(const TfheMi355Context *c, uint32_t nbits, size_t npoly);
size_t vp_scratch_bytes(const TfheMi355Context *c, size_t npoly, size_t nout, size_t count);
size_t ggsw_std_words(const TfheMi355Context *c, uint32_t level);
size_t ggsw_fourier_bytes(const TfheMi355Context *c, uint32_t level);
void require_ggsw_shape(const TfheMi355Context *c, uint32_t base_log, uint32_t level);
void ggsw_list_to_fourier_dev(TfheMi355Context *c, const uint64_t *d_std, double2 *d_fourier, size_t ggsw_count,
                              uint32_t level, hipStream_t s);
void launch_vertical_packing_dev(TfheMi355Context *c, const double2 *d_fggsw, uint32_t base_log, uint32_t level,
                                 uint32_t nbits, const uint64_t *d_luts, size_t lut_count, size_t nout, size_t npoly,
                                 const uint32_t *d_lut_idx, size_t count, uint64_t *d_lwe_out, void *scratch,
                                 size_t scratch_bytes, hipStream_t s);

// capi_wopbs.cpp, WoP-PBS: host-pointer form of a call whose items go in chunks through device buffers of the call's
// own, on the context's stream; f(d_in, d_out, d_idx, n, d_scratch, scratch_bytes, stream) launches one chunk
constexpr size_t kWopChunkRows = 4096;  // PBS rows per chunk of the host-pointer forms
void host_wop_call(TfheMi355Context *ctx, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                   const uint32_t *idx, size_t count, size_t chunk, const std::function<size_t(size_t)> &scratch_bytes,
                   const std::function<void(const uint64_t *, uint64_t *, const uint32_t *, size_t, void *, size_t,
                                            hipStream_t)> &f);

}  // namespace capi
}  // namespace tfhe_mi355
