// capi.cpp -- C ABI implementation (include/tfhe_mi355.h).  Host-side runtime of the engine:
// context = device + parameter set + key material + FFT tables, guarded by a mutex so that
// concurrent callers (the reference's rayon workers, shortint/engine/mod.rs:23-25) can share one
// key.  Error convention: 0/1 return + thread-local message (tfhe/src/c_api/utils.rs:3-73).
// This file: errors, contexts, key transactions and the bootstrap-key and keyswitch-key uploads; the other
// subsystems are the capi_*.cpp files (capi_internal.h).
#include "capi_internal.h"

namespace {
// the contexts under a key write of this thread (KeyWrite, KeyRead): one list for the whole library
thread_local std::vector<const TfheMi355Context *> tl_key_writes;

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

hipError_t convert_bsk(TfheMi355Context *c, const uint64_t *d_std, size_t npoly, hipStream_t s) {
    if (large_pbs_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level))
        return launch_large_bsk_to_fourier(d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
    return launch_bsk_to_fourier((int)c->N(), d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
}

// The device-pointer key uploads wait for their stream before they return, which a capturing stream cannot
// do (the wait fails and invalidates the caller's capture): they refuse first, before anything is locked,
// marked not ready or enqueued.
void refuse_capture(const char *entry, hipStream_t s) {
    if (stream_is_capturing(s))
        fail("%s cannot run under stream capture (the stream is being captured, or its capture state cannot be "
             "read): the call waits for its stream, so it belongs outside the graph", entry);
}

// AES tables of a compression seed on the device (a few KiB, one per call)
void upload_aes_tables(TfheMi355Context *c, uint64_t seed_lo, uint64_t seed_hi, DeviceBuffer &d) {
    std::vector<unsigned char> host(aes_tables_bytes());
    aes_tables_build(seed_lo, seed_hi, host.data());
    d.reserve(host.size());
    check(hipMemcpyAsync(d.ptr, host.data(), host.size(), hipMemcpyHostToDevice, c->stream), "upload aes tables");
    check(hipStreamSynchronize(c->stream), "aes tables sync");
}
}  // namespace

namespace tfhe_mi355 {
namespace capi {

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

bool env_flag(const char *name) {
    const char *e = std::getenv(name);
    return e && *e && std::strcmp(e, "0") != 0;
}

KeyWrite::KeyWrite(TfheMi355Context *c_) {
    if (std::find(tl_key_writes.begin(), tl_key_writes.end(), c_) != tl_key_writes.end()) return;
    c = c_;
    c->key_writers.fetch_add(1, std::memory_order_acq_rel);
    g = std::unique_lock<std::mutex>(c->mu);
    k = std::unique_lock<std::shared_mutex>(c->keys_mu);
    tl_key_writes.push_back(c);
}
KeyWrite::~KeyWrite() {
    if (!c) return;
    tl_key_writes.erase(std::find(tl_key_writes.begin(), tl_key_writes.end(), c));
    k.unlock();
    g.unlock();
    c->key_writers.fetch_sub(1, std::memory_order_acq_rel);
}
KeyRead::KeyRead(TfheMi355Context *c) {
    if (std::find(tl_key_writes.begin(), tl_key_writes.end(), c) != tl_key_writes.end()) return;
    while (c->key_writers.load(std::memory_order_acquire) > 0)
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    k = std::shared_lock<std::shared_mutex>(c->keys_mu);
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

// an ABI call made from inside another one: its failure text becomes ours
void abi(int rc) {
    if (rc != TFHE_MI355_OK) fail("%s", tfhe_mi355_last_error());
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
        {  // AES tables for the ingress kernels (their Te0 and S-box; each call brings its own seeds)
            std::vector<unsigned char> host(aes_tables_bytes());
            aes_tables_build(0, 0, host.data());
            c->aes_base.reserve(host.size());
            check(hipMemcpy(c->aes_base.ptr, host.data(), host.size(), hipMemcpyHostToDevice), "upload aes tables");
        }
    } catch (...) {
        tfhe_mi355_context_destroy(c);
        throw;
    }
    return c;
}

}  // namespace capi
}  // namespace tfhe_mi355

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

int tfhe_mi355_context_destroy(TfheMi355Context *ctx) {
    return guarded([&] {
        if (!ctx) return;
        if (ctx->owner) fail("this context belongs to a multi-device context: destroy that one");
        if (ctx->multi()) return destroy_multi(ctx);
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
        refuse_capture("tfhe_mi355_bootstrap_key_convert_async", (hipStream_t)stream);
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
        refuse_capture("tfhe_mi355_keyswitch_key_upload_async", (hipStream_t)stream);
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

int tfhe_mi355_debug_pbs_resident(TfheMi355Context *ctx, size_t *count) {
    return guarded([&] {
        ctx = primary(ctx);  // every shard has the same shape; the first device answers
        if (!ctx || !count) fail("null argument");
        require_width64(ctx);
        const TfheMi355Parameters &p = ctx->p;
        if (p.grouping_factor || is_large(ctx) ||
            !classic_pbs_supported((int)p.polynomial_size, (int)p.glwe_dimension, (int)p.pbs_level))
            fail("no classic 64-bit-torus PBS kernel for N=%u k=%u pbs_level=%u grouping_factor=%u", p.polynomial_size,
                 p.glwe_dimension, p.pbs_level, p.grouping_factor);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        *count = (size_t)classic_pbs_resident_blocks((int)ctx->N(), (int)ctx->k(), (int)p.pbs_level);
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
