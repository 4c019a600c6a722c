// capi.cpp -- C ABI implementation (include/tfhe_mi355.h).  Host-side runtime of the engine:
// context = device + parameter set + key material + FFT tables, guarded by a mutex so that
// concurrent callers (the reference's rayon workers, shortint/engine/mod.rs:23-25) can share one
// key.  Error convention: 0/1 return + thread-local message (tfhe/src/c_api/utils.rs:3-73).
// This file: contexts, key transactions and uploads, the kernel-form policy with its scratch sizes, the u64
// PBS and keyswitch launchers and entry points; the other subsystems are the capi_*.cpp files (capi_internal.h).
#include "capi_internal.h"

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

}  // namespace capi
}  // namespace tfhe_mi355

namespace {
// the contexts under a key write of this thread (KeyWrite, KeyRead): one list for the whole library
thread_local std::vector<const TfheMi355Context *> tl_key_writes;
}  // namespace

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

namespace {

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
}  // namespace

namespace tfhe_mi355::capi {
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
}  // namespace tfhe_mi355::capi

namespace {
hipError_t convert_bsk(TfheMi355Context *c, const uint64_t *d_std, size_t npoly, hipStream_t s) {
    if (large_pbs_supported((int)c->N(), (int)c->k(), (int)c->p.pbs_level))
        return launch_large_bsk_to_fourier(d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
    return launch_bsk_to_fourier((int)c->N(), d_std, (double2 *)c->fbsk.ptr, npoly, c->tables, s);
}
}  // namespace

// ---- scratch sizes -----------------------------------------------------------------------------
// Every launcher takes its device scratch explicitly: the _async entry points pass the caller's
// d_scratch (sized by the *_scratch queries), the host-pointer entry points a lane's own buffer.
namespace tfhe_mi355::capi {

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
}  // namespace tfhe_mi355::capi

namespace {
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
    return !ks_mfma_disabled() && ks_mfma_supported((int)c->big_dim(), (int)c->p.ks_level, (int)c->p.ks_base_log);
}

// KS -> PBS and PBS -> KS: the intermediate LWE rows (of `words`; the small ones for KS -> PBS, the big ones
// for PBS -> KS), then (reused in stream order) the KS digits or the PBS chunk scratch
TailLayout fused_layout(const TfheMi355Context *c, size_t words, size_t count) {
    TailLayout l;
    l.rest = align256(count * words * 8);  // the intermediate is at 0
    l.rest_bytes = std::max(ks_scratch_bytes(c, count), pbs_scratch_bytes(c, count));
    return l;
}
}  // namespace

namespace tfhe_mi355::capi {
bool ks_mfma_disabled() {
    static const bool disabled = env_flag("TFHE_MI355_KS_NO_MFMA");
    return disabled;
}

size_t ks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (!c->ksk_planes_ready && !ks_use_mfma(c)) return 0;
    return count ? ks_mfma_scratch_bytes((int)c->big_dim(), (int)c->p.ks_level, (int)count) : 0;
}

size_t ks_pbs_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return fused_layout(c, c->n() + 1, count).total();
}
size_t pbs_ks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return fused_layout(c, c->big_dim() + 1, count).total();
}

// The device-pointer key uploads wait for their stream before they return, which a capturing stream cannot
// do (the wait fails and invalidates the caller's capture): they refuse first, before anything is locked,
// marked not ready or enqueued.
void refuse_capture(const char *entry, hipStream_t s) {
    if (stream_is_capturing(s))
        fail("%s cannot run under stream capture (the stream is being captured, or its capture state cannot be "
             "read): the call waits for its stream, so it belongs outside the graph", entry);
}

void require_scratch(size_t have, size_t need) {
    if (have < need) fail("device scratch too small: %zu bytes given, %zu needed (see the *_scratch queries)", have, need);
}

// ---- launchers ---------------------------------------------------------------------------------

void launch_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                    size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                    hipStream_t s, bool glwe_out) {
    require_fbsk(c);
    if (lut_count == 0) fail("lut_count must be >= 1");
    if (lut_count > 0xffffffffu) fail("lut_count too large");
    if (count > 0x7fffffff) fail("batch too large");
    if (count == 0) return;
    // the fields that the classic, multi-bit and large launch arguments share
    auto common = [&](auto &a) {
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
    };
    if (c->p.grouping_factor && !is_large(c)) {
        MultiBitPbsLaunch a;
        common(a);
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
        common(a);
        a.wtop = c->tables.wtop;
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
    common(a);
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
        check(launch_zero_words(a.ticket, 1, s), "zero pbs ticket");  // a kernel: it replays from a graph
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
}  // namespace tfhe_mi355::capi

namespace {
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


// The packing key's decomposition (base, level) is part of the key, not of the parameter set, so
// this size is defined from the key's upload on (the scratch query fails before it); it follows
// from the decomposition and the MFMA eligibility alone, not from the repack having run.
bool pks_use_mfma(const TfheMi355Context *c) {
    return !ks_mfma_disabled() && c->pks_level &&
           ks_mfma_supported((int)c->big_dim(), (int)c->pks_level, (int)c->pks_base_log);
}
size_t pks_scratch_bytes(const TfheMi355Context *c, size_t count) {
    if (!pks_use_mfma(c) || count == 0) return 0;
    return ks_mfma_scratch_bytes((int)c->big_dim(), (int)c->pks_level, (int)count);
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
}  // namespace

namespace tfhe_mi355::capi {
// shortint KS -> PBS on device: scratch = [small LWE intermediate | KS digits or PBS chunk scratch]
void launch_ks_pbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s) {
    require_fbsk(c);
    require_ksk(c);
    if (count == 0) return;
    const TailLayout l = fused_layout(c, c->n() + 1, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    uint64_t *small = scratch_at<uint64_t>(scratch, 0);
    void *rest = scratch_at(scratch, l.rest);
    launch_ks_dev(c, d_in, small, count, rest, scratch_bytes - l.rest, s);
    launch_pbs_dev(c, small, d_out, d_luts, lut_count, d_idx, count, rest, scratch_bytes - l.rest, s);
}

// shortint PBS -> KS on device: scratch = [big LWE intermediate | PBS or KS scratch]
void launch_pbs_ks_dev(TfheMi355Context *c, const uint64_t *d_in, uint64_t *d_out, const uint64_t *d_luts,
                       size_t lut_count, const uint32_t *d_idx, size_t count, void *scratch, size_t scratch_bytes,
                       hipStream_t s) {
    require_fbsk(c);
    require_ksk(c);
    if (count == 0) return;
    const TailLayout l = fused_layout(c, c->big_dim() + 1, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    uint64_t *big = scratch_at<uint64_t>(scratch, 0);
    void *rest = scratch_at(scratch, l.rest);
    launch_pbs_dev(c, d_in, big, d_luts, lut_count, d_idx, count, rest, scratch_bytes - l.rest, s);
    launch_ks_dev(c, big, d_out, count, rest, scratch_bytes - l.rest, s);
}
}  // namespace tfhe_mi355::capi

namespace {
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
struct LweMultLayout : TailLayout {
    size_t packed;  // the rows are at 0
};
LweMultLayout lwe_mult_layout(const TfheMi355Context *c, size_t count) {
    ScratchCursor at;
    LweMultLayout l;
    at.take(2 * count * (c->big_dim() + 1) * 8);
    l.packed = at.take(2 * count * c->glwe_len() * 8);
    l.rest = at.off;
    l.rest_bytes = std::max(align256(pks_scratch_bytes(c, 2 * count)), glwe_mult_scratch(c, count));
    return l;
}
size_t lwe_mult_scratch(const TfheMi355Context *c, size_t count) { return lwe_mult_layout(c, count).total(); }

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
    const LweMultLayout l = lwe_mult_layout(c, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    uint64_t *rows = scratch_at<uint64_t>(scratch, 0);
    uint64_t *packed = scratch_at<uint64_t>(scratch, l.packed);
    void *p = scratch_at(scratch, l.rest);
    const size_t rest = scratch_bytes - l.rest;
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
}  // namespace

namespace tfhe_mi355::capi {
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

void ggsw_list_to_fourier_dev(TfheMi355Context *c, const uint64_t *d_std, double2 *d_fourier, size_t ggsw_count,
                              uint32_t level, hipStream_t s) {
    TimedLaunch tl(c->timer_or_null(), "ggsw_to_fourier", s);
    check(launch_bsk_to_fourier((int)c->N(), d_std, d_fourier, ggsw_count * ggsw_polys(c, level), c->tables, s),
          "launch GGSW list conversion");
}
}  // namespace tfhe_mi355::capi

namespace {
void validate_ggsw_indexes(const uint32_t *idx, size_t count, size_t ggsw_count) {
    if (!idx) {
        if (ggsw_count < count) fail("GGSW list has %zu ciphertexts for %zu items (no ggsw_indexes)", ggsw_count, count);
        return;
    }
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= ggsw_count) fail("ggsw_indexes[%zu] = %u out of range (ggsw_count %zu)", i, idx[i], ggsw_count);
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

// two ping-pong GLWE buffers per (item, output): the tree's first level leaves npoly/2 nodes, the next
// npoly/4; without a tree the first holds the rotation steps' accumulator
// (the first at 0, the second at `rest`)
TailLayout vp_layout(const TfheMi355Context *c, size_t npoly, size_t nout, size_t count) {
    const size_t a = std::max<size_t>(npoly / 2, 1), b = std::max<size_t>(npoly / 4, 1);
    TailLayout l;
    l.rest = align256(count * nout * a * c->glwe_len() * 8);
    l.rest_bytes = align256(count * nout * b * c->glwe_len() * 8);
    return l;
}

// TFHE_MI355_VP_STEPWISE=1: one launch per rotation step instead of the chain launch (A/B arm); read at
// every call, so that one process can run both arms
bool vp_stepwise() { return env_flag("TFHE_MI355_VP_STEPWISE"); }
}  // namespace

namespace tfhe_mi355::capi {
// vertical packing: log2(npoly) tree bits, then nbits - log2(npoly) rotation bits
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

size_t vp_scratch_bytes(const TfheMi355Context *c, size_t npoly, size_t nout, size_t count) {
    return vp_layout(c, npoly, nout, count).total();
}

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
    const TailLayout l = vp_layout(c, npoly, nout, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    const size_t glwe = c->glwe_len();
    uint64_t *buf[2] = {scratch_at<uint64_t>(scratch, 0), scratch_at<uint64_t>(scratch, l.rest)};
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
}  // namespace tfhe_mi355::capi

namespace {

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
struct ExtractBitsLayout : TailLayout {
    size_t shifted, pbs_out, ks_out, lut;  // the running input is at 0
};
ExtractBitsLayout extract_bits_layout(const TfheMi355Context *c, size_t count) {
    const size_t big = count * (c->big_dim() + 1) * 8, small = count * (c->n() + 1) * 8;
    ScratchCursor at;
    ExtractBitsLayout l;
    at.take(big);
    l.shifted = at.take(big);
    l.pbs_out = at.take(big);
    l.ks_out = at.take(small);
    l.lut = at.take(c->glwe_len() * 8);
    l.rest = at.off;
    l.rest_bytes = std::max<size_t>(std::max(ks_scratch_bytes(c, count), pbs_scratch_bytes(c, count)), 256);
    return l;
}
size_t extract_bits_scratch_bytes(const TfheMi355Context *c, size_t count) {
    return extract_bits_layout(c, count).total();
}
void launch_extract_bits_dev(TfheMi355Context *c, const uint64_t *d_in, uint32_t delta_log, uint32_t nbits,
                             uint64_t *d_out, size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_wop_shape(c);
    require_fbsk(c);
    require_ksk(c);
    validate_extract_bits(delta_log, nbits);
    if (count == 0) return;
    if (count > 0x7fffffffu / nbits) fail("count too large");
    const ExtractBitsLayout l = extract_bits_layout(c, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    const size_t bw = c->big_dim() + 1, sw = c->n() + 1;
    uint64_t *cur = scratch_at<uint64_t>(scratch, 0);
    uint64_t *shifted = scratch_at<uint64_t>(scratch, l.shifted);
    uint64_t *pbs_out = scratch_at<uint64_t>(scratch, l.pbs_out);
    uint64_t *ks_out = scratch_at<uint64_t>(scratch, l.ks_out);
    uint64_t *lut = scratch_at<uint64_t>(scratch, l.lut);
    void *rest = scratch_at(scratch, l.rest);
    const size_t rest_bytes = scratch_bytes - l.rest;
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
struct CbsLayout : TailLayout {
    size_t luts, idx, pbs_out;  // the shifted rows are at 0
};
CbsLayout cbs_layout(const TfheMi355Context *c, uint32_t level, size_t count) {
    const size_t rows = count * level;
    ScratchCursor at;
    CbsLayout l;
    at.take(rows * (c->n() + 1) * 8);
    l.luts = at.take((size_t)level * c->glwe_len() * 8);
    l.idx = at.take(rows * 4);
    l.pbs_out = at.take(rows * (c->big_dim() + 1) * 8);
    l.rest = at.off;
    l.rest_bytes = std::max<size_t>(std::max(pbs_scratch_bytes(c, rows), pfpks_scratch_bytes(c, rows)), 256);
    return l;
}
size_t cbs_scratch_bytes(const TfheMi355Context *c, uint32_t level, size_t count) {
    return cbs_layout(c, level, count).total();
}
void launch_cbs_dev(TfheMi355Context *c, const uint64_t *d_in, uint32_t delta_log, uint32_t base_log, uint32_t level,
                    uint64_t *d_ggsw_out, size_t count, void *scratch, size_t scratch_bytes, hipStream_t s) {
    require_wop_shape(c);
    validate_cbs(c, delta_log, base_log, level);
    require_fbsk(c);
    require_pfpksk(c);
    if (count == 0) return;
    if (count > kPfpksMaxRows / level) fail("count too large");
    const CbsLayout l = cbs_layout(c, level, count);
    require_scratch(scratch ? scratch_bytes : 0, l.total());
    const size_t rows = count * level, sw = c->n() + 1, bw = c->big_dim() + 1;
    uint64_t *shifted = scratch_at<uint64_t>(scratch, 0);
    uint64_t *luts = scratch_at<uint64_t>(scratch, l.luts);
    uint32_t *idx = scratch_at<uint32_t>(scratch, l.idx);
    uint64_t *pbs_out = scratch_at<uint64_t>(scratch, l.pbs_out);
    void *rest = scratch_at(scratch, l.rest);
    const size_t rest_bytes = scratch_bytes - l.rest;
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
}  // namespace

namespace tfhe_mi355::capi {
void validate_lut_indexes(const uint32_t *idx, size_t count, size_t lut_count) {
    if (!idx) return;
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= lut_count) fail("lut_indexes[%zu] = %u out of range (lut_count %zu)", i, idx[i], lut_count);
}

// an ABI call made from inside another one: its failure text becomes ours
void abi(int rc) {
    if (rc != TFHE_MI355_OK) fail("%s", tfhe_mi355_last_error());
}
}  // namespace tfhe_mi355::capi

// ---- host-pointer pipeline ------------------------------------------------------------------------
// The synchronous entry points (host buffers in and out, the form the Rust binding calls) run the
// batch in chunks: per chunk, the host input slice is copied into a lane's page-locked buffer and
// DMA'd up on the lane's copy stream, the kernels run on ctx->stream (chunks in order, so the GPU
// stays busy), and the output is DMA'd back on the copy stream and copied into the caller's
// buffer while the next chunk's kernels run.  The LUTs go up once per call.  Callers are
// serialised by ctx->mu.
namespace {

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
}  // namespace

namespace tfhe_mi355::capi {
void run_host_pipeline(TfheMi355Context *c, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                       const uint64_t *luts, size_t lut_words, size_t lut_count, const uint32_t *idx, size_t count,
                       ChunkLaunch launch, ScratchSize scratch_size, const ChunkSource *from) {
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
    const bool pin_in = !from && is_pinned(in, count * in_words * 8), pin_out = is_pinned(out, count * out_words * 8);
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
            if (!pin_in && !from) L.h_in.reserve(chunk * in_words * 8);
            if (!pin_out) L.h_out.reserve(chunk * out_words * 8);
            L.d_in.reserve(chunk * in_words * 8);
            L.d_out.reserve(chunk * out_words * 8);
            if (from) {  // the rows are written on the device from a compressed source
                from->stage(L, next, cnt);
            } else {
                const uint64_t *src = in + next * in_words;
                if (!pin_in) {
                    std::memcpy(L.h_in.ptr, src, cnt * in_words * 8);
                    src = (const uint64_t *)L.h_in.ptr;
                }
                check(hipMemcpyAsync(L.d_in.ptr, src, cnt * in_words * 8, hipMemcpyHostToDevice, L.stream), "H2D in");
            }
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
            if (from) from->expand(L, next, cnt, cs);
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
void chunk_ks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
              size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_ks_dev(c, i, o, n, sc, sb, s);
}
}  // namespace tfhe_mi355::capi

namespace {
void chunk_blind_rotate(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *l, size_t lc,
                        const uint32_t *x, size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_pbs_dev(c, i, o, l, lc, x, n, sc, sb, s, true);
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
}  // namespace

namespace tfhe_mi355::capi {
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
}  // namespace tfhe_mi355::capi

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

// ---- WoP-PBS, the bootstrapped half: entry points -----------------------------------------------------

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
}  // namespace

namespace tfhe_mi355::capi {
// host-pointer form of a WoP-PBS call: items in chunks through device buffers of the call's own, on
// the context's stream; f(d_in, d_out, d_idx, n, d_scratch, scratch_bytes, stream) launches one chunk
void host_wop_call(TfheMi355Context *ctx, const uint64_t *in, size_t in_words, uint64_t *out, size_t out_words,
                   const uint32_t *idx, size_t count, size_t chunk, const std::function<size_t(size_t)> &scratch_bytes,
                   const std::function<void(const uint64_t *, uint64_t *, const uint32_t *, size_t, void *, size_t,
                                            hipStream_t)> &f) {
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
}  // namespace tfhe_mi355::capi

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
        const bool mfma = !ks_mfma_disabled() && ks_mfma_supported((int)in_dim, (int)level, (int)base_log);
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

static_assert(sizeof(TfheMi355BlockOp) == sizeof(BlockLayerOp) && TFHE_MI355_BLOCK_OP_TERMS == BLOCK_LAYER_TERMS &&
                  offsetof(TfheMi355BlockOp, body_add) == offsetof(BlockLayerOp, body_add) &&
                  offsetof(TfheMi355BlockOp, term) == offsetof(BlockLayerOp, term) &&
                  sizeof(((TfheMi355BlockOp *)0)->term[0]) == sizeof(((BlockLayerOp *)0)->term[0]),
              "TfheMi355BlockOp and the launcher's BlockLayerOp are one layout");

int tfhe_mi355_lwe_block_layer_async(TfheMi355Context *ctx, const TfheMi355BlockOp *ops, size_t n_ops, size_t rows,
                                     size_t words, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!ops && n_ops)) fail("null argument");
        if (n_ops && words == 0) fail("block layer: rows of zero words");
        for (size_t i = 0; i < n_ops; i++) {
            if (!ops[i].dst) fail("block layer: op %zu has a null destination", i);
            if (ops[i].dst_stride < words)
                fail("block layer: op %zu: destination row stride smaller than the row", i);
            for (int t = 0; t < TFHE_MI355_BLOCK_OP_TERMS; t++)
                if (ops[i].term[t].src && ops[i].term[t].stride < words)
                    fail("block layer: op %zu term %d: row stride smaller than the row", i, t);
        }
        if (n_ops == 0 || rows == 0) return;
        check(hipSetDevice(ctx->device), "hipSetDevice");
        check(launch_lwe_block_layer(reinterpret_cast<const BlockLayerOp *>(ops), n_ops, rows, words,
                                     (hipStream_t)stream),
              "lwe block layer");
    });
}

static_assert(sizeof(TfheMi355ClearBlockOp) == sizeof(ClearBlockLayerOp) &&
                  offsetof(TfheMi355ClearBlockOp, op) == offsetof(ClearBlockLayerOp, op) &&
                  offsetof(TfheMi355ClearBlockOp, d_clear) == offsetof(ClearBlockLayerOp, d_clear) &&
                  offsetof(TfheMi355ClearBlockOp, clear_scale) == offsetof(ClearBlockLayerOp, clear_scale) &&
                  offsetof(TfheMi355ClearBlockOp, d_lut_index) == offsetof(ClearBlockLayerOp, d_lut_index) &&
                  offsetof(TfheMi355ClearBlockOp, clear_negate) == offsetof(ClearBlockLayerOp, clear_negate) &&
                  offsetof(TfheMi355ClearBlockOp, clear_shift) == offsetof(ClearBlockLayerOp, clear_shift) &&
                  offsetof(TfheMi355ClearBlockOp, clear_bits) == offsetof(ClearBlockLayerOp, clear_bits) &&
                  offsetof(TfheMi355ClearBlockOp, lut_base) == offsetof(ClearBlockLayerOp, lut_base),
              "TfheMi355ClearBlockOp and the launcher's ClearBlockLayerOp are one layout");

int tfhe_mi355_lwe_clear_block_layer_async(TfheMi355Context *ctx, const TfheMi355ClearBlockOp *ops, size_t n_ops,
                                           size_t rows, size_t words, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!ops && n_ops)) fail("null argument");
        if (n_ops && words == 0) fail("block layer: rows of zero words");
        for (size_t i = 0; i < n_ops; i++) {
            const TfheMi355BlockOp &op = ops[i].op;
            if (!op.dst) fail("block layer: op %zu has a null destination", i);
            if (op.dst_stride < words) fail("block layer: op %zu: destination row stride smaller than the row", i);
            for (int t = 0; t < TFHE_MI355_BLOCK_OP_TERMS; t++)
                if (op.term[t].src && op.term[t].stride < words)
                    fail("block layer: op %zu term %d: row stride smaller than the row", i, t);
            if (ops[i].clear_shift > 63) fail("block layer: op %zu: clear_shift %u above 63", i, ops[i].clear_shift);
            if (ops[i].clear_bits > (uint32_t)CLEAR_BLOCK_LAYER_MAX_BITS)
                fail("block layer: op %zu: clear_bits %u above %d", i, ops[i].clear_bits, CLEAR_BLOCK_LAYER_MAX_BITS);
            if (ops[i].d_lut_index && !ops[i].d_clear && ops[i].clear_bits)
                fail("block layer: op %zu: a LUT index from %u clear bits, but no clear operand", i, ops[i].clear_bits);
        }
        if (n_ops == 0 || rows == 0) return;
        check(hipSetDevice(ctx->device), "hipSetDevice");
        check(launch_lwe_clear_block_layer(reinterpret_cast<const ClearBlockLayerOp *>(ops), n_ops, rows, words,
                                           (hipStream_t)stream),
              "lwe clear block layer");
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
