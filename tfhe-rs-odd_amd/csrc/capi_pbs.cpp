// capi_pbs.cpp -- the 64-bit PBS and keyswitch family behind include/tfhe_mi355.h (capi_internal.h): the
// kernel-form policy with its scratch sizes, the PBS, keyswitch and fused KS/PBS launchers, and their entry
// points (tfhe_mi355_programmable_bootstrap*, _blind_rotate*, _keyswitch*, the block layers), over the
// pbs_*.hip, keyswitch.hip and lwe_ops.hip kernels.
#include "capi_internal.h"

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

size_t quad_sub_blocks(const TfheMi355Context *c) { return c->N() / 2048; }

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

void chunk_blind_rotate(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *l, size_t lc,
                        const uint32_t *x, size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_pbs_dev(c, i, o, l, lc, x, n, sc, sb, s, true);
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

// The quad CMUX (N = 8192, L = 1 or 2 classic, four CUs per ciphertext, pbs_large.hip; N = 4096: two CUs,
// the "duo") for batches of at most this many ciphertexts: one pass of CUs / R by default (R = N / 2048
// sub-blocks); TFHE_MI355_QUAD_MAX overrides (0 = never)
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

void validate_lut_indexes(const uint32_t *idx, size_t count, size_t lut_count) {
    if (!idx) return;
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= lut_count) fail("lut_indexes[%zu] = %u out of range (lut_count %zu)", i, idx[i], lut_count);
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

extern "C" {

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

}  // extern "C"
