// capi_wopbs.cpp -- the bootstrapped half of WoP-PBS behind include/tfhe_mi355.h (capi_internal.h): the private
// functional packing keyswitch (pfpks.hip), bit extraction, the circuit bootstrap and its composition with
// vertical packing (capi_gadget.cpp), over the PBS and keyswitch launchers of capi_pbs.cpp and the glue
// kernels of lwe_ops.hip.
#include "capi_internal.h"

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

// ---- WoP-PBS, the bootstrapped half: entry points -----------------------------------------------------
extern "C" {

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

}  // extern "C"
