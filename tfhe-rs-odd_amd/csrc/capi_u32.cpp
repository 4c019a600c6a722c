// capi_u32.cpp -- the 32-bit torus behind include/tfhe_mi355.h ("32-bit torus"; capi_internal.h): the Boolean
// module's u32 PBS, keyswitch, gate and mux batches.
#include "capi_internal.h"

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
    return !ks_mfma_disabled() && ks32_mfma_supported((int)c->big_dim(), (int)c->p.ks_level, (int)c->p.ks_base_log);
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

void pbs32_host(TfheMi355Context *ctx, const uint32_t *lwe_in, uint32_t *out, const uint32_t *luts, size_t lut_count,
                const uint32_t *lut_indexes, size_t count, bool glwe_out) {
    require_single32(ctx);
    if ((!lwe_in && count) || (!out && count) || !luts) fail("null argument");
    if (count == 0) return;
    require_fbsk32(ctx);
    if (lut_count == 0) fail("lut_count must be >= 1");
    validate_lut_indexes(lut_indexes, count, lut_count);
    const size_t wi = ctx->n() + 1, wo = glwe_out ? ctx->glwe_len() : ctx->big_dim() + 1;
    HostCall h(ctx, align256(count * wi * 4) + align256(lut_count * ctx->glwe_len() * 4) + align256(count * 4),
               count * wo * 4, 0, 256, "u32 call sync");
    const uint32_t *d_in = h.up(lwe_in, count * wi);
    const uint32_t *d_luts = h.up(luts, lut_count * ctx->glwe_len());
    const uint32_t *d_idx = h.up(lut_indexes, lut_indexes ? count : 0);
    launch_pbs32_dev(ctx, d_in, h.out<uint32_t>(), d_luts, lut_count, d_idx, count, ctx->stream, glwe_out);
    h.down(out, count * wo * 4);
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
        HostCall h(ctx, align256(count * wi * 4), count * wo * 4, sb, 256, "u32 call sync");
        const uint32_t *d_in = h.up(lwe_in, count * wi);
        launch_ks32_dev(ctx, d_in, h.out<uint32_t>(), count, h.scratch(), sb, ctx->stream);
        h.down(lwe_out, count * wo * 4);
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
        HostCall h(ctx, 2 * align256(words * 4) + align256(count), words * 4, l.total(), 256, "u32 call sync");
        const uint32_t *d_lhs = h.up(lhs, words);
        const uint32_t *d_rhs = h.up(rhs, words);
        const uint8_t *d_ops = h.up(ops, count);
        launch_gates32_dev(ctx, d_ops, d_lhs, d_rhs, h.out<uint32_t>(), count, pbs_order, h.scratch(), l.total(),
                           ctx->stream);
        h.down(out, words * 4);
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
        HostCall h(ctx, 3 * align256(words * 4), words * 4, l.total(), 256, "u32 call sync");
        const uint32_t *d_c = h.up(cond, words);
        const uint32_t *d_t = h.up(then_ct, words);
        const uint32_t *d_e = h.up(else_ct, words);
        launch_mux32_dev(ctx, d_c, d_t, d_e, h.out<uint32_t>(), count, pbs_order, h.scratch(), l.total(), ctx->stream);
        h.down(out, words * 4);
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
