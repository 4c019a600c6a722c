// capi_gadget.cpp -- the gadget layer behind include/tfhe_mi355.h (capi_internal.h): the LWE -> GLWE packing
// keyswitch, the GLWE x polynomial, GLWE x GLWE and LWE x LWE products (glwe_ops.hip, glwe_mult.hip), the
// per-item GGSW external product and CMUX, and vertical packing (ggsw_ops.hip), with their entry points.
#include "capi_internal.h"

namespace {
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

void chunk_pks(TfheMi355Context *c, const uint64_t *i, uint64_t *o, const uint64_t *, size_t, const uint32_t *,
               size_t n, void *sc, size_t sb, hipStream_t s) {
    launch_packing_ks_dev(c, i, o, n, sc, sb, s);
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

// ---- GGSW operations (ggsw_ops.hip): per-item GGSW ciphertexts, decomposition chosen per call ----
size_t ggsw_polys(const TfheMi355Context *c, uint32_t level) { return (size_t)level * (c->k() + 1) * (c->k() + 1); }

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

extern "C" {

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

}  // extern "C"
