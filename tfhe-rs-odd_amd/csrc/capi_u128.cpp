// capi_u128.cpp -- the 128-bit torus behind include/tfhe_mi355.h (capi_internal.h): pbs_f128.hip, the
// reference's fft128 path.
#include "capi_internal.h"

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
    const size_t sb = pbs128_scratch_bytes(ctx, count);  // > 0: count > 0
    // a u128 word is two u64 words of the caller's arrays
    HostCall h(ctx, in_b + lut_b + align256(count * 4), std::max<size_t>(count * wo * 16, 256), sb, 0,
               "u128 call sync");
    const uint64_t *d_in = h.up(lwe_in, count * wi * 2);
    const uint64_t *d_luts = h.up(luts, lut_count * ctx->glwe_len() * 2);
    const uint32_t *d_idx = h.up(lut_indexes, lut_indexes ? count : 0);
    launch_pbs128_dev(ctx, d_in, h.out(), d_luts, lut_count, d_idx, count, modulus_log, h.scratch(), sb, ctx->stream,
                      glwe_out);
    h.down(out, count * wo * 16);
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
