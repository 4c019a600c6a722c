// capi_ingress.cpp -- compressed ciphertext sources behind include/tfhe_mi355.h (capi_internal.h): the
// TfheMi355LweSource descriptor, expansion alone (tfhe_mi355_lwe_expand*) and expansion composed with the
// keyed operations (tfhe_mi355_apply_from*), over lwe_ingress.hip and csprng.hip.
#include "capi_internal.h"

namespace {

enum : uint32_t { SRC_ROWS = 0, SRC_COMPACT, SRC_SEEDED_LIST, SRC_SEEDED_ROWS, SRC_KINDS };

void require_kind(uint32_t kind, uint32_t n) {
    if (kind >= SRC_KINDS)
        fail("unknown source kind %u (0 expanded rows, 1 compact list, 2 seeded list, 3 seeded rows)", kind);
    if (n == 0 || n > 0x3fffffffu) fail("source lwe_dimension %u out of range", n);
    if (kind == SRC_COMPACT && !is_pow2(n)) fail("compact list: lwe_dimension %u is not a power of two", n);
}

void require_source(const TfheMi355LweSource *src, size_t count) {
    if (!src) fail("null source");
    require_kind(src->kind, src->lwe_dimension);
    if (count && !src->data) fail("null source data");
    if (count && (src->kind == SRC_SEEDED_LIST || src->kind == SRC_SEEDED_ROWS) && !src->seeds)
        fail("source kind %u needs seeds", src->kind);
}

size_t compact_mask_words(size_t n, size_t count) { return (count + n - 1) / n * n; }

// u64 words of src.data and src.seeds for `count` ciphertexts
size_t data_words(uint32_t kind, size_t n, size_t count) {
    switch (kind) {
    case SRC_ROWS: return count * (n + 1);
    case SRC_COMPACT: return compact_mask_words(n, count) + count;
    default: return count;
    }
}
size_t seed_words(uint32_t kind, size_t count) {
    return kind == SRC_SEEDED_LIST ? 2 : kind == SRC_SEEDED_ROWS ? 2 * count : 0;
}

// ---- expansion ------------------------------------------------------------------------------------
// Rows [first, first + count) of a source, written to d_out (those rows').  a: the rows (kind 0), the bin masks
// of the whole list (1), unused (2, 3); d_bodies, d_seeds: those rows' (2: d_seeds unused, d_tables the AES
// tables of the list's seed).
void expand_rows(TfheMi355Context *c, uint32_t kind, size_t n, const uint64_t *a, const uint64_t *d_bodies,
                 const uint64_t *d_seeds, const void *d_tables, size_t first, size_t count, uint64_t *d_out,
                 hipStream_t s) {
    if (count == 0) return;
    switch (kind) {
    case SRC_ROWS:
        check(hipMemcpyAsync(d_out, a, count * (n + 1) * 8, hipMemcpyDeviceToDevice, s), "copy rows");
        break;
    case SRC_COMPACT:
        check(launch_lwe_compact_expand(a, d_bodies, n, first, count, d_out, s), "compact list expansion");
        break;
    case SRC_SEEDED_LIST:
        check(launch_seeded_decompress_from(d_tables, d_bodies, first, count, n, 1, d_out, s),
              "seeded list decompression");
        break;
    default:
        check(launch_csprng_rows(c->aes_base.ptr, d_seeds, d_bodies, n, count, d_out, s), "seeded rows decompression");
    }
}

// the device scratch of an expansion: the AES tables of a seeded list's seed (it is device data)
struct ExpandLayout {
    size_t tables = 0, bytes = 0;
    size_t total() const { return bytes; }
};
ExpandLayout expand_layout(uint32_t kind) {
    ScratchCursor cur;
    ExpandLayout l;
    if (kind == SRC_SEEDED_LIST) l.tables = cur.take(aes_tables_bytes());
    l.bytes = cur.off;
    return l;
}

// a whole source in device memory -> rows [0, count)
void launch_lwe_expand_dev(TfheMi355Context *c, const TfheMi355LweSource &d, size_t count, uint64_t *d_out,
                           void *scratch, size_t scratch_bytes, hipStream_t s) {
    if (count == 0) return;
    const size_t n = d.lwe_dimension;
    const ExpandLayout l = expand_layout(d.kind);
    require_scratch(scratch_bytes, l.total());
    if (l.total() && !scratch) fail("null scratch");
    const void *tables = nullptr;
    if (d.kind == SRC_SEEDED_LIST) {
        check(launch_aes_schedule(c->aes_base.ptr, d.seeds, scratch_at(scratch, l.tables), s), "aes key schedule");
        tables = scratch_at(scratch, l.tables);
    }
    const uint64_t *bodies = d.kind == SRC_COMPACT ? d.data + compact_mask_words(n, count) : d.data;
    expand_rows(c, d.kind, n, d.data, bodies, d.seeds, tables, 0, count, d_out, s);
}

// ---- the keyed operations, numbered as tfhe_mi355_submit ----------------------------------------------
struct OpShape {
    size_t in_dim, out_words;
    ChunkLaunch launch;
    ScratchSize scratch;
    bool luts, ksk;
};
OpShape op_shape(const TfheMi355Context *c, int op) {
    switch (op) {
    case CO_PBS: return {c->n(), c->big_dim() + 1, chunk_pbs, pbs_scratch_bytes, true, false};
    case CO_KS_PBS: return {c->big_dim(), c->big_dim() + 1, launch_ks_pbs_dev, ks_pbs_scratch_bytes, true, true};
    case CO_PBS_KS: return {c->n(), c->n() + 1, launch_pbs_ks_dev, pbs_ks_scratch_bytes, true, true};
    case CO_KS: return {c->big_dim(), c->n() + 1, chunk_ks, ks_scratch_bytes, false, true};
    default: fail("unknown op %d (0 PBS, 1 KS->PBS, 2 PBS->KS, 3 KS)", op);
    }
}

void require_apply_from(TfheMi355Context *c, int op, uint32_t kind, uint32_t n) {
    if (!c) fail("null ctx");
    if (c->multi()) fail("apply_from calls are not available on a multi-device context: expand and split the rows");
    require_kind(kind, n);
    const OpShape o = op_shape(c, op);
    if (o.luts)
        require_fbsk(c);
    if (o.ksk) require_ksk(c);
    if (n != o.in_dim)
        fail("source lwe_dimension %u, but op %d takes rows of dimension %zu on this context", n, op, o.in_dim);
}

// device scratch of apply_from_async: the expanded rows, the expansion's own, then the operation's
struct ApplyFromLayout : TailLayout {
    size_t rows = 0, expand = 0;
};
ApplyFromLayout apply_from_layout(const TfheMi355Context *c, const OpShape &o, uint32_t kind, size_t count) {
    ScratchCursor cur;
    ApplyFromLayout l;
    if (kind != SRC_ROWS) {
        l.rows = cur.take(count * (o.in_dim + 1) * 8);
        l.expand = cur.take(expand_layout(kind).total());
    }
    l.rest = cur.off;
    l.rest_bytes = o.scratch(c, count);
    return l;
}

}  // namespace

extern "C" {

int tfhe_mi355_lwe_expand_scratch(TfheMi355Context *ctx, uint32_t kind, uint32_t lwe_dimension, size_t count,
                                  size_t *bytes) {
    return guarded([&] {
        if (!ctx || !bytes) fail("null argument");
        require_kind(kind, lwe_dimension);
        *bytes = count ? expand_layout(kind).total() : 0;
    });
}

int tfhe_mi355_lwe_expand_async(TfheMi355Context *ctx, const TfheMi355LweSource *d_src, size_t count,
                                uint64_t *d_lwe_out, void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        ctx = primary(ctx);  // device pointers: the first device's shard
        if (!ctx || (!d_lwe_out && count)) fail("null argument");
        require_source(d_src, count);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        launch_lwe_expand_dev(ctx, *d_src, count, d_lwe_out, d_scratch, scratch_bytes, (hipStream_t)stream);
    });
}

int tfhe_mi355_lwe_expand(TfheMi355Context *ctx, const TfheMi355LweSource *src, size_t count, uint64_t *lwe_out) {
    return guarded([&] {
        ctx = primary(ctx);
        if (!ctx || (!lwe_out && count)) fail("null argument");
        require_source(src, count);
        if (count == 0) return;
        const uint32_t kind = src->kind;
        const size_t n = src->lwe_dimension;
        if (kind == SRC_ROWS) {
            std::memcpy(lwe_out, src->data, count * (n + 1) * 8);
            return;
        }
        std::lock_guard<std::mutex> g(ctx->mu);
        check(hipSetDevice(ctx->device), "hipSetDevice");
        hipStream_t s = ctx->stream;
        // the compressed source goes up whole: [data | seeds | expansion scratch]
        const size_t dw = data_words(kind, n, count), sw = seed_words(kind, count);
        ScratchCursor cur;
        const size_t at_data = cur.take(dw * 8), at_seeds = cur.take(sw * 8), at_scratch = cur.off;
        const size_t scratch_bytes = expand_layout(kind).total();
        ctx->io_src.reserve(at_scratch + scratch_bytes);
        check(hipMemcpyAsync(scratch_at(ctx->io_src.ptr, at_data), src->data, dw * 8, hipMemcpyHostToDevice, s), "H2D source");
        if (sw)
            check(hipMemcpyAsync(scratch_at(ctx->io_src.ptr, at_seeds), src->seeds, sw * 8, hipMemcpyHostToDevice, s),
                  "H2D seeds");
        const uint64_t *d_data = scratch_at<uint64_t>(ctx->io_src.ptr, at_data);
        const uint64_t *d_seeds = scratch_at<uint64_t>(ctx->io_src.ptr, at_seeds);
        const void *tables = nullptr;
        if (kind == SRC_SEEDED_LIST) {
            check(launch_aes_schedule(ctx->aes_base.ptr, d_seeds, scratch_at(ctx->io_src.ptr, at_scratch), s),
                  "aes key schedule");
            tables = scratch_at(ctx->io_src.ptr, at_scratch);
        }
        const uint64_t *d_bodies = kind == SRC_COMPACT ? d_data + compact_mask_words(n, count) : d_data;
        // the rows come back in slices of at most 64 MiB through lane 0's output buffer
        const size_t slice = std::min(count, std::max<size_t>(1, ((size_t)64 << 20) / ((n + 1) * 8)));
        ctx->lanes[0].d_out.reserve(slice * (n + 1) * 8);
        uint64_t *d_out = (uint64_t *)ctx->lanes[0].d_out.ptr;
        for (size_t first = 0; first < count; first += slice) {
            const size_t cnt = std::min(slice, count - first);
            expand_rows(ctx, kind, n, d_data, d_bodies + first, kind == SRC_SEEDED_ROWS ? d_seeds + 2 * first : d_seeds,
                        tables, first, cnt, d_out, s);
            check(hipMemcpyAsync(lwe_out + first * (n + 1), d_out, cnt * (n + 1) * 8, hipMemcpyDeviceToHost, s), "D2H rows");
            check(hipStreamSynchronize(s), "lwe expansion sync");
        }
    });
}

int tfhe_mi355_apply_from_scratch(TfheMi355Context *ctx, int op, uint32_t kind, size_t count, size_t *bytes) {
    return guarded([&] {
        if (!ctx || !bytes) fail("null argument");
        if (ctx->multi()) fail("apply_from calls are not available on a multi-device context: expand and split the rows");
        const OpShape o = op_shape(ctx, op);
        require_kind(kind, (uint32_t)o.in_dim);
        require_width64(ctx);
        std::lock_guard<std::mutex> g(ctx->mu);
        *bytes = apply_from_layout(ctx, o, kind, count).total();
    });
}

int tfhe_mi355_apply_from_async(TfheMi355Context *ctx, int op, const TfheMi355LweSource *d_src, uint64_t *d_lwe_out,
                                const uint64_t *d_luts, size_t lut_count, const uint32_t *d_lut_indexes, size_t count,
                                void *d_scratch, size_t scratch_bytes, void *stream) {
    return guarded([&] {
        if (!d_src) fail("null source");
        require_apply_from(ctx, op, d_src->kind, d_src->lwe_dimension);
        require_source(d_src, count);
        const OpShape o = op_shape(ctx, op);
        if ((!d_lwe_out && count) || (o.luts && !d_luts)) fail("null argument");
        if (count == 0) return;
        check(hipSetDevice(ctx->device), "hipSetDevice");
        hipStream_t s = (hipStream_t)stream;
        const ApplyFromLayout l = apply_from_layout(ctx, o, d_src->kind, count);
        require_scratch(scratch_bytes, l.total());
        if (l.total() && !d_scratch) fail("null scratch");
        const uint64_t *rows = d_src->data;
        if (d_src->kind != SRC_ROWS) {
            uint64_t *d_rows = scratch_at<uint64_t>(d_scratch, l.rows);
            launch_lwe_expand_dev(ctx, *d_src, count, d_rows, scratch_at(d_scratch, l.expand),
                                  expand_layout(d_src->kind).total(), s);
            rows = d_rows;
        }
        o.launch(ctx, rows, d_lwe_out, o.luts ? d_luts : nullptr, o.luts ? lut_count : 0,
                 o.luts ? d_lut_indexes : nullptr, count, l.rest_bytes ? scratch_at(d_scratch, l.rest) : nullptr,
                 l.rest_bytes ? scratch_bytes - l.rest : 0, s);
    });
}

int tfhe_mi355_apply_from(TfheMi355Context *ctx, int op, const TfheMi355LweSource *src, uint64_t *lwe_out,
                          const uint64_t *luts, size_t lut_count, const uint32_t *lut_indexes, size_t count) {
    return guarded([&] {
        if (!src) fail("null source");
        require_apply_from(ctx, op, src->kind, src->lwe_dimension);
        require_source(src, count);
        const OpShape o = op_shape(ctx, op);
        if ((!lwe_out && count) || (o.luts && !luts)) fail("null argument");
        if (o.luts) {
            if (lut_count == 0) fail("lut_count must be >= 1");
            validate_lut_indexes(lut_indexes, count, lut_count);
        }
        if (src->kind == SRC_ROWS) {  // the operation's own call
            switch (op) {
            case CO_PBS: return abi(tfhe_mi355_programmable_bootstrap(ctx, src->data, lwe_out, luts, lut_count, lut_indexes, count));
            case CO_KS_PBS:
                return abi(tfhe_mi355_keyswitch_programmable_bootstrap(ctx, src->data, lwe_out, luts, lut_count, lut_indexes, count));
            case CO_PBS_KS:
                return abi(tfhe_mi355_programmable_bootstrap_keyswitch(ctx, src->data, lwe_out, luts, lut_count, lut_indexes, count));
            default: return abi(tfhe_mi355_keyswitch(ctx, src->data, lwe_out, count));
            }
        }
        if (count == 0) return;
        check(hipSetDevice(ctx->device), "hipSetDevice");
        std::lock_guard<std::mutex> g(ctx->mu);
        const uint32_t kind = src->kind;
        const size_t n = src->lwe_dimension;
        hipStream_t cs = ctx->stream;
        // once per call, on the kernel stream ahead of every chunk: the compact container (small: one mask
        // per n ciphertexts), or the AES tables of the list's seed
        const uint64_t *d_masks = nullptr, *d_all_bodies = nullptr;
        const void *tables = nullptr;
        if (kind == SRC_COMPACT) {
            const size_t dw = data_words(kind, n, count);
            ctx->io_src.reserve(dw * 8);
            check(hipMemcpyAsync(ctx->io_src.ptr, src->data, dw * 8, hipMemcpyHostToDevice, cs), "H2D compact list");
            d_masks = (const uint64_t *)ctx->io_src.ptr;
            d_all_bodies = d_masks + compact_mask_words(n, count);
        } else if (kind == SRC_SEEDED_LIST) {
            ScratchCursor cur;
            const size_t at_seed = cur.take(16), at_tables = cur.take(aes_tables_bytes());
            ctx->io_src.reserve(cur.off);
            check(hipMemcpyAsync(scratch_at(ctx->io_src.ptr, at_seed), src->seeds, 16, hipMemcpyHostToDevice, cs), "H2D seed");
            check(launch_aes_schedule(ctx->aes_base.ptr, scratch_at<uint64_t>(ctx->io_src.ptr, at_seed),
                                      scratch_at(ctx->io_src.ptr, at_tables), cs),
                  "aes key schedule");
            tables = scratch_at(ctx->io_src.ptr, at_tables);
        }
        ChunkSource from;
        // per chunk, on the lane's copy stream: its bodies (and seeds) -> [bodies | seeds] in the lane's buffer
        from.stage = [&](TfheMi355Context::Lane &L, size_t first, size_t cnt) {
            if (kind == SRC_COMPACT) return;
            const size_t at_seeds = align256(cnt * 8);
            L.d_src.reserve(at_seeds + (kind == SRC_SEEDED_ROWS ? cnt * 16 : 0));
            check(hipMemcpyAsync(L.d_src.ptr, src->data + first, cnt * 8, hipMemcpyHostToDevice, L.stream), "H2D bodies");
            if (kind == SRC_SEEDED_ROWS)
                check(hipMemcpyAsync(scratch_at(L.d_src.ptr, at_seeds), src->seeds + 2 * first, cnt * 16,
                                     hipMemcpyHostToDevice, L.stream),
                      "H2D seeds");
        };
        from.expand = [&](TfheMi355Context::Lane &L, size_t first, size_t cnt, hipStream_t s) {
            if (kind == SRC_COMPACT)
                return expand_rows(ctx, kind, n, d_masks, d_all_bodies + first, nullptr, nullptr, first, cnt,
                                   (uint64_t *)L.d_in.ptr, s);
            expand_rows(ctx, kind, n, nullptr, (const uint64_t *)L.d_src.ptr,
                        scratch_at<uint64_t>(L.d_src.ptr, align256(cnt * 8)), tables, first, cnt, (uint64_t *)L.d_in.ptr, s);
        };
        run_host_pipeline(ctx, nullptr, o.in_dim + 1, lwe_out, o.out_words, o.luts ? luts : nullptr, ctx->glwe_len(),
                          o.luts ? lut_count : 0, o.luts ? lut_indexes : nullptr, count, o.launch, o.scratch, &from);
    });
}

}  // extern "C"
