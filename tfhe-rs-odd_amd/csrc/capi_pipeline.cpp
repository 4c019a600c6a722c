// capi_pipeline.cpp -- how host-pointer calls reach the device behind include/tfhe_mi355.h (capi_internal.h):
// the two-lane host-pointer pipeline of the batched entry points (run_host_pipeline), the request coalescer
// of the small ones (coalesced_call), and the submit / wait entry points (tfhe_mi355_submit, _wait,
// _coalesce_stats).
#include "capi_internal.h"

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
}  // namespace tfhe_mi355::capi

extern "C" {

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

}  // extern "C"
