// engine.h -- internal launchers of the MI355X PBS engine (host side, no torch types).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

struct TfheMi355Context;  // include/tfhe_mi355.h (opaque there), capi_internal.h

namespace tfhe_mi355 {

// Key transaction (capi.cpp): holds the context's key locks (every shard's, for a multi-device
// context) exclusively until the returned holder is released.  Key uploads made from this thread in
// the meantime skip their own locking, so a multi-call upload (serde.cpp: keyswitching key, Fourier
// buffer, ready flag) is seen by coalesced batches only as a whole.
std::shared_ptr<void> begin_key_transaction(TfheMi355Context *ctx);

// True while `s` is being captured into a graph, and when its capture state cannot be read: what must not
// run under capture (event timing, a stream wait, a key upload) is then left out or refused.  The query
// itself is legal under capture and enqueues nothing.
inline bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
}

// Per-kernel durations measured on the launch stream (a profiling aid, off unless enabled through
// tfhe_mi355_kernel_timing_enable): the launchers bracket every `every`-th launch of a kernel
// family with HIP events; collect() waits for them and accumulates per-name totals.  bench.py
// reads the dominant kernel's average from here for its roofline.  Nothing is recorded while the
// stream is being captured into a graph.
struct KernelTimer {
    int every = 0;  // 0: off
    std::mutex mu;
    struct Rec {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    std::map<std::string, std::pair<double, uint64_t>> totals;  // name -> (ms, launches)
    std::map<std::string, uint64_t> calls;                      // launches seen per name (sampling)

    // true when this launch of `name` is to be timed
    bool want(const char *name, hipStream_t s) {
        if (every <= 0) return false;
        if (stream_is_capturing(s)) return false;
        std::lock_guard<std::mutex> g(mu);
        return calls[name]++ % (uint64_t)every == 0;
    }
    hipEvent_t record(hipStream_t s) {
        hipEvent_t e = nullptr;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!pool.empty()) {
                e = pool.back();
                pool.pop_back();
            }
        }
        if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
        (void)hipEventRecord(e, s);
        return e;
    }
    void done(const char *name, hipEvent_t a, hipStream_t s) {
        hipEvent_t b = record(s);
        if (!a || !b) return;
        std::lock_guard<std::mutex> g(mu);
        pending.push_back({name, a, b});
    }
    void collect() {
        std::vector<Rec> recs;
        {
            std::lock_guard<std::mutex> g(mu);
            recs.swap(pending);
        }
        for (auto &r : recs) {
            float ms = 0.f;
            if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                std::lock_guard<std::mutex> g(mu);
                auto &t = totals[r.name];
                t.first += ms;
                t.second += 1;
            }
            std::lock_guard<std::mutex> g(mu);
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
    }
    void reset() {
        collect();
        std::lock_guard<std::mutex> g(mu);
        totals.clear();
        calls.clear();
    }
    ~KernelTimer() {
        collect();
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

// RAII bracket of one kernel launch (no-op without a timer or when this launch is not sampled)
struct TimedLaunch {
    KernelTimer *t;
    const char *name;
    hipStream_t s;
    hipEvent_t a = nullptr;
    TimedLaunch(KernelTimer *t_, const char *name_, hipStream_t s_) : t(t_), name(name_), s(s_) {
        if (t && t->want(name, s)) a = t->record(s);
        else t = nullptr;
    }
    ~TimedLaunch() {
        if (t) t->done(name, a, s);
    }
};

// test hook: TFHE_MI355_GRID_CAP=<n>, read at every launch, caps the workgroups of the launches whose grid is
// capped already and whose kernel walks the rest of the work in a loop -- the persistent grid of the classic PBS
// (pbs_classic.hip), the AES mask stream (csprng.hip) and the ingress row kernels (lwe_ingress.hip) -- so that
// the loop wraps at small counts (unset or 0: no cap; the GGSW launches have TFHE_MI355_GGSW_GRID)
inline size_t grid_cap() {
    const char *e = std::getenv("TFHE_MI355_GRID_CAP");
    const long v = e && *e ? std::atol(e) : 0;
    return v > 0 ? (size_t)v : ~(size_t)0;
}

struct FftTables {
    // device tables, M entries each (M = N/2)
    double2 *W = nullptr;          // exp(-2 pi i t / M)
    double2 *twist = nullptr;      // exp(i pi j / N)            (fft/mod.rs:58-69)
    double2 *wtop = nullptr;       // N = 32768: top-stage twiddles wtop[c-1][a] = W[a c] (a < M/16, c < 16)
    int N = 0;
};

struct ClassicPbsLaunch {
    const uint64_t *lwe_in;      // [count][n+1]
    uint64_t *lwe_out;           // [count][k*N+1]
    const uint64_t *luts;        // [lut_count][(k+1)*N]
    const uint32_t *lut_indexes; // [count] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    const double2 *fbsk;         // engine Fourier layout
    const double2 *W, *twist;
    int n;
    int base_log;
    int count;
    int glwe_out;                // 1: write the rotated accumulator [count][(k+1)N] (no sample extract)
    uint32_t *ticket = nullptr;  // zeroed device word: dynamic ciphertext queue of the persistent grid (null: one pass)
    int cpw_eff = 0;             // set by the launcher: ciphertexts per workgroup actually used (0: all slots)
};

// Returns false if (N, k, L) has no compiled specialisation.
bool classic_pbs_supported(int N, int k, int L);
// device scratch (zeroed by the caller before each launch) for the persistent grid's ticket
size_t classic_pbs_ticket_bytes(int N, int k, int L);
// workgroups of the shape's kernel resident at once on the current device: the persistent grid's size before
// grid_cap() (0: the shape has no persistent grid, or no kernel)
int classic_pbs_resident_blocks(int N, int k, int L);
hipError_t launch_classic_pbs(int N, int k, int L, const ClassicPbsLaunch &a, hipStream_t s);
// latency form (pbs_latency.hip): one ciphertext per workgroup of 8 waves, same outputs; for small
// batches (the one-ciphertext-per-call pattern).  N = 2048, k = 1, L = 1 only; no ticket, no scratch.
bool latency_pbs_supported(int N, int k, int L);
hipError_t launch_latency_pbs(const ClassicPbsLaunch &a, hipStream_t s);
// diagnostic builds: the latency kernel writes s_memtime per CMUX phase of block 0 into the buffer
// the host passes as `ticket` (capi.cpp), read by scripts/latency_probe.py
#ifndef LAT_STAMPS
#define LAT_STAMPS 0
#endif

struct MultiBitPbsLaunch {
    const uint64_t *lwe_in;      // [count][n+1]
    uint64_t *lwe_out;           // [count][k*N+1]
    const uint64_t *luts;        // [lut_count][(k+1)*N]
    const uint32_t *lut_indexes; // [count] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    const double2 *fbsk;         // [n/g][2^g][L][k+1][k+1] polys, engine Fourier layout
    const double2 *W, *twist;
    int n;
    int base_log;
    int count;
    int glwe_out;                // 1: write the rotated accumulator [count][(k+1)N] (no sample extract)
};
bool multibit_pbs_supported(int N, int k, int L, int g);
hipError_t launch_multibit_pbs(int N, int k, int L, int g, const MultiBitPbsLaunch &a, hipStream_t s);
// latency form (pbs_latency.hip): one ciphertext per workgroup of 8 waves, keybundle built into LDS
// beside the forward transform; same outputs.  N = 2048, k = 1, L = 1, g = 2 / 3; no scratch.
bool latency_multibit_supported(int N, int k, int L, int g);
hipError_t launch_latency_multibit_pbs(int g, const MultiBitPbsLaunch &a, hipStream_t s);

// N = 32768 classic PBS: accumulator and spectra in device scratch, three launches per CMUX
struct LargePbsLaunch {
    const uint64_t *lwe_in;      // [count][n+1]
    uint64_t *lwe_out;           // [count][k*N+1]
    const uint64_t *luts;        // [lut_count][(k+1)*N]
    const uint32_t *lut_indexes; // [count] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    const double2 *fbsk;         // engine Fourier layout
    const double2 *W, *twist;
    const double2 *wtop;         // FftTables::wtop
    int n;
    int base_log;
    int count;
    void *scratch;               // >= large_pbs_scratch_per_ct() bytes per ciphertext of a chunk
    size_t scratch_bytes;
    uint64_t *acc;               // set by the launcher
    double2 *spectra;            // set by the launcher
    int levels;                  // set by the launcher (= pbs_level)
    int chunk_count;             // set by the launcher: ciphertexts in the current chunk
    KernelTimer *timer = nullptr;  // optional per-kernel timing
    int grouping = 0;              // > 0: multi-bit PBS (fbsk = [n/g][2^g][L][k+1][k+1] polys)
    int onchip_min_count = 0;      // N = 8192, L = 2 classic: the on-chip CMUX from this many ciphertexts on
    // N = 8192, L = 2 classic: the quad CMUX (R workgroups per ciphertext) for batches
    // of at most quad_max_count ciphertexts, quad_pass ciphertexts per launch (CUs / R: one workgroup
    // per CU, all resident at once); 0 = never
    int quad_pass = 0, quad_max_count = 0;
    uint32_t *quad_fail = nullptr;  // device word set by a quad workgroup whose partners never arrived
};
bool large_pbs_supported(int N, int k, int L);
bool large_multibit_supported(int N, int k, int L, int g);
size_t large_pbs_scratch_per_ct(int N, int k, int L);
hipError_t launch_large_pbs(int N, int k, int L, const LargePbsLaunch &a, hipStream_t s);
hipError_t launch_large_bsk_to_fourier(const uint64_t *std_polys, double2 *fourier, size_t npoly,
                                       const FftTables &t, hipStream_t s);

// standard BSK polys (npoly x N u64) -> Fourier (npoly x M double2, engine layout)
hipError_t launch_bsk_to_fourier(int N, const uint64_t *std_polys, double2 *fourier, size_t npoly,
                                 const FftTables &t, hipStream_t s);

struct KeyswitchLaunch {
    const uint64_t *lwe_in;  // [count][in_dim+1]
    uint64_t *lwe_out;       // [count][out_dim+1]
    const uint64_t *ksk;     // [in_dim][level][out_dim+1]
    int in_dim, out_dim, base_log, level;
    int count;
    // output column receiving the input body: out_dim for an LWE keyswitch, k*N for the LWE ->
    // GLWE packing keyswitch (lwe_packing_keyswitch.rs:159-161, the GLWE body's constant term)
    int body_col = -1;
    __host__ __device__ int body() const { return body_col < 0 ? out_dim : body_col; }
};
hipError_t launch_keyswitch(const KeyswitchLaunch &a, hipStream_t s);
// the scalar kernel with 16-bit digits (8 <= base_log <= 15); decompositions either scalar launch takes
hipError_t launch_keyswitch_wide(const KeyswitchLaunch &a, hipStream_t s);
bool keyswitch_scalar_supported(int base_log, int level);
// int8-MFMA keyswitch: KSK repacked once into 8 byte planes (ks_mfma_cols x ks_mfma_rows each)
bool ks_mfma_supported(int in_dim, int level, int base_log);
size_t ks_mfma_rows(int in_dim, int level);
size_t ks_mfma_cols(int out_dim);
size_t ks_mfma_scratch_bytes(int in_dim, int level, int count);
hipError_t launch_ksk_repack(const uint64_t *ksk, int8_t *kt, int in_dim, int level, int out_dim, hipStream_t s);
hipError_t launch_keyswitch_mfma(const KeyswitchLaunch &a, const int8_t *kt, void *scratch, hipStream_t s);

// Private functional packing keyswitch with every key of a pfpksk list (pfpks.hip):
//   glwe_out[c][g][j] = - sum_{i < in_rows} sum_{lvl} digit_lvl(lwe_in[c][i]) * key[g][i][lvl-1][j]
// the input body (i = kN) is decomposed like the mask words and nothing is added to the output.
struct PfpksLaunch {
    const uint64_t *lwe_in;  // [count][in_rows]
    uint64_t *glwe_out;      // [count][ncols]
    const uint64_t *key;     // [k+1][in_rows][level][glwe], level 1 first (the reference's order)
    int in_rows;             // kN + 1
    int glwe;                // (k+1)N, a multiple of 64
    int ncols;               // (k+1) * glwe
    int base_log, level;     // 1 <= base_log <= 31, base_log * level <= 63
    int count;
};
hipError_t launch_pfpks(const PfpksLaunch &a, hipStream_t s);
// int8-MFMA form (base_log <= 15): key repacked once into 8 byte planes (pfpks_mfma_cols x pfpks_mfma_rows each)
bool pfpks_mfma_supported(int in_rows, int level, int base_log);
size_t pfpks_mfma_rows(int in_rows, int level);
size_t pfpks_mfma_cols(int ncols);
size_t pfpks_mfma_scratch_bytes(int in_rows, int level, int count);
hipError_t launch_pfpksk_repack(const uint64_t *key, int8_t *kt, int keys, int in_rows, int level, int glwe,
                                hipStream_t s);
hipError_t launch_pfpks_mfma(const PfpksLaunch &a, const int8_t *kt, void *scratch, hipStream_t s);

// elementwise glue of bit extraction and circuit bootstrap (lwe_ops.hip, wop_pbs/mod.rs:158-224, 369-444)
//   shift_rows: dst[r][w] = (src[r / reps][w] << shift) + (w == words - 1 ? body_add : 0), dst rows dst_stride apart
//   add_body:   buf[r][words - 1] += 2^(first - step * (r % mod))
//   sub_rows:   cur[r][w] -= x[r][w] + (w == words - 1 ? body_add : 0)
//   fill_luts:  luts[l] = trivial GLWE whose body is all -2^(first - step * l); lut_indexes[r] = r % nluts
hipError_t launch_wop_shift_rows(uint64_t *dst, const uint64_t *src, size_t rows, size_t words, size_t dst_stride,
                                 size_t reps, int shift, uint64_t body_add, hipStream_t s);
hipError_t launch_wop_add_body(uint64_t *buf, size_t rows, size_t words, int first, int step, size_t mod,
                               hipStream_t s);
hipError_t launch_wop_sub_rows(uint64_t *cur, const uint64_t *x, size_t rows, size_t words, uint64_t body_add,
                               hipStream_t s);
hipError_t launch_wop_fill_luts(uint64_t *luts, size_t nluts, size_t glwe, size_t body_off, int first, int step,
                                uint32_t *lut_indexes, size_t rows, hipStream_t s);

// words[0, n) = 0 on the stream (lwe_ops.hip).  The launchers reset their ticket and flag words in the
// caller's scratch with this kernel and not with hipMemsetAsync: captured into a hipGraph, the memset node
// zeroes all its words on the first replay only (tests/test_async_graph_gpu.py, classic-1024-pbs-1100: the
// second replay found its ticket as the previous contents of the scratch left it; a bare memset -> kernel
// graph shows the same on an MI355X: of 4 bytes none, of 1792 and of 65536 bytes three quarters are zeroed
// from the second replay on), while kernel nodes run in stream order on every replay.
hipError_t launch_zero_words(uint32_t *words, size_t n, hipStream_t s);

// batched LWE linear algebra / trivial PBS (lwe_ops.hip)
hipError_t launch_torus_from_fraction(const double *fr, uint64_t *acc, uint64_t *set, size_t n, hipStream_t s);
hipError_t launch_lwe_scalar_mul_add(uint64_t *y, const uint64_t *x, uint64_t scalar, size_t rows, size_t words,
                                     size_t y_stride, size_t x_stride, hipStream_t s);
hipError_t launch_trivial_pbs(uint64_t *body, size_t rows, size_t stride, const uint64_t *lut_body, uint64_t delta,
                              uint64_t modulus_sup, uint64_t box, hipStream_t s);

// One layer of block arithmetic (lwe_ops.hip lwe_block_layer_kernel): for every op, r < rows, w < words
//   dst[r][w] = sum_t scalar_t * src_t[r][w] + (w == words - 1 ? body_add : 0)   (wrapping; src == nullptr: absent).
// The layout is TfheMi355BlockOp's (include/tfhe_mi355.h; capi.cpp asserts it).  `ops` is host memory, copied
// into the kernel arguments before the call returns: BLOCK_LAYER_OPS_PER_LAUNCH entries of 120 bytes stay under
// the 4 KiB of kernel arguments, longer lists take several launches.  No allocation, no copy, no wait.
constexpr int BLOCK_LAYER_TERMS = 4;
constexpr int BLOCK_LAYER_OPS_PER_LAUNCH = 32;
constexpr size_t BLOCK_LAYER_MAX_WORKGROUPS = 2048;
struct BlockLayerOp {
    uint64_t *dst;
    uint64_t dst_stride;
    uint64_t body_add;
    struct {
        const uint64_t *src;
        uint64_t stride;
        uint64_t scalar;
    } term[BLOCK_LAYER_TERMS];
};
hipError_t launch_lwe_block_layer(const BlockLayerOp *ops, size_t n_ops, size_t rows, size_t words, hipStream_t s);

// The block layer with a clear digit per row (lwe_ops.hip lwe_clear_block_layer_kernel): the plain op, and per row
//   digit(r) = ((negate ? 0 - d_clear[r] : d_clear[r]) >> clear_shift) & (2^clear_bits - 1)    (d_clear == nullptr: 0)
//   dst[r][words - 1] += digit(r) * clear_scale,   d_lut_index[r] = lut_base + digit(r)        (where not nullptr).
// A clear operand of a radix op reaches a PBS layer as a plaintext on the body or as the choice of a LUT out of a
// family; read per row from the device, neither is part of the op table, so one table (and one captured graph of
// it) serves any clear operands.  The layout is TfheMi355ClearBlockOp's (capi.cpp asserts it).  The entries per
// launch follow from the entry's size, so the table and the three row counts stay under the 4 KiB of kernel
// arguments.  No allocation, no copy, no wait; the launcher does not check the fields (the entry point does).
struct ClearBlockLayerOp {
    BlockLayerOp op;
    const uint64_t *d_clear;
    uint64_t clear_scale;
    uint32_t *d_lut_index;
    uint32_t clear_negate;
    uint32_t clear_shift;
    uint32_t clear_bits;
    uint32_t lut_base;
};
constexpr int CLEAR_BLOCK_LAYER_MAX_BITS = 8;
constexpr int CLEAR_BLOCK_LAYER_OPS_PER_LAUNCH = (int)((4096 - 3 * sizeof(uint32_t)) / sizeof(ClearBlockLayerOp));
hipError_t launch_lwe_clear_block_layer(const ClearBlockLayerOp *ops, size_t n_ops, size_t rows, size_t words,
                                        hipStream_t s);

// GLWE x plaintext-polynomial products (glwe_ops.hip):
//   out[c][i] = sum_{j<J} glwe_in[c][j] * polys[i][j]   in (Z/2^64)[X]/(X^N+1), per GLWE polynomial,
// optionally sample-extracted at degree 0.  Serves the fork's MVB products v0 * v_i
// (gadget/engine/bootstrapping.rs:567-620) and the window sums of the tree-bootstrapping packing
// (:690-773).  Cost scales with the polys' nonzero count.
struct GlwePolyMulLaunch {
    const uint64_t *glwe_in;  // [count][J][(k+1)N]
    const uint64_t *polys;    // [npoly][J][N]
    uint64_t *out;            // [count][npoly][(k+1)N], or [count][npoly][kN+1] when extract
    int k, N, J, npoly;
    size_t count;
    bool extract;
};
hipError_t launch_glwe_poly_mul(const GlwePolyMulLaunch &a, hipStream_t s);

// GLWE x GLWE product with relinearisation (glwe_mult.hip; the fork's glwe_mult,
// custom_glwe_glwe_product.rs:13-321), per pair c:
//   tensor kernel: both GLWEs shifted right by 32 - log_p/2, then with (A, B), (A', B') their masks and bodies
//     out.mask_i = A_i B' + A'_i B,  out.body = B B',  tr[n(i,i)] = A_i A'_i,  tr[n(i,j)] = A_i A'_j + A_j A'_i
//     (j < i, n(i,j) = i(i+1)/2 + j), negacyclic products over Z/2^64;
//   relinearisation kernel: out_q += sum_n sum_l digit_l(tr[n]) * rlk[n][l][q], digit 0 = level L (the key's
//     first GLWE per block), SignedDecomposer(base_log, level).
// extract: out holds the degree-0 sample of the result, [count][kN+1] (of the body only coefficient 0
// is computed).
struct GlweMultLaunch {
    const uint64_t *lhs, *rhs;  // [count][(k+1)N]
    uint64_t *out;              // [count][(k+1)N], or [count][kN+1] when extract
    uint64_t *tr;               // scratch [count][k(k+1)/2][N] (glwe_mult_scratch_bytes)
    const uint64_t *rlk;        // [k(k+1)/2][level][(k+1)N], the reference's layout
    int k, N;
    int log_p;                  // even, 0..64
    int base_log, level;        // 1 <= base_log <= 31, base_log * level <= 63
    int extract;
    size_t count;
    KernelTimer *timer = nullptr;
};
// N a power of two in [256, 2048], 1 <= k <= 5, (k+1) N <= 4096
bool glwe_mult_supported(int N, int k);
size_t glwe_mult_scratch_bytes(int N, int k, size_t count);
hipError_t launch_glwe_mult(const GlweMultLaunch &a, hipStream_t s);

// Batched GGSW x GLWE nodes (ggsw_ops.hip): out = base + G (x) d per node, every node with its own
// Fourier GGSW and the decomposition (base_log, level; base_log * level <= 32) of the call.
//   GGSW_EP    d = in1 (glwe_in), base = out (accumulated)      add_external_product_assign
//   GGSW_CMUX  d = in1 - in0, base = in0 (out == in0 allowed)    cmux
//   GGSW_ROT   d = in0 / X^rot - in0, base = in0                 one step of blind_rotate_assign (wop_pbs)
// Node nd belongs to item nd / nodes_per_item and uses GGSW (block(item) * ggsw_per_item + ggsw_sel)
// with block(item) = ggsw_indexes[item] (clamped to ggsw_blocks - 1) or item.  Its operands sit at
// in0 / in1 + nd * in_stride words, its output at out + nd * (k+1)N (or nd * (kN+1) when extract:
// degree-0 sample extraction of the result).  leaf: the operands are trivial GLWEs (zero mask) whose
// bodies are polynomials of the item's LUT, in0 = luts [lut_count][nout][npoly][N]: polynomials 2s, 2s+1
// of output o for node s of the item (CMUX), polynomial s (ROT).
// nout > 1 adds an output dimension between the item and its nodes: node nd is node nd % nodes_per_item
// of output (nd / nodes_per_item) % nout of item nd / (nodes_per_item nout); the GGSW depends on the
// item alone, the leaves of output o are read in place from the LUT's slice o.
// chain > 0 (GGSW_ROT, nodes_per_item 1): the node runs `chain` rotation steps in the one launch, step i
// under GGSW ggsw_sel - i with degree rot << i, then writes out / extracts as a single step does after
// the last; acc [nodes][(k+1)N] holds the running accumulators (it may be in0 when not leaf).
enum GgswMode { GGSW_EP = 0, GGSW_CMUX = 1, GGSW_ROT = 2 };
struct GgswCmuxLaunch {
    const double2 *fggsw;          // [ggsw_blocks][ggsw_per_item][L][k+1][k+1] polys, engine Fourier layout
    const uint32_t *ggsw_indexes;  // [items] or null
    size_t ggsw_blocks;
    int ggsw_per_item, ggsw_sel;
    const uint64_t *in0, *in1;
    uint64_t *out;
    const uint32_t *lut_indexes;   // leaf: [items] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    int npoly;                     // leaf: polynomials per LUT
    int mode, leaf, rot, extract;
    int nout = 1;                  // outputs per item (LUT slices under one set of GGSWs)
    int chain = 0;                 // rotation steps run inside the launch (0: one plain node)
    uint64_t *acc = nullptr;       // chain: the nodes' accumulator slots
    size_t nodes, nodes_per_item;
    size_t in_stride;
    int base_log, level;
    const double2 *W, *twist;
};
bool ggsw_ops_supported(int N, int k);
hipError_t launch_ggsw_cmux(int N, int k, const GgswCmuxLaunch &a, hipStream_t s);

// ---- 32-bit torus (the reference's boolean module: pbs_classic32.hip, keyswitch32.hip, boolean_ops.hip) ----
struct ClassicPbs32Launch {
    const uint32_t *lwe_in;      // [count][n+1]
    uint32_t *lwe_out;           // [count][k*N+1], or [count][(k+1)N] when glwe_out
    const uint32_t *luts;        // [lut_count][(k+1)*N]
    const uint32_t *lut_indexes; // [count] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    const double2 *fbsk;         // engine Fourier layout (of the key widened to u64)
    const double2 *W, *twist;
    int n;
    int base_log;                // 2 <= base_log, base_log * L <= 30
    int count;
    int glwe_out;
};
bool classic_pbs32_supported(int N, int k, int L);
// workgroups (= ciphertexts) of the shape's kernel resident at once on the current device
int classic_pbs32_resident_blocks(int N, int k, int L);
hipError_t launch_classic_pbs32(int N, int k, int L, const ClassicPbs32Launch &a, hipStream_t s);
// out[e] = (uint64_t)in[e] << 32: the u32 standard BSK as launch_bsk_to_fourier reads it
hipError_t launch_widen32(const uint32_t *in, uint64_t *out, size_t n, hipStream_t s);

struct Keyswitch32Launch {
    const uint32_t *lwe_in;  // [count][in_dim+1]
    uint32_t *lwe_out;       // [count][out_dim+1]
    const uint32_t *ksk;     // [in_dim][level][out_dim+1]
    int in_dim, out_dim, base_log, level;  // base_log * level <= 30
    int count;
};
// plain integer arm: 1 <= base_log <= 15, level <= 16
bool keyswitch32_scalar_supported(int base_log, int level);
hipError_t launch_keyswitch32(const Keyswitch32Launch &a, hipStream_t s);
// int8-MFMA arm: KSK repacked once into 4 byte planes (ks_mfma_cols x ks_mfma_rows each)
bool ks32_mfma_supported(int in_dim, int level, int base_log);
size_t ks32_mfma_scratch_bytes(int in_dim, int level, int count);
hipError_t launch_ksk32_repack(const uint32_t *ksk, int8_t *kt, int in_dim, int level, int out_dim, hipStream_t s);
hipError_t launch_keyswitch32_mfma(const Keyswitch32Launch &a, const int8_t *kt, void *scratch, hipStream_t s);

// linear parts of the boolean gates (boolean_ops.hip; boolean/engine/mod.rs:461-837), mod 2^32:
//   gates:        out[i] = s(op[i]) (lhs[i] + rhs[i]) + (0, ..., 0, c(op[i]))
//   mux prologue: out[2i] = cond[i] + then[i] + (0.., F), out[2i+1] = -cond[i] + else[i] + (0.., F)
//   mux epilogue: out[i] = in[2i] + in[2i+1] + (0.., T)
//   negate:       out[i] = -in[i]
// an opcode above 5 (refused by the host-pointer entry point) writes a row of zeros
hipError_t launch_bool_gates_prologue(const uint8_t *ops, const uint32_t *lhs, const uint32_t *rhs, uint32_t *out,
                                      size_t count, size_t words, hipStream_t s);
hipError_t launch_bool_mux_prologue(const uint32_t *cond, const uint32_t *then_, const uint32_t *else_, uint32_t *out,
                                    size_t count, size_t words, hipStream_t s);
hipError_t launch_bool_mux_epilogue(const uint32_t *in, uint32_t *out, size_t count, size_t words, hipStream_t s);
hipError_t launch_bool_negate(const uint32_t *in, uint32_t *out, size_t total, hipStream_t s);
hipError_t launch_torus32_from_fraction(const double *fr, uint32_t *acc, uint32_t *set, size_t n, hipStream_t s);

// ---- 128-bit torus (the reference's fft128 path: pbs_f128.hip, dd_device.h, fft128_tables.cpp) ----
// A u128 word is two little-endian uint64_t (low, high), as unsigned __int128 on host and device.
struct PbsF128Launch {
    const unsigned __int128 *lwe_in;   // [count][n+1]
    unsigned __int128 *lwe_out;        // [count][k*N+1], or [count][(k+1)N] when glwe_out
    const unsigned __int128 *luts;     // [lut_count][(k+1)*N]
    const uint32_t *lut_indexes;       // [count] or null; entries >= lut_count read LUT lut_count-1
    uint32_t lut_count;
    const double *fbsk;                // [n][level][k+1][k+1][4][M]: planes re.hi, re.lo, im.hi, im.lo
    const double *twist, *tw;          // [4][M] exp(i pi j / N), [4][M/2] exp(-2 pi i t / M)
    uint32_t *degrees;                 // scratch [count][n+1]: the modulus-switched input words
    int n;
    int base_log, level;               // 2 <= base_log <= 31, level <= 4, base_log * level < 128
    int modulus_log;                   // 65..128 (128 = native)
    int count;
    int glwe_out;
};
bool pbs_f128_supported(int N, int k);
// workgroups (= ciphertexts) of the shape's kernel resident at once on the current device
int pbs_f128_resident_blocks(int N, int k);
hipError_t launch_pbs_f128(int N, int k, const PbsF128Launch &a, hipStream_t s);
// standard u128 key polynomials [npoly][N] -> Fourier planes [npoly][4][M]
hipError_t launch_bsk128_to_fourier(int N, const void *d_bsk, double *d_fbsk, size_t npoly, const double *twist,
                                    const double *tw, hipStream_t s);
// out[i] = acc[i] (0 when null) + backward conversion of the fraction (hi[i], lo[i])
hipError_t launch_torus128_from_f128(const double *hi, const double *lo, const void *acc, void *out, size_t n,
                                     hipStream_t s);
// Canonical host tables (fft128_tables.cpp): every entry hi = RN(x), lo = RN(x - hi) of the exact real x,
// computed in 256-bit fixed point.  twist: 4 planes of N/2 (cos, sin of pi j / N as re.hi, re.lo, im.hi,
// im.lo); twiddles: 4 planes of N/4 (exp(-2 pi i t / (N/2))).
void fft128_host_tables(int N, double *twist, double *twiddles);

// seeded-key decompression (csprng.hip): AES-CTR mask stream of the compression seed written as
// `row_words` mask words per row, followed by `body_words` copied from d_bodies, for `rows` rows
size_t aes_tables_bytes();
void aes_tables_build(uint64_t seed_lo, uint64_t seed_hi, void *host_tables);
void aes128_encrypt_host(const void *host_tables, uint32_t s[4]);
hipError_t launch_seeded_decompress(const void *d_tables, const uint64_t *d_bodies, size_t rows, size_t row_words,
                                    size_t body_words, uint64_t *d_out, hipStream_t s);
// the same for rows [first_row, first_row + rows) of the entity (d_bodies and d_out are those rows')
hipError_t launch_seeded_decompress_from(const void *d_tables, const uint64_t *d_bodies, size_t first_row, size_t rows,
                                         size_t row_words, size_t body_words, uint64_t *d_out, hipStream_t s);

// compressed ciphertext ingress (lwe_ingress.hip): LWE rows of n + 1 words written from a compact list or
// from seeded ciphertexts.  d_base_tables: AES tables of any seed (their Te0 and S-box are read).
// rows [first, first + count) of the compact list whose bin masks are d_masks[bin][n]; d_bodies and d_out
// are those rows'
hipError_t launch_lwe_compact_expand(const uint64_t *d_masks, const uint64_t *d_bodies, size_t n, size_t first,
                                     size_t count, uint64_t *d_out, hipStream_t s);
// the tables of the seed {lo, hi} at d_seed, written to d_tables (aes_tables_bytes())
hipError_t launch_aes_schedule(const void *d_base_tables, const uint64_t *d_seed, void *d_tables, hipStream_t s);
// row r: mask = stream bytes [1, 1 + 8n) of the seed d_seeds[2r], d_seeds[2r + 1]; body = d_bodies[r]
hipError_t launch_csprng_rows(const void *d_base_tables, const uint64_t *d_seeds, const uint64_t *d_bodies, size_t n,
                              size_t count, uint64_t *d_out, hipStream_t s);

}  // namespace tfhe_mi355
