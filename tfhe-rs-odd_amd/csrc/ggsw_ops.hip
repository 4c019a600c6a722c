// ggsw_ops.hip -- batched GGSW x GLWE external product, CMUX and the CMUX nodes of vertical packing
// on gfx950, with one Fourier GGSW per node and a decomposition chosen per call.
//
// Replaces (reference tfhe-rs-odd, CPU Rust):
//   add_external_product_assign / update_with_fmadd   fft64/crypto/ggsw.rs:477-697
//   cmux                                              fft64/crypto/ggsw.rs:766-777
//   cmux_tree_memory_optimized                        fft64/crypto/wop_pbs/mod.rs:468-592
//   blind_rotate_assign (by GGSWs)                    fft64/crypto/wop_pbs/mod.rs:866-892
//   polynomial_wrapping_monic_monomial_div            algorithms/polynomial_algorithms.rs:219-282
//   extract_lwe_sample_from_glwe_ciphertext (deg 0)   algorithms/glwe_sample_extraction.rs:91-147
//
// Design: one node is out = base + G (x) d with d = glwe_in (external product),
// ct1 - ct0 (CMUX) or ct0 / X^r - ct0 (rotation step; the monomial division is done on the loads).
// As in pbs_classic_kernel a node is computed by (k+1) wavefronts, one per GLWE polynomial: wave r
// decomposes polynomial r of d (32-bit states, base_log * level <= 32), and per level -- a runtime
// loop, levels L..1 -- twists and forward-FFTs its digits, publishes the row spectrum in LDS under
// GroupSync, and accumulates output column c = r: sum over rows of F_row * G[lvl][row][c]
// (update_with_fmadd order: the first term a plain product, the others fma chains).  One inverse
// FFT per column, backward conversion added onto the base polynomial.  The Fourier GGSW carries the
// 1/M (launch_bsk_to_fourier) and is streamed from global memory, 16 B per lane, read once.
// A workgroup holds SLOTS independent nodes ((k+1) SLOTS waves) that share the twiddle and twist
// tables in LDS; the grid is persistent over the nodes of a launch (stride gridDim.x * SLOTS).
#include <algorithm>
#include <cstdlib>

#include "engine.h"
#include "pbs_common.h"

namespace tfhe_mi355 {

template <int N, int K>
struct GgswConfig {
    static constexpr int M = N / 2;
    // nodes per workgroup: up to 8 waves (2 per SIMD: every shape stays under 256 VGPRs, no scratch)
    // within a CU's LDS
    static constexpr int slots_fit(int s) {
        return s <= 1 ? 1 : (PbsLds<M>::bytes((K + 1) * s) + 4 * (K + 1) * s <= 160 * 1024 ? s : slots_fit(s - 1));
    }
    static constexpr int SLOTS = slots_fit(8 / (K + 1));
    // MAC slots per scheduling region: bounds the GGSW and spectrum loads in flight ((k+1) pairs each)
    static constexpr int MAC_GROUP = K >= 4 ? 1 : K >= 2 ? 2 : 4;
    static constexpr size_t flags_off() { return PbsLds<M>::bytes((K + 1) * SLOTS); }
    static constexpr size_t lds_bytes() { return flags_off() + 4 * (K + 1) * SLOTS; }
    static_assert(lds_bytes() <= 160 * 1024, "LDS per workgroup exceeds a CU");
};

// One signed digit of the 32-bit decomposer (decomp_digit32, pbs_common.h) as a double, for every
// base_log <= 32 without a branch: the shifts by base_log are taken mod 32 and masked to 0 when
// base_log = 32 (one level: the state is the digit).  A digit lies in (-2^(beta-1), 2^(beta-1)], so
// its 32-bit image is 0x80000000 only for +2^31 at base_log = 32, which the int32 conversion would
// turn into -2^31.
struct GgswDigit {
    uint32_t mask, keep;  // 2^beta - 1; all ones, or 0 when beta = 32
    int sh, shc;          // beta mod 32, beta - 1
    __device__ __forceinline__ explicit GgswDigit(int beta)
        : mask(beta == 32 ? 0xffffffffu : (1u << beta) - 1), keep(beta == 32 ? 0u : 0xffffffffu), sh(beta & 31),
          shc(beta - 1) {}
    __device__ __forceinline__ double operator()(uint32_t &state) const {
        const uint32_t res = state & mask;
        state = (state >> sh) & keep;
        uint32_t carry = ((res - 1) | state) & res;
        carry >>= shc;
        state += carry;
        const uint32_t x = res - ((carry << sh) & keep);
        return x == 0x80000000u ? 0x1p31 : (double)(int32_t)x;
    }
};

// CHAIN: a node is one (item, output) and runs a.chain rotation steps back to back (GGSW ggsw_sel - i,
// degree rot << i), each the single node op for op; between steps a wave's polynomial stays with the
// wave (its LDS exchange buffer holds it for the next step's loads, the node's global accumulator slot
// a.acc for the base the product is added onto: every lane writes and reads its own positions).
template <int N, int K, bool CHAIN>
__global__ void __launch_bounds__((64 * (K + 1) * GgswConfig<N, K>::SLOTS)) ggsw_cmux_kernel(GgswCmuxLaunch a) {
    constexpr int M = N / 2;
    constexpr int V = M / 64;
    using Cfg = GgswConfig<N, K>;
    using Fft = WaveFft<M>;
    using Lay = PbsLds<M>;
    constexpr int XL = Lay::XL;
    static_assert(sizeof(cx) * XL >= sizeof(uint64_t) * N, "exchange buffer holds one polynomial");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *lds = reinterpret_cast<double2 *>(smem);
    const double2 *s_twist = lds + Lay::twist_off;

    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    const int wave = wid % (K + 1);  // polynomial of the node this wave owns
    const int slot = wid / (K + 1);  // node slot in the workgroup
    const int beta = a.base_log, L = a.level;
    const GgswDigit digit(beta);
    const int sshift = 63 - beta * L;  // >= 31
    BlockSync sync;
    WaveLocalSync wsync;

    for (int e = threadIdx.x; e < M; e += blockDim.x) lds[Lay::twist_off + e] = a.twist[e];
    uint32_t *gflags = reinterpret_cast<uint32_t *>(smem + Cfg::flags_off());
    if (threadIdx.x < (K + 1) * Cfg::SLOTS) gflags[threadIdx.x] = 0;
    Fft::Lds::template fill<M>(lds + Lay::s1_off, lds + Lay::s2_off, a.W, threadIdx.x, blockDim.x);
    const typename Fft::Lds tw{lds + Lay::s1_off, lds + Lay::s2_off};
    sync();  // tables visible to every wave (the node loop only syncs within a slot)

    cx *xct = reinterpret_cast<cx *>(lds + Lay::xbuf_off) + (size_t)slot * (K + 1) * XL;  // this slot's buffers
    GroupSync<K + 1> xsync{lds_addr(gflags + slot * (K + 1)), lds_addr(gflags + slot * (K + 1) + wave)};
    cx *xb = xct + wave * XL;
    uint64_t *xb64 = reinterpret_cast<uint64_t *>(xb);
    const double k32 = torus_k32();
    const size_t glwe = (size_t)(K + 1) * N;
    const size_t ggsw_len = (size_t)L * (K + 1) * (K + 1) * M;

    // the slots of a workgroup never wait on each other (GroupSync is per slot)
    for (size_t nd = (size_t)blockIdx.x * Cfg::SLOTS + slot; nd < a.nodes; nd += (size_t)gridDim.x * Cfg::SLOTS) {
        // nodes run (item, output, node of the item's tree level); the GGSW is chosen by the item alone
        const size_t io = nd / a.nodes_per_item, sub = nd % a.nodes_per_item;
        const size_t item = io / a.nout, o = io % a.nout;
        size_t gi = a.ggsw_indexes ? min((size_t)a.ggsw_indexes[item], a.ggsw_blocks - 1) : item;
        const int nsteps = CHAIN ? a.chain : 1;  // a single node is a chain of one step
#pragma unroll 1
        for (int step = 0; step < nsteps; step++) {
            const bool carried = CHAIN && step > 0;  // the operand is the step before's result
            // this node's GGSW as a buffer resource: wave-uniform base, per-lane byte offset 16 lane, the
            // (level, row, column, slot) part of the address in an SGPR offset -- no per-load VALU
            // address arithmetic and no lane-derived 64-bit addresses for the compiler to hoist and spill
            const __amdgpu_buffer_rsrc_t grs =
                make_rsrc(a.fggsw + (gi * a.ggsw_per_item + (a.ggsw_sel - step)) * ggsw_len);

            // operands of this wave's polynomial.  Leaves are trivial GLWEs of LUT polynomials: zero
            // mask, body = polynomial (2 sub, 2 sub + 1) of the item's LUT (CMUX) or polynomial sub
            const bool zero = a.leaf && wave < K && !carried;
            const uint64_t *p0, *p1;
            if (a.leaf) {
                const size_t li = a.lut_indexes ? min(a.lut_indexes[item], a.lut_count - 1u) : 0u;
                p0 = a.in0 + ((li * a.nout + o) * a.npoly + (a.mode == GGSW_CMUX ? 2 * sub : sub)) * N;
                p1 = p0 + N;
            } else {
                p0 = a.in0 + nd * a.in_stride + (size_t)wave * N;
                p1 = a.in1 + nd * a.in_stride + (size_t)wave * N;
            }
            // the polynomial the product is added onto: glwe_inout (external product), else ct0
            uint64_t *slot = CHAIN ? a.acc + nd * glwe + (size_t)wave * N : nullptr;
            const uint64_t *pb = carried ? slot : a.mode == GGSW_EP ? a.out + nd * glwe + (size_t)wave * N : p0;
            const bool bzero = a.mode != GGSW_EP && zero;

            // decomposer states of d = s xa - xb at positions lane + 64 h (h < V: j < M; h >= V: j + M),
            // branch-free over the modes: xa = glwe_in / ct1 / ct0 at position j + rot (rot = 0 unless a
            // rotation step: (p / X^r)[j] = p[j + r], negated once j + r wraps past N), xb = ct0 or 0
            const uint64_t *pa = a.mode == GGSW_ROT ? p0 : p1;
            const uint64_t *ps = a.mode == GGSW_EP ? p1 : p0;  // (always a readable address)
            const uint64_t ma = zero ? 0 : ~0ull, ms = (zero || a.mode == GGSW_EP) ? 0 : ~0ull;
            const int rot = a.mode == GGSW_ROT ? a.rot << step : 0;
            // per-node opaque copy of the lane id: lane-derived addresses are recomputed per node (and
            // per level below) instead of being hoisted out of the loops, where they pin registers
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            uint32_t st[2 * V];
            if (carried) {
#pragma unroll
                for (int h = 0; h < 2 * V; h++) {
                    const int pos = lane + 64 * h, src = pos + rot;
                    const uint64_t xa = xb64[src & (N - 1)];
                    const uint64_t d = (src >= N ? 0 - xa : xa) - xb64[pos];
                    st[h] = (uint32_t)(((d >> sshift) + 1) >> 1);
                }
                wsync();  // the loads of the carried polynomial precede the forward FFT's reuse of the buffer
            } else {
#pragma unroll
                for (int h = 0; h < 2 * V; h++) {
                    const int pos = lane + 64 * h, src = pos + rot;
                    const uint64_t xa = pa[src & (N - 1)] & ma;
                    const uint64_t d = (src >= N ? 0 - xa : xa) - (ps[pos] & ms);
                    st[h] = (uint32_t)(((d >> sshift) + 1) >> 1);
                }
            }

            // The accumulator starts at +0 and every term is an fma chain.  update_with_fmadd writes the
            // first term as a plain product instead: fma(-gi, di, +0) is -(gi di) rounded once, the same
            // value, and only the sign of a zero can differ, which no later operation observes
            cx acc[V];
#pragma unroll
            for (int s = 0; s < V; s++) acc[s] = cx{0.0, 0.0};
#pragma unroll 1
            for (int lvl = L; lvl >= 1; lvl--) {
                cx v[V];
                int lane = lane0;
                asm volatile("" : "+v"(lane));
#pragma unroll
                for (int b = 0; b < V; b++) {
                    const cx z = {digit(st[b]), digit(st[V + b])};
                    const double2 w = s_twist[lane + 64 * b];
                    v[b] = cmulw(z, w.x, w.y);  // convert_forward_integer (x86.rs:505-596)
                }
                Fft::forward(v, xb, tw, lane, wsync);
                wsync();
#pragma unroll
                for (int s = 0; s < V; s++)
                    reinterpret_cast<double2 *>(xb)[s * 64 + lane] = make_double2(v[s].re, v[s].im);
                xsync();  // the node's row spectra are published
                // output column c = wave: sum_r F_r * G[lvl][r][c]   (ggsw.rs:524-567, update_with_fmadd)
                const uint32_t lm = (uint32_t)(((lvl - 1) * (K + 1) * (K + 1) + wave) * M) * 16u;
#pragma unroll
                for (int s = 0; s < V; s++) {
                    if (s % Cfg::MAC_GROUP == 0) __builtin_amdgcn_sched_barrier(0);
                    cx o = acc[s];
#pragma unroll
                    for (int r = 0; r <= K; r++) {
                        const double2 gg =
                            buffer_ld_d2(grs, 16u * lane, lm + (uint32_t)(r * (K + 1) * M + s * 64) * 16u);
                        const double2 ff = reinterpret_cast<const double2 *>(xct + r * XL)[s * 64 + lane];
                        o.re = fma(gg.x, ff.x, fma(-gg.y, ff.y, o.re));
                        o.im = fma(gg.x, ff.y, fma(gg.y, ff.x, o.im));
                    }
                    acc[s] = o;
                }
                xsync();  // every wave of the node is done reading the published spectra
            }
            asm volatile("" : "+v"(lane));
            Fft::inverse(acc, xb, tw, lane, wsync);

            const uint64_t mb = bzero ? 0 : ~0ull;
            uint64_t c[2 * V];
#pragma unroll
            for (int b = 0; b < V; b++) {
                c[b] = pb[lane + 64 * b] & mb;
                c[V + b] = pb[M + lane + 64 * b] & mb;
                const double2 w = s_twist[lane + 64 * b];  // the Fourier GGSW carries the 1/M
                backward_add(acc[b], cx{w.x, w.y}, c[b], c[V + b], k32);
            }
            if (CHAIN && step + 1 < nsteps) {
                wsync();
#pragma unroll
                for (int h = 0; h < 2 * V; h++) {
                    xb64[lane + 64 * h] = c[h];
                    slot[lane + 64 * h] = c[h];
                }
                wsync();
            } else if (!a.extract) {
                uint64_t *o = a.out + nd * glwe + (size_t)wave * N;
#pragma unroll
                for (int h = 0; h < 2 * V; h++) o[lane + 64 * h] = c[h];
            } else {
                // sample extract at degree 0 (glwe_sample_extraction.rs:91-147): out[0] = a[0],
                // out[j] = -a[N - j] per mask polynomial, body = b[0]
                wsync();
#pragma unroll
                for (int h = 0; h < 2 * V; h++) xb64[lane + 64 * h] = c[h];
                wsync();
                uint64_t *o = a.out + nd * (size_t)(K * N + 1);
                if (wave < K) {
                    for (int j = lane; j < N; j += 64) o[wave * N + j] = j == 0 ? xb64[0] : 0 - xb64[N - j];
                } else if (lane == 0) {
                    o[K * N] = c[0];
                }
                wsync();  // the extract's reads of xb64 precede the next node's FFT writes
            }
        }
    }
}

// test hook: TFHE_MI355_GGSW_GRID=<n>, read at every launch, caps the workgroups of a GGSW launch so the
// persistent node loop wraps at small node counts (unset or 0: no cap)
static size_t ggsw_grid_cap() {
    const char *e = std::getenv("TFHE_MI355_GGSW_GRID");
    const long v = e && *e ? std::atol(e) : 0;
    return v > 0 ? (size_t)v : ~(size_t)0;
}

template <int N, int K, bool CHAIN>
static hipError_t launch_ggsw_t(const GgswCmuxLaunch &a, hipStream_t s) {
    using Cfg = GgswConfig<N, K>;
    const size_t lds = Cfg::lds_bytes();
    const int threads = 64 * (K + 1) * Cfg::SLOTS;
    const size_t want = (a.nodes + Cfg::SLOTS - 1) / Cfg::SLOTS;
    const int res = resident_blocks((const void *)ggsw_cmux_kernel<N, K, CHAIN>, threads, lds);
    const unsigned blocks = (unsigned)std::min(std::min<size_t>(want, (size_t)res), ggsw_grid_cap());
    hipLaunchKernelGGL((ggsw_cmux_kernel<N, K, CHAIN>), dim3(blocks), dim3(threads), lds, s, a);
    return hipGetLastError();
}

bool ggsw_ops_supported(int N, int k) {
    return (N == 256 || N == 512 || N == 1024 || N == 2048) && k >= 1 && k <= 5;
}

hipError_t launch_ggsw_cmux(int N, int k, const GgswCmuxLaunch &a, hipStream_t s) {
    if (a.nodes == 0) return hipSuccess;
    if (!ggsw_ops_supported(N, k) || a.level < 1 || a.base_log < 1 || a.base_log * a.level > 32 ||
        a.nodes_per_item == 0 || a.nout < 1 || a.ggsw_blocks == 0 || (a.mode == GGSW_ROT && (a.rot < 0 || a.rot >= N)))
        return hipErrorInvalidValue;
    // a chain: rotation steps of degrees rot, 2 rot, ... < N under GGSWs ggsw_sel, ggsw_sel - 1, ... >= 0
    if (a.chain && (a.mode != GGSW_ROT || a.chain < 0 || a.rot < 1 || ((int64_t)a.rot << (a.chain - 1)) >= N ||
                    a.ggsw_sel - (a.chain - 1) < 0 || !a.acc || a.nodes_per_item != 1))
        return hipErrorInvalidValue;
#define GGSW_LAUNCH(n_, k_)                                                              \
    if (N == n_ && k == k_)                                                              \
        return a.chain ? launch_ggsw_t<n_, k_, true>(a, s) : launch_ggsw_t<n_, k_, false>(a, s);
#define GGSW_LAUNCH_N(n_) GGSW_LAUNCH(n_, 1) GGSW_LAUNCH(n_, 2) GGSW_LAUNCH(n_, 3) GGSW_LAUNCH(n_, 4) GGSW_LAUNCH(n_, 5)
    GGSW_LAUNCH_N(256) GGSW_LAUNCH_N(512) GGSW_LAUNCH_N(1024) GGSW_LAUNCH_N(2048)
#undef GGSW_LAUNCH_N
#undef GGSW_LAUNCH
    return hipErrorInvalidValue;
}

}  // namespace tfhe_mi355
