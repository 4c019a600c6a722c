// Check of the classic PBS rotation on a negated accumulator (tfhe-rs-odd_amd/csrc/rot_mask.h, the
// text pbs_classic.hip compiles): for N in {256, 512, 1024, 2048}, every mask target a~ in [0, 2N],
// every lane and every h, the header's hcut / wbits / mbits / gather address and hi32 formula
// applied to n = -p give the top 32 bits of (X^a~ p - p)[lane + 64 h], with X^a~ p - p computed on a
// random p as polynomial_wrapping_monic_monomial_mul_and_subtract defines it
// (polynomial_algorithms.rs:425-490).  Also the hi32 identity itself on random and edge pairs.
//   g++ -O2 -fopenmp scripts/check_rot_mask.cpp -o check_rot_mask && ./check_rot_mask
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tfhe-rs-odd_amd/csrc/rot_mask.h"

using namespace tfhe_mi355;

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// out = X^a p - p (mod X^N + 1, mod 2^64), a in [0, 2N]: the monomial degree is reduced mod 2N,
// a full turn by N flips every sign, then coefficient i moves to i + rem, negated when it wraps.
static void mul_and_subtract(std::vector<uint64_t> &out, const std::vector<uint64_t> &p, int a) {
    const int N = (int)p.size();
    const int d = a % (2 * N);
    const int full = d / N, rem = d % N;
    for (int i = 0; i < N; i++) {
        const int j = i + rem;
        uint64_t v = p[i];
        if (full & 1) v = 0 - v;
        if (j >= N) out[j - N] = (0 - v) - p[j - N];
        else out[j] = v - p[j];
    }
}

int main() {
    long bad = 0;
    uint64_t seed = 2024;

    // the identity hi32(s x - c) = hi32(y + (n ^ M)) ^ m with y = -x, n = -c
    {
        const uint64_t edge[] = {0, 1, 2, (1ull << 63), (1ull << 63) - 1, (1ull << 63) + 1, (1ull << 32) - 1,
                                 (1ull << 32), (1ull << 32) + 1, ~0ull, ~0ull - 1, 0xffffffff00000000ull,
                                 0x00000000ffffffffull, 0x8000000080000000ull, 0x7fffffff7fffffffull};
        const int ne = sizeof(edge) / sizeof(edge[0]);
        long bb = 0;
        auto one = [&](uint64_t x, uint64_t c) {
            for (int sp = 0; sp < 2; sp++) {
                const uint32_t m = sp ? ~0u : 0u;
                const uint64_t T = (sp ? x : 0 - x) - c;
                if (rot_ct1_hi(0 - x, 0 - c, m) != (uint32_t)(T >> 32)) bb++;
            }
        };
        for (int i = 0; i < ne; i++)
            for (int j = 0; j < ne; j++) {
                one(edge[i], edge[j]);
                one(edge[i], edge[i] + edge[j]);  // c = x + small, equal low words
                one(edge[i], edge[i] - edge[j]);
            }
        for (long t = 0; t < 4000000; t++) {
            const uint64_t x = splitmix(seed), c = splitmix(seed);
            one(x, c);
            one(x, (c & 0xffffffff00000000ull) | (uint32_t)x);  // equal low words
        }
        printf("identity mismatches %ld\n", bb);
        bad += bb;
    }

    for (int N = 256; N <= 2048; N *= 2) {
        const int V2 = N / 64;  // 2V coefficients per lane
        std::vector<uint64_t> p(N), nbuf(N);
        for (int i = 0; i < N; i++) {
            p[i] = splitmix(seed);
            nbuf[i] = 0 - p[i];  // the wave's LDS copy of its negated accumulator
        }
        // a few values that stress the carries
        p[0] = 0; p[1] = 1ull << 63; p[2] = ~0ull; p[3] = 1ull << 32; p[N - 1] = 1;
        for (int i : {0, 1, 2, 3, N - 1}) nbuf[i] = 0 - p[i];
        long bb = 0, top = 0;
#pragma omp parallel for reduction(+ : bb, top)
        for (int a = 0; a <= 2 * N; a++) {
            std::vector<uint64_t> ref(N);
            mul_and_subtract(ref, p, a);
            const bool full_odd = (a / N) & 1;  // as the kernel: a = 2N gives full = 2, rem = 0
            const int rem = a % N;
            for (int lane = 0; lane < 64; lane++) {
                const int hcut = rot_hcut(lane, rem);
                if (hcut < 0 || hcut > V2) { bb++; continue; }
                if (hcut == 32) top++;
                const uint32_t wbits = rot_wbits(hcut);
                const uint32_t mbits = rot_mbits(wbits, full_odd);
                for (int h = 0; h < V2; h++) {
                    const int j = lane + 64 * h, jj = j - rem;
                    const bool wrap = rot_wrap(hcut, h);
                    if (wrap != (jj < 0) || wrap != (bool)((wbits >> h) & 1)) { bb++; continue; }
                    const int src = wrap ? jj + N : jj;  // xneg / xpos
                    if (src < 0 || src >= N) { bb++; continue; }
                    const uint32_t m = rot_mask(mbits, h);
                    if (m != (wrap == full_odd ? ~0u : 0u)) { bb++; continue; }
                    if (rot_ct1_hi(nbuf[src], nbuf[j], m) != (uint32_t)(ref[j] >> 32)) bb++;
                }
            }
        }
        for (int h = V2; h < 32; h++)  // bits above 2V are never read; wbits has none of them set
            if (rot_wbits(V2) >> h) bb++;
        printf("N %d mismatches %ld hcut32 %ld\n", N, bb, top);
        bad += bb;
        if (N == 2048 && top == 0) {
            printf("N 2048: the hcut = 2V = 32 case was not reached\n");
            bad++;
        }
    }
    return bad != 0;
}
