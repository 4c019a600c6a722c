// aes_device.h -- the AES-128 block function and table layout of the concrete-csprng AES-CTR generator,
// shared by the .hip files that regenerate seeded masks (csprng.hip: keys; lwe_ingress.hip: ciphertexts).
// T-table form: Te0 and the S-box live in LDS, Te1..Te3 are byte rotations of Te0.  The tables are built once
// on the host (aes_tables_build, csprng.hip); the round keys are expanded on the host for a key's seed and on
// the device (aes128_expand_key) where the seed is device data.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tfhe_mi355 {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// columns packed little-endian: word c = s[4c] | s[4c+1] << 8 | s[4c+2] << 16 | s[4c+3] << 24
__device__ __forceinline__ void aes128_encrypt_block(const uint32_t *__restrict__ rk, const uint32_t *te,
                                                     const uint8_t *sb, uint32_t s[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] ^= rk[c];
#pragma unroll
    for (int round = 1; round < 10; round++) {
        uint32_t t[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            t[c] = te[s[c] & 0xff] ^ rotl32(te[(s[(c + 1) & 3] >> 8) & 0xff], 8) ^
                   rotl32(te[(s[(c + 2) & 3] >> 16) & 0xff], 16) ^ rotl32(te[s[(c + 3) & 3] >> 24], 24) ^
                   rk[4 * round + c];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = t[c];
    }
    uint32_t t[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        t[c] = ((uint32_t)sb[s[c] & 0xff] | ((uint32_t)sb[(s[(c + 1) & 3] >> 8) & 0xff] << 8) |
                ((uint32_t)sb[(s[(c + 2) & 3] >> 16) & 0xff] << 16) | ((uint32_t)sb[s[(c + 3) & 3] >> 24] << 24)) ^
               rk[40 + c];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = t[c];
}

struct AesTables {
    uint32_t rk[44];
    uint32_t te0[256];
    uint8_t sbox[256];
};

// FIPS-197 key expansion in the block function's packing (word i = bytes 4i .. 4i+3, little-endian), one
// thread: key[c] is word c of the 128-bit seed's little-endian bytes.  `sb` is the S-box (LDS).
__device__ __forceinline__ void aes128_expand_key(const uint8_t *sb, const uint32_t key[4], uint32_t *rk) {
    for (int c = 0; c < 4; c++) rk[c] = key[c];
    uint32_t rcon = 1;
    for (int i = 4; i < 44; i += 4) {
        const uint32_t w = rk[i - 1];  // RotWord, SubWord, Rcon on the low byte
        const uint32_t t = ((uint32_t)sb[(w >> 8) & 0xff] | ((uint32_t)sb[(w >> 16) & 0xff] << 8) |
                            ((uint32_t)sb[w >> 24] << 16) | ((uint32_t)sb[w & 0xff] << 24)) ^ rcon;
        rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x1b : 0)) & 0xff;
        rk[i] = rk[i - 4] ^ t;
        rk[i + 1] = rk[i - 3] ^ rk[i];
        rk[i + 2] = rk[i - 2] ^ rk[i + 1];
        rk[i + 3] = rk[i - 1] ^ rk[i + 2];
    }
}

}  // namespace tfhe_mi355
