// Host-only check of the compressed-ciphertext ingress code that runs without a GPU, meant for the sanitizers:
// the two bincode readers of tfhe-rs-odd_amd/csrc/serde.cpp on valid bytes, on every truncation of them and on
// corrupted headers, and the client side of tfhe-rs-odd_amd/csrc/client.cpp -- compact public key, compact-list
// encryption at n = 256 (three bins, the last partial), expansion restated here, decryption, and the two seeded
// encryptions.  The ABI calls serde.cpp makes for key uploads are stubbed: nothing here touches a device.
//   cd tfhe-rs-odd_amd && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       ../scripts/check_ingress_host.cpp csrc/serde.cpp csrc/client.cpp csrc/csprng.hip -o /tmp/check_ingress_host \
//       && /tmp/check_ingress_host
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../include/tfhe_mi355.h"

// what serde.cpp's key uploads call (never reached here)
namespace tfhe_mi355 {
std::shared_ptr<void> begin_key_transaction(TfheMi355Context *) { return nullptr; }
}  // namespace tfhe_mi355
extern "C" {
int tfhe_mi355_context_parameters(TfheMi355Context *, TfheMi355Parameters *) { return 1; }
int tfhe_mi355_keyswitch_key_upload(TfheMi355Context *, const uint64_t *, size_t) { return 1; }
int tfhe_mi355_keyswitch_key_upload_seeded(TfheMi355Context *, const uint64_t *, size_t, uint64_t, uint64_t) { return 1; }
int tfhe_mi355_bootstrap_key_upload_seeded(TfheMi355Context *, const uint64_t *, size_t, uint64_t, uint64_t) { return 1; }
int tfhe_mi355_bootstrap_key_fourier(TfheMi355Context *, void **, size_t *) { return 1; }
int tfhe_mi355_bootstrap_key_fourier_set_ready(TfheMi355Context *) { return 1; }
const char *tfhe_mi355_last_error(void) { return ""; }
}

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static void put(std::vector<uint8_t> &b, uint64_t v, int bytes = 8) {
    for (int i = 0; i < bytes; i++) b.push_back((uint8_t)(v >> (8 * i)));
}
static void tail(std::vector<uint8_t> &b) {
    put(b, 3), put(b, 4), put(b, 4), put(b, 1, 4), put(b, 1);  // degree, moduli, pbs_order, noise_level
}

int main() {
    // ---- serde: a compact list of 19 ciphertexts at n = 8, a compressed ciphertext at n = 742
    const uint64_t n = 8, count = 19, words = (count + n - 1) / n * n + count;
    std::vector<uint8_t> list;
    put(list, words);
    for (uint64_t w = 0; w < words; w++) put(list, w * 0x9E3779B97F4A7C15ull);
    put(list, n + 1), put(list, count), put(list, 0), put(list, 0), put(list, 64);
    tail(list);
    std::vector<uint8_t> one;
    put(one, 0xDEADBEEF12345678ull), put(one, 743), put(one, 5), put(one, 6), put(one, 0), put(one, 0), put(one, 64);
    tail(one);
    TfheMi355CiphertextInfo info;
    for (int which = 0; which < 2; which++) {
        const std::vector<uint8_t> &full = which ? one : list;
        auto inspect = which ? tfhe_mi355_compressed_ciphertext_inspect : tfhe_mi355_compact_ciphertext_list_inspect;
        CHECK(inspect(full.data(), full.size(), &info) == 0);
        CHECK(info.lwe_dimension == (which ? 742u : 8u) && info.count == (which ? 1u : 19u) && info.pbs_order == 1);
        CHECK(info.data_offset == (which ? 0u : 8u) && info.data_words == (which ? 1u : words));
        if (which) CHECK(info.seed_lo == 5 && info.seed_hi == 6);
        for (size_t cut = 0; cut < full.size(); cut++) {  // every truncation, from a buffer of exactly that size
            std::vector<uint8_t> part(full.begin(), full.begin() + cut);
            CHECK(inspect(part.data() ? part.data() : full.data(), cut, &info) == 1);
        }
        for (size_t at = 0; at < full.size(); at += 3) {  // corrupted bytes: any answer, no bad access
            std::vector<uint8_t> bad(full);
            bad[at] ^= 0xff;
            (void)inspect(bad.data(), bad.size(), &info);
        }
    }
    // ---- client: compact encryption at n = 256, expansion, decryption
    {
        const uint32_t N = 256;
        const size_t cnt = 2 * N + 3, bins = (cnt + N - 1) / N;
        const uint64_t delta = 1ull << 59;
        std::vector<uint64_t> sk(N), pk(2 * N), pts(cnt), box(bins * N + cnt), row(N + 1), dec(1);
        CHECK(tfhe_mi355_client_gen_binary_key(3, 1, sk.data(), N) == 0);
        CHECK(tfhe_mi355_client_gen_compact_public_key(4, sk.data(), N, 0x1p-40, pk.data()) == 0);
        for (size_t i = 0; i < cnt; i++) pts[i] = (i * 7 % 16) * delta;
        CHECK(tfhe_mi355_client_compact_encrypt(5, pk.data(), N, pts.data(), cnt, 0x1p-40, 0x1p-40, box.data()) == 0);
        for (size_t i = 0; i < cnt; i++) {
            const uint64_t *m = box.data() + i / N * N;
            const size_t d = N - (i % N + 1);
            for (size_t j = 0; j < N; j++) row[j] = j < d ? 0 - m[j + N - d] : m[j - d];
            row[N] = box[bins * N + i];
            CHECK(tfhe_mi355_client_lwe_decrypt(sk.data(), N, row.data(), 1, dec.data()) == 0);
            CHECK(((dec[0] + delta / 2) / delta) % 16 == i * 7 % 16);
        }
        CHECK(tfhe_mi355_client_compact_encrypt(5, pk.data(), 6, pts.data(), 1, 0, 0, box.data()) == 1);
        // seeded: the masks are the AES-CTR words, so decrypting with them gives the plaintext back
        std::vector<uint64_t> seeds{0, 0, ~0ull, ~0ull, 5, 9}, bodies(3), mask(7);
        CHECK(tfhe_mi355_client_seeded_lwe_encrypt(1, seeds.data(), sk.data(), 7, pts.data(), 3, 0x1p-40, bodies.data()) == 0);
        for (size_t c = 0; c < 3; c++) {
            CHECK(tfhe_mi355_client_csprng_mask_words(seeds[2 * c], seeds[2 * c + 1], 0, 7, row.data()) == 0);
            row[7] = bodies[c];
            CHECK(tfhe_mi355_client_lwe_decrypt(sk.data(), 7, row.data(), 1, dec.data()) == 0);
            CHECK(((dec[0] + delta / 2) / delta) % 16 == c * 7 % 16);
        }
        CHECK(tfhe_mi355_client_seeded_lwe_encrypt_list(2, 5, 9, sk.data(), 7, pts.data(), 3, 0x1p-40, bodies.data()) == 0);
        for (size_t c = 0; c < 3; c++) {
            CHECK(tfhe_mi355_client_csprng_mask_words(5, 9, 7 * c, 7, row.data()) == 0);
            row[7] = bodies[c];
            CHECK(tfhe_mi355_client_lwe_decrypt(sk.data(), 7, row.data(), 1, dec.data()) == 0);
            CHECK(((dec[0] + delta / 2) / delta) % 16 == c * 7 % 16);
        }
    }
    std::printf(failures ? "%d checks failed\n" : "ingress host checks passed\n", failures);
    return failures != 0;
}
