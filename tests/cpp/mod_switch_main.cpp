// mod_switch_main.cpp -- the SEAL-free adapter (include/pasta_seal_gfx950.hpp) on levels: SEALZpCipher::get_cipher_size(ct),
// (ct, true, 0) and (ct, true, 1), sealhelper::decrypting on the switched ciphertexts, and the refusals.  With two arguments the
// input / output are raw uint64 blobs written / read by tests/test_cpp_mod_switch.py; without arguments it runs on three primes
// of the library's own, stand-alone for a sanitizer build of the host sources against the emulator sources (no GPU, nothing
// loaded into another process):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/mod_switch_main.cpp tests/emu/hhe_launch_emu.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_{api,context,pasta_public,client,seal_wire}.cpp -ldl -o mod_switch_main
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "failed: %s\n", #x); return 1; } } while (0)

int main(int argc, char **argv)
{
    int logn = 10;
    uint64_t t = 65537;
    std::vector<uint64_t> q;
    if (argc >= 3) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        auto hdr = read_words(f, 3);  // logn, K, t
        logn = (int)hdr[0]; t = hdr[2];
        q = read_words(f, hdr[1]);
        fclose(f);
    } else {
        size_t cnt = 64;
        uint64_t all[64];
        if (hhe_bfv_default_coeff_modulus(16384, all, &cnt)) return 2;  // 48/49-bit primes = 1 mod 32768, valid for every smaller N
        q = {all[0], all[1], all[2], all[3]};
    }
    const size_t n = (size_t)1 << logn, L = q.size() - 1, header = 16 + 32 + 1 + 40 + 16 + 8;
    std::vector<uint64_t> ssk(256);
    for (size_t i = 0; i < 256; i++) ssk[i] = (i * 2654435761ULL + 12345) % t;
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::keygen(*ctx, seed, sk, pk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, pasta::RelinKeys{}, pasta::GaloisKeys{});
        const pasta::Ciphertext top = HHE.encrypt_key_2(ssk, seed)[0];
        pasta::Ciphertext same = top, last = top, second = top;
        const size_t s_top = HHE.get_cipher_size(same), s_last = HHE.get_cipher_size(last, true, 0), s_second = HHE.get_cipher_size(second, true, 1);
        printf("sizes: %zu %zu %zu\n", s_top, s_second, s_last);
        REQUIRE(same.words == top.words && same.limbs == 0);
        REQUIRE(s_top == header + 2 * L * n * 8 && s_second == header + 2 * 2 * n * 8 && s_last == header + 2 * 1 * n * 8);
        REQUIRE(last.limbs == 1 && last.words.size() == 2 * n && second.limbs == 2 && second.words.size() == 2 * 2 * n);
        REQUIRE(HHE.get_cipher_size(last) == s_last && HHE.get_cipher_size(second) == s_second);   // measuring a switched result
        // further down from a lower level equals the direct switch, word for word; to the level it is at: unchanged
        pasta::Ciphertext again = second, stay = second;
        REQUIRE(HHE.get_cipher_size(again, true, 0) == s_last && again.words == last.words);
        REQUIRE(HHE.get_cipher_size(stay, true, 1) == s_second && stay.words == second.words);
        // decrypting accepts the switched ciphertexts: the packed key comes back (words 0..127 at slots 0..)
        for (const pasta::Ciphertext *ct : std::vector<const pasta::Ciphertext *>{&top, &second, &last}) {
            auto vals = sealhelper::decrypting(*ct, sk, *ctx, 128);
            for (size_t i = 0; i < 128; i++) {
                const int64_t want = ssk[i] > (t + 1) / 2 ? (int64_t)ssk[i] - (int64_t)t : (int64_t)ssk[i];
                if (vals[i] != want) { fprintf(stderr, "slot %zu at %zu limbs: %lld, expected %lld\n", i, ct->limbs, (long long)vals[i], (long long)want); return 1; }
            }
        }
        // out of range, up the chain, and evaluation on a lower level
        pasta::Ciphertext c1 = top, c2 = last, c3 = last;
        std::vector<uint64_t> mask(4, 1);
        REQUIRE(throws_invalid([&] { HHE.get_cipher_size(c1, true, L); }) && c1.words == top.words && c1.limbs == 0);
        REQUIRE(throws_invalid([&] { HHE.get_cipher_size(c2, true, 1); }) && c2.words == last.words && c2.limbs == 1);
        REQUIRE(throws_invalid([&] { HHE.mask(c3, mask); }) && c3.words == last.words);
        FILE *o = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(o, sk.words); put(o, top.words); put(o, second.words); put(o, last.words);
        if (o) fclose(o);
        printf("backend: %s\n", hhe_backend());
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
