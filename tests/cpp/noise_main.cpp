// noise_main.cpp -- the SEAL-free adapter (include/pasta_seal_gfx950.hpp) on the noise budget: the three forms of
// SEALZpCipher::print_noise and sealhelper::invariant_noise_budget on the encrypted PASTA key, a decomposition result, a result
// switched with get_cipher_size(ct, true, 0), a size-3 product and a vector that mixes levels; the empty vector and the missing key.
// Everything goes to std::cout, the reference's lines and a "returned:" line per call; with two arguments the input / output are raw
// uint64 blobs written / read by tests/test_cpp_noise.py, which makes the same budgets through the C ABI and compares line by line.
// Without arguments it runs on the library's own primes, stand-alone for a sanitizer build of the host sources against the emulator
// sources (no GPU, nothing loaded into another process):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/noise_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_{api,context,pasta_public,client,seal_wire}.cpp -ldl -o noise_main
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

#define REQUIRE(x) do { if (!(x)) { std::cout.flush(); fprintf(stderr, "failed: %s\n", #x); return 1; } } while (0)
static int returned(int v) { std::cout << "returned: " << v << std::endl; return v; }

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
        q.assign(all, all + cnt);
    }
    std::vector<uint64_t> ssk(256), pt(256);
    for (size_t i = 0; i < 256; i++) { ssk[i] = (i * 2654435761ULL + 12345) % t; pt[i] = (7 * i + 3) % 256; }
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)(3 * i + 1); seed_b[i] = (uint8_t)(7 * i + 3); }
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        HHE.add_gk_indices();
        HHE.create_gk(seed_b);
        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        REQUIRE(throws_invalid([&] { HHE.print_noise(); }));   // no encrypted key yet: the empty vector
        HHE.set_encrypted_key(enc_ssk[0]);
        const int key_budget = returned(HHE.print_noise());                         // 1. the encrypted PASTA key
        pasta::PASTA cipher(ctx, ssk, t);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        REQUIRE(blocks.size() == 2);
        const int blocks_min = returned(HHE.print_noise(blocks));                   // 2. a decomposition result, batched
        const int b0 = returned(HHE.print_noise(blocks[0])), b1 = returned(HHE.print_noise(blocks[1]));
        pasta::Ciphertext last = blocks[0];
        HHE.get_cipher_size(last, true, 0);
        REQUIRE(last.limbs == 1);
        const int last_budget = returned(HHE.print_noise(last));                    // 3. switched to the last level
        pasta::Ciphertext prod;
        HHE.packed_enc_mul(enc_ssk[0], enc_ssk[0], prod);
        REQUIRE(prod.size == 3);
        const int prod_budget = returned(HHE.print_noise(prod));                    // 4. three polynomials
        std::vector<pasta::Ciphertext> mixed = {blocks[1], last, prod, blocks[0]};
        const int mixed_min = returned(HHE.print_noise(mixed));                     // 5. levels and sizes in one vector
        std::cout << "free: " << sealhelper::invariant_noise_budget(last, sk, *ctx) << std::endl;
        REQUIRE(key_budget > blocks_min && blocks_min == (b0 < b1 ? b0 : b1) && blocks_min > 0);
        REQUIRE(mixed_min == std::min(std::min(b0, b1), std::min(last_budget, prod_budget)));
        REQUIRE(sealhelper::invariant_noise_budget(blocks[1], sk, *ctx) == b1);
        // refusals: the empty vector, the missing key, a ciphertext that does not fit its level
        std::vector<pasta::Ciphertext> none;
        REQUIRE(throws_invalid([&] { HHE.print_noise(none); }));
        pasta::PASTA_SEAL keyless(ctx, pk, pasta::SecretKey{}, rk, pasta::GaloisKeys{});
        REQUIRE(throws_invalid([&] { keyless.print_noise(blocks[0]); }) && throws_invalid([&] { keyless.print_noise(blocks); }));
        REQUIRE(throws_invalid([&] { sealhelper::invariant_noise_budget(blocks[0], pasta::SecretKey{}, *ctx); }));
        pasta::Ciphertext bad = last;
        bad.limbs = 2;
        REQUIRE(throws_invalid([&] { HHE.print_noise(bad); }));
        FILE *o = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(o, sk.words); put(o, enc_ssk[0].words); put(o, blocks[0].words); put(o, blocks[1].words); put(o, last.words); put(o, prod.words);
        if (o) fclose(o);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
