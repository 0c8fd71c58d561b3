// fc_sum_main.cpp -- the packed encrypted FC with one BEHZ floor per item through the SEAL-free adapter (include/pasta_seal_gfx950.hpp):
// keygen on the device including a Galois key for each of 1 .. r-1, one decomposition of a two-block record, flatten, a 10 x 256 layer,
// sealhelper::fc_packed_sum and EncMatrix::apply_sum with both rotation schedules, sealhelper::decrypting -- the ten slots against plain
// integers and against sealhelper::fc_packed --, the same on SEALZpCipher::level(k) with the record and the diagonals switched down;
// then the refusals.  With two arguments the input / output are raw uint64 blobs written / read by tests/test_cpp_fc_sum.py, which
// decrypts the results again through the C ABI; without arguments it runs on nine primes of the library's own.
//
// Stand-alone sanitizer build of the host side (own main, nothing preloaded), against the tests-only emulator's sources:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/fc_sum_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o fc_sum_san && ./fc_sum_san
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

#define REQUIRE(x) do { if (!(x)) { std::cout.flush(); fprintf(stderr, "failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    int logn = 10;
    uint64_t t = 65537;
    size_t k = 3;  // levels_from_last: the level with 4 data primes
    std::vector<uint64_t> q;
    if (argc >= 3) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        auto hdr = read_words(f, 4);  // logn, K, t, levels_from_last
        logn = (int)hdr[0]; t = hdr[2]; k = hdr[3];
        q = read_words(f, hdr[1]);
        fclose(f);
    } else {
        size_t cnt = 64;
        uint64_t all[64];
        if (hhe_bfv_default_coeff_modulus(16384, all, &cnt)) return 2;  // 48/49-bit primes = 1 mod 32768, valid for every smaller N
        q.assign(all, all + cnt);
    }
    const size_t n = (size_t)1 << logn, l = k + 1, rows = 10, cols = 256;
    std::vector<uint64_t> ssk(256), pt(cols);
    for (size_t i = 0; i < 256; i++) { ssk[i] = (i * 2654435761ULL + 12345) % t; pt[i] = (7 * i + 3) % 256; }
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)(3 * i + 1); seed_b[i] = (uint8_t)(7 * i + 3); }
    std::vector<uint64_t> M(rows * cols), want(rows);
    for (size_t r = 0; r < rows; r++) {
        unsigned __int128 acc = 0;
        for (size_t c = 0; c < cols; c++) {
            const int w = (int)((31 * r + 17 * c + 1) % 17) - 8;
            M[r * cols + c] = w < 0 ? t - (uint64_t)(-w) : (uint64_t)w;
            acc += (unsigned __int128)M[r * cols + c] * pt[c];
        }
        want[r] = (uint64_t)(acc % t);
    }
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        const auto shape = ctx->fc_packed_shape(rows, cols);
        const size_t r = shape.first, c = shape.second;
        REQUIRE(r == 16 && c == 256);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        HHE.add_gk_indices();
        size_t nsteps = 64;
        std::vector<int> steps(64);
        REQUIRE(hhe_fc_packed_hoisted_galois_steps(n, rows, cols, steps.data(), &nsteps) == HHE_OK);   // -c, 1 .. r-1, the tail: both schedules
        steps.resize(nsteps);
        steps.push_back(-128);      // flatten
        HHE.add_some_gk_indices(steps);
        HHE.create_gk(seed_b);
        const pasta::GaloisKeys &gk = HHE.get_galois_keys();

        std::vector<uint64_t> diag(r * c);
        REQUIRE(hhe_fc_packed_diagonals(t, M.data(), rows, cols, diag.data()) == HHE_OK);
        std::vector<pasta::Ciphertext> W(r);
        for (size_t i = 0; i < r; i++) {
            uint8_t seed[32];
            for (int b = 0; b < 32; b++) seed[b] = (uint8_t)(seed_a[b] ^ (uint8_t)(i + 1));
            ctx->encrypt(pk.words.data(), diag.data() + i * c, c, seed, pasta::detail::into(*ctx, W[i]));
        }
        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        pasta::PASTA cipher(ctx, ssk, t);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        REQUIRE(blocks.size() == 2);
        pasta::Ciphertext flat;
        HHE.flatten(blocks, flat);   // slots [0, 256) of row 0 hold pt, the other slots of row 0 are zero

        // the layer: r floors per item, then one floor with the chain and with the hoisted rotations, all under the same handle
        sealhelper::EncMatrix mat(ctx, W, rows, cols);
        pasta::Ciphertext chain, sum_chain, sum_hoisted;
        sealhelper::fc_packed(flat, mat, rk, gk, chain);
        sealhelper::fc_packed_sum(flat, mat, rk, gk, sum_chain);
        sealhelper::fc_packed_sum(flat, mat, rk, gk, sum_hoisted, true);
        auto slots_chain = sealhelper::decrypting(chain, sk, *ctx, rows);
        for (pasta::Ciphertext *y : {&sum_chain, &sum_hoisted}) {
            REQUIRE(y->size == 2 && y->limbs == 0 && y->words.size() == ctx->ct_words());
            REQUIRE(sealhelper::invariant_noise_budget(*y, sk, *ctx) > 0);
            auto slots = sealhelper::decrypting(*y, sk, *ctx, rows);
            for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t) && slots_chain[i] == slots[i]);
            REQUIRE(y->words != chain.words);   // the words of another composition: one floor instead of r
        }
        REQUIRE(sum_chain.words != sum_hoisted.words);
        pasta::Ciphertext again;
        mat.apply_sum(flat, rk, gk, again, true);   // the member
        REQUIRE(again.words == sum_hoisted.words);
        pasta::Ciphertext chain_again;
        sealhelper::fc_packed(flat, mat, rk, gk, chain_again);
        REQUIRE(chain_again.words == chain.words);   // the per-product form on the same handle kept its words

        // the same at a level
        pasta::Ciphertext flat_l = flat;
        HHE.get_cipher_size(flat_l, true, k);
        std::vector<pasta::Ciphertext> W_l = W;
        for (auto &d : W_l) HHE.get_cipher_size(d, true, k);
        pasta::SEALZpLevel LV = HHE.level(k);
        REQUIRE(LV.limbs() == l);
        pasta::EncMatrix mat_l = LV.enc_matrix(W_l, rows, cols);
        pasta::Ciphertext logits_l, logits_lh;
        LV.fc_packed_sum(flat_l, mat_l, rk, gk, logits_l);
        LV.fc_packed_sum(flat_l, mat_l, rk, gk, logits_lh, true);
        for (pasta::Ciphertext *y : {&logits_l, &logits_lh}) {
            REQUIRE(y->limbs == l && y->words.size() == 2 * l * n);
            REQUIRE(LV.print_noise(*y) > 0);
            auto slots = LV.decrypting(*y, rows);
            for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t));
        }
        REQUIRE(LV.level_core().keys().uploads() == 0);  // the level's key sets were derived on the device

        // refusals: a ciphertext or a handle of another level, no handle, keys that cannot serve a step
        REQUIRE(throws_invalid([&] { pasta::Ciphertext x; LV.fc_packed_sum(flat_l, mat, rk, gk, x); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext x; sealhelper::fc_packed_sum(flat_l, mat, rk, gk, x); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext x; sealhelper::fc_packed_sum(flat, sealhelper::EncMatrix{}, rk, gk, x); }));
        pasta::GaloisKeys pasta_only;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            G.add_gk_indices();
            G.create_gk(seed_a);
            pasta_only = G.get_galois_keys();
        }
        for (bool hoisted : {false, true}) {
            pasta::Ciphertext untouched;
            untouched.words.assign(3, 12345);
            REQUIRE(throws_invalid([&] { sealhelper::fc_packed_sum(flat, mat, rk, pasta_only, untouched, hoisted); }));
            REQUIRE(untouched.words == std::vector<uint64_t>(3, 12345));
        }

        FILE *out = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(out, sk.words);
        put(out, sum_chain.words);
        put(out, sum_hoisted.words);
        put(out, logits_l.words);
        put(out, logits_lh.words);
        if (out) fclose(out);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
