// fc_packed_main.cpp -- the packed encrypted FC layer through the SEAL-free adapter (include/pasta_seal_gfx950.hpp), as a CSP and an
// analyst would drive it: keygen on the device, the generalized diagonals of a 10 x 256 weight matrix encrypted with hhe_encrypt, one
// decomposition of a two-block record, flatten, sealhelper::fc_packed, sealhelper::decrypting -- the ten slots against plain
// integers -- and the same on SEALZpCipher::level(k) with the record and the diagonals switched down; then the refusals.
// With two arguments the input / output are raw uint64 blobs written / read by tests/test_cpp_fc_packed.py, which decrypts the two
// results again through the C ABI; without arguments it runs on nine primes of the library's own.
//
// Stand-alone sanitizer build of the host side (own main, nothing preloaded), against the tests-only emulator's sources:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/fc_packed_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o fc_packed_san && ./fc_packed_san
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
    // the analyst's weights (entries mod t, negative ones among them) and what the layer must return
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
        size_t nsteps = 16;
        std::vector<int> steps(nsteps);
        REQUIRE(hhe_fc_packed_galois_steps(n, rows, cols, steps.data(), &nsteps) == HHE_OK);
        steps.resize(nsteps);
        REQUIRE(steps == (std::vector<int>{-256, 1, 16, 32, 64, 128}));
        steps.push_back(-128);  // flatten
        HHE.add_some_gk_indices(steps);
        HHE.create_gk(seed_b);
        const pasta::GaloisKeys &gk = HHE.get_galois_keys();

        // the analyst: the r generalized diagonals, each encrypted under a seed of its own
        std::vector<uint64_t> diag(r * c);
        REQUIRE(hhe_fc_packed_diagonals(t, M.data(), rows, cols, diag.data()) == HHE_OK);
        std::vector<pasta::Ciphertext> W(r);
        for (size_t i = 0; i < r; i++) {
            uint8_t seed[32];
            for (int b = 0; b < 32; b++) seed[b] = (uint8_t)(seed_a[b] ^ (uint8_t)(i + 1));
            ctx->encrypt(pk.words.data(), diag.data() + i * c, c, seed, pasta::detail::into(*ctx, W[i]));
        }
        // the CSP: one record of two full blocks side by side in one ciphertext (slots [256, N/2) of row 0 are zero: the layer's precondition)
        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        pasta::PASTA cipher(ctx, ssk, t);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        REQUIRE(blocks.size() == 2);
        pasta::Ciphertext flat;
        HHE.flatten(blocks, flat);
        // once per model, once per record
        sealhelper::EncMatrix mat(ctx, W, rows, cols);
        pasta::Ciphertext logits;
        sealhelper::fc_packed(flat, mat, rk, gk, logits);
        REQUIRE(logits.size == 2 && logits.limbs == 0 && logits.words.size() == ctx->ct_words());
        REQUIRE(sealhelper::invariant_noise_budget(logits, sk, *ctx) > 0);
        auto slots = sealhelper::decrypting(logits, sk, *ctx, rows);
        for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t));
        // the handle is resident: a second record costs no upload of the weights, and gives the same words
        pasta::Ciphertext again;
        sealhelper::fc_packed(flat, mat, rk, gk, again);
        REQUIRE(again.words == logits.words);

        // the same at a level: record and diagonals switched once, the handle made on the level's context
        pasta::Ciphertext flat_l = flat;
        HHE.get_cipher_size(flat_l, true, k);
        std::vector<pasta::Ciphertext> W_l = W;
        for (auto &d : W_l) HHE.get_cipher_size(d, true, k);
        pasta::SEALZpLevel LV = HHE.level(k);
        REQUIRE(LV.limbs() == l);
        pasta::EncMatrix mat_l = LV.enc_matrix(W_l, rows, cols);
        pasta::Ciphertext logits_l;
        LV.fc_packed(flat_l, mat_l, rk, gk, logits_l);
        REQUIRE(logits_l.limbs == l && logits_l.words.size() == 2 * l * n);
        REQUIRE(LV.print_noise(logits_l) > 0);
        slots = LV.decrypting(logits_l, rows);
        for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t));
        REQUIRE(LV.level_core().keys().uploads() == 0);  // the level's key sets were derived on the device

        // refusals: a handle of another level, a ciphertext of another level, too few or too many diagonals, an empty key object,
        // a GaloisKeys object without the layer's steps
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; LV.fc_packed(flat_l, mat, rk, gk, o); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; sealhelper::fc_packed(flat_l, mat, rk, gk, o); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; LV.fc_packed(flat, mat_l, rk, gk, o); }));
        REQUIRE(throws_invalid([&] { std::vector<pasta::Ciphertext> few(W.begin(), W.begin() + 10); sealhelper::EncMatrix m(ctx, few, rows, cols); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; sealhelper::fc_packed(flat, mat, pasta::RelinKeys{}, gk, o); }));
        pasta::GaloisKeys pasta_only;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            G.add_gk_indices();
            G.create_gk(seed_a);
            pasta_only = G.get_galois_keys();
        }
        pasta::Ciphertext untouched;
        untouched.words.assign(3, 12345);
        REQUIRE(throws_invalid([&] { sealhelper::fc_packed(flat, mat, rk, pasta_only, untouched); }));
        REQUIRE(untouched.words == std::vector<uint64_t>(3, 12345));
        try {
            ctx->fc_packed_shape(3, n);  // c = N: too few slots
            REQUIRE(false);
        } catch (const std::runtime_error &e) { REQUIRE(std::string(e.what()).find("too little slots") != std::string::npos); }

        FILE *o = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(o, sk.words);
        put(o, logits.words);
        put(o, logits_l.words);
        if (o) fclose(o);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
