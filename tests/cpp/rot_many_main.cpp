// rot_many_main.cpp -- hoisted rotations and the packed encrypted FC with a hoisted chain through the SEAL-free adapter
// (include/pasta_seal_gfx950.hpp): keygen on the device including a Galois key for each of 1 .. r-1, one decomposition of a two-block
// record, flatten, SEALZpCipher::rotate_rows_many / sealhelper::rotate_rows_many -- every rotation decrypted against the rotated plain
// integers --, sealhelper::fc_packed_hoisted, sealhelper::decrypting -- the ten slots against plain integers and against
// sealhelper::fc_packed --, the same on SEALZpCipher::level(k) with the record and the diagonals switched down; then the refusals.
// With two arguments the input / output are raw uint64 blobs written / read by tests/test_cpp_rot_many.py, which decrypts the
// results again through the C ABI; without arguments it runs on nine primes of the library's own.
//
// Stand-alone sanitizer build of the host side (own main, nothing preloaded), against the tests-only emulator's sources:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/rot_many_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o rot_many_san && ./rot_many_san
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
        size_t nsteps = 2;
        std::vector<int> steps(64);
        REQUIRE(hhe_fc_packed_hoisted_galois_steps(n, rows, cols, steps.data(), &nsteps) == HHE_ERR_CAPACITY && nsteps == 20);
        nsteps = steps.size();
        REQUIRE(hhe_fc_packed_hoisted_galois_steps(n, rows, cols, steps.data(), &nsteps) == HHE_OK);
        steps.resize(nsteps);
        std::vector<int> expect{-256};
        for (int i = 1; i < 16; i++) expect.push_back(i);
        for (int s = 16; s < 256; s *= 2) expect.push_back(s);
        REQUIRE(steps == expect);   // the keys that make the chain one node with r - 1 children
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

        // hoisted rotations: 3 by its own key, 17 = 1 + 16 through its NAF terms, 0 and a repeated step as copies
        const std::vector<int> rs{1, 3, 17, 0, 3, 15};
        std::vector<pasta::Ciphertext> rot;
        HHE.rotate_rows_many(flat, rs, gk, rot);
        REQUIRE(rot.size() == rs.size());
        for (size_t j = 0; j < rs.size(); j++) {
            REQUIRE(rot[j].size == 2 && rot[j].limbs == 0 && rot[j].words.size() == ctx->ct_words());
            auto slots = sealhelper::decrypting(rot[j], sk, *ctx, cols);
            for (size_t i = 0; i < cols; i++) REQUIRE(slots[i] == (i + rs[j] < cols ? (int64_t)pt[i + rs[j]] : 0));   // rotate_rows(x, s): slot i <- slot i + s
        }
        REQUIRE(rot[3].words == flat.words && rot[1].words == rot[4].words);
        std::vector<pasta::Ciphertext> rot2;
        sealhelper::rotate_rows_many(*ctx, flat, rs, gk, rot2);
        for (size_t j = 0; j < rs.size(); j++) REQUIRE(rot2[j].words == rot[j].words);

        // the layer, chain and hoisted, under the same handle
        sealhelper::EncMatrix mat(ctx, W, rows, cols);
        pasta::Ciphertext chain, logits;
        sealhelper::fc_packed(flat, mat, rk, gk, chain);
        sealhelper::fc_packed_hoisted(flat, mat, rk, gk, logits);
        REQUIRE(logits.size == 2 && logits.limbs == 0 && logits.words.size() == ctx->ct_words());
        REQUIRE(sealhelper::invariant_noise_budget(logits, sk, *ctx) > 0);
        auto slots = sealhelper::decrypting(logits, sk, *ctx, rows), slots_chain = sealhelper::decrypting(chain, sk, *ctx, rows);
        for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t) && slots_chain[i] == slots[i]);
        REQUIRE(logits.words != chain.words);   // the words of another composition: the noise differs
        pasta::Ciphertext again;
        sealhelper::fc_packed_hoisted(flat, mat, rk, gk, again);
        REQUIRE(again.words == logits.words);

        // the same at a level
        pasta::Ciphertext flat_l = flat;
        HHE.get_cipher_size(flat_l, true, k);
        std::vector<pasta::Ciphertext> W_l = W;
        for (auto &d : W_l) HHE.get_cipher_size(d, true, k);
        pasta::SEALZpLevel LV = HHE.level(k);
        REQUIRE(LV.limbs() == l);
        std::vector<pasta::Ciphertext> rot_l;
        LV.rotate_rows_many(flat_l, rs, gk, rot_l);
        for (size_t j = 0; j < rs.size(); j++) {
            REQUIRE(rot_l[j].limbs == l && rot_l[j].words.size() == 2 * l * n);
            auto sl = LV.decrypting(rot_l[j], cols);
            for (size_t i = 0; i < cols; i++) REQUIRE(sl[i] == (i + rs[j] < cols ? (int64_t)pt[i + rs[j]] : 0));
        }
        pasta::EncMatrix mat_l = LV.enc_matrix(W_l, rows, cols);
        pasta::Ciphertext logits_l;
        LV.fc_packed_hoisted(flat_l, mat_l, rk, gk, logits_l);
        REQUIRE(logits_l.limbs == l && logits_l.words.size() == 2 * l * n);
        REQUIRE(LV.print_noise(logits_l) > 0);
        slots = LV.decrypting(logits_l, rows);
        for (size_t i = 0; i < rows; i++) REQUIRE(slots[i] == centred(want[i], t));
        REQUIRE(LV.level_core().keys().uploads() == 0);  // the level's key sets were derived on the device

        // refusals: no step, a step of N/2, a ciphertext or a handle of another level, an empty key object, keys that cannot serve a step
        std::vector<pasta::Ciphertext> o;
        REQUIRE(throws_invalid([&] { HHE.rotate_rows_many(flat, {}, gk, o); }));
        REQUIRE(throws_invalid([&] { HHE.rotate_rows_many(flat, {1, (int)(n / 2)}, gk, o); }));
        REQUIRE(throws_invalid([&] { HHE.rotate_rows_many(flat_l, rs, gk, o); }));
        REQUIRE(throws_invalid([&] { LV.rotate_rows_many(flat, rs, gk, o); }));
        REQUIRE(throws_invalid([&] { HHE.rotate_rows_many(flat, rs, pasta::GaloisKeys{}, o); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext x; LV.fc_packed_hoisted(flat_l, mat, rk, gk, x); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext x; sealhelper::fc_packed_hoisted(flat_l, mat, rk, gk, x); }));
        pasta::GaloisKeys pasta_only;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            G.add_gk_indices();
            G.create_gk(seed_a);
            pasta_only = G.get_galois_keys();
        }
        REQUIRE(throws_invalid([&] { HHE.rotate_rows_many(flat, {3}, pasta_only, o); }));
        pasta::Ciphertext untouched;
        untouched.words.assign(3, 12345);
        REQUIRE(throws_invalid([&] { sealhelper::fc_packed_hoisted(flat, mat, rk, pasta_only, untouched); }));
        REQUIRE(untouched.words == std::vector<uint64_t>(3, 12345));

        FILE *out = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(out, sk.words);
        put(out, logits.words);
        put(out, logits_l.words);
        put(out, rot[2].words);
        if (out) fclose(out);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
