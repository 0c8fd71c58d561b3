// level_main.cpp -- the SEAL-free adapter (include/pasta_seal_gfx950.hpp) evaluating at a level: keygen, encrypt_key_2, one
// decomposition, get_cipher_size(ct, true, k), then on SEALZpCipher::level(k): mask, flatten of two blocks, packed_affine of dim 16,
// packed_square, print_noise and decrypting -- slots against plain integers, refusals, and how often keys and matrices travelled.
// With two arguments the input / output are raw uint64 blobs written / read by tests/test_cpp_level.py, which compares the printed
// budgets with the C ABI's; without arguments it runs on nine primes of the library's own.
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
    const size_t n = (size_t)1 << logn, L = q.size() - 1, l = k + 1, dim = 16;
    std::vector<uint64_t> ssk(256), pt(256);
    for (size_t i = 0; i < 256; i++) { ssk[i] = (i * 2654435761ULL + 12345) % t; pt[i] = (7 * i + 3) % 256; }
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)(3 * i + 1); seed_b[i] = (uint8_t)(7 * i + 3); }
    pasta::SEALZpCipher::matrix M(dim, pasta::SEALZpCipher::vector(dim));
    pasta::SEALZpCipher::vector bias(dim);
    for (size_t r = 0; r < dim; r++) {
        bias[r] = (5 * r + 2) % t;
        for (size_t c = 0; c < dim; c++) M[r][c] = (31 * r + 17 * c + 1) % 23;
    }
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        HHE.add_gk_indices();
        std::vector<int> flatten_step = {-128};
        HHE.add_some_gk_indices(flatten_step);
        HHE.add_bsgs_indices(4, 4);  // the steps of the diagonal method among them
        HHE.create_gk(seed_b);
        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        pasta::PASTA cipher(ctx, ssk, t);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        REQUIRE(blocks.size() == 2);
        const std::vector<pasta::Ciphertext> top = blocks;
        for (auto &b : blocks) HHE.get_cipher_size(b, true, k);
        REQUIRE(blocks[0].limbs == l && blocks[0].words.size() == 2 * l * n);

        pasta::SEALZpLevel LV = HHE.level(k);
        REQUIRE(LV.limbs() == l);
        const uint64_t up0 = ctx->keys().uploads();
        // mask: the first 16 slots of block 0 stay, the rest become 0
        std::vector<uint64_t> ones(dim, 1);
        pasta::Ciphertext x = blocks[0];
        LV.mask(x, ones);
        REQUIRE(x.limbs == l && x.size == 2);
        auto slots = LV.decrypting(x, 256);
        for (size_t i = 0; i < 256; i++) REQUIRE(slots[i] == (i < dim ? (int64_t)pt[i] : 0));
        // flatten of the two blocks: the 256 words side by side
        pasta::Ciphertext flat;
        LV.flatten(blocks, flat);
        slots = LV.decrypting(flat, 256);
        for (size_t i = 0; i < 256; i++) REQUIRE(slots[i] == (int64_t)pt[i]);
        pasta::Ciphertext flat2;
        LV.flatten(blocks, flat2, HHE.get_galois_keys());  // the key object the call names: the same keys, the same words
        REQUIRE(flat2.words == flat.words);
        // packed_affine of dim 16 on the masked block: M x + b mod t (the diagonal method; babystep-giantstep below)
        std::vector<uint64_t> want(dim);
        for (size_t r = 0; r < dim; r++) {
            unsigned __int128 acc = bias[r];
            for (size_t c = 0; c < dim; c++) acc += (unsigned __int128)M[r][c] * pt[c];
            want[r] = (uint64_t)(acc % t);
        }
        pasta::Ciphertext aff;
        LV.packed_affine(aff, M, x, bias);
        slots = LV.decrypting(aff, dim);
        for (size_t r = 0; r < dim; r++) REQUIRE(slots[r] == centred(want[r], t));
        // packed_square of the layer's output
        pasta::Ciphertext sq;
        LV.packed_square(sq, aff);
        slots = LV.decrypting(sq, dim);
        for (size_t r = 0; r < dim; r++) REQUIRE(slots[r] == centred((uint64_t)((unsigned __int128)want[r] * want[r] % t), t));
        // multiply + relinearize_inplace + encrypted_vec_sum with the key objects the call names
        pasta::Ciphertext prod, sum;
        LV.packed_enc_mul(x, x, prod);
        REQUIRE(prod.size == 3 && prod.limbs == l);
        LV.relinearize_inplace(prod, rk);
        REQUIRE(prod.size == 2);
        pasta::GaloisKeys sum_gk;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            std::vector<int> steps = {-1, -2, -3};
            G.add_some_gk_indices(steps);
            G.create_gk(seed_a);
            sum_gk = G.get_galois_keys();
        }
        LV.encrypted_vec_sum(prod, sum, sum_gk, 4);
        slots = LV.decrypting(sum, 4);
        REQUIRE(slots[3] == centred((pt[0] * pt[0] + pt[1] * pt[1] + pt[2] * pt[2] + pt[3] * pt[3]) % t, t));
        // budgets, for the C ABI to repeat
        std::vector<int> budgets;
        for (pasta::Ciphertext *ct : std::vector<pasta::Ciphertext *>{&blocks[0], &x, &flat, &aff, &sq}) {
            budgets.push_back(LV.print_noise(*ct));
            std::cout << "returned: " << budgets.back() << std::endl;
        }
        REQUIRE(budgets.back() > 0 && budgets.back() == sealhelper::invariant_noise_budget(sq, sk, *ctx));
        // nothing was uploaded twice: the level's sets were derived, once per parent set, and the matrix went up once per method
        // (the object's rk and gk -- the key objects the calls named are those same sets by content -- and sum_gk)
        REQUIRE(LV.level_core().keys().uploads() == 0 && LV.level_core().derivations == 3 && LV.level_core().derived_resident() == 3);
        REQUIRE(LV.level_core().matrices().uploads() == 1);
        // refusals: another level on the level object, the switched ciphertext on the parent object, a level the chain does not have
        pasta::Ciphertext other = top[0], lower = blocks[0];
        HHE.get_cipher_size(lower, true, k - 1);
        REQUIRE(throws_invalid([&] { LV.mask(other, ones); }) && other.words == top[0].words);
        REQUIRE(throws_invalid([&] { LV.mask(lower, ones); }));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; LV.packed_square(o, other); }));
        REQUIRE(throws_invalid([&] { LV.print_noise(lower); }) && throws_invalid([&] { LV.decrypting(other, 4); }));
        pasta::Ciphertext keep = blocks[0];
        REQUIRE(throws_invalid([&] { HHE.mask(keep, ones); }) && keep.words == blocks[0].words);
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; HHE.packed_square(o, blocks[0]); }));
        REQUIRE(throws_invalid([&] { HHE.level(L); }));
        // the level with every data prime takes the parent's ciphertexts, and a second object of one level shares its core
        pasta::SEALZpLevel LT = HHE.level(L - 1), LV2 = HHE.level(k);
        pasta::Ciphertext y = top[0];
        LT.mask(y, ones);
        REQUIRE(y.limbs == L);
        REQUIRE(&LV2.level_core() == &LV.level_core());
        pasta::Ciphertext sq2;
        LV2.packed_square(sq2, aff);
        REQUIRE(sq2.words == sq.words && ctx->keys().uploads() == up0 + 1);  // sum_gk was the one upload since the level object exists
        // an object made after activate_bsgs takes the babystep-giantstep method: another handle, the same slots
        HHE.activate_bsgs(true);
        HHE.set_bsgs_params(4, 4);
        pasta::SEALZpLevel LB = HHE.level(k);
        pasta::Ciphertext aff2;
        LB.packed_affine(aff2, M, x, bias);
        slots = LB.decrypting(aff2, dim);
        for (size_t r = 0; r < dim; r++) REQUIRE(slots[r] == centred(want[r], t));
        REQUIRE(LV.level_core().matrices().uploads() == 2 && LV.level_core().derivations == 3);
        FILE *o = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(o, sk.words);
        for (const pasta::Ciphertext *ct : std::vector<const pasta::Ciphertext *>{&blocks[0], &x, &flat, &aff, &sq}) put(o, ct->words);
        if (o) fclose(o);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
