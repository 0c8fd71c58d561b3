// plain_sum_main.cpp -- the open FC layer under plain weights and the sum of rotations times plaintexts under one mod-down through the
// SEAL-free adapter (include/pasta_seal_gfx950.hpp): keygen on the device including a key for every step of hhe_fc_open_galois_steps, a
// 10 x 250 layer with bias (member and free function, two requests, ONE upload of the matrix) and the primitive on three pairs, both
// decrypted against plain integers; the same on SEALZpCipher::level(3) with the record switched down; then the refusals.  The input
// carries a random value in every slot of both rows outside [0, 250).  With two arguments the input / output are raw uint64 blobs written
// / read by tests/test_cpp_plain_sum.py, which decrypts the results again through the C ABI; without arguments it runs on nine primes of
// the library's own.
//
// Stand-alone sanitizer build of the host side (own main, nothing preloaded), against the tests-only emulator's sources:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/plain_sum_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o plain_sum_san && ./plain_sum_san
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

#define REQUIRE(x) do { if (!(x)) { std::cout.flush(); fprintf(stderr, "failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)
typedef std::vector<std::vector<uint64_t>> matrix;
static const size_t ROWS = 10, COLS = 250;
// the same formulas in tests/test_cpp_plain_sum.py
static uint64_t weight(size_t r, size_t c, uint64_t t)
{
    const int w = (int)((31 * r + 17 * c + 1) % 17) - 8;
    return w < 0 ? t - (uint64_t)(-w) : (uint64_t)w;
}
static uint64_t slot_value(size_t s, uint64_t t) { return s < COLS ? (7 * s + 3) % 4 : (s * 2654435761ULL + 99) % t; }
static uint64_t plain_value(size_t k, size_t s, uint64_t t) { return ((k + 1) * 40503ULL + s * 2246822519ULL + 7) % t; }

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
    const size_t n = (size_t)1 << logn, half = n / 2;
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)(3 * i + 1); seed_b[i] = (uint8_t)(7 * i + 3); }
    matrix M(ROWS, std::vector<uint64_t>(COLS));
    std::vector<uint64_t> bias(ROWS), x(n);
    for (size_t r = 0; r < ROWS; r++) {
        bias[r] = (1000 * r + 5) % t;
        for (size_t c = 0; c < COLS; c++) M[r][c] = weight(r, c, t);
    }
    for (size_t s = 0; s < n; s++) x[s] = slot_value(s, t);
    std::vector<uint64_t> want(ROWS);
    for (size_t r = 0; r < ROWS; r++) {
        unsigned __int128 acc = bias[r];
        for (size_t c = 0; c < COLS; c++) acc += (unsigned __int128)M[r][c] * x[c];
        want[r] = (uint64_t)(acc % t);
    }
    const std::vector<int> steps = {-1, 0, -3};
    matrix plains(steps.size(), std::vector<uint64_t>(n));
    std::vector<uint64_t> want_sum(n);
    for (size_t k = 0; k < steps.size(); k++)
        for (size_t s = 0; s < n; s++) plains[k][s] = plain_value(k, s, t);
    for (size_t s = 0; s < n; s++) {
        unsigned __int128 acc = 0;
        const size_t row = s / half * half, j = s % half;
        for (size_t k = 0; k < steps.size(); k++)   // slot s of rotate_rows(x, step) is x[(s + step) mod N/2] of the same row
            acc += (unsigned __int128)plains[k][s] * x[row + (j + half + steps[k]) % half];
        want_sum[s] = (uint64_t)(acc % t);
    }
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        std::vector<int> need(64);
        size_t cnt = need.size();
        REQUIRE(hhe_fc_open_galois_steps(n, ROWS, COLS, need.data(), &cnt) == HHE_OK);   // -1 .. -15, then 16 .. 256: each a key of its own
        need.resize(cnt);
        REQUIRE(cnt == 15 + 5);
        HHE.add_some_gk_indices(need);
        HHE.create_gk(seed_b);
        const pasta::GaloisKeys &gk = HHE.get_galois_keys();
        pasta::Ciphertext ct;
        ctx->encrypt(pk.words.data(), x.data(), n, seed_a, pasta::detail::into(*ctx, ct));

        // the layer: made resident ahead, then two requests through the member and the free function -- one upload
        const uint64_t up0 = ctx->matrices().uploads();
        HHE.plain_fc_open(M, bias);
        REQUIRE(ctx->matrices().uploads() == up0 + 1);
        pasta::Ciphertext y, y_free, z, z_free;
        HHE.fc_open_plain(ct, M, bias, gk, y);
        sealhelper::fc_open_plain(*ctx, ct, M, bias, gk, y_free);
        REQUIRE(ctx->matrices().uploads() == up0 + 1);
        REQUIRE(y.size == 2 && y.limbs == 0 && y.words.size() == ctx->ct_words() && y_free.words == y.words);
        const int budget = sealhelper::invariant_noise_budget(y, sk, *ctx);
        std::cout << "noise budget: " << budget << std::endl;
        REQUIRE(budget > 0);
        auto slots = sealhelper::decrypting(y, sk, *ctx, ROWS);
        for (size_t i = 0; i < ROWS; i++) REQUIRE(slots[i] == centred(want[i], t));
        pasta::Ciphertext y_nobias;
        HHE.fc_open_plain(ct, M, {}, gk, y_nobias);   // another matrix by content: a second upload
        REQUIRE(ctx->matrices().uploads() == up0 + 2 && y_nobias.words != y.words);
        // the primitive
        HHE.rotate_plain_sum(ct, plains, steps, gk, z);
        sealhelper::rotate_plain_sum(*ctx, ct, plains, steps, gk, z_free);
        REQUIRE(ctx->matrices().uploads() == up0 + 3 && z_free.words == z.words);
        REQUIRE(sealhelper::invariant_noise_budget(z, sk, *ctx) > 0);
        auto sum_slots = sealhelper::decrypting(z, sk, *ctx, n);
        for (size_t s = 0; s < n; s++) REQUIRE(sum_slots[s] == centred(want_sum[s], t));

        // the same on level(3): the record switched down, the handles made on the level's context, the keys derived on the device
        const size_t k = 3;
        pasta::Ciphertext ct_l = ct, y_l, y_l2, z_l;
        HHE.get_cipher_size(ct_l, true, k);
        pasta::SEALZpLevel LV = HHE.level(k);
        LV.fc_open_plain(ct_l, M, bias, gk, y_l);
        LV.fc_open_plain(ct_l, M, bias, gk, y_l2);
        REQUIRE(y_l.limbs == k + 1 && y_l2.words == y_l.words);
        REQUIRE(LV.level_core().matrices().uploads() == 1 && LV.level_core().keys().uploads() == 0);
        REQUIRE(LV.print_noise(y_l) > 0);
        auto slots_l = LV.decrypting(y_l, ROWS);
        for (size_t i = 0; i < ROWS; i++) REQUIRE(slots_l[i] == centred(want[i], t));
        LV.rotate_plain_sum(ct_l, plains, steps, gk, z_l);
        auto sum_l = LV.decrypting(z_l, n);
        for (size_t s = 0; s < n; s++) REQUIRE(sum_l[s] == centred(want_sum[s], t));
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; HHE.fc_open_plain(ct_l, M, bias, gk, o); }));   // a level's ciphertext at the top
        REQUIRE(throws_invalid([&] { pasta::Ciphertext o; LV.fc_open_plain(ct, M, bias, gk, o); }));

        // refusals, the destination untouched
        auto refused = [&](auto &&call) {
            pasta::Ciphertext untouched;
            untouched.words.assign(3, 12345);
            return throws_invalid([&] { call(untouched); }) && untouched.words == std::vector<uint64_t>(3, 12345);
        };
        matrix ragged = M, big = M;
        ragged[3].pop_back();
        big[2][7] = t;
        pasta::GaloisKeys pasta_only;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            G.add_gk_indices();
            G.create_gk(seed_a);
            pasta_only = G.get_galois_keys();
        }
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, matrix{}, {}, gk, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, ragged, bias, gk, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, big, bias, gk, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, M, std::vector<uint64_t>(ROWS + 1, 1), gk, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, M, bias, pasta_only, o); }));   // -2 .. -15 have no key of their own there
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.fc_open_plain(ct, M, bias, pasta::GaloisKeys{}, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { sealhelper::fc_open_plain(*ctx, ct, M, bias, pasta_only, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.rotate_plain_sum(ct, plains, {-1, 0}, gk, o); }));          // one plaintext per step
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.rotate_plain_sum(ct, plains, {-1, 0, 5}, gk, o); }));       // 5 has no key of its own
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.rotate_plain_sum(ct, plains, {-1, 0, (int)half}, gk, o); }));
        REQUIRE(refused([&](pasta::Ciphertext &o) { HHE.rotate_plain_sum(ct, matrix{}, {}, gk, o); }));
        {
            bool threw = false;   // too few slots is the reference's runtime_error
            pasta::Ciphertext o;
            try { HHE.fc_open_plain(ct, matrix(3, std::vector<uint64_t>(half, 1)), {}, gk, o); } catch (const std::runtime_error &) { threw = true; }
            REQUIRE(threw && o.words.empty());
        }

        FILE *out = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(out, sk.words);
        put(out, y.words);
        put(out, z.words);
        if (out) fclose(out);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
