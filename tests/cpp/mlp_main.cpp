// mlp_main.cpp -- the chainable packed FC and the FC-square-FC network through the SEAL-free adapter (include/pasta_seal_gfx950.hpp):
// keygen on the device including the keys of hhe_fc_open_galois_steps of both layers, a two-layer model (6 x 256, 3 x 6) whose open
// diagonals are encrypted with hhe_encrypt, one decomposition of a two-block record, flatten, sealhelper::mlp and the members,
// sealhelper::decrypting -- the three slots against plain integers --, then fc_open + packed_square + fc_open by hand, which gives the
// words of the network call; then the refusals.  With two arguments the input / output are raw uint64 blobs written / read by
// tests/test_cpp_mlp.py, which decrypts the result again through the C ABI; without arguments it runs on nine primes of the library's own.
//
// Stand-alone sanitizer build of the host side (own main, nothing preloaded), against the tests-only emulator's sources:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/mlp_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o mlp_san && ./mlp_san
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

#define REQUIRE(x) do { if (!(x)) { std::cout.flush(); fprintf(stderr, "failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)
// weights in [-8, 8] mod t, the same formula in tests/test_cpp_mlp.py
static std::vector<uint64_t> weights(size_t rows, size_t cols, size_t salt, uint64_t t)
{
    std::vector<uint64_t> M(rows * cols);
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < cols; c++) {
            const int w = (int)((31 * r + 17 * c + salt) % 17) - 8;
            M[r * cols + c] = w < 0 ? t - (uint64_t)(-w) : (uint64_t)w;
        }
    return M;
}
static std::vector<uint64_t> times(const std::vector<uint64_t> &M, size_t rows, size_t cols, const std::vector<uint64_t> &x, uint64_t t)
{
    std::vector<uint64_t> y(rows);
    for (size_t r = 0; r < rows; r++) {
        unsigned __int128 acc = 0;
        for (size_t c = 0; c < cols; c++) acc += (unsigned __int128)M[r * cols + c] * x[c];
        y[r] = (uint64_t)(acc % t);
    }
    return y;
}

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
    const size_t n = (size_t)1 << logn;
    const size_t shapes[2][2] = {{6, 256}, {3, 6}};
    std::vector<uint64_t> ssk(256), pt(256);
    for (size_t i = 0; i < 256; i++) { ssk[i] = (i * 2654435761ULL + 12345) % t; pt[i] = (7 * i + 3) % 4; }
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)(3 * i + 1); seed_b[i] = (uint8_t)(7 * i + 3); }
    const std::vector<uint64_t> M1 = weights(6, 256, 1, t), M2 = weights(3, 6, 5, t);
    std::vector<uint64_t> hidden = times(M1, 6, 256, pt, t);
    for (auto &v : hidden) v = (uint64_t)((unsigned __int128)v * v % t);
    const std::vector<uint64_t> want = times(M2, 3, 6, hidden, t);
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, t, 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        HHE.add_gk_indices();
        std::vector<int> steps;
        for (auto &s : shapes) {
            size_t cnt = 64;
            int buf[64];
            REQUIRE(hhe_fc_open_galois_steps(n, s[0], s[1], buf, &cnt) == HHE_OK);   // -1 .. -(r-1), then the tail
            steps.insert(steps.end(), buf, buf + cnt);
        }
        steps.push_back(-128);      // flatten
        HHE.add_some_gk_indices(steps);
        HHE.create_gk(seed_b);
        const pasta::GaloisKeys &gk = HHE.get_galois_keys();

        // the analyst's model: the open diagonals of both layers, encrypted
        auto encrypt_layer = [&](const std::vector<uint64_t> &M, size_t rows, size_t cols, uint8_t salt, std::vector<pasta::Ciphertext> &W) {
            const auto shape = ctx->fc_open_shape(rows, cols);
            const size_t r = shape.first, c = shape.second;
            std::vector<uint64_t> diag(r * c);
            if (hhe_fc_open_diagonals(t, M.data(), rows, cols, diag.data()) != HHE_OK) throw std::runtime_error("hhe_fc_open_diagonals");
            W.resize(r);
            for (size_t i = 0; i < r; i++) {
                uint8_t seed[32];
                for (int b = 0; b < 32; b++) seed[b] = (uint8_t)(seed_a[b] ^ (uint8_t)(i + 1) ^ salt);
                ctx->encrypt(pk.words.data(), diag.data() + i * c, c, seed, pasta::detail::into(*ctx, W[i]));
            }
        };
        REQUIRE(ctx->fc_open_shape(6, 256) == std::make_pair((size_t)8, (size_t)512));
        REQUIRE(ctx->fc_open_shape(3, 6) == std::make_pair((size_t)4, (size_t)16));
        std::vector<pasta::Ciphertext> W1, W2;
        encrypt_layer(M1, 6, 256, 0x40, W1);
        encrypt_layer(M2, 3, 6, 0x80, W2);
        sealhelper::EncMatrix m1 = HHE.enc_matrix_open(W1, 6, 256), m2 = HHE.enc_matrix_open(W2, 3, 6);
        REQUIRE(m1.open && m2.open);

        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        pasta::PASTA cipher(ctx, ssk, t);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        REQUIRE(blocks.size() == 2);
        pasta::Ciphertext flat;
        HHE.flatten(blocks, flat);

        // the network: the free function, the member, and the layers by hand
        pasta::Ciphertext net, net_member, y1, x2, y2;
        sealhelper::mlp({&m1, &m2}, flat, rk, gk, net);
        HHE.mlp({&m1, &m2}, flat, rk, gk, net_member);
        REQUIRE(net.size == 2 && net.limbs == 0 && net.words.size() == ctx->ct_words());
        REQUIRE(net_member.words == net.words);
        const int budget = sealhelper::invariant_noise_budget(net, sk, *ctx);
        std::cout << "noise budget: " << budget << std::endl;
        REQUIRE(budget > 0);
        auto slots = sealhelper::decrypting(net, sk, *ctx, 3);
        for (size_t i = 0; i < 3; i++) REQUIRE(slots[i] == centred(want[i], t));
        sealhelper::fc_open(flat, m1, rk, gk, y1);
        HHE.packed_square(x2, y1);
        HHE.fc_open(x2, m2, rk, gk, y2);
        auto slots_hand = sealhelper::decrypting(y2, sk, *ctx, 3);
        for (size_t i = 0; i < 3; i++) REQUIRE(slots_hand[i] == slots[i]);
        REQUIRE(y2.words == net.words);   // the composition of the public calls, word for word
        pasta::Ciphertext one;
        sealhelper::mlp({&m1}, flat, rk, gk, one);
        REQUIRE(one.words == y1.words);   // one layer is the open layer

        // refusals: a cyclic handle, no handle, layers that do not chain, an open handle in a cyclic call, keys that cannot serve a step
        sealhelper::EncMatrix cyc(ctx, std::vector<pasta::Ciphertext>(W2.begin(), W2.begin() + 4), 3, 4);
        REQUIRE(!cyc.open);
        auto refused = [&](auto &&call) {
            pasta::Ciphertext untouched;
            untouched.words.assign(3, 12345);
            return throws_invalid([&] { call(untouched); }) && untouched.words == std::vector<uint64_t>(3, 12345);
        };
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::mlp({&m1, &cyc}, flat, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::fc_open(flat, cyc, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::mlp({}, flat, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::mlp({&m1, nullptr}, flat, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::fc_open(flat, sealhelper::EncMatrix{}, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::mlp({&m2, &m1}, flat, rk, gk, x); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::fc_packed_sum(flat, m1, rk, gk, x, true); }));
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::fc_packed(flat, m1, rk, gk, x); }));
        pasta::GaloisKeys pasta_only;
        {
            pasta::PASTA_SEAL G(ctx, pk, sk, rk, pasta::GaloisKeys{});
            G.add_gk_indices();
            G.create_gk(seed_a);
            pasta_only = G.get_galois_keys();
        }
        REQUIRE(refused([&](pasta::Ciphertext &x) { sealhelper::mlp({&m1, &m2}, flat, rk, pasta_only, x); }));

        FILE *out = argc >= 3 ? fopen(argv[2], "wb") : nullptr;
        put(out, sk.words);
        put(out, net.words);
        put(out, y1.words);
        if (out) fclose(out);
        std::cout << "backend: " << hhe_backend() << std::endl;
    } catch (const std::exception &e) {
        std::cout.flush();
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
