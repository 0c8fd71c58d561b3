// level_lifecycle_main.cpp -- level contexts and key sets derived on the device, host side, stand-alone for a sanitizer build against
// the emulator sources (no GPU, nothing loaded into another process):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/level_lifecycle_main.cpp tests/emu/hhe_launch_emu.cpp \
//       tests/emu/emu_order.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_{api,context,pasta_public,client,seal_wire}.cpp \
//       -ldl -o level_lifecycle
// Every entry point at the levels with 2 and 1 data primes (K = 3 and K = 2: the smallest workspaces there are), keys derived, derived
// again, refused; a level of a level; parent and level destroyed in both orders, sets left to their context.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hhe_gfx950.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, hhe_last_error()); exit(1); } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s -> %d, expected %d\n", #x, rc_, (int)(code)); exit(1); } } while (0)
#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "%s failed (line %d)\n", #x, __LINE__); exit(1); } } while (0)

static uint64_t *dev(size_t words) { uint64_t *p = (uint64_t *)hhe_malloc(words * 8); REQUIRE(p); return p; }

// rows {0..l-1, K-1} of [polys][K][N] device words, as a new device buffer [polys][l+1][N] (api.py: level_rows)
static uint64_t *level_rows(hhe_ctx *c, const uint64_t *src, int polys, int K, int l, size_t n)
{
    std::vector<uint64_t> h((size_t)polys * K * n), g((size_t)polys * (l + 1) * n);
    CHECK(hhe_copy_d2h(c, h.data(), src, h.size() * 8));
    for (int p = 0; p < polys; p++)
        for (int j = 0; j <= l; j++)
            memcpy(&g[((size_t)p * (l + 1) + j) * n], &h[((size_t)p * K + (j == l ? K - 1 : j)) * n], n * 8);
    uint64_t *d = dev(g.size());
    CHECK(hhe_copy_h2d(c, d, g.data(), g.size() * 8));
    return d;
}

int main()
{
    for (int logn : {10, 12}) {  // separate-kernel path with ragged tiles, and the fused row kernels
        const size_t n = (size_t)1 << logn;
        const int K = 4, L = 3, B = 2;
        uint64_t q[K];
        {
            size_t cnt = 64;
            uint64_t all[64];
            CHECK(hhe_bfv_default_coeff_modulus(16384, all, &cnt));  // 48/49-bit primes = 1 mod 32768, valid for every smaller N
            q[0] = all[0]; q[1] = all[1]; q[2] = all[2]; q[3] = all[3];
        }
        const uint64_t t = 65537;
        hhe_ctx *c = nullptr;
        CHECK(hhe_ctx_create(logn, K, q, t, 0, &c));
        uint8_t seed[32], seed2[32];
        for (int i = 0; i < 32; i++) { seed[i] = (uint8_t)i; seed2[i] = (uint8_t)(200 - i); }
        uint64_t *sk = dev(K * n), *pk = dev(2 * K * n);
        CHECK(hhe_keygen_secret(c, seed, sk));
        CHECK(hhe_keygen_public(c, sk, seed, pk));
        hhe_keyset *ks = nullptr;
        CHECK(hhe_keyset_create(c, &ks));
        CHECK(hhe_keyset_generate_relin(ks, sk, seed));
        CHECK(hhe_keyset_generate_galois(ks, sk, nullptr, 0, seed));  // the default elements: steps +-2^k and the column swap
        // two items at the top: slot i of item b holds (3 i + b) mod 256
        std::vector<uint64_t> vals((size_t)B * n);
        for (int b = 0; b < B; b++)
            for (size_t i = 0; i < n; i++) vals[b * n + i] = (3 * i + b) % 256;
        uint64_t *d_vals = dev(B * n), *plain = dev(B * n), *top = dev((size_t)B * 2 * L * n), *top3 = dev((size_t)B * 3 * L * n);
        CHECK(hhe_copy_h2d(c, d_vals, vals.data(), vals.size() * 8));
        CHECK(hhe_encode(c, d_vals, B, n, plain));
        CHECK(hhe_encrypt(c, pk, plain, 0, seed2, B, top));
        CHECK(hhe_multiply(c, top, top, top3, B));
        CHECK(hhe_ctx_sync(c));

        hhe_ctx *kept = nullptr;  // the level-1 context outlives its parent
        for (int l : {2, 1}) {
            hhe_ctx *x = nullptr;
            EXPECT(hhe_ctx_create_level(c, 0, &x), HHE_ERR_INVALID);
            EXPECT(hhe_ctx_create_level(c, L + 1, &x), HHE_ERR_INVALID);
            EXPECT(hhe_ctx_create_level(nullptr, l, &x), HHE_ERR_INVALID);
            EXPECT(hhe_ctx_create_level(c, l, nullptr), HHE_ERR_INVALID);
            CHECK(hhe_ctx_create_level(c, l, &x));
            const size_t ctw = (size_t)2 * l * n, ksk = (size_t)l * 2 * (l + 1) * n;
            hhe_keyset *dl = nullptr, *up = nullptr;
            CHECK(hhe_keyset_create(x, &dl));
            CHECK(hhe_keyset_create(c, &up));
            EXPECT(hhe_keyset_derive_level(nullptr, ks), HHE_ERR_INVALID);
            EXPECT(hhe_keyset_derive_level(dl, nullptr), HHE_ERR_INVALID);
            CHECK(hhe_keyset_derive_level(dl, ks));
            EXPECT(hhe_keyset_derive_level(up, dl), HHE_ERR_INVALID);  // upward
            EXPECT(hhe_keyset_derive_level(dl, dl), HHE_ERR_INVALID);
            REQUIRE(hhe_keyset_has_relin(dl) == 1 && hhe_keyset_has_galois(dl, 3) == 1 && hhe_keyset_has_relin(up) == 0);
            uint64_t nkeys = 1;  // one launch per key: the relin key and every Galois key of the source
            for (uint32_t e = 1; e < 2 * n; e += 2) {
                REQUIRE(hhe_keyset_has_galois(dl, e) == hhe_keyset_has_galois(ks, e));
                nkeys += (uint64_t)hhe_keyset_has_galois(ks, e);
            }
            REQUIRE(nkeys > 2 && hhe_ctx_query(x, "key_proj_launches", 0) == nkeys);
            // the projected words, against a gather on the host
            {
                std::vector<uint64_t> full((size_t)L * 2 * K * n), got(ksk);
                CHECK(hhe_keyset_get_relin(ks, full.data()));
                CHECK(hhe_keyset_get_relin(dl, got.data()));
                for (int I = 0; I < l; I++)
                    for (int k = 0; k < 2; k++)
                        for (int J = 0; J <= l; J++)
                            REQUIRE(!memcmp(&got[(((size_t)I * 2 + k) * (l + 1) + J) * n], &full[(((size_t)I * 2 + k) * K + (J == l ? K - 1 : J)) * n], n * 8));
            }
            uint64_t *sk_l = level_rows(c, sk, 1, K, l, n), *pk_l = level_rows(c, pk, 2, K, l, n);
            std::vector<uint64_t> h_sk((size_t)(l + 1) * n);
            CHECK(hhe_copy_d2h(x, h_sk.data(), sk_l, h_sk.size() * 8));
            uint64_t *low = dev(B * ctw), *low3 = dev((size_t)B * 3 * l * n), *a = dev(B * ctw), *b2 = dev(B * ctw), *o3 = dev((size_t)B * 3 * l * n);
            CHECK(hhe_mod_switch(c, top, 2, B, L, l, low));
            CHECK(hhe_mod_switch(c, top3, 3, B, L, l, low3));
            CHECK(hhe_ctx_reserve(x, B));
            // rotations (a key, NAF terms, columns), checked through decryption
            CHECK(hhe_rotate_rows_ks(x, dl, low, 1, a, B));
            CHECK(hhe_rotate_rows_ks(x, dl, low, 3, b2, B));
            CHECK(hhe_rotate_columns_ks(x, dl, low, b2, B));
            CHECK(hhe_ctx_sync(x));
            int32_t budget[B];
            uint32_t bits[B];
            CHECK(hhe_noise_budget(x, h_sk.data(), a, 2, l, B, budget, bits));
            REQUIRE(budget[0] > 0 && budget[1] > 0);
            uint64_t *slots = dev(B * n);
            std::vector<uint64_t> h_slots((size_t)B * n);
            CHECK(hhe_decrypt(x, h_sk.data(), a, B, slots));
            CHECK(hhe_copy_d2h(x, h_slots.data(), slots, h_slots.size() * 8));
            for (int b = 0; b < B; b++)
                for (size_t i = 0; i < n; i++) {
                    const size_t h = n / 2, row = i / h, col = (i % h + 1) % h;
                    REQUIRE(h_slots[b * n + i] == vals[b * n + row * h + col]);
                }
            // multiply, relinearize (also of the product switched at size 3), mask, flatten, an FC row, affine layers, encryption
            CHECK(hhe_multiply(x, low, a, o3, B));
            CHECK(hhe_relinearize_ks(x, dl, o3, b2, B));
            CHECK(hhe_relinearize_ks(x, dl, low3, b2, B));
            std::vector<uint64_t> mv(44, 1);
            CHECK(hhe_mask(x, low, mv.data(), mv.size(), b2, B));
            CHECK(hhe_flatten_ks(x, dl, low, 2, b2, 1));
            CHECK(hhe_fc_row_ks(x, dl, dl, low, a, 1, 9, b2, B));
            std::vector<uint64_t> M(16 * 16), bias(16);
            for (size_t i = 0; i < M.size(); i++) M[i] = (7 * i + 1) % t;
            for (size_t i = 0; i < bias.size(); i++) bias[i] = i + 1;
            for (int bsgs = 0; bsgs < 2; bsgs++) {
                hhe_matrix *m = nullptr;
                CHECK(hhe_matrix_create(x, M.data(), 16, bias.data(), bsgs ? 4 : 0, bsgs ? 4 : 0, &m));
                CHECK(hhe_packed_affine_ks(x, dl, m, low, b2, B));
                if (bsgs) hhe_matrix_destroy(m);  // the other handle is left to its context
            }
            CHECK(hhe_encrypt(x, pk_l, plain, 0, seed, B, b2));
            CHECK(hhe_decrypt(x, h_sk.data(), b2, B, slots));
            CHECK(hhe_copy_d2h(x, h_slots.data(), slots, h_slots.size() * 8));
            REQUIRE(h_slots == vals);
            // transciphering at the level: any ciphertext serves as the key ciphertext here, the words are not looked at
            {
                const size_t items = 13;  // past the threshold of the shared first layer
                std::vector<uint64_t> cw(items * 128), idx(items);
                std::vector<uint32_t> ncw(items, 128);
                for (size_t i = 0; i < cw.size(); i++) cw[i] = (11 * i + 5) % t;
                for (size_t i = 0; i < items; i++) idx[i] = i % 2;
                uint64_t *tout = dev(items * ctw);
                CHECK(hhe_pasta3_transcipher_ks(x, dl, dl, low, cw.data(), ncw.data(), idx.data(), items, 0, tout));
                CHECK(hhe_pasta3_transcipher_ks(x, dl, dl, low, cw.data(), ncw.data(), idx.data(), 2, 0, tout));
                hhe_free(tout);
            }
            // derived again (the tables built from the first derivation go), and a level of a level
            CHECK(hhe_keyset_derive_level(dl, ks));
            CHECK(hhe_rotate_rows_ks(x, dl, low, 1, a, B));
            CHECK(hhe_fc_row_ks(x, dl, dl, low, a, 1, 9, b2, B));
            hhe_ctx *xx = nullptr;
            CHECK(hhe_ctx_create_level(x, 1, &xx));
            hhe_keyset *dll = nullptr;
            CHECK(hhe_keyset_create(xx, &dll));
            CHECK(hhe_keyset_derive_level(dll, dl));
            if (l > 1) EXPECT(hhe_keyset_derive_level(dl, dll), HHE_ERR_INVALID);
            uint64_t *one = dev((size_t)B * 2 * n);
            CHECK(hhe_mod_switch(x, low, 2, B, l, 1, one));
            CHECK(hhe_rotate_rows_ks(xx, dll, one, -1, one, B));
            CHECK(hhe_ctx_sync(xx));
            hhe_ctx_destroy(xx);  // with its set
            CHECK(hhe_ctx_sync(x));
            for (uint64_t *p : {sk_l, pk_l, low, low3, a, b2, o3, slots, one}) hhe_free(p);
            hhe_keyset_destroy(up);
            if (l == 1) kept = x;         // dl stays with it
            else { hhe_keyset_destroy(dl); hhe_ctx_destroy(x); }
        }
        hhe_ctx_destroy(c);  // the parent first: with ks
        // the level context is independent of the parent it was made from
        {
            uint64_t *ct = dev((size_t)B * 2 * n), *pl = dev(B * n);
            std::vector<uint64_t> zeros((size_t)B * 2 * n, 0);
            CHECK(hhe_copy_h2d(kept, pl, zeros.data(), (size_t)B * n * 8));
            CHECK(hhe_copy_h2d(kept, ct, zeros.data(), zeros.size() * 8));
            CHECK(hhe_add_plain(kept, ct, pl, 0, 0, ct, B));
            CHECK(hhe_ctx_sync(kept));
            hhe_free(ct); hhe_free(pl);
        }
        hhe_ctx_destroy(kept);
        for (uint64_t *p : {sk, pk, d_vals, plain, top, top3}) hhe_free(p);
        printf("logn %d ok\n", logn);
    }
    return 0;
}
