// keygen_lifecycle_main.cpp -- host side of key generation into a key set, stand-alone for a sanitizer build against the emulator
// sources (no GPU, nothing loaded into another process):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/keygen_lifecycle_main.cpp tests/emu/hhe_launch_emu.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_{api,context,pasta_public,client,seal_wire}.cpp -ldl -o keygen_lifecycle
// Generate, rotate (builds what the context derives from a key), replace, failed lists, read back, destroy in both orders.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hhe_gfx950.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, hhe_last_error()); exit(1); } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s -> %d, expected %d\n", #x, rc_, (int)(code)); exit(1); } } while (0)

int main()
{
    for (int logn : {10, 12}) {  // separate-kernel path and the fused row kernel (Shoup tables per key)
        const size_t n = (size_t)1 << logn;
        uint64_t q[3];
        // three NTT primes from the library itself
        {
            size_t cnt = 64;
            uint64_t all[64];
            CHECK(hhe_bfv_default_coeff_modulus(16384, all, &cnt));  // 48/49-bit primes = 1 mod 32768, valid for every smaller N
            q[0] = all[0]; q[1] = all[1]; q[2] = all[3];
        }
        hhe_ctx *c = nullptr;
        CHECK(hhe_ctx_create(logn, 3, q, 65537, 0, &c));
        const int K = 3, L = 2;
        const size_t ksk = (size_t)L * 2 * K * n, ctw = 2 * L * n;
        uint8_t seed[32], seed2[32];
        for (int i = 0; i < 32; i++) { seed[i] = (uint8_t)i; seed2[i] = (uint8_t)(200 - i); }
        uint64_t *sk = (uint64_t *)hhe_malloc(K * n * 8), *pk = (uint64_t *)hhe_malloc(2 * K * n * 8);
        CHECK(hhe_keygen_secret(c, seed, sk));
        CHECK(hhe_keygen_public(c, sk, seed, pk));
        hhe_keyset *ks = nullptr, *ks2 = nullptr;
        CHECK(hhe_keyset_create(c, &ks));
        CHECK(hhe_keyset_create(c, &ks2));
        const uint32_t e1 = (uint32_t)hhe_ctx_query(c, "galois_elt", 1), em = (uint32_t)hhe_ctx_query(c, "galois_elt", -1);
        uint32_t elts[2] = {e1, em};
        CHECK(hhe_keyset_generate_galois(ks, sk, elts, 2, seed));
        CHECK(hhe_keyset_generate_relin(ks, sk, seed));
        CHECK(hhe_keyset_generate_galois(ks2, sk, nullptr, 0, seed));  // the default elements
        if (hhe_keyset_has_galois(ks2, (uint32_t)(2 * n - 1)) != 1 || hhe_keyset_has_galois(ks2, 3) != 1) { fprintf(stderr, "default set incomplete\n"); return 1; }
        // encrypt, rotate with the generated key, regenerate, rotate again
        uint64_t *plain = (uint64_t *)hhe_malloc(n * 8), *ct = (uint64_t *)hhe_malloc(ctw * 8), *out = (uint64_t *)hhe_malloc(ctw * 8);
        std::vector<uint64_t> zeros(n, 0), a(ctw), b(ctw), k_old(ksk), k_new(ksk);
        CHECK(hhe_copy_h2d(c, plain, zeros.data(), n * 8));
        CHECK(hhe_encrypt(c, pk, plain, 1, seed2, 1, ct));
        CHECK(hhe_rotate_rows_ks(c, ks, ct, 1, out, 1));
        CHECK(hhe_copy_d2h(c, a.data(), out, ctw * 8));
        CHECK(hhe_keyset_get_galois(ks, e1, k_old.data()));
        uint32_t bad1[2] = {e1, 4}, bad2[1] = {(uint32_t)(2 * n + 1)};
        EXPECT(hhe_keyset_generate_galois(ks, sk, bad1, 2, seed2), HHE_ERR_INVALID);
        EXPECT(hhe_keyset_generate_galois(ks, sk, bad2, 1, seed2), HHE_ERR_INVALID);
        EXPECT(hhe_keyset_generate_galois(ks, sk, nullptr, 1, seed2), HHE_ERR_INVALID);
        CHECK(hhe_keyset_get_galois(ks, e1, k_new.data()));
        if (k_old != k_new) { fprintf(stderr, "a failed list changed the set\n"); return 1; }
        CHECK(hhe_keyset_generate_galois(ks, sk, elts, 1, seed2));  // replace e1
        CHECK(hhe_keyset_get_galois(ks, e1, k_new.data()));
        if (k_old == k_new) { fprintf(stderr, "regeneration kept the old key\n"); return 1; }
        CHECK(hhe_rotate_rows_ks(c, ks, ct, 1, out, 1));
        CHECK(hhe_copy_d2h(c, b.data(), out, ctw * 8));
        if (a == b) { fprintf(stderr, "rotation still uses the old key\n"); return 1; }
        CHECK(hhe_keyset_generate_relin(ks, sk, seed2));  // replace the relin key
        EXPECT(hhe_keyset_get_galois(ks, 5, k_new.data()), hhe_keyset_has_galois(ks, 5) ? HHE_OK : HHE_ERR_NO_GALOIS_KEY);
        hhe_keyset *empty = nullptr;
        CHECK(hhe_keyset_create(c, &empty));
        EXPECT(hhe_keyset_get_relin(empty, k_new.data()), HHE_ERR_NO_RELIN_KEY);
        hhe_keyset_destroy(ks);          // a set destroyed before its context ...
        hhe_free(sk); hhe_free(pk); hhe_free(plain); hhe_free(ct); hhe_free(out);
        hhe_ctx_destroy(c);              // ... and two (ks2, empty) released by the context
        printf("logn %d ok\n", logn);
    }
    return 0;
}
