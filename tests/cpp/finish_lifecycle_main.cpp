// finish_lifecycle_main.cpp -- host side of the transciphering call's finishing pass (the context's host staging and device block, the
// pointer table into the keystream cache), stand-alone for a sanitizer build against the emulator sources (no GPU, nothing loaded into
// another process):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iinclude -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/finish_lifecycle_main.cpp tests/emu/hhe_launch_emu.cpp \
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_{api,context,pasta_public,client,seal_wire}.cpp -ldl -o finish_lifecycle
// Create a context (fused and unfused finishing pass), call with growing and shrinking batches against kept keystreams, replace a key,
// reserve beyond every batch so far, call again, destroy with keystreams resident.  The two contexts must return the same words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hhe_gfx950.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, hhe_last_error()); exit(1); } } while (0)

int main()
{
    const int logn = 10, K = 3, L = 2;
    const size_t n = (size_t)1 << logn, ctw = 2 * L * n;
    uint64_t q[3];
    {
        size_t cnt = 64;
        uint64_t all[64];
        CHECK(hhe_bfv_default_coeff_modulus(16384, all, &cnt));  // 48/49-bit primes = 1 mod 32768, valid for every smaller N
        q[0] = all[0]; q[1] = all[1]; q[2] = all[3];
    }
    std::vector<std::vector<uint64_t>> results[2];
    for (int fused = 1; fused >= 0; fused--) {
        setenv("HHE_FIN_FUSED", fused ? "1" : "0", 1);
        hhe_ctx *c = nullptr;
        CHECK(hhe_ctx_create(logn, K, q, 65537, 0, &c));
        if (hhe_ctx_query(c, "fin_fused", 0) != (uint64_t)fused) { fprintf(stderr, "fin_fused reads %d\n", (int)hhe_ctx_query(c, "fin_fused", 0)); return 1; }
        uint8_t seed[32], seed2[32];
        for (int i = 0; i < 32; i++) { seed[i] = (uint8_t)i; seed2[i] = (uint8_t)(200 - i); }
        uint64_t *sk = (uint64_t *)hhe_malloc(K * n * 8), *pk = (uint64_t *)hhe_malloc(2 * K * n * 8);
        CHECK(hhe_keygen_secret(c, seed, sk));
        CHECK(hhe_keygen_public(c, sk, seed, pk));
        hhe_keyset *ks = nullptr;
        CHECK(hhe_keyset_create(c, &ks));
        CHECK(hhe_keyset_generate_galois(ks, sk, nullptr, 0, seed));  // the default elements: steps -1, 128 and the column swap among them
        CHECK(hhe_keyset_generate_relin(ks, sk, seed));
        uint64_t *plain = (uint64_t *)hhe_malloc(n * 8), *key = (uint64_t *)hhe_malloc(ctw * 8);
        std::vector<uint64_t> pv(n);
        for (size_t i = 0; i < n; i++) pv[i] = (i * 2654435761ULL + 12345) % 65537;
        CHECK(hhe_copy_h2d(c, plain, pv.data(), n * 8));
        CHECK(hhe_encrypt(c, pk, plain, 1, seed2, 1, key));
        const size_t maxB = 9;
        uint64_t *out = (uint64_t *)hhe_malloc(maxB * ctw * 8);
        auto call = [&](size_t B, uint32_t len, uint64_t salt) {
            std::vector<uint64_t> cw(B * 128), idx(B);
            std::vector<uint32_t> ncw(B);
            for (size_t b = 0; b < B; b++) {
                idx[b] = b % 3;
                ncw[b] = b == 1 ? 0 : len;
                for (size_t i = 0; i < 128; i++) cw[b * 128 + i] = (b * 131 + i * 7 + salt) % 65537;
            }
            CHECK(hhe_pasta3_transcipher_ks(c, ks, ks, key, cw.data(), ncw.data(), idx.data(), B, 0, out));
            std::vector<uint64_t> h(B * ctw);
            CHECK(hhe_copy_d2h(c, h.data(), out, B * ctw * 8));
            results[fused].push_back(h);
        };
        call(1, 128, 1);   // one evaluation
        call(9, 128, 2);   // the staging and the device block grow; counter 0 is kept, 1 and 2 are evaluated
        call(2, 5, 3);     // short blocks where the last call had full ones; every counter kept
        if (hhe_ctx_query(c, "ks_cache_hits", 0) != 2) { fprintf(stderr, "expected two kept keystreams\n"); return 1; }
        CHECK(hhe_keyset_generate_relin(ks, sk, seed2));  // replace a key: what was kept under the old one goes
        call(4, 77, 4);
        if (hhe_ctx_query(c, "ks_cache_hits", 0) != 0 || hhe_ctx_query(c, "transcipher_evaluated", 0) != 3) { fprintf(stderr, "a replaced key kept its keystreams\n"); return 1; }
        CHECK(hhe_ctx_reserve(c, 16));
        call(9, 1, 5);
        hhe_keyset_destroy(ks);
        hhe_free(sk); hhe_free(pk); hhe_free(plain); hhe_free(key); hhe_free(out);
        hhe_ctx_destroy(c);  // keystreams and a snapshot resident
        printf("fin_fused %d ok\n", fused);
    }
    if (results[0] != results[1]) { fprintf(stderr, "fused and unfused finishing passes differ\n"); return 1; }
    printf("same words\n");
    return 0;
}
