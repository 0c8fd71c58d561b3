// keygen_main.cpp -- the SEAL-free adapter (include/pasta_seal_gfx950.hpp) with no key from anywhere else: keygen, create_relin_keys,
// create_gk, encrypt_key_2 on the device from two seeds, the plain cipher, one decomposition, decrypting.  Input / output are raw
// uint64 blobs written / read by tests/test_cpp_keygen.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pasta_seal_gfx950.hpp"
#include "driver_common.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    auto hdr = read_words(f, 4);  // logn, K, t, plaintext words
    const int logn = (int)hdr[0], K = (int)hdr[1];
    auto q = read_words(f, K);
    auto ssk = read_words(f, 256);
    auto pt = read_words(f, hdr[3]);
    fclose(f);
    uint8_t seed_a[32], seed_b[32];
    for (int i = 0; i < 32; i++) { seed_a[i] = (uint8_t)i; seed_b[i] = (uint8_t)(7 * i + 3); }
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, hdr[2], 0);
        pasta::SecretKey sk;
        pasta::PublicKey pk;
        pasta::RelinKeys rk;
        pasta::keygen(*ctx, seed_a, sk, pk);
        pasta::create_relin_keys(*ctx, sk, seed_b, rk);
        pasta::PASTA_SEAL HHE(ctx, pk, sk, rk, pasta::GaloisKeys{});
        HHE.add_gk_indices();
        HHE.create_gk(seed_b);
        const pasta::GaloisKeys &gk = HHE.get_galois_keys();
        printf("galois keys:");
        for (auto &kv : gk.keys) printf(" %u", kv.first);
        printf("\n");
        auto enc_ssk = HHE.encrypt_key_2(ssk, seed_b);
        pasta::PASTA cipher(ctx, ssk, hdr[2]);
        auto sym = cipher.encrypt(pt);
        auto blocks = HHE.decomposition(sym, enc_ssk);
        auto vals = sealhelper::decrypting(blocks[0], sk, *ctx, pt.size());
        FILE *o = fopen(argv[2], "wb");
        put(o, sk.words); put(o, pk.words); put(o, rk.key);
        for (auto &kv : gk.keys) { put(o, std::vector<uint64_t>(1, kv.first)); put(o, kv.second); }
        put(o, enc_ssk[0].words); put(o, sym); put(o, blocks[0].words);
        put(o, std::vector<uint64_t>(vals.begin(), vals.end()));
        fclose(o);
        printf("blocks: %zu, key set uploads: %llu\n", blocks.size(), (unsigned long long)ctx->keys().uploads());
        printf("backend: %s\n", hhe_backend());
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
