// nonce_main.cpp -- drives the SEAL-free adapter (include/pasta_seal_gfx950.hpp) under caller's nonces: the client encrypts two records
// under two nonces, the server transciphers one with `decomposition(..., nonce)` and both with `decompose(..., nonces)`.
// Input/output are raw uint64 blobs written/read by tests/test_cpp_nonce.py, which compares the words with the C ABI's.
//
// The host side as a stand-alone program under the sanitizers, against the emulator sources instead of the emulator library (no
// device code, nothing loaded into another process), from the repository root:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK -Iinclude
//       -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/nonce_main.cpp tests/emu/hhe_launch_emu.cpp tests/emu/emu_order.cpp
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_api.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_context.cpp
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_pasta_public.cpp privacy-preserving-ml-through-hhe_amd/csrc/hhe_client.cpp
//       privacy-preserving-ml-through-hhe_amd/csrc/hhe_seal_wire.cpp -ldl -o nonce_asan
//   ./nonce_asan in.bin out.bin        (in.bin: what tests/test_cpp_nonce.py writes; it keeps the file when NONCE_KEEP_BLOB names a path)
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
    auto hdr = read_words(f, 7);  // logn, K, t, n_galois, n_words, nonce 0, nonce 1
    const int logn = (int)hdr[0], K = (int)hdr[1];
    const size_t n = (size_t)1 << logn, L = K - 1, ksk = L * 2 * K * n, ctw = 2 * L * n, nwords = hdr[4];
    const uint64_t nonce0 = hdr[5], nonce1 = hdr[6];
    auto q = read_words(f, K);
    pasta::RelinKeys rk{read_words(f, ksk)};
    pasta::GaloisKeys gk;
    for (uint64_t i = 0; i < hdr[3]; i++) {
        uint32_t elt = (uint32_t)read_words(f, 1)[0];
        gk.keys[elt] = read_words(f, ksk);
    }
    pasta::Ciphertext enc_key{read_words(f, ctw), 2};
    auto sym_key = read_words(f, 256);
    auto plain0 = read_words(f, nwords), plain1 = read_words(f, nwords);
    fclose(f);
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, hdr[2], 0);
        // client (User.cpp): PASTA::encrypt under a nonce per record
        pasta::PASTA sym(ctx, sym_key, hdr[2]);
        auto ct0 = sym.encrypt(plain0, nonce0), ct1 = sym.encrypt(plain1, nonce1);
        auto back0 = sym.decrypt(ct0, nonce0), wrong = sym.decrypt(ct0, nonce1), fixed = sym.encrypt(plain0);
        if (back0 != plain0 || wrong == plain0 || fixed == ct0 || sym.encrypt(plain0, 123456789) != fixed) { printf("client round trip failed\n"); return 1; }
        // server (CSP.cpp:238-278)
        pasta::PASTA_SEAL HHE(ctx, pasta::PublicKey{}, pasta::SecretKey{}, rk, gk);
        HHE.add_gk_indices();
        std::vector<pasta::Ciphertext> blocks = HHE.decomposition(ct0, {enc_key}, true, nonce0);
        std::vector<pasta::Ciphertext> recs = HHE.decompose({ct0, ct1}, {enc_key}, gk, true, {nonce0, nonce1});
        bool threw = false;
        try { HHE.decompose({ct0, ct1}, {enc_key}, gk, true, {nonce0}); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) { printf("a nonce list of the wrong length was accepted\n"); return 1; }
        FILE *o = fopen(argv[2], "wb");
        if (!o) return 2;
        uint64_t nb = blocks.size();
        fwrite(&nb, 8, 1, o);
        put(o, ct0), put(o, ct1);
        for (auto &b : blocks) put(o, b.words);
        for (auto &r : recs) put(o, r.words);
        fclose(o);
        printf("nonce driver OK on %s\n", hhe_backend());
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
