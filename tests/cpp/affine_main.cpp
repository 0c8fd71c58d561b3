// affine_main.cpp -- drives SEALZpCipher::packed_matMul / packed_affine of include/pasta_seal_gfx950.hpp (the SEAL-free adapter): two
// requests, each building its own cipher object from the same key objects and applying the same public matrix, by the diagonal method
// and by babystep-giantstep.  Input / output are raw uint64 blobs written / read by tests/test_cpp_affine.py.
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
    auto hdr = read_words(f, 8);  // logn, K, t, n_galois, dim, n1, n2, requests
    const int logn = (int)hdr[0], K = (int)hdr[1];
    const size_t n = (size_t)1 << logn, L = K - 1, ksk = L * 2 * K * n, ctw = 2 * L * n, dim = hdr[4], requests = hdr[7];
    auto q = read_words(f, K);
    pasta::GaloisKeys gk;
    for (uint64_t i = 0; i < hdr[3]; i++) {
        uint32_t elt = (uint32_t)read_words(f, 1)[0];
        gk.keys[elt] = read_words(f, ksk);
    }
    pasta::SEALZpCipher::matrix M(dim);
    for (auto &row : M) row = read_words(f, dim);
    pasta::SEALZpCipher::vector b = read_words(f, dim);
    std::vector<pasta::Ciphertext> in(requests);
    for (auto &ct : in) ct = pasta::Ciphertext{read_words(f, ctw), 2};
    fclose(f);
    try {
        auto ctx = std::make_shared<pasta::HheContext>(logn, q, hdr[2], 0);
        FILE *o = fopen(argv[2], "wb");
        std::vector<int> first_indices;
        for (int use_bsgs = 0; use_bsgs < 2; use_bsgs++) {
            for (size_t r = 0; r < requests; r++) {
                // one cipher object per request, built from the key objects by value (BaseCSP::decompose does the same, CSP.cpp:238-242)
                pasta::PASTA_SEAL HHE(ctx, pasta::PublicKey{}, pasta::SecretKey{}, pasta::RelinKeys{}, gk);
                HHE.activate_bsgs(use_bsgs != 0);
                HHE.set_bsgs_params(hdr[5], hdr[6]);
                if (use_bsgs) HHE.add_bsgs_indices(hdr[5], hdr[6]);
                else HHE.add_diagonal_indices(dim);
                printf("%s gk_indices:", use_bsgs ? "bsgs" : "diagonal");
                for (int s : HHE.get_gk_indices()) printf(" %d", s);
                printf("\n");
                pasta::Ciphertext mm, aff = in[r];
                HHE.packed_matMul(mm, M, in[r]);
                HHE.packed_affine(aff, M, aff, b);   // in place: vo and vi are the same object
                fwrite(mm.words.data(), 8, mm.words.size(), o);
                fwrite(aff.words.data(), 8, aff.words.size(), o);
            }
            // matMul + affine of one method are two handles (without and with the bias), whatever the number of requests
            printf("%s: matrix uploads: %llu, resident: %zu\n", use_bsgs ? "bsgs" : "diagonal", (unsigned long long)ctx->matrices().uploads(),
                   ctx->matrices().resident());
        }
        {   // a cipher object without the Galois key for step +1
            pasta::GaloisKeys none;
            pasta::PASTA_SEAL HHE(ctx, pasta::PublicKey{}, pasta::SecretKey{}, pasta::RelinKeys{}, none);
            pasta::Ciphertext out;
            try { HHE.packed_matMul(out, M, in[0]); printf("no throw\n"); }
            catch (const std::invalid_argument &e) { printf("throws: %s\n", e.what()); }
        }
        {   // too few slots: a matrix of dim with dim * 2 != N and dim * 4 > N
            pasta::PASTA_SEAL HHE(ctx, pasta::PublicKey{}, pasta::SecretKey{}, pasta::RelinKeys{}, gk);
            pasta::SEALZpCipher::matrix big(n / 4 + 1, pasta::SEALZpCipher::vector(n / 4 + 1, 1));
            pasta::Ciphertext out;
            try { HHE.packed_matMul(out, big, in[0]); printf("no throw\n"); }
            catch (const std::runtime_error &e) { printf("throws: %s\n", e.what()); }
        }
        fclose(o);
        printf("backend: %s\n", hhe_backend());
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
