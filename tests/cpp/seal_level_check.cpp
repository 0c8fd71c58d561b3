// TESTS ONLY -- type-checks the level object of include/pasta_seal_gfx950_seal.hpp (pasta::SEALZpCipher::level, pasta::SEALZpLevel)
// against the reference's SEAL 4.0.0 headers: a CSP that switches a decomposition result and the weight rows once and runs the rest
// at that level.  Compiled with g++ -fsyntax-only (tests/test_cpp_level.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_at_a_level(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                    GaloisKeys csp_gk, RelinKeys csp_rk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key, Ciphertext enc_weight_row,
                    pasta::SEALZpCipher::matrix &M, pasta::SEALZpCipher::vector &bias, int inputLen, vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    const size_t levels_from_last = 3;
    for (Ciphertext &b : blocks) HHE.get_cipher_size(b, true, levels_from_last);
    HHE.get_cipher_size(enc_weight_row, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    parms_id_type id = LV.parms_id();
    (void)id;
    vector<uint64_t> mask(inputLen % 128, 1);
    LV.mask(blocks.back(), mask);
    Ciphertext flat, prod, sum, aff, sq;
    LV.flatten(blocks, flat, csp_gk);
    LV.packed_enc_mul(flat, enc_weight_row, prod);
    LV.relinearize_inplace(prod, csp_rk);
    LV.encrypted_vec_sum(prod, sum, analyst_gk, (size_t)inputLen);
    LV.packed_enc_add(sum, sum, sum);
    LV.packed_affine(aff, M, flat, bias);
    LV.packed_matMul(aff, M, flat);
    LV.packed_square(sq, aff);
    int budget = LV.print_noise(sq);
    (void)budget;
    result = LV.decrypting(sq, 16);
}
