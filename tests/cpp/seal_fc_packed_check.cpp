// TESTS ONLY -- type-checks the packed encrypted FC of include/pasta_seal_gfx950_seal.hpp (sealhelper::EncMatrix, sealhelper::fc_packed,
// pasta::SEALZpLevel::enc_matrix / fc_packed) against the reference's SEAL 4.0.0 headers: a CSP that receives the analyst's encrypted
// generalized diagonals once per model and evaluates the whole layer per record, at the data level and at a level.
// Compiled with g++ -fsyntax-only (tests/test_cpp_fc_packed.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_packed_fc(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                   GaloisKeys csp_gk, RelinKeys csp_rk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key,
                   vector<Ciphertext> enc_weight_diagonals, size_t rows, size_t cols, vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    Ciphertext flat, logits;
    HHE.flatten(blocks, flat, csp_gk);
    // once per model
    sealhelper::EncMatrix W(context, enc_weight_diagonals, rows, cols);
    // once per record
    sealhelper::fc_packed(flat, W, csp_rk, analyst_gk, logits);

    // the same at a level: record and diagonals switched once, the handle made on the level's context
    const size_t levels_from_last = 3;
    HHE.get_cipher_size(flat, true, levels_from_last);
    for (Ciphertext &d : enc_weight_diagonals) HHE.get_cipher_size(d, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    sealhelper::EncMatrix WL = LV.enc_matrix(enc_weight_diagonals, rows, cols);
    LV.fc_packed(flat, WL, csp_rk, analyst_gk, logits);
    result = LV.decrypting(logits, rows);
}
