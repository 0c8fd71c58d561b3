// TESTS ONLY -- type-checks the one-floor packed encrypted FC of include/pasta_seal_gfx950_seal.hpp (sealhelper::fc_packed_sum,
// sealhelper::EncMatrix::apply_sum, pasta::SEALZpLevel::fc_packed_sum) against the reference's SEAL 4.0.0 headers: a CSP that evaluates
// the whole layer with one BEHZ floor per record, with either rotation schedule, at the data level and at a level.
// Compiled with g++ -fsyntax-only (tests/test_cpp_fc_sum.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_one_floor(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                   GaloisKeys csp_gk, RelinKeys csp_rk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key,
                   vector<Ciphertext> enc_weight_diagonals, size_t rows, size_t cols, vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    Ciphertext flat, logits;
    HHE.flatten(blocks, flat, csp_gk);
    // once per model, once per record
    sealhelper::EncMatrix W(context, enc_weight_diagonals, rows, cols);
    sealhelper::fc_packed_sum(flat, W, csp_rk, analyst_gk, logits);
    sealhelper::fc_packed_sum(flat, W, csp_rk, analyst_gk, logits, true);
    W.apply_sum(flat, csp_rk, analyst_gk, logits, true);

    // the same at a level
    const size_t levels_from_last = 3;
    HHE.get_cipher_size(flat, true, levels_from_last);
    for (Ciphertext &d : enc_weight_diagonals) HHE.get_cipher_size(d, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    sealhelper::EncMatrix WL = LV.enc_matrix(enc_weight_diagonals, rows, cols);
    LV.fc_packed_sum(flat, WL, csp_rk, analyst_gk, logits);
    LV.fc_packed_sum(flat, WL, csp_rk, analyst_gk, logits, true);
    result = LV.decrypting(logits, rows);
}
