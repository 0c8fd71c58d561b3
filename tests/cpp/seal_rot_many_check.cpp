// TESTS ONLY -- type-checks the hoisted rotations and the hoisted packed encrypted FC of include/pasta_seal_gfx950_seal.hpp
// (pasta::SEALZpCipher::rotate_rows_many, sealhelper::rotate_rows_many, sealhelper::fc_packed_hoisted, pasta::SEALZpLevel::rotate_rows_many /
// fc_packed_hoisted) against the reference's SEAL 4.0.0 headers: a CSP that rotates one flattened record by many steps and evaluates the
// whole layer with its chain hoisted, at the data level and at a level.
// Compiled with g++ -fsyntax-only (tests/test_cpp_rot_many.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_hoisted(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                 GaloisKeys csp_gk, RelinKeys csp_rk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key,
                 vector<Ciphertext> enc_weight_diagonals, size_t rows, size_t cols, const Evaluator &evaluator, vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    Ciphertext flat, logits;
    HHE.flatten(blocks, flat, csp_gk);
    // many rotations of one ciphertext: the member and the free function
    vector<int> steps{1, 2, 3, -5, 0};
    vector<Ciphertext> rotations;
    HHE.rotate_rows_many(flat, steps, analyst_gk, rotations);
    sealhelper::rotate_rows_many(flat, steps, analyst_gk, rotations, evaluator);
    // once per model, once per record
    sealhelper::EncMatrix W(context, enc_weight_diagonals, rows, cols);
    sealhelper::fc_packed_hoisted(flat, W, csp_rk, analyst_gk, logits);

    // the same at a level
    const size_t levels_from_last = 3;
    HHE.get_cipher_size(flat, true, levels_from_last);
    for (Ciphertext &d : enc_weight_diagonals) HHE.get_cipher_size(d, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    LV.rotate_rows_many(flat, steps, analyst_gk, rotations);
    sealhelper::EncMatrix WL = LV.enc_matrix(enc_weight_diagonals, rows, cols);
    LV.fc_packed_hoisted(flat, WL, csp_rk, analyst_gk, logits);
    result = LV.decrypting(logits, rows);
}
