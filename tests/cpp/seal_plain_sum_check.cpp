// TESTS ONLY -- type-checks the plain-weights FC of include/pasta_seal_gfx950_seal.hpp (SEALZpCipher::plain_fc_open / fc_open_plain /
// rotate_plain_sum, the level object's, sealhelper::fc_open_plain / rotate_plain_sum) against the reference's SEAL 4.0.0 headers: a CSP
// that holds the model of the one-layer network in the clear, at the data level and at a level.
// Compiled with g++ -fsyntax-only (tests/test_cpp_plain_sum.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_plain_layer(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                     GaloisKeys csp_gk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key, vector<vector<uint64_t>> fc1_weights,
                     vector<uint64_t> fc1_bias, vector<vector<uint64_t>> kernel_rows, vector<int> kernel_steps, vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    Ciphertext flat, logits, conv;
    HHE.flatten(blocks, flat, csp_gk);
    // once per model
    HHE.plain_fc_open(fc1_weights, fc1_bias);
    HHE.plain_fc_open(fc1_weights);
    // once per record
    HHE.fc_open_plain(flat, fc1_weights, fc1_bias, analyst_gk, logits);
    sealhelper::fc_open_plain(flat, fc1_weights, fc1_bias, analyst_gk, logits);
    HHE.rotate_plain_sum(flat, kernel_rows, kernel_steps, analyst_gk, conv);
    sealhelper::rotate_plain_sum(flat, kernel_rows, kernel_steps, analyst_gk, conv);

    // the same at a level
    const size_t levels_from_last = 3;
    HHE.get_cipher_size(flat, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    LV.plain_fc_open(fc1_weights, fc1_bias);
    LV.fc_open_plain(flat, fc1_weights, fc1_bias, analyst_gk, logits);
    LV.rotate_plain_sum(flat, kernel_rows, kernel_steps, analyst_gk, conv);
    result = LV.decrypting(logits, fc1_weights.size());
}
