// TESTS ONLY -- type-checks the chainable packed FC of include/pasta_seal_gfx950_seal.hpp (the open kind of sealhelper::EncMatrix,
// SEALZpCipher::enc_matrix_open / fc_open / mlp, the level object's, sealhelper::fc_open / mlp) against the reference's SEAL 4.0.0
// headers: a CSP that finishes the two-layer network the reference's example leaves at its TODOs, at the data level and at a level.
// Compiled with g++ -fsyntax-only (tests/test_cpp_mlp.py); never linked or run.
#include "pasta_seal_gfx950_seal.hpp"

using namespace seal;
using namespace std;

void csp_two_layers(shared_ptr<SEALContext> context, PublicKey analyst_pk, SecretKey csp_sk, RelinKeys analyst_rk, GaloisKeys analyst_gk,
                    GaloisKeys csp_gk, RelinKeys csp_rk, vector<uint64_t> &record, vector<Ciphertext> user_enc_sym_key,
                    vector<Ciphertext> enc_fc1_diagonals, vector<Ciphertext> enc_fc2_diagonals, size_t hidden, size_t inputs, size_t outputs,
                    vector<int64_t> &result)
{
    pasta::PASTA_SEAL HHE(context, analyst_pk, csp_sk, analyst_rk, analyst_gk);
    vector<Ciphertext> blocks = HHE.decomposition(record, user_enc_sym_key, true);
    Ciphertext flat, logits, y1, x2;
    HHE.flatten(blocks, flat, csp_gk);
    // once per model
    sealhelper::EncMatrix fc1 = HHE.enc_matrix_open(enc_fc1_diagonals, hidden, inputs), fc2 = HHE.enc_matrix_open(enc_fc2_diagonals, outputs, hidden);
    // once per record: the network in one call, or layer by layer
    sealhelper::mlp({&fc1, &fc2}, flat, csp_rk, analyst_gk, logits);
    HHE.mlp({&fc1, &fc2}, flat, csp_rk, analyst_gk, logits);
    sealhelper::fc_open(flat, fc1, csp_rk, analyst_gk, y1);
    HHE.packed_square(x2, y1);
    HHE.fc_open(x2, fc2, csp_rk, analyst_gk, logits);
    fc2.apply_open(x2, csp_rk, analyst_gk, logits);
    bool kinds = fc1.open && !sealhelper::EncMatrix(context, enc_fc2_diagonals, outputs, hidden).open;

    // the same at a level
    const size_t levels_from_last = 3;
    HHE.get_cipher_size(flat, true, levels_from_last);
    for (Ciphertext &d : enc_fc1_diagonals) HHE.get_cipher_size(d, true, levels_from_last);
    for (Ciphertext &d : enc_fc2_diagonals) HHE.get_cipher_size(d, true, levels_from_last);
    pasta::SEALZpLevel LV = HHE.level(levels_from_last);
    sealhelper::EncMatrix l1 = LV.enc_matrix_open(enc_fc1_diagonals, hidden, inputs), l2 = LV.enc_matrix_open(enc_fc2_diagonals, outputs, hidden);
    LV.mlp({&l1, &l2}, flat, csp_rk, analyst_gk, logits);
    LV.fc_open(flat, l1, csp_rk, analyst_gk, y1);
    LV.packed_square(x2, y1);
    LV.fc_open(x2, l2, csp_rk, analyst_gk, logits);
    result = LV.decrypting(logits, outputs);
    (void)kinds;
}
