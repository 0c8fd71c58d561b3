// pasta_seal_gfx950.hpp -- C++ host-side mirror of the reference's cipher-layer interface for the
// CSP hot path, implemented over the C ABI of libhhe_gfx950.so (include/hhe_gfx950.h).
//
// Mirrors (same names, argument meaning and error behaviour):
//   pasta::SEALZpCipher   src/pasta/SEAL_Cipher.h:11-129   (get_plain_size, mask, flatten, activate_bsgs, ...)
//   pasta::PASTA_SEAL     src/pasta/pasta_3_seal.h:8-54    (HE_decrypt, decomposition, add_gk_indices, ...)
//   sealhelper::packed_enc_multiply / encrypted_vec_sum   src/util/sealhelper.h:84-129
//   pasta::PASTA          src/pasta/pasta_3_plain.h:17-30  (client side: encrypt / decrypt)
//   sealhelper::decrypting                                 src/util/sealhelper.cpp:252-266 (analyst side)
//   KeyGenerator as the parties use it (Analyst.cpp:38-93), SEALZpCipher::create_gk (SEAL_Cipher.cpp:359) and
//   PASTA_SEAL::encrypt_key_2 (pasta_3_seal.cpp:23-38): keys and the encrypted PASTA key made on the device from a 32-byte seed the
//   caller supplies -- the only entropy, fresh for every call (include/hhe_gfx950.h)
// The reference passes seal:: objects; SEAL is not linked here, so the boundary types below are plain
// word containers with SEAL's in-memory layouts (what Ciphertext::data(), KSwitchKeys::data() hold).
// What lives here: those containers, the context class, the boundary policy (pasta::Boundary: validity checks and conversions between
// the containers and plain words), the members only this world has (the client's PASTA, key generation and encryption from a seed,
// set_encrypted_key, decrypting, invariant_noise_budget) and one-line forwards where a signature is spelled per header.  The encrypted
// matrix, the level object, the cipher classes' device members and the free functions' bodies are the templates of
// hhe_adapter_front.hpp instantiated with that policy -- the same source text pasta_seal_gfx950_seal.hpp instantiates on seal:: types
// -- over the call bodies of hhe::AdapterCore (hhe_adapter_core.hpp); this header is the one the tests execute.  Errors surface as the
// C++ exceptions the reference / SEAL throw (std::runtime_error, std::invalid_argument, std::logic_error).
#pragma once
#include <cstdint>
#include <iostream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "hhe_adapter_front.hpp"

namespace pasta {

struct ZpCipherParams {  // src/pasta/Cipher.h:14-18
    size_t key_size, plain_size, cipher_size;
};
constexpr ZpCipherParams PASTA_PARAMS = {256, 128, 128};  // src/pasta/pasta_3_plain.h:15

// seal::Ciphertext stand-in: data() words, [size][L][N], data level, non-NTT form.  limbs: coeff_modulus_size() of a ciphertext that
// get_cipher_size switched down ([size][limbs][N]); 0 = the data level, which is all that a cipher object's evaluation accepts -- a
// switched ciphertext is evaluated by the object of its level (SEALZpCipher::level)
struct Ciphertext {
    std::vector<uint64_t> words;
    size_t size = 0;
    size_t limbs = 0;
};
// one KSwitchKeys::data()[index] entry: [L digits][2][K][N], NTT form
typedef std::vector<uint64_t> KSwitchKey;
struct RelinKeys { KSwitchKey key; };                       // RelinKeys::key(2)
struct GaloisKeys { std::map<uint32_t, KSwitchKey> keys; }; // by Galois element (GaloisKeys::get_index = (elt-1)/2)
struct PublicKey { std::vector<uint64_t> words; };          // PublicKey::data(): [2][K][N], NTT form (read by encrypt_key_2 only)
struct SecretKey { std::vector<uint64_t> words; };          // SecretKey::data(): [K][N], NTT form
typedef const uint8_t *Seed;                                // 32 bytes: the only entropy of a key-generation call / an encryption

// seal::SEALContext stand-in: (N, coeff_modulus incl. the special prime, plain_modulus) plus everything the adapter core keeps per
// context (keys(): the key-set cache, key_uploads); max_key_sets is the cache's capacity
class HheContext : public hhe::AdapterCore {
public:
    HheContext(int logn, std::vector<uint64_t> coeff_modulus, uint64_t plain_modulus, int device = 0, size_t max_key_sets = 16, size_t max_matrices = 8)
    try : hhe::AdapterCore(logn, coeff_modulus, plain_modulus, device, max_key_sets, max_matrices) {}
    catch (const std::invalid_argument &e) { throw std::invalid_argument(std::string("encryption parameters are not set correctly: ") + e.what()); }
};

// the boundary policy of hhe_adapter_front.hpp on the word containers.  A level is named by its data primes; 0 = the chain's data level,
// which is what the results of a cipher object, a free function and a top-level encrypted matrix carry
struct Boundary {
    typedef pasta::Ciphertext Ciphertext;
    typedef pasta::RelinKeys RelinKeys;
    typedef pasta::GaloisKeys GaloisKeys;
    typedef pasta::SecretKey SecretKey;
    typedef HheContext Context;
    typedef std::shared_ptr<HheContext> Binding;
    typedef size_t Level;
    static std::shared_ptr<Context> chain(const Binding &con) { return con; }
    static Level top(const Context &) { return 0; }
    static Level level_id(const Context &ctx, size_t levels_from_last) { return ctx.level_limbs(levels_from_last); }
    static size_t limbs_of(const Context &ctx, Level id) { return id ? id : ctx.data_limbs(); }
    static const uint64_t *in(const Context &ctx, Level id, const Ciphertext &ct, size_t size)
    {
        const size_t l = limbs_of(ctx, id);
        const bool at_level = ct.limbs == l || (ct.limbs == 0 && l == ctx.data_limbs());
        return ct.words.size() == size * l * ctx.poly_modulus_degree() && at_level ? ct.words.data() : nullptr;
    }
    static const uint64_t *in_any(const Context &ctx, const Ciphertext &ct)
    {
        const bool ok = ct.size >= 2 && ct.limbs <= ctx.data_limbs() && ct.words.size() == ct.size * limbs_of(ctx, ct.limbs) * ctx.poly_modulus_degree();
        return ok ? ct.words.data() : nullptr;
    }
    static auto out(const Context &ctx, Level id, Ciphertext &ct, size_t size)
    {
        return [&ctx, &ct, id, size](size_t) {
            ct.words.resize(size * limbs_of(ctx, id) * ctx.poly_modulus_degree());
            ct.size = size;
            ct.limbs = id;
            return ct.words.data();
        };
    }
    static size_t size(const Ciphertext &ct) { return ct.size; }
    static size_t limbs(const Ciphertext &ct) { return ct.limbs; }
    static hhe::RelinWords words(const RelinKeys &rk) { return {rk.key.data(), rk.key.size(), {}}; }
    static hhe::GaloisWords words(const GaloisKeys &gk)
    {
        hhe::GaloisWords g;
        for (auto &kv : gk.keys) g.keys.emplace_back(kv.first, kv.second.data());
        if (!gk.keys.empty()) g.words = gk.keys.begin()->second.size();
        return g;
    }
    static std::pair<const uint64_t *, size_t> secret(const SecretKey &sk) { return {sk.words.data(), sk.words.size()}; }
};

namespace detail {
// the sink of a data-level result, for callers of the context's own members (HheContext::encrypt)
inline auto into(const HheContext &ctx, Ciphertext &ct, size_t size = 2) { return Boundary::out(ctx, Boundary::top(ctx), ct, size); }
}  // namespace detail

typedef hhe::EncMatrixT<Boundary> EncMatrix;

// What SEALZpCipher::level(levels_from_last) returns (hhe::LevelT): every member takes and produces ciphertexts with
// Ciphertext::limbs == limbs()
class SEALZpLevel : public hhe::LevelT<Boundary> {
public:
    SEALZpLevel(hhe::LevelT<Boundary> level) : hhe::LevelT<Boundary>(std::move(level)) {}
    size_t limbs() const { return id; }
};

class SEALZpCipher : public hhe::CipherT<Boundary> {
public:
    SEALZpCipher(ZpCipherParams params, std::shared_ptr<HheContext> con, PublicKey pk, SecretKey sk, RelinKeys rk, GaloisKeys gk)
        : hhe::CipherT<Boundary>(std::move(con), std::move(sk), rk, gk), params(params), he_pk(std::move(pk))
    {
        mod_degree = device->poly_modulus_degree();
        plain_mod = device->plain_modulus();
    }
    virtual ~SEALZpCipher() = default;

    size_t get_key_size() const { return params.key_size; }
    size_t get_plain_size() const { return params.plain_size; }
    size_t get_cipher_size() const { return params.cipher_size; }
    using hhe::CipherT<Boundary>::get_cipher_size;
    virtual std::string get_cipher_name() const = 0;
    virtual std::vector<Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder = false) = 0;
    virtual void add_gk_indices() = 0;

    // SEALZpCipher::create_context (src/pasta/SEAL_Cipher.cpp:38-68)
    static std::shared_ptr<HheContext> create_context(size_t mod_degree, uint64_t plain_mod, int seclevel = 128, int device = 0)
    {
        if (seclevel != 128) throw std::runtime_error("Security Level not supported");
        uint64_t q[64];
        size_t cnt = 64;
        if (hhe_bfv_default_coeff_modulus(mod_degree, q, &cnt) != HHE_OK) throw std::invalid_argument(hhe_last_error());
        int logn = 0;
        while (((size_t)1 << logn) < mod_degree) logn++;
        return std::make_shared<HheContext>(logn, std::vector<uint64_t>(q, q + cnt), plain_mod, device);
    }

    // SEALZpCipher::create_gk (SEAL_Cipher.cpp:359): keygen.create_galois_keys(gk_indices, he_gk) with this object's secret key, on the
    // device; the object then rotates with these keys.  get_galois_keys(): what the analyst ships to the CSP
    void create_gk(Seed seed)
    {
        if (he_sk.words.size() != device->key_limbs() * device->poly_modulus_degree()) throw std::invalid_argument("create_gk: no secret key");
        device->generate_galois(he_sk.words.data(), gk_indices, seed, he_gk.keys);
        gk_set = device->keys().galois(Boundary::words(he_gk));
    }
    const GaloisKeys &get_galois_keys() const { return he_gk; }

protected:
    ZpCipherParams params;
    uint64_t plain_mod = 0, mod_degree = 0;
    PublicKey he_pk;
    GaloisKeys he_gk;  // filled by create_gk only
};

class PASTA_SEAL : public SEALZpCipher {
public:
    PASTA_SEAL(std::shared_ptr<HheContext> con, PublicKey pk, SecretKey sk, RelinKeys rk, GaloisKeys gk)
        : SEALZpCipher(PASTA_PARAMS, std::move(con), std::move(pk), std::move(sk), std::move(rk), std::move(gk)),
          slots(mod_degree), halfslots(mod_degree >> 1) {}

    virtual std::string get_cipher_name() const { return "PASTA-SEAL (n=128,r=3)"; }
    virtual void add_gk_indices() { pasta_gk_indices(PASTA_PARAMS.plain_size, BSGS_N1, BSGS_N2); }

    // supply the BFV encryption of the PASTA key that HE_decrypt reads (secret_key_encrypted[0],
    // pasta_3_seal.cpp:58; filled by encrypt_key() on the client side of the reference)
    void set_encrypted_key(const Ciphertext &enc_key) { secret_key_encrypted.assign(1, enc_key); }

    // PASTA_SEAL::encrypt_key_2 (pasta_3_seal.cpp:23-38): the BFV encryption of the 256-word PASTA key ssk under this object's public
    // key, packed as the reference packs it (words 0..127 at slots 0.., words 128..255 at slots N/2..)
    std::vector<Ciphertext> encrypt_key_2(const std::vector<uint64_t> &ssk, Seed seed)
    {
        if (ssk.size() != PASTA_PARAMS.key_size) throw std::runtime_error("Invalid Key length");
        if (he_pk.words.size() != 2 * device->key_limbs() * slots) throw std::invalid_argument("encrypt_key_2: no public key");
        std::vector<uint64_t> key_tmp(halfslots + PASTA_PARAMS.plain_size, 0);
        for (size_t i = 0; i < PASTA_PARAMS.plain_size; i++) {
            key_tmp[i] = ssk[i];
            key_tmp[i + halfslots] = ssk[i + PASTA_PARAMS.plain_size];
        }
        std::vector<Ciphertext> enc_sk(1);
        device->encrypt(he_pk.words.data(), key_tmp.data(), key_tmp.size(), seed, out(enc_sk[0]));
        return enc_sk;
    }

    // PASTA_SEAL::HE_decrypt (pasta_3_seal.cpp:42-104) == decomposition(ciphertexts, secret_key_encrypted); PASTA_SEAL::decomposition
    // (pasta_3_seal.cpp:106-172), batch_encoder ignored as by the reference (:113)
    virtual std::vector<Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertexts, bool batch_encoder = false)
    {
        return decomposition(ciphertexts, encrypted_key(), batch_encoder);
    }
    virtual std::vector<Ciphertext> decomposition(std::vector<uint64_t> &ciphertexts, std::vector<Ciphertext> enc_ssk, bool batch_encoder = false)
    {
        return transcipher(ciphertexts, enc_ssk);
    }
    // ... of a record that was encrypted under `nonce` (PASTA::encrypt with a nonce below): block b runs under the pair (nonce, b).
    // Under one PASTA key a pair encrypts one block, ever (hhe_gfx950.h "PASTA under a caller's nonce"); nobody checks it
    std::vector<Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertexts, bool batch_encoder, uint64_t nonce)
    {
        return decomposition(ciphertexts, encrypted_key(), batch_encoder, nonce);
    }
    std::vector<Ciphertext> decomposition(std::vector<uint64_t> &ciphertexts, std::vector<Ciphertext> enc_ssk, bool batch_encoder, uint64_t nonce)
    {
        return transcipher(ciphertexts, enc_ssk, nonce);
    }

    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call (hhe::CipherT::decompose_records).  mask_last: as
    // hhe_pktnn_examples.cpp:620-626; the CSP's own loop masks a copy, i.e. pass false to reproduce that
    std::vector<Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<Ciphertext> enc_ssk,
                                      const GaloisKeys &flatten_gk, bool mask_last)
    {
        return decompose_records(records, enc_ssk, flatten_gk, mask_last);
    }
    // ... with one nonce per record
    std::vector<Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<Ciphertext> enc_ssk,
                                      const GaloisKeys &flatten_gk, bool mask_last, const std::vector<uint64_t> &nonces)
    {
        return decompose_records(records, enc_ssk, flatten_gk, mask_last, &nonces);
    }

private:
    static constexpr uint64_t BSGS_N1 = 16, BSGS_N2 = 8;  // pasta_3_seal.h:35-36
    size_t slots, halfslots;
};

// pasta::PASTA (src/pasta/pasta_3_plain.h:17-30; base ZpCipher src/pasta/Cipher.h:20-58): the client's symmetric
// cipher, evaluated by the device kernels.  Differs from the reference ctor only by the context handle in front.
class PASTA {
public:
    PASTA(std::shared_ptr<HheContext> con, std::vector<uint64_t> secret_key, uint64_t modulus)
        : context(std::move(con)), secret_key(std::move(secret_key)), modulus(modulus), params(PASTA_PARAMS)
    {
        if (this->secret_key.size() != params.key_size) throw std::runtime_error("Invalid Key length");  // Cipher.h:30-31
        if (modulus != context->plain_modulus()) throw std::invalid_argument("PASTA modulus differs from the plain modulus of the context");
    }
    virtual ~PASTA() = default;
    virtual std::string get_cipher_name() const { return "PASTA (n=128,r=3)"; }
    size_t get_key_size() const { return params.key_size; }
    size_t get_plain_size() const { return params.plain_size; }
    size_t get_cipher_size() const { return params.cipher_size; }
    virtual std::vector<uint64_t> encrypt(std::vector<uint64_t> plaintext) const { return crypt(std::move(plaintext), 0); }
    virtual std::vector<uint64_t> decrypt(std::vector<uint64_t> ciphertext) const { return crypt(std::move(ciphertext), 1); }
    // the record under a caller's nonce, block counters from 0 (Pasta::keystream(nonce, block_counter), pasta_3_plain.cpp:156-178, with
    // the nonce of PASTA::encrypt :9-27 a parameter).  Under one key a nonce encrypts one record, ever; nobody checks it
    std::vector<uint64_t> encrypt(std::vector<uint64_t> plaintext, uint64_t nonce) const { return crypt(std::move(plaintext), 0, nonce); }
    std::vector<uint64_t> decrypt(std::vector<uint64_t> ciphertext, uint64_t nonce) const { return crypt(std::move(ciphertext), 1, nonce); }

private:
    std::vector<uint64_t> crypt(std::vector<uint64_t> v, int dec, uint64_t nonce = HheContext::fixed_nonce) const
    {
        context->pasta_crypt(secret_key.data(), v.data(), v.size(), dec != 0, nonce);
        return v;
    }
    std::shared_ptr<HheContext> context;
    std::vector<uint64_t> secret_key;
    uint64_t modulus;
    ZpCipherParams params;
};

// seal::KeyGenerator as the parties use it (Analyst.cpp:38-66, hhe_pktnn_examples.cpp:435-441): secret + public key, and
// create_relin_keys, on the device
inline void keygen(HheContext &ctx, Seed seed, SecretKey &sk, PublicKey &pk) { ctx.generate_keys(seed, sk.words, pk.words); }
inline void create_relin_keys(HheContext &ctx, const SecretKey &sk, Seed seed, RelinKeys &rk)
{
    if (sk.words.size() != ctx.key_limbs() * ctx.poly_modulus_degree()) throw std::invalid_argument("create_relin_keys: no secret key");
    ctx.generate_relin(sk.words.data(), seed, rk.key);
}

}  // namespace pasta

namespace sealhelper {
// sealhelper::decrypting (src/util/sealhelper.cpp:252-266): Decryptor::decrypt + BatchEncoder::decode into signed values
// (SEAL: slot value v > (t+1)/2 reads as v - t), first `size` slots.  he_sk.words: SecretKey::data() [K][N], NTT form.
inline std::vector<int64_t> decrypting(const pasta::Ciphertext &enc_input, const pasta::SecretKey &he_sk, pasta::HheContext &ctx,
                                       size_t size)
{
    const size_t n = ctx.poly_modulus_degree(), w = 2 * ctx.limbs_or_data(enc_input.limbs) * n;  // a switched-down result decrypts at its level
    if (enc_input.words.size() != w || he_sk.words.size() < ctx.data_limbs() * n || size > n)
        throw std::invalid_argument("decrypting: ciphertext / secret key do not match the context");
    std::vector<uint64_t> u(n);
    ctx.decrypt(he_sk.words.data(), enc_input.words.data(), u.data(), enc_input.limbs);
    std::vector<int64_t> out(size);
    for (size_t i = 0; i < size; i++) out[i] = hhe::centred(u[i], ctx.plain_modulus());
    return out;
}

// Decryptor::invariant_noise_budget (seal/decryptor.h:103) of a ciphertext of size 2 or 3 at its level, on the device: what tells whether
// `decrypting` returns the right slots (a budget of 0 means it does not)
inline int invariant_noise_budget(const pasta::Ciphertext &enc_input, const pasta::SecretKey &he_sk, pasta::HheContext &ctx)
{
    return hhe::noise_budgets<pasta::Boundary>(ctx, {&enc_input}, he_sk)[0];
}

// sealhelper::packed_enc_multiply, Evaluator::relinearize_inplace(record, csp_rk) and sealhelper::encrypted_vec_sum as
// CSP_hhe_pktnn_1fc::evaluateModel calls them one after the other, the three as one call for a weight row, and hoisted rotations
// (hhe::FreeT); the context stands in for the Evaluator argument
typedef hhe::FreeT<pasta::Boundary> Free;
inline void packed_enc_multiply(pasta::HheContext &ctx, const pasta::Ciphertext &encrypted1, const pasta::Ciphertext &encrypted2,
                                pasta::Ciphertext &destination)
{
    Free::packed_enc_multiply(ctx, encrypted1, encrypted2, destination);
}
inline void relinearize_inplace(pasta::HheContext &ctx, pasta::Ciphertext &encrypted, const pasta::RelinKeys &relin_keys)
{
    Free::relinearize_inplace(ctx, encrypted, relin_keys);
}
inline void encrypted_vec_sum(pasta::HheContext &ctx, const pasta::Ciphertext &encrypted_inp, pasta::Ciphertext &destination,
                              const pasta::GaloisKeys &gal_keys, const size_t vec_size)
{
    Free::encrypted_vec_sum(ctx, encrypted_inp, destination, gal_keys, vec_size);
}
inline void fc_row(pasta::HheContext &ctx, const pasta::Ciphertext &vi, const pasta::Ciphertext &w_row, const pasta::RelinKeys &csp_rk,
                   const pasta::GaloisKeys &gal_keys, size_t vec_size, pasta::Ciphertext &destination)
{
    Free::fc_row(ctx, vi, w_row, csp_rk, gal_keys, vec_size, destination);
}
inline void rotate_rows_many(pasta::HheContext &ctx, const pasta::Ciphertext &ct, const std::vector<int> &steps, const pasta::GaloisKeys &gal_keys,
                             std::vector<pasta::Ciphertext> &out)
{
    Free::rotate_rows_many(ctx, ct, steps, gal_keys, out);
}
// The open FC layer under PLAIN weights, vo = M vi + b in slots [0, rows) (b empty: no bias), and the primitive under it, a sum of
// rotations times plaintexts with one mod-down (hhe_gfx950.h "Plain-weights sum of rotations"); the matrix is uploaded once per content
inline void fc_open_plain(pasta::HheContext &ctx, const pasta::Ciphertext &vi, const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> &b,
                          const pasta::GaloisKeys &gal_keys, pasta::Ciphertext &vo)
{
    Free::fc_open_plain(ctx, vi, M, b, gal_keys, vo);
}
inline void rotate_plain_sum(pasta::HheContext &ctx, const pasta::Ciphertext &ct, const std::vector<std::vector<uint64_t>> &plains, const std::vector<int> &steps,
                             const pasta::GaloisKeys &gal_keys, pasta::Ciphertext &vo)
{
    Free::rotate_plain_sum(ctx, ct, plains, steps, gal_keys, vo);
}
// The whole FC layer under the analyst's encrypted weights as ONE device call and one result ciphertext (the hybrid diagonal method,
// hhe_gfx950.h "packed encrypted FC"), in place of fc_row per neuron: mat holds the r encrypted generalized diagonals, rk / gal_keys are
// the key objects CSP.cpp:306 and :312-316 name.  Slots [0, rows) of the decryption are the neurons.
typedef pasta::EncMatrix EncMatrix;
inline void fc_packed(const pasta::Ciphertext &vi, const EncMatrix &mat, const pasta::RelinKeys &rk, const pasta::GaloisKeys &gal_keys,
                      pasta::Ciphertext &out)
{
    mat.apply(vi, rk, gal_keys, out);
}
// ... with the layer's rotation chain hoisted: every rot_i = rotate_rows(x, i, gal_keys).  With a key for each of 1 .. r-1 in gal_keys
// (hhe_fc_packed_hoisted_galois_steps) the chain is one dependent step; the slots are the same, the words are not
inline void fc_packed_hoisted(const pasta::Ciphertext &vi, const EncMatrix &mat, const pasta::RelinKeys &rk, const pasta::GaloisKeys &gal_keys,
                              pasta::Ciphertext &out)
{
    mat.apply(vi, rk, gal_keys, out, true);
}
// ... with ONE BEHZ floor per item: the r products are summed before the floor (hhe_gfx950.h hhe_fc_packed_sum_ks); hoisted chooses the
// rotations of fc_packed_hoisted instead of fc_packed's chain.  The slots are the same, the words are not
inline void fc_packed_sum(const pasta::Ciphertext &vi, const EncMatrix &mat, const pasta::RelinKeys &rk, const pasta::GaloisKeys &gal_keys,
                          pasta::Ciphertext &out, bool hoisted = false)
{
    mat.apply_sum(vi, rk, gal_keys, out, hoisted);
}
// The open layer (mat from enc_matrix_open) and the FC-square-FC network as ONE device call (hhe_gfx950.h "Chainable packed FC"): no slot
// of vi outside [0, cols) of the first layer needs to be zero, and no mask stands between two layers
inline void fc_open(const pasta::Ciphertext &vi, const EncMatrix &mat, const pasta::RelinKeys &rk, const pasta::GaloisKeys &gal_keys,
                    pasta::Ciphertext &out)
{
    mat.apply_open(vi, rk, gal_keys, out);
}
inline void mlp(const std::vector<const EncMatrix *> &layers, const pasta::Ciphertext &vi, const pasta::RelinKeys &rk,
                const pasta::GaloisKeys &gal_keys, pasta::Ciphertext &vo)
{
    EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
}
}  // namespace sealhelper
