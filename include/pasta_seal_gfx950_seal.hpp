// pasta_seal_gfx950_seal.hpp -- the SEAL-typed drop-in: pasta::SEALZpCipher / pasta::PASTA_SEAL with the reference's exact
// signatures (src/pasta/SEAL_Cipher.h:11-129, src/pasta/pasta_3_seal.h:8-54) and sealhelper::packed_enc_multiply /
// encrypted_vec_sum (src/util/sealhelper.h:84-129), implemented over the C ABI of libhhe_gfx950.so.
//
// Use in the reference tree: include this header where src/Common.h:19-21 includes "pasta_3_seal.h" / "SEAL_Cipher.h"
// (it replaces both; it still includes the reference's Cipher.h and pasta_3_plain.h for ZpCipherParams / PASTA_PARAMS and
// SEAL's own headers for the boundary types) and link libhhe_gfx950.so.  src/examples/CSP/CSP.cpp:235-323 then compiles
// unchanged: decomposition / mask / flatten / packed_enc_multiply / encrypted_vec_sum run on the MI355X, everything else
// (key generation, encrypt_key, decrypt_result, serialization) stays on SEAL.
// SEAL objects cross the boundary as their own words: Ciphertext::data() is [size][L][N] at the data level in coefficient
// form, KSwitchKeys::data()[index][digit].data() is [2][K][N] in NTT form -- the layouts include/hhe_gfx950.h takes.
//
// What lives here: the registry of device contexts, the boundary policy (pasta::gfx950::Boundary: validity checks and conversions
// between SEAL objects and plain words, the walk that finds a level's parms_id), the members that stay on SEAL (the SEAL object members,
// create_context, encrypt_key, encrypt_key_2, decrypt_result, create_gk) and one-line forwards where the reference spells a signature.
// The encrypted matrix, the level object, the cipher classes' device members and the free functions' bodies are the templates of
// hhe_adapter_front.hpp instantiated with that policy -- the source text pasta_seal_gfx950.hpp instantiates on word containers and the
// tests execute -- over the call bodies of hhe::AdapterCore (hhe_adapter_core.hpp).  tests/test_seal_adapter.py type-checks this file,
// every member of those instantiations and the CSP's call sequence against the reference's SEAL 4.0.0 headers (g++ -fsyntax-only; the
// prebuilt libseal is never linked or loaded): it is not executed here.
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "Cipher.h"         // reference: pasta::ZpCipherParams
#include "pasta_3_plain.h"  // reference: PASTA_PARAMS, PASTA_T
#include "seal/seal.h"

#include "hhe_adapter_front.hpp"

namespace pasta {
namespace gfx950 {

// One device context per SEAL parameter set, shared by every cipher object of the process: BaseCSP::decompose builds a
// fresh PASTA_SEAL per request (CSP.cpp:238-242), the key-switch keys stay in HBM between requests.  Every RelinKeys /
// GaloisKeys OBJECT that reaches the adapter (a constructor argument, the galois_keys of flatten, the keys of the FC calls) maps
// to one device key set, recognised by a hash over all of its words (hhe::KeySetCache): analyst_he_gk and csp_he_gk, which
// share elements but not words (Analyst.cpp:62-94), live side by side and every call uses the one it names.
class DeviceContext : public hhe::AdapterCore {
public:
    explicit DeviceContext(const seal::SEALContext &context, int device = 0)
        : hhe::AdapterCore(seal::util::get_power_of_two(context.key_context_data()->parms().poly_modulus_degree()),
                           primes(context.key_context_data()->parms()), context.key_context_data()->parms().plain_modulus().value(), device),
          seal_(context) {}
    // the SEALContext of this parameter set (a SEALContext is a handle on shared context data): what resizes a destination, also
    // for a free function, whose ciphertexts do not carry theirs
    const seal::SEALContext &seal() const { return seal_; }

    // process-wide registry keyed by the data-level parms_id (what every ciphertext of the path carries)
    static std::shared_ptr<DeviceContext> get(const seal::SEALContext &context)
    {
        std::unique_lock<std::mutex> lk(registry_mutex());
        auto &reg = registry();
        auto it = reg.find(context.first_parms_id());
        if (it != reg.end()) return it->second;
        auto dc = std::make_shared<DeviceContext>(context);
        reg.emplace(context.first_parms_id(), dc);
        return dc;
    }
    static std::shared_ptr<DeviceContext> find(const seal::parms_id_type &id)
    {
        std::unique_lock<std::mutex> lk(registry_mutex());
        auto it = registry().find(id);
        if (it == registry().end()) throw std::invalid_argument("no gfx950 device context for these encryption parameters (construct a pasta::PASTA_SEAL first)");
        return it->second;
    }

private:
    static std::map<seal::parms_id_type, std::shared_ptr<DeviceContext>> &registry()
    {
        static std::map<seal::parms_id_type, std::shared_ptr<DeviceContext>> r;
        return r;
    }
    static std::mutex &registry_mutex()
    {
        static std::mutex m;
        return m;
    }
    static std::vector<std::uint64_t> primes(const seal::EncryptionParameters &parms)
    {
        std::vector<std::uint64_t> q;
        for (const auto &m : parms.coeff_modulus()) q.push_back(m.value());
        return q;
    }
    seal::SEALContext seal_;
};

// the boundary policy of hhe_adapter_front.hpp on seal:: types.  A level is named by its parms_id
struct Boundary {
    typedef seal::Ciphertext Ciphertext;
    typedef seal::RelinKeys RelinKeys;
    typedef seal::GaloisKeys GaloisKeys;
    typedef seal::SecretKey SecretKey;
    typedef DeviceContext Context;
    typedef std::shared_ptr<seal::SEALContext> Binding;
    typedef seal::parms_id_type Level;
    static std::shared_ptr<Context> chain(const Binding &con) { return DeviceContext::get(*con); }
    static Level top(const Context &ctx) { return ctx.seal().first_parms_id(); }
    // the walk last_context_data() -> prev_context_data(), as the reference walks (SEAL_Cipher.cpp:363-378)
    static Level level_id(const Context &ctx, std::size_t levels_from_last)
    {
        auto c = ctx.seal().last_context_data();
        for (std::size_t i = 0; i < levels_from_last; i++) c = c->prev_context_data();
        return c->parms_id();
    }
    static const std::uint64_t *in(const Context &ctx, const Level &id, const Ciphertext &ct, std::size_t size)
    {
        const auto data = ctx.seal().get_context_data(id);
        const bool ok = data && !ct.is_ntt_form() && ct.parms_id() == id && ct.poly_modulus_degree() == ctx.poly_modulus_degree() &&
                        ct.coeff_modulus_size() == data->parms().coeff_modulus().size() && ct.size() == size;
        return ok ? ct.data() : nullptr;
    }
    static const std::uint64_t *in_any(const Context &ctx, const Ciphertext &ct)
    {
        const bool ok = !ct.is_ntt_form() && ct.poly_modulus_degree() == ctx.poly_modulus_degree() && ct.size() >= 2 && ct.coeff_modulus_size() <= ctx.data_limbs();
        return ok ? ct.data() : nullptr;
    }
    static auto out(const Context &ctx, const Level &id, Ciphertext &ct, std::size_t size)
    {
        return [&ctx, &ct, id, size](std::size_t) {
            ct.resize(ctx.seal(), id, size);
            ct.is_ntt_form() = false;
            ct.scale() = 1.0;
            return ct.data();
        };
    }
    static std::size_t size(const Ciphertext &ct) { return ct.size(); }
    static std::size_t limbs(const Ciphertext &ct) { return ct.coeff_modulus_size(); }

    // KSwitchKeys::data()[index] = one PublicKey per digit, each a size-2 K-limb NTT-form ciphertext -> [L][2][K][N]
    static std::vector<std::uint64_t> flatten_ksk(const std::vector<seal::PublicKey> &digits)
    {
        std::vector<std::uint64_t> out;
        for (const auto &pk : digits) {
            const seal::Ciphertext &ct = pk.data();
            out.insert(out.end(), ct.data(), ct.data() + ct.size() * ct.coeff_modulus_size() * ct.poly_modulus_degree());
        }
        return out;
    }
    // the words of a key object (empty for an empty object: the call then reports the missing key as SEAL would)
    static hhe::RelinWords words(const RelinKeys &rk)
    {
        hhe::RelinWords r;
        if (rk.data().empty() || rk.data()[0].empty()) return r;
        r.own = flatten_ksk(rk.data()[seal::RelinKeys::get_index(2)]);
        r.key = r.own.data();
        r.words = r.own.size();
        return r;
    }
    static hhe::GaloisWords words(const GaloisKeys &gk)
    {
        hhe::GaloisWords g;
        for (std::size_t idx = 0; idx < gk.data().size(); idx++) {
            if (gk.data()[idx].empty()) continue;
            g.own.push_back(flatten_ksk(gk.data()[idx]));   // GaloisKeys::get_index(elt) = (elt - 1) / 2
            g.keys.emplace_back(static_cast<std::uint32_t>(2 * idx + 1), nullptr);
        }
        for (std::size_t i = 0; i < g.keys.size(); i++) g.keys[i].second = g.own[i].data();
        if (!g.own.empty()) g.words = g.own[0].size();
        return g;
    }
    static std::pair<const std::uint64_t *, std::size_t> secret(const SecretKey &sk) { return {sk.data().data(), sk.data().coeff_count()}; }
};

}  // namespace gfx950

typedef hhe::EncMatrixT<gfx950::Boundary> EncMatrix;

// What SEALZpCipher::level(levels_from_last) returns (hhe::LevelT): every member takes and produces coefficient-form ciphertexts whose
// parms_id is parms_id()
class SEALZpLevel : public hhe::LevelT<gfx950::Boundary> {
public:
    SEALZpLevel(hhe::LevelT<gfx950::Boundary> level) : hhe::LevelT<gfx950::Boundary>(std::move(level)) {}
    const seal::parms_id_type &parms_id() const { return id; }
};

// ---------------------------------------------------------------------------------------------------------------------
// pasta::SEALZpCipher (src/pasta/SEAL_Cipher.h:11-129).  The members the CSP path uses run on the device (hhe::CipherT: `device` is
// the shared DeviceContext of the parameter set, he_sk the secret key); the SEAL objects the reference keeps as members are kept too
// (encrypt_key, decrypt_result and the analyst/user sides use them unchanged).
class SEALZpCipher : public hhe::CipherT<gfx950::Boundary> {
protected:
    std::vector<uint64_t> secret_key;
    ZpCipherParams params;
    uint64_t plain_mod;
    uint64_t mod_degree;

    std::shared_ptr<seal::SEALContext> context;
    seal::KeyGenerator keygen;

    seal::PublicKey he_pk;
    seal::RelinKeys he_rk;
    seal::GaloisKeys he_gk;

    seal::Encryptor encryptor;
    seal::Evaluator evaluator;
    seal::Decryptor decryptor;
    seal::BatchEncoder batch_encoder;

public:
    // src/pasta/SEAL_Cipher.cpp:9-36 (all arguments by value, as the reference takes them)
    SEALZpCipher(ZpCipherParams params, std::shared_ptr<seal::SEALContext> con, seal::PublicKey pk, seal::SecretKey sk,
                 seal::RelinKeys rk, seal::GaloisKeys gk)
        : hhe::CipherT<gfx950::Boundary>(gfx950::DeviceContext::get(*con), sk, rk, gk), params(params), context(con), keygen(*context, sk),
          he_pk(pk), he_rk(rk), he_gk(gk), encryptor(*context, pk), evaluator(*context), decryptor(*context, sk), batch_encoder(*context)
    {
        encryptor.set_public_key(pk);
        mod_degree = context->first_context_data()->parms().poly_modulus_degree();
        plain_mod = context->first_context_data()->parms().plain_modulus().value();
    }
    virtual ~SEALZpCipher() = default;

    size_t get_key_size() const { return params.key_size; }
    size_t get_plain_size() const { return params.plain_size; }
    size_t get_cipher_size() const { return params.cipher_size; }
    using hhe::CipherT<gfx950::Boundary>::get_cipher_size;

    void create_gk() { keygen.create_galois_keys(gk_indices, he_gk); gk_set = device->keys().galois(gfx950::Boundary::words(he_gk)); }

    virtual std::string get_cipher_name() const = 0;

    // src/pasta/SEAL_Cipher.cpp:38-68
    static std::shared_ptr<seal::SEALContext> create_context(size_t mod_degree, uint64_t plain_mod, int seclevel = 128)
    {
        if (seclevel != 128) throw std::runtime_error("Security Level not supported");
        seal::sec_level_type sec = seal::sec_level_type::tc128;
        seal::EncryptionParameters parms(seal::scheme_type::bfv);
        parms.set_poly_modulus_degree(mod_degree);
        if (mod_degree == 65536) {
            sec = seal::sec_level_type::none;
            uint64_t q[64];
            size_t cnt = 64;
            hhe::check(hhe_bfv_default_coeff_modulus(mod_degree, q, &cnt));  // the reference's hard-coded 29-prime chain (:50-60)
            std::vector<seal::Modulus> mods;
            for (size_t i = 0; i < cnt; i++) mods.emplace_back(q[i]);
            parms.set_coeff_modulus(mods);
        } else {
            parms.set_coeff_modulus(seal::CoeffModulus::BFVDefault(mod_degree));
        }
        parms.set_plain_modulus(plain_mod);
        return std::make_shared<seal::SEALContext>(parms, true, sec);
    }

    virtual std::vector<seal::Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder = false) = 0;
    virtual std::vector<uint64_t> decrypt_result(std::vector<seal::Ciphertext> &ciphertext, bool batch_encoder = false) = 0;
    virtual void add_gk_indices() = 0;
};

// ---------------------------------------------------------------------------------------------------------------------
// pasta::PASTA_SEAL (src/pasta/pasta_3_seal.h:8-54)
class PASTA_SEAL : public SEALZpCipher {
public:
    typedef PASTA Plain;
    PASTA_SEAL(std::shared_ptr<seal::SEALContext> con, seal::PublicKey pk, seal::SecretKey sk, seal::RelinKeys rk, seal::GaloisKeys gk)
        : SEALZpCipher(PASTA_PARAMS, con, pk, sk, rk, gk), slots(this->batch_encoder.slot_count()), halfslots(slots >> 1) {}

    virtual ~PASTA_SEAL() = default;

    virtual std::string get_cipher_name() const { return "PASTA-SEAL (n=128,r=3)"; }

    // pasta_3_seal.cpp:8-21 (client-side key encryption stays on SEAL: one encode + one encrypt)
    virtual void encrypt_key(bool batch_encoder = false)
    {
        (void)batch_encoder;
        secret_key_encrypted = encrypt_key_2(secret_key, batch_encoder);
    }
    // pasta_3_seal.cpp:23-38
    virtual std::vector<seal::Ciphertext> encrypt_key_2(std::vector<uint64_t> ssk, bool batch_encoder = false)
    {
        (void)batch_encoder;
        std::vector<seal::Ciphertext> enc_sk(1);
        seal::Plaintext k;
        std::vector<uint64_t> key_tmp(halfslots + PASTA_T, 0);
        for (size_t i = 0; i < PASTA_T; i++) {
            key_tmp[i] = ssk[i];
            key_tmp[i + halfslots] = ssk[i + PASTA_T];
        }
        this->batch_encoder.encode(key_tmp, k);
        encryptor.encrypt(k, enc_sk[0]);
        return enc_sk;
    }

    // pasta_3_seal.cpp:42-104 == decomposition(ciphertexts, secret_key_encrypted) without the debug noise printing (:73; print_noise() is
    // there to call); pasta_3_seal.cpp:106-172, batch_encoder ignored as by the reference (:113)
    virtual std::vector<seal::Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder = false)
    {
        return decomposition(ciphertext, encrypted_key(), batch_encoder);
    }
    virtual std::vector<seal::Ciphertext> decomposition(std::vector<uint64_t> &ciphertext, std::vector<seal::Ciphertext> enc_ssk,
                                                        bool batch_encoder = false)
    {
        (void)batch_encoder;
        return transcipher(ciphertext, enc_ssk);
    }
    // ... of a record that was encrypted under `nonce`: block b runs under the pair (nonce, b).  Under one PASTA key a pair encrypts
    // one block, ever (hhe_gfx950.h "PASTA under a caller's nonce"); nobody checks it
    std::vector<seal::Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder, uint64_t nonce)
    {
        return decomposition(ciphertext, encrypted_key(), batch_encoder, nonce);
    }
    std::vector<seal::Ciphertext> decomposition(std::vector<uint64_t> &ciphertext, std::vector<seal::Ciphertext> enc_ssk, bool batch_encoder,
                                                uint64_t nonce)
    {
        (void)batch_encoder;
        return transcipher(ciphertext, enc_ssk, nonce);
    }

    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call (hhe::CipherT::decompose_records).  mask_last: as
    // hhe_pktnn_examples.cpp:620-626; the CSP's own loop masks a copy, i.e. pass false to reproduce that
    std::vector<seal::Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<seal::Ciphertext> enc_ssk,
                                            const seal::GaloisKeys &flatten_gk, bool mask_last)
    {
        return decompose_records(records, enc_ssk, flatten_gk, mask_last);
    }
    // ... with one nonce per record
    std::vector<seal::Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<seal::Ciphertext> enc_ssk,
                                            const seal::GaloisKeys &flatten_gk, bool mask_last, const std::vector<uint64_t> &nonces)
    {
        return decompose_records(records, enc_ssk, flatten_gk, mask_last, &nonces);
    }

    // pasta_3_seal.cpp:176-188 (analyst side, one decrypt + decode: stays on SEAL)
    virtual std::vector<uint64_t> decrypt_result(std::vector<seal::Ciphertext> &ciphertext, bool batch_encoder = false)
    {
        (void)batch_encoder;
        seal::Plaintext p;
        std::vector<uint64_t> res;
        decryptor.decrypt(ciphertext[0], p);
        this->batch_encoder.decode(p, res);
        res.resize(params.plain_size);
        return res;
    }

    virtual void add_gk_indices() { pasta_gk_indices(PASTA_T, BSGS_N1, BSGS_N2); }  // pasta_3_seal.cpp:190-201

private:
    static constexpr uint64_t BSGS_N1 = 16;
    static constexpr uint64_t BSGS_N2 = 8;
    size_t slots;
    size_t halfslots;
};

}  // namespace pasta

// ---------------------------------------------------------------------------------------------------------------------
// sealhelper::packed_enc_multiply / encrypted_vec_sum (src/util/sealhelper.h:84-129, sealhelper.cpp:268-274,379-392) with the
// reference's signatures, Evaluator::relinearize_inplace(record, csp_rk) as the CSP calls it between the two (CSP.cpp:306), the three
// as one call for a weight row, and hoisted rotations (hhe::FreeT).  The Evaluator argument is unused: the device context is found
// through the ciphertext's parms_id.
namespace sealhelper {
using pasta::gfx950::DeviceContext;
typedef hhe::FreeT<pasta::gfx950::Boundary> Free;

inline void packed_enc_multiply(const seal::Ciphertext &encrypted1, const seal::Ciphertext &encrypted2, seal::Ciphertext &destination,
                                const seal::Evaluator &evaluator)
{
    (void)evaluator;
    Free::packed_enc_multiply(*DeviceContext::find(encrypted1.parms_id()), encrypted1, encrypted2, destination);
}
inline void relinearize_inplace(seal::Ciphertext &encrypted, const seal::RelinKeys &relin_keys)
{
    Free::relinearize_inplace(*DeviceContext::find(encrypted.parms_id()), encrypted, relin_keys);
}
inline void encrypted_vec_sum(const seal::Ciphertext &encrypted_inp, seal::Ciphertext &destination, const seal::Evaluator &evaluator,
                              const seal::GaloisKeys &gal_keys, const size_t vec_size)
{
    (void)evaluator;
    Free::encrypted_vec_sum(*DeviceContext::find(encrypted_inp.parms_id()), encrypted_inp, destination, gal_keys, vec_size);
}
inline void fc_row(const seal::Ciphertext &vi, const seal::Ciphertext &w_row, const seal::RelinKeys &csp_rk, const seal::GaloisKeys &gal_keys,
                   size_t vec_size, seal::Ciphertext &destination)
{
    Free::fc_row(*DeviceContext::find(vi.parms_id()), vi, w_row, csp_rk, gal_keys, vec_size, destination);
}
inline void rotate_rows_many(const seal::Ciphertext &ct, const std::vector<int> &steps, const seal::GaloisKeys &gal_keys,
                             std::vector<seal::Ciphertext> &out, const seal::Evaluator &evaluator)
{
    (void)evaluator;
    Free::rotate_rows_many(*DeviceContext::find(ct.parms_id()), ct, steps, gal_keys, out);
}
// The open FC layer under PLAIN weights, vo = M vi + b in slots [0, rows) (b empty: no bias), and the primitive under it, a sum of
// rotations times plaintexts with one mod-down (hhe_gfx950.h "Plain-weights sum of rotations"); the matrix is uploaded once per content
inline void fc_open_plain(const seal::Ciphertext &vi, const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> &b,
                          const seal::GaloisKeys &gal_keys, seal::Ciphertext &vo)
{
    Free::fc_open_plain(*DeviceContext::find(vi.parms_id()), vi, M, b, gal_keys, vo);
}
inline void rotate_plain_sum(const seal::Ciphertext &ct, const std::vector<std::vector<uint64_t>> &plains, const std::vector<int> &steps,
                             const seal::GaloisKeys &gal_keys, seal::Ciphertext &vo)
{
    Free::rotate_plain_sum(*DeviceContext::find(ct.parms_id()), ct, plains, steps, gal_keys, vo);
}

// The whole FC layer under the analyst's encrypted weights as ONE device call and one result ciphertext (the hybrid diagonal method,
// hhe_gfx950.h "packed encrypted FC"), in place of fc_row per neuron: mat holds the r encrypted generalized diagonals, rk / gal_keys are
// the key objects CSP.cpp:306 and :312-316 name.  Slots [0, rows) of the decryption are the neurons.
typedef pasta::EncMatrix EncMatrix;
inline void fc_packed(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
{
    mat.apply(vi, rk, gal_keys, out);
}
// ... with the layer's rotation chain hoisted: every rot_i = rotate_rows(x, i, gal_keys).  With a key for each of 1 .. r-1 in gal_keys
// (hhe_fc_packed_hoisted_galois_steps) the chain is one dependent step; the slots are the same, the words are not
inline void fc_packed_hoisted(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
                              seal::Ciphertext &out)
{
    mat.apply(vi, rk, gal_keys, out, true);
}
// ... with ONE BEHZ floor per item: the r products are summed before the floor (hhe_gfx950.h hhe_fc_packed_sum_ks); hoisted chooses the
// rotations of fc_packed_hoisted instead of fc_packed's chain.  The slots are the same, the words are not
inline void fc_packed_sum(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
                          seal::Ciphertext &out, bool hoisted = false)
{
    mat.apply_sum(vi, rk, gal_keys, out, hoisted);
}
// The open layer (mat from enc_matrix_open) and the FC-square-FC network as ONE device call (hhe_gfx950.h "Chainable packed FC"): no slot
// of vi outside [0, cols) of the first layer needs to be zero, and no mask stands between two layers
inline void fc_open(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
{
    mat.apply_open(vi, rk, gal_keys, out);
}
inline void mlp(const std::vector<const EncMatrix *> &layers, const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
                seal::Ciphertext &vo)
{
    EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
}

}  // namespace sealhelper
