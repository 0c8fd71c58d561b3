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
// Only what needs seal:: types lives here: the registry of device contexts, the validity checks and the conversions between SEAL
// objects and plain words.  Every call body is hhe::AdapterCore (hhe_adapter_core.hpp), the code pasta_seal_gfx950.hpp runs in
// the tests on word containers.  tests/test_seal_adapter.py type-checks this file and the CSP's call sequence against the
// reference's SEAL 4.0.0 headers (g++ -fsyntax-only; the prebuilt libseal is never linked or loaded): it is not executed here.
#pragma once

#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "Cipher.h"         // reference: pasta::ZpCipherParams
#include "pasta_3_plain.h"  // reference: PASTA_PARAMS, PASTA_T
#include "seal/seal.h"

#include "hhe_adapter_core.hpp"

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
          first_parms_id_(context.first_parms_id()) {}

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
    static hhe::RelinWords words(const seal::RelinKeys &rk)
    {
        hhe::RelinWords r;
        if (rk.data().empty() || rk.data()[0].empty()) return r;
        r.own = flatten_ksk(rk.data()[seal::RelinKeys::get_index(2)]);
        r.key = r.own.data();
        r.words = r.own.size();
        return r;
    }
    static hhe::GaloisWords words(const seal::GaloisKeys &gk)
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
    hhe::KeySet relin_set(const seal::RelinKeys &rk) { return keys().relin(words(rk)); }
    hhe::KeySet galois_set(const seal::GaloisKeys &gk) { return keys().galois(words(gk)); }

    // a data-level, coefficient-form ciphertext of `size` polynomials as its words
    const std::uint64_t *words(const seal::Ciphertext &ct, std::size_t size = 2) const
    {
        if (ct.is_ntt_form() || ct.poly_modulus_degree() != poly_modulus_degree() || ct.coeff_modulus_size() != data_limbs() || ct.size() != size)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        return ct.data();
    }
    // a coefficient-form ciphertext at any level of the modulus switching chain (get_cipher_size): its words, [size][coeff_modulus_size][N]
    const std::uint64_t *level_words(const seal::Ciphertext &ct) const
    {
        if (ct.is_ntt_form() || ct.poly_modulus_degree() != poly_modulus_degree() || ct.size() < 2) throw std::invalid_argument("encrypted is not valid for encryption parameters");
        limbs_or_data(ct.coeff_modulus_size());
        return ct.data();
    }
    // ... and the sink that resizes the destination at the level `id` names
    static auto into_level(const seal::SEALContext &context, seal::Ciphertext &ct, seal::parms_id_type id, std::size_t size)
    {
        return [&context, &ct, id, size](std::size_t) {
            ct.resize(context, id, size);
            ct.is_ntt_form() = false;
            ct.scale() = 1.0;
            return ct.data();
        };
    }
    std::vector<const std::uint64_t *> words(const std::vector<seal::Ciphertext> &cts) const
    {
        std::vector<const std::uint64_t *> p;
        for (const auto &ct : cts) p.push_back(words(ct));
        return p;
    }
    // output sinks.  With the SEALContext at hand (cipher objects) the destination is resized at the data level ...
    auto into(const seal::SEALContext &context, seal::Ciphertext &ct, std::size_t size = 2) const
    {
        return [this, &context, &ct, size](std::size_t) {
            ct.resize(context, first_parms_id_, size);
            ct.is_ntt_form() = false;
            ct.scale() = 1.0;
            return ct.data();
        };
    }
    auto into(const seal::SEALContext &context, std::vector<seal::Ciphertext> &cts) const
    {
        return [this, &context, &cts](std::size_t i) { return into(context, cts[i])(0); };
    }
    // ... without it (free functions: a Ciphertext does not carry its SEALContext) it takes the parameters of an input of the
    // call (same parms_id, pool) and is resized to `size` polynomials
    static auto into(seal::Ciphertext &ct, const seal::Ciphertext &like, std::size_t size = 2)
    {
        return [&ct, &like, size](std::size_t) { ct = like; ct.resize(size); return ct.data(); };
    }

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
    seal::parms_id_type first_parms_id_{};
};

}  // namespace gfx950

// ---------------------------------------------------------------------------------------------------------------------
// The analyst's encrypted weight matrix of a packed encrypted FC layer, resident on the device (hhe_gfx950.h "packed encrypted FC"; no
// reference counterpart: the reference evaluates one encrypted row per neuron, CSP.cpp:296-316).  diagonals: the r encryptions of the
// generalized diagonals at the data level -- or, made by SEALZpLevel::enc_matrix, at that level's parms_id.  A conversion into
// hhe::AdapterCore and nothing else; the object holds the cores it needs.
struct EncMatrix {
    EncMatrix() = default;
    EncMatrix(std::shared_ptr<seal::SEALContext> con, const std::vector<seal::Ciphertext> &diagonals, std::size_t rows, std::size_t cols)
        : EncMatrix(con, gfx950::DeviceContext::get(*con), nullptr, con->first_parms_id(), diagonals, rows, cols) {}
    // at: the core of a level (null: the chain's own), level_id: that level's parms_id
    // open: the diagonals that do not wrap (hhe_fc_open_diagonals) -- the kind fc_open and mlp take; a cyclic one takes the fc_packed forms
    EncMatrix(std::shared_ptr<seal::SEALContext> con, std::shared_ptr<gfx950::DeviceContext> dev, std::shared_ptr<hhe::AdapterCore> at,
              seal::parms_id_type level_id, const std::vector<seal::Ciphertext> &diagonals, std::size_t rows, std::size_t cols, bool open = false)
        : context(std::move(con)), device(std::move(dev)), core(at ? std::move(at) : std::shared_ptr<hhe::AdapterCore>(device)), id(level_id), rows(rows), cols(cols),
          open(open)
    {
        std::vector<const std::uint64_t *> p;
        for (const auto &ct : diagonals) p.push_back(in(ct));
        handle = open ? core->enc_matrix_open(p, rows, cols) : core->enc_matrix(p, rows, cols);
    }
    // the network layers[0], square + relinearize, layers[1], ... on one ciphertext (hhe_mlp_ks); one layer is the open layer alone.
    // Every layer is an open matrix of one core; rk / gal_keys: the parties' ordinary, top-level key objects
    static void mlp(const std::vector<const EncMatrix *> &layers, const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
                    seal::Ciphertext &out)
    {
        if (layers.empty() || !layers[0] || !layers[0]->core) throw std::invalid_argument("mlp: no encrypted matrix");
        const EncMatrix &first = *layers[0];
        std::vector<hhe::EncMatrix> handles;
        for (const EncMatrix *m : layers) {
            if (!m || !m->core) throw std::invalid_argument("mlp: no encrypted matrix");
            if (m->core.get() != first.core.get()) throw std::invalid_argument("mlp: the layers are not at one level");
            handles.push_back(m->handle);
        }
        hhe::KeySet r = first.device->relin_set(rk), g = first.device->galois_set(gal_keys);
        if (first.core.get() != first.device.get()) { r = first.core->derived(r); g = first.core->derived(g); }
        first.core->mlp(first.in(vi), handles, r, g, gfx950::DeviceContext::into_level(*first.context, out, first.id, 2));
    }
    void apply_open(const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out) const
    {
        mlp({this}, vi, rk, gal_keys, out);
    }
    // slots [0, rows) of the decryption of `out` are (M x) mod t; rk / gal_keys: the parties' ordinary, top-level key objects
    // hoisted: the rotation chain of the layer as rotations of one ciphertext (fc_packed_hoisted)
    // sum: one BEHZ floor over the sum of the layer's r products (fc_packed_sum), with either rotation schedule
    void apply(const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out, bool hoisted = false,
               bool sum = false) const
    {
        if (!core) throw std::invalid_argument("fc_packed: no encrypted matrix");
        hhe::KeySet r = device->relin_set(rk), g = device->galois_set(gal_keys);
        if (core.get() != device.get()) { r = core->derived(r); g = core->derived(g); }
        if (sum) core->fc_packed_sum(in(vi), handle, r, g, gfx950::DeviceContext::into_level(*context, out, id, 2), hoisted);
        else if (hoisted) core->fc_packed_hoisted(in(vi), handle, r, g, gfx950::DeviceContext::into_level(*context, out, id, 2));
        else core->fc_packed(in(vi), handle, r, g, gfx950::DeviceContext::into_level(*context, out, id, 2));
    }
    void apply_sum(const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out, bool hoisted = false) const
    {
        apply(vi, rk, gal_keys, out, hoisted, true);
    }
    std::shared_ptr<seal::SEALContext> context;
    std::shared_ptr<gfx950::DeviceContext> device;  // the chain's core: its key-set cache holds the sets the calls name
    std::shared_ptr<hhe::AdapterCore> core;         // where the handle lives: the chain's core, or a level's
    seal::parms_id_type id{};                       // the level of the diagonals, the inputs and the results
    hhe::EncMatrix handle;                          // declared after the cores: released before them
    std::size_t rows = 0, cols = 0;
    bool open = false;

private:
    const std::uint64_t *in(const seal::Ciphertext &ct) const
    {
        if (ct.is_ntt_form() || ct.parms_id() != id || ct.poly_modulus_degree() != core->poly_modulus_degree() ||
            ct.coeff_modulus_size() != core->data_limbs() || ct.size() != 2)
            throw std::invalid_argument("encrypted is not at the level of this object");
        return ct.data();
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// What SEALZpCipher::level(levels_from_last) returns: the evaluation members of a cipher object bound to one level of the modulus
// switching chain, named by its parms_id.  Every member takes and produces coefficient-form ciphertexts whose parms_id is that
// level's and refuses any other with std::invalid_argument.  The object keeps no keys of its own: the device core of the level
// (hhe::AdapterCore::level) derives, on the device and on first use, the projections of the key sets of the cipher object it came
// from and of the top-level key objects a call names.
class SEALZpLevel {
    const std::uint64_t *in(const seal::Ciphertext &ct, std::size_t size = 2) const
    {
        if (ct.is_ntt_form() || ct.parms_id() != id || ct.poly_modulus_degree() != core->poly_modulus_degree() ||
            ct.coeff_modulus_size() != core->data_limbs() || ct.size() != size)
            throw std::invalid_argument("encrypted is not at the level of this object");
        return ct.data();
    }
    auto out(seal::Ciphertext &ct, std::size_t size = 2) const { return gfx950::DeviceContext::into_level(*context, ct, id, size); }
    std::vector<const std::uint64_t *> pointers(const std::vector<seal::Ciphertext> &cts) const
    {
        std::vector<const std::uint64_t *> p;
        for (const auto &ct : cts) p.push_back(in(ct));
        return p;
    }

public:
    typedef std::vector<uint64_t> vector;
    typedef std::vector<std::vector<uint64_t>> matrix;
    SEALZpLevel(std::shared_ptr<seal::SEALContext> con, std::shared_ptr<gfx950::DeviceContext> dev, seal::parms_id_type level_id, std::size_t limbs,
                const seal::SecretKey &sk, hhe::KeySet rk, hhe::KeySet gk, bool use_bsgs, size_t n1, size_t n2)
        : context(std::move(con)), device(std::move(dev)), core(device->level(limbs)), id(level_id), use_bsgs(use_bsgs), bsgs_n1(n1), bsgs_n2(n2),
          rk_top(std::move(rk)), gk_top(std::move(gk))
    {
        if (sk.data().coeff_count() == device->key_limbs() * device->poly_modulus_degree()) sk_level = device->level_rows(sk.data().data(), 1, limbs);
    }
    const seal::parms_id_type &parms_id() const { return id; }

    void mask(seal::Ciphertext &cipher, std::vector<uint64_t> &mask_vec) { core->mask(in(cipher), mask_vec.data(), mask_vec.size(), out(cipher)); }
    void flatten(std::vector<seal::Ciphertext> &in_cts, seal::Ciphertext &o, const seal::GaloisKeys &galois_keys)
    {
        core->flatten(pointers(in_cts), core->derived(device->galois_set(galois_keys)), out(o));
    }
    void packed_matMul(seal::Ciphertext &vo, const matrix &M, const seal::Ciphertext &vi)
    {
        core->packed_affine(M, nullptr, use_bsgs, bsgs_n1, bsgs_n2, in(vi), core->derived(gk_top), out(vo));
    }
    void packed_affine(seal::Ciphertext &vo, const matrix &M, const seal::Ciphertext &vi, const vector &b)
    {
        core->packed_affine(M, &b, use_bsgs, bsgs_n1, bsgs_n2, in(vi), core->derived(gk_top), out(vo));
    }
    void packed_square(seal::Ciphertext &vo, const seal::Ciphertext &vi) { core->square_relinearize(in(vi), core->derived(rk_top), out(vo)); }
    void packed_enc_mul(const seal::Ciphertext &e1, const seal::Ciphertext &e2, seal::Ciphertext &destination)
    {
        core->multiply(in(e1), in(e2), out(destination, 3));
    }
    void packed_enc_add(const seal::Ciphertext &e1, const seal::Ciphertext &e2, seal::Ciphertext &destination)
    {
        if (e1.size() != e2.size()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        core->add(in(e1, e1.size()), in(e2, e1.size()), e1.size(), out(destination, e1.size()));
    }
    // Evaluator::relinearize_inplace(encrypted, relin_keys) and sealhelper::encrypted_vec_sum with the key object the call names
    void relinearize_inplace(seal::Ciphertext &encrypted, const seal::RelinKeys &relin_keys)
    {
        core->relinearize(in(encrypted, 3), core->derived(device->relin_set(relin_keys)), out(encrypted));
    }
    void encrypted_vec_sum(const seal::Ciphertext &encrypted_inp, seal::Ciphertext &destination, const seal::GaloisKeys &gal_keys, size_t vec_size)
    {
        core->vec_sum(in(encrypted_inp), core->derived(device->galois_set(gal_keys)), vec_size, out(destination));
    }
    // packed encrypted FC at this level: the handle is made on the level's context from diagonals of this level
    EncMatrix enc_matrix(const std::vector<seal::Ciphertext> &diagonals, std::size_t rows, std::size_t cols)
    {
        return EncMatrix(context, device, core, id, diagonals, rows, cols);
    }
    void fc_packed(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply(vi, rk, gal_keys, out);
    }
    // chainable packed FC at this level: open diagonals, one open layer, the FC-square-FC network
    EncMatrix enc_matrix_open(const std::vector<seal::Ciphertext> &diagonals, std::size_t rows, std::size_t cols)
    {
        return EncMatrix(context, device, core, id, diagonals, rows, cols, true);
    }
    void fc_open(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
    {
        mlp({&mat}, vi, rk, gal_keys, out);
    }
    void mlp(const std::vector<const EncMatrix *> &layers, const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
             seal::Ciphertext &vo)
    {
        for (const EncMatrix *m : layers)
            if (m && m->core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
    }
    void fc_packed_hoisted(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply(vi, rk, gal_keys, out, true);
    }
    void fc_packed_sum(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out,
                       bool hoisted = false)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply_sum(vi, rk, gal_keys, out, hoisted);
    }
    // hoisted rotations at this level: o[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys) with the key object the call names
    void rotate_rows_many(const seal::Ciphertext &ct, const std::vector<int> &steps, const seal::GaloisKeys &gal_keys, std::vector<seal::Ciphertext> &o)
    {
        o.resize(steps.size());
        core->rotate_rows_many(in(ct), steps, core->derived(device->galois_set(gal_keys)), [&](std::size_t i) { return out(o[i])(0); });
    }
    // SEALZpCipher::print_noise / sealhelper::decrypting on the level's device context, with the rows of the secret key that level has
    int print_noise(seal::Ciphertext &ciph)
    {
        if (sk_level.empty()) throw std::invalid_argument("invariant_noise_budget: no secret key");
        if (ciph.size() < 2) throw std::invalid_argument("encrypted is not at the level of this object");
        const int noise = core->noise_budget({in(ciph, ciph.size())}, ciph.size(), 0, sk_level.data())[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }
    std::vector<int64_t> decrypting(const seal::Ciphertext &enc_input, size_t size)
    {
        const std::size_t n = core->poly_modulus_degree();
        if (sk_level.empty() || size > n) throw std::invalid_argument("decrypting: ciphertext / secret key do not match the context");
        std::vector<std::uint64_t> u(n);
        core->decrypt(sk_level.data(), in(enc_input), u.data());
        const std::uint64_t t = core->plain_modulus(), half = (t + 1) >> 1;
        std::vector<int64_t> o(size);
        for (size_t i = 0; i < size; i++) o[i] = u[i] > half ? (int64_t)u[i] - (int64_t)t : (int64_t)u[i];
        return o;
    }

private:
    std::shared_ptr<seal::SEALContext> context;
    std::shared_ptr<gfx950::DeviceContext> device;  // the chain's core: its key-set cache holds the sets the level's are derived from
    std::shared_ptr<hhe::AdapterCore> core;         // the level's
    seal::parms_id_type id;
    bool use_bsgs;
    size_t bsgs_n1, bsgs_n2;
    std::vector<std::uint64_t> sk_level;            // [limbs + 1][N]
    hhe::KeySet rk_top, gk_top;                     // the cipher object's sets, kept alive; declared after the contexts
};

// ---------------------------------------------------------------------------------------------------------------------
// pasta::SEALZpCipher (src/pasta/SEAL_Cipher.h:11-129).  The members the CSP path uses run on the device; the SEAL objects
// the reference keeps as members are kept too (encrypt_key, decrypt_result and the analyst/user sides use them unchanged).
class SEALZpCipher {
public:
    typedef std::vector<uint64_t> vector;
    typedef std::vector<std::vector<uint64_t>> matrix;

protected:
    std::vector<uint64_t> secret_key;
    ZpCipherParams params;
    uint64_t plain_mod;
    uint64_t mod_degree;

    std::vector<seal::Ciphertext> secret_key_encrypted;

    std::shared_ptr<seal::SEALContext> context;
    seal::KeyGenerator keygen;

    seal::SecretKey he_sk;
    seal::PublicKey he_pk;
    seal::RelinKeys he_rk;
    seal::GaloisKeys he_gk;

    seal::Encryptor encryptor;
    seal::Evaluator evaluator;
    seal::Decryptor decryptor;
    seal::BatchEncoder batch_encoder;

    std::vector<int> gk_indices;

    bool use_bsgs = false;
    size_t bsgs_n1 = 0;
    size_t bsgs_n2 = 0;

    std::shared_ptr<gfx950::DeviceContext> device;  // HBM-resident keys and tables, shared per parameter set
    // the device key sets of he_rk / he_gk, shared with the device context's cache and kept alive by this object when the cache
    // evicts them; null for an empty key object (declared after `device`: released while the context exists)
    hhe::KeySet rk_set, gk_set;

    std::vector<int> noise_budgets(const std::vector<const seal::Ciphertext *> &cts)
    {
        if (he_sk.data().coeff_count() != device->key_limbs() * mod_degree) throw std::invalid_argument("invariant_noise_budget: no secret key");
        std::vector<hhe::AdapterCore::NoiseItem> items;
        for (const seal::Ciphertext *ct : cts) items.push_back({device->level_words(*ct), ct->size(), ct->coeff_modulus_size()});
        return device->noise_budget(items, he_sk.data().data());
    }

public:
    // src/pasta/SEAL_Cipher.cpp:9-36 (all arguments by value, as the reference takes them)
    SEALZpCipher(ZpCipherParams params, std::shared_ptr<seal::SEALContext> con, seal::PublicKey pk, seal::SecretKey sk,
                 seal::RelinKeys rk, seal::GaloisKeys gk)
        : params(params), context(con), keygen(*context, sk), he_sk(sk), he_pk(pk), he_rk(rk), he_gk(gk),
          encryptor(*context, pk), evaluator(*context), decryptor(*context, sk), batch_encoder(*context),
          device(gfx950::DeviceContext::get(*context))
    {
        encryptor.set_public_key(pk);
        mod_degree = context->first_context_data()->parms().poly_modulus_degree();
        plain_mod = context->first_context_data()->parms().plain_modulus().value();
        rk_set = device->relin_set(he_rk);
        gk_set = device->galois_set(he_gk);
    }
    virtual ~SEALZpCipher() = default;

    size_t get_key_size() const { return params.key_size; }
    size_t get_plain_size() const { return params.plain_size; }
    size_t get_cipher_size() const { return params.cipher_size; }
    // SEALZpCipher::get_cipher_size(ct, mod_switch, levels_from_last) (SEAL_Cipher.cpp:363-378): the switch runs on the device
    // (hhe_mod_switch = Evaluator::mod_switch_to_inplace) and the destination takes the parms_id found by walking
    // last_context_data() -> prev_context_data(), as the reference walks.  The size returned is that of an UNCOMPRESSED save
    // (compr_mode_type::none); the reference's ct.save(s) takes SEAL's default, zstd.  levels_from_last beyond the chain throws
    // std::invalid_argument (the reference dereferences a null pointer there).
    size_t get_cipher_size(seal::Ciphertext &ct, bool mod_switch = false, size_t levels_from_last = 0)
    {
        if (mod_switch) {
            const std::size_t target = device->level_limbs(levels_from_last);
            auto c = context->last_context_data();
            for (uint64_t _ = 0; _ < levels_from_last; _++) c = c->prev_context_data();
            device->mod_switch(device->level_words(ct), ct.size(), ct.coeff_modulus_size(), target,
                               gfx950::DeviceContext::into_level(*context, ct, c->parms_id(), ct.size()));
        } else device->level_words(ct);
        return device->saved_size(ct.size(), ct.coeff_modulus_size());
    }

    // Evaluation at a level (no reference counterpart): the object bound to the level `levels_from_last` steps above
    // last_context_data(), the numbering of get_cipher_size, found by the same walk.  It evaluates what
    // get_cipher_size(ct, true, levels_from_last) produced, with this object's keys (their projections, derived on the device) and its
    // BSGS settings as they are now.  This object itself keeps refusing lower-level ciphertexts.
    SEALZpLevel level(size_t levels_from_last)
    {
        const std::size_t limbs = device->level_limbs(levels_from_last);
        auto c = context->last_context_data();
        for (uint64_t _ = 0; _ < levels_from_last; _++) c = c->prev_context_data();
        return SEALZpLevel(context, device, c->parms_id(), limbs, he_sk, rk_set, gk_set, use_bsgs, bsgs_n1, bsgs_n2);
    }
    // SEALZpCipher::print_noise (SEAL_Cipher.cpp:71-99): Decryptor::invariant_noise_budget with he_sk, on the device (one batched call for
    // the vector; a ciphertext below the data level at its coeff_modulus_size), the reference's lines on std::cout and its return
    // values.  An empty vector, where the reference reads ciphs[0], and an object without a secret key throw std::invalid_argument
    int print_noise() { return print_noise(secret_key_encrypted); }
    int print_noise(std::vector<seal::Ciphertext> &ciphs)
    {
        if (ciphs.empty()) throw std::invalid_argument("print_noise: no ciphertext");
        std::vector<const seal::Ciphertext *> p;
        for (auto &ct : ciphs) p.push_back(&ct);
        const std::vector<int> budget = noise_budgets(p);
        int min = budget[0], max = min;
        for (int b : budget) {
            if (b > max) max = b;
            if (b < min) min = b;
        }
        std::cout << "min noise budget: " << min << std::endl;
        std::cout << "max noise budget: " << max << std::endl;
        return min;
    }
    int print_noise(seal::Ciphertext &ciph)
    {
        const int noise = noise_budgets({&ciph})[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }

    void add_some_gk_indices(std::vector<int> &gk_ind)
    {
        for (auto &it : gk_ind) gk_indices.push_back(it);
    }
    void add_bsgs_indices(uint64_t bsgs_n1, uint64_t bsgs_n2) { hhe::bsgs_indices(batch_encoder.slot_count(), bsgs_n1, bsgs_n2, gk_indices); }
    void add_diagonal_indices(size_t size) { hhe::diagonal_indices(batch_encoder.slot_count(), size, gk_indices); }
    void create_gk() { keygen.create_galois_keys(gk_indices, he_gk); gk_set = device->galois_set(he_gk); }

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

    void activate_bsgs(bool activate) { use_bsgs = activate; }
    void set_bsgs_params(uint64_t bsgs_n1, uint64_t bsgs_n2) { this->bsgs_n1 = bsgs_n1; this->bsgs_n2 = bsgs_n2; }

    // SEALZpCipher::mask (SEAL_Cipher.cpp:161-166): batch_encoder.encode(mask) + multiply_plain_inplace
    void mask(seal::Ciphertext &cipher, std::vector<uint64_t> &mask)
    {
        device->mask(device->words(cipher), mask.data(), mask.size(), device->into(*context, cipher));
    }
    // SEALZpCipher::flatten (SEAL_Cipher.cpp:170-181): out = sum_i rotate_rows(in[i], -i * plain_size, galois_keys), with the GaloisKeys
    // object THIS call names (CSP.cpp:271-278: csp_he_gk)
    void flatten(std::vector<seal::Ciphertext> &in, seal::Ciphertext &out, const seal::GaloisKeys &galois_keys)
    {
        device->flatten(device->words(in), gfx950::DeviceContext::words(galois_keys), device->into(*context, out));
    }

    // Hoisted rotations (no reference counterpart: SEAL rotates one step per call): out[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys)
    // with the GaloisKeys object the call names, every rotation from the one set of digit transforms of ct
    void rotate_rows_many(const seal::Ciphertext &ct, const std::vector<int> &steps, const seal::GaloisKeys &gal_keys, std::vector<seal::Ciphertext> &out)
    {
        out.resize(steps.size());
        device->rotate_rows_many(device->words(ct), steps, gfx950::DeviceContext::words(gal_keys), device->into(*context, out));
    }

    // SEALZpCipher::packed_matMul / packed_affine (SEAL_Cipher.cpp:522-543): vo = M * vi (+ b), M public, rotations with he_gk
    void packed_matMul(seal::Ciphertext &vo, const matrix &M, const seal::Ciphertext &vi)
    {
        device->packed_affine(M, nullptr, use_bsgs, bsgs_n1, bsgs_n2, device->words(vi), gk_set, device->into(*context, vo));
    }
    void packed_affine(seal::Ciphertext &vo, const matrix &M, const seal::Ciphertext &vi, const vector &b)
    {
        device->packed_affine(M, &b, use_bsgs, bsgs_n1, bsgs_n2, device->words(vi), gk_set, device->into(*context, vo));
    }

    // packed helpers of the FC (SEAL_Cipher.cpp:547-566)
    void packed_square(seal::Ciphertext &vo, const seal::Ciphertext &vi)
    {
        device->square_relinearize(device->words(vi), rk_set, device->into(*context, vo));
    }
    // Chainable packed FC (no reference counterpart: hhe_pktnn_2fc_inference stops after fc1): the analyst's open diagonals as a resident
    // matrix, one open layer, and the FC-square-FC network as one device call, with the key objects the call names
    EncMatrix enc_matrix_open(const std::vector<seal::Ciphertext> &diagonals, std::size_t rows, std::size_t cols)
    {
        return EncMatrix(context, device, nullptr, context->first_parms_id(), diagonals, rows, cols, true);
    }
    void fc_open(const seal::Ciphertext &vi, const EncMatrix &mat, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys, seal::Ciphertext &out)
    {
        EncMatrix::mlp({&mat}, vi, rk, gal_keys, out);
    }
    void mlp(const std::vector<const EncMatrix *> &layers, const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
             seal::Ciphertext &vo)
    {
        EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
    }
    void packed_enc_mul(const seal::Ciphertext &encrypted1, const seal::Ciphertext &encrypted2, seal::Ciphertext &destination)
    {
        device->multiply(device->words(encrypted1), device->words(encrypted2), device->into(*context, destination, 3));
    }
    void packed_enc_add(const seal::Ciphertext &encrypted1, const seal::Ciphertext &encrypted2, seal::Ciphertext &destination)
    {
        if (encrypted1.size() != encrypted2.size()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        const size_t size = encrypted1.size();
        device->add(device->words(encrypted1, size), device->words(encrypted2, size), size, device->into(*context, destination, size));
    }
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

    // pasta_3_seal.cpp:42-104 == decomposition(ciphertexts, secret_key_encrypted) without the debug noise printing (:73; print_noise() is there to call)
    virtual std::vector<seal::Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder = false)
    {
        return decomposition(ciphertext, secret_key_encrypted, batch_encoder);
    }

    // pasta_3_seal.cpp:106-172: every 128-word block of the record on the device, one batched call
    virtual std::vector<seal::Ciphertext> decomposition(std::vector<uint64_t> &ciphertext, std::vector<seal::Ciphertext> enc_ssk,
                                                        bool batch_encoder = false)
    {
        (void)batch_encoder;  // ignored by the reference as well (:113)
        if (enc_ssk.empty()) throw std::invalid_argument("decomposition: enc_ssk is empty");
        std::vector<seal::Ciphertext> res(device->blocks_of(ciphertext.size()));
        // state <- enc_ssk[0] (:126); uploaded when its contents change
        device->transcipher(ciphertext, device->words(enc_ssk[0]), rk_set, gk_set, use_bsgs, device->into(*context, res));
        return res;
    }
    // ... of a record that was encrypted under `nonce`: block b runs under the pair (nonce, b).  Under one PASTA key a pair encrypts
    // one block, ever (hhe_gfx950.h "PASTA under a caller's nonce"); nobody checks it
    std::vector<seal::Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertext, bool batch_encoder, uint64_t nonce)
    {
        return decomposition(ciphertext, secret_key_encrypted, batch_encoder, nonce);
    }
    std::vector<seal::Ciphertext> decomposition(std::vector<uint64_t> &ciphertext, std::vector<seal::Ciphertext> enc_ssk, bool batch_encoder,
                                                uint64_t nonce)
    {
        (void)batch_encoder;
        if (enc_ssk.empty()) throw std::invalid_argument("decomposition: enc_ssk is empty");
        std::vector<seal::Ciphertext> res(device->blocks_of(ciphertext.size()));
        device->transcipher(ciphertext, device->words(enc_ssk[0]), rk_set, gk_set, use_bsgs, device->into(*context, res), nonce);
        return res;
    }

    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call: decomposition of every record, the mask of the
    // ragged last block (mask_last: as hhe_pktnn_examples.cpp:620-626; the CSP's own loop masks a copy, i.e. pass false to reproduce
    // that) and flatten with the GaloisKeys object `flatten_gk` -- the blocks never leave HBM.  One flattened ciphertext per record.
    std::vector<seal::Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<seal::Ciphertext> enc_ssk,
                                            const seal::GaloisKeys &flatten_gk, bool mask_last)
    {
        std::vector<seal::Ciphertext> res(records.size());
        if (records.empty()) return res;
        if (enc_ssk.empty()) throw std::invalid_argument("decompose: enc_ssk is empty");
        device->decompose(records, device->words(enc_ssk[0]), rk_set, gk_set, gfx950::DeviceContext::words(flatten_gk), mask_last,
                          device->into(*context, res));
        return res;
    }
    // ... with one nonce per record
    std::vector<seal::Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<seal::Ciphertext> enc_ssk,
                                            const seal::GaloisKeys &flatten_gk, bool mask_last, const std::vector<uint64_t> &nonces)
    {
        std::vector<seal::Ciphertext> res(records.size());
        if (records.empty()) return res;
        if (enc_ssk.empty()) throw std::invalid_argument("decompose: enc_ssk is empty");
        if (nonces.size() != records.size()) throw std::invalid_argument("decompose: one nonce per record");
        device->decompose(records, device->words(enc_ssk[0]), rk_set, gk_set, gfx950::DeviceContext::words(flatten_gk), mask_last,
                          device->into(*context, res), nonces);
        return res;
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

    // pasta_3_seal.cpp:190-201
    virtual void add_gk_indices()
    {
        gk_indices.push_back(0);
        gk_indices.push_back(-1);
        if (PASTA_T * 2 != batch_encoder.slot_count()) gk_indices.push_back(static_cast<int>(PASTA_T));
        if (use_bsgs)
            for (uint64_t k = 1; k < BSGS_N2; k++) gk_indices.push_back(-static_cast<int>(k * BSGS_N1));
    }

private:
    static constexpr uint64_t BSGS_N1 = 16;
    static constexpr uint64_t BSGS_N2 = 8;
    size_t slots;
    size_t halfslots;
};

}  // namespace pasta

// ---------------------------------------------------------------------------------------------------------------------
// sealhelper::packed_enc_multiply / encrypted_vec_sum (src/util/sealhelper.h:84-129, sealhelper.cpp:268-274,379-392) with the
// reference's signatures; the Evaluator argument is unused (the device context is found through the ciphertext's parms_id).
namespace sealhelper {
using pasta::gfx950::DeviceContext;

inline void packed_enc_multiply(const seal::Ciphertext &encrypted1, const seal::Ciphertext &encrypted2, seal::Ciphertext &destination,
                                const seal::Evaluator &evaluator)
{
    (void)evaluator;
    auto dev = DeviceContext::find(encrypted1.parms_id());
    dev->multiply(dev->words(encrypted1), dev->words(encrypted2), DeviceContext::into(destination, encrypted1, 3));
}

// Evaluator::relinearize_inplace(record, csp_rk) as the CSP calls it between the two (CSP.cpp:306), on the device, with the
// RelinKeys object the call names (its key set is uploaded the first time the object is seen).
inline void relinearize_inplace(seal::Ciphertext &encrypted, const seal::RelinKeys &relin_keys)
{
    auto dev = DeviceContext::find(encrypted.parms_id());
    dev->relinearize(dev->words(encrypted, 3), DeviceContext::words(relin_keys), DeviceContext::into(encrypted, encrypted));
}

inline void encrypted_vec_sum(const seal::Ciphertext &encrypted_inp, seal::Ciphertext &destination, const seal::Evaluator &evaluator,
                              const seal::GaloisKeys &gal_keys, const size_t vec_size)
{
    (void)evaluator;
    auto dev = DeviceContext::find(encrypted_inp.parms_id());
    dev->vec_sum(dev->words(encrypted_inp), DeviceContext::words(gal_keys), vec_size, DeviceContext::into(destination, encrypted_inp));
}

// The three FC calls of CSP_hhe_pktnn_1fc::evaluateModel (CSP.cpp:296-316) as ONE device call: multiply, relinearize with
// the CSP's RelinKeys, NAF-trie rotation sum with the analyst's default Galois keys -- identical ciphertext words.
inline void fc_row(const seal::Ciphertext &vi, const seal::Ciphertext &w_row, const seal::RelinKeys &csp_rk, const seal::GaloisKeys &gal_keys,
                   size_t vec_size, seal::Ciphertext &destination)
{
    auto dev = DeviceContext::find(vi.parms_id());
    dev->fc_row(dev->words(vi), dev->words(w_row), DeviceContext::words(csp_rk), DeviceContext::words(gal_keys), vec_size, DeviceContext::into(destination, vi));
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
    EncMatrix::mlp({&mat}, vi, rk, gal_keys, out);
}
inline void mlp(const std::vector<const EncMatrix *> &layers, const seal::Ciphertext &vi, const seal::RelinKeys &rk, const seal::GaloisKeys &gal_keys,
                seal::Ciphertext &vo)
{
    EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
}
// out[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys), hoisted (hhe_gfx950.h "Hoisted rotations"); the Evaluator argument is unused
inline void rotate_rows_many(const seal::Ciphertext &ct, const std::vector<int> &steps, const seal::GaloisKeys &gal_keys,
                             std::vector<seal::Ciphertext> &out, const seal::Evaluator &evaluator)
{
    (void)evaluator;
    auto dev = DeviceContext::find(ct.parms_id());
    out.resize(steps.size());
    dev->rotate_rows_many(dev->words(ct), steps, DeviceContext::words(gal_keys), [&](std::size_t i) { return DeviceContext::into(out[i], ct)(0); });
}

}  // namespace sealhelper
