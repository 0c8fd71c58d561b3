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
// Only the conversions between those containers and plain words live here: every call body is hhe::AdapterCore
// (hhe_adapter_core.hpp), the same code pasta_seal_gfx950_seal.hpp calls on seal:: types, and this header is the one the
// tests execute.  Errors surface as the C++ exceptions the reference / SEAL throw (std::runtime_error,
// std::invalid_argument, std::logic_error).
#pragma once
#include <cstdint>
#include <iostream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "hhe_adapter_core.hpp"

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

namespace detail {
// boundary types -> the core's plain words
inline hhe::RelinWords words(const RelinKeys &rk) { return {rk.key.data(), rk.key.size(), {}}; }
inline hhe::GaloisWords words(const GaloisKeys &gk)
{
    hhe::GaloisWords g;
    for (auto &kv : gk.keys) g.keys.emplace_back(kv.first, kv.second.data());
    if (!gk.keys.empty()) g.words = gk.keys.begin()->second.size();
    return g;
}
inline const uint64_t *words(const HheContext &ctx, const Ciphertext &ct, size_t size = 2)
{
    if (ct.words.size() != ctx.ct_words(size) || (ct.limbs && ct.limbs != ctx.data_limbs()))
        throw std::invalid_argument("encrypted is not valid for encryption parameters");
    return ct.words.data();
}
// output sinks: item i lands in a ciphertext of `size` polynomials
inline auto into(const HheContext &ctx, Ciphertext &ct, size_t size = 2)
{
    return [&ctx, &ct, size](size_t) { ct.words.resize(ctx.ct_words(size)); ct.size = size; ct.limbs = 0; return ct.words.data(); };
}
inline auto into(const HheContext &ctx, std::vector<Ciphertext> &cts) { return [&ctx, &cts](size_t i) { return into(ctx, cts[i])(0); }; }
// Decryptor::invariant_noise_budget of ciphertexts at any level (size 2 or 3, a switched-down result at its limbs): one device call
// for ciphertexts of one size and level
inline std::vector<int> noise_budgets(HheContext &ctx, const std::vector<const Ciphertext *> &cts, const SecretKey &he_sk)
{
    const size_t n = ctx.poly_modulus_degree();
    if (he_sk.words.size() != ctx.key_limbs() * n) throw std::invalid_argument("invariant_noise_budget: no secret key");
    std::vector<hhe::AdapterCore::NoiseItem> items;
    for (const Ciphertext *ct : cts) {
        if (ct->size < 2 || ct->words.size() != ct->size * ctx.limbs_or_data(ct->limbs) * n)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        items.push_back({ct->words.data(), ct->size, ct->limbs});
    }
    return ctx.noise_budget(items, he_sk.words.data());
}
// ... and at a level: `core` is the core of that level (hhe::AdapterCore::level), whose data level the ciphertext must be at
inline const uint64_t *level_words(const hhe::AdapterCore &core, size_t chain_limbs, const Ciphertext &ct, size_t size = 2)
{
    const size_t l = core.data_limbs();
    if (ct.words.size() != core.ct_words(size) || !(ct.limbs == l || (ct.limbs == 0 && l == chain_limbs)))
        throw std::invalid_argument("encrypted is not at the level of this object");
    return ct.words.data();
}
inline auto into_level(const hhe::AdapterCore &core, Ciphertext &ct, size_t size = 2)
{
    return [&core, &ct, size](size_t) { ct.words.resize(core.ct_words(size)); ct.size = size; ct.limbs = core.data_limbs(); return ct.words.data(); };
}
}  // namespace detail

// The analyst's encrypted weight matrix of a packed encrypted FC layer, resident on the device (hhe_gfx950.h "packed encrypted FC";
// no reference counterpart: the reference evaluates one encrypted row per neuron, CSP.cpp:296-316).  diagonals: the r encryptions of the
// generalized diagonals hhe_fc_packed_diagonals lays out, at the data level -- or, made by SEALZpLevel::enc_matrix, at that level.  The
// object holds the cores it needs, so it may outlive the cipher objects; a conversion into hhe::AdapterCore and nothing else.
struct EncMatrix {
    EncMatrix() = default;
    EncMatrix(std::shared_ptr<HheContext> con, const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols)
        : EncMatrix(con, con, diagonals, rows, cols) {}
    // open: the diagonals that do not wrap (hhe_fc_open_diagonals) -- the kind fc_open and mlp take; a cyclic one takes the fc_packed forms
    EncMatrix(std::shared_ptr<HheContext> con, std::shared_ptr<hhe::AdapterCore> at, const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols,
              bool open = false)
        : context(std::move(con)), core(std::move(at)), rows(rows), cols(cols), open(open)
    {
        std::vector<const uint64_t *> p;
        for (auto &ct : diagonals) p.push_back(detail::level_words(*core, context->data_limbs(), ct));
        handle = open ? core->enc_matrix_open(p, rows, cols) : core->enc_matrix(p, rows, cols);
    }
    // the network layers[0], square + relinearize, layers[1], ... on one ciphertext (hhe_mlp_ks); one layer is the open layer alone.
    // Every layer is an open matrix of one core; rk / gal_keys: the parties' ordinary, top-level key objects
    static void mlp(const std::vector<const EncMatrix *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        if (layers.empty() || !layers[0] || !layers[0]->core) throw std::invalid_argument("mlp: no encrypted matrix");
        const EncMatrix &first = *layers[0];
        std::vector<hhe::EncMatrix> handles;
        for (const EncMatrix *m : layers) {
            if (!m || !m->core) throw std::invalid_argument("mlp: no encrypted matrix");
            if (m->core.get() != first.core.get()) throw std::invalid_argument("mlp: the layers are not at one level");
            handles.push_back(m->handle);
        }
        const bool top = first.core.get() == first.context.get();
        hhe::KeySet r = first.context->keys().relin(detail::words(rk)), g = first.context->keys().galois(detail::words(gal_keys));
        if (!top) { r = first.core->derived(r); g = first.core->derived(g); }
        const uint64_t *x = detail::level_words(*first.core, first.context->data_limbs(), vi);
        first.core->mlp(x, handles, r, g, detail::into_level(*first.core, out));
        if (top) out.limbs = 0;  // the data level, as every cipher object's results
    }
    void apply_open(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out) const { mlp({this}, vi, rk, gal_keys, out); }
    // slots [0, rows) of the decryption of `out` are (M x) mod t; rk / gal_keys: the parties' ordinary, top-level key objects
    // hoisted: the rotation chain of the layer as rotations of one ciphertext (fc_packed_hoisted)
    // sum: one BEHZ floor over the sum of the layer's r products (fc_packed_sum), with either rotation schedule
    void apply(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out, bool hoisted = false, bool sum = false) const
    {
        if (!core) throw std::invalid_argument("fc_packed: no encrypted matrix");
        const bool top = core.get() == context.get();
        hhe::KeySet r = context->keys().relin(detail::words(rk)), g = context->keys().galois(detail::words(gal_keys));
        if (!top) { r = core->derived(r); g = core->derived(g); }
        const uint64_t *x = detail::level_words(*core, context->data_limbs(), vi);
        if (sum) core->fc_packed_sum(x, handle, r, g, detail::into_level(*core, out), hoisted);
        else if (hoisted) core->fc_packed_hoisted(x, handle, r, g, detail::into_level(*core, out));
        else core->fc_packed(x, handle, r, g, detail::into_level(*core, out));
        if (top) out.limbs = 0;  // the data level, as every cipher object's results
    }
    void apply_sum(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out, bool hoisted = false) const
    {
        apply(vi, rk, gal_keys, out, hoisted, true);
    }
    std::shared_ptr<HheContext> context;      // the chain's core: its key-set cache holds the sets the calls name
    std::shared_ptr<hhe::AdapterCore> core;   // where the handle lives: the chain's core, or a level's
    hhe::EncMatrix handle;                    // declared after the cores: released before them
    size_t rows = 0, cols = 0;
    bool open = false;
};

// What SEALZpCipher::level(levels_from_last) returns: the evaluation members of a cipher object, bound to one level of the modulus
// switching chain.  Every member takes and produces ciphertexts of exactly that level (Ciphertext::limbs == limbs()) and refuses any
// other with std::invalid_argument.  The object keeps no keys of its own: it names the key sets of the cipher object it came from,
// and the core derives their projections on the device on first use (hhe::AdapterCore::derived).  Key objects a call names
// (flatten, relinearize_inplace, encrypted_vec_sum) are the parties' ordinary, top-level objects.
class SEALZpLevel {
    // boundary conversions at this level (before their users: `out` has a deduced return type)
    const uint64_t *in(const Ciphertext &ct, size_t size = 2) const { return detail::level_words(*core, context->data_limbs(), ct, size); }
    auto out(Ciphertext &ct, size_t size = 2) const { return detail::into_level(*core, ct, size); }
    std::vector<const uint64_t *> pointers(const std::vector<Ciphertext> &cts) const
    {
        std::vector<const uint64_t *> p;
        for (auto &ct : cts) p.push_back(in(ct));
        return p;
    }

public:
    typedef std::vector<uint64_t> vector;
    typedef std::vector<std::vector<uint64_t>> matrix;
    SEALZpLevel(std::shared_ptr<HheContext> con, size_t limbs, const SecretKey &sk, hhe::KeySet rk, hhe::KeySet gk, bool use_bsgs, size_t n1, size_t n2)
        : context(std::move(con)), core(context->level(limbs)), use_bsgs(use_bsgs), bsgs_n1(n1), bsgs_n2(n2), rk_top(std::move(rk)), gk_top(std::move(gk))
    {
        if (sk.words.size() == context->key_limbs() * context->poly_modulus_degree()) sk_level = context->level_rows(sk.words.data(), 1, limbs);
    }
    size_t limbs() const { return core->data_limbs(); }

    void mask(Ciphertext &cipher, std::vector<uint64_t> &mask_vec) { core->mask(in(cipher), mask_vec.data(), mask_vec.size(), out(cipher)); }
    void flatten(std::vector<Ciphertext> &in_cts, Ciphertext &o, const GaloisKeys &galois_keys)
    {
        core->flatten(pointers(in_cts), core->derived(context->keys().galois(detail::words(galois_keys))), out(o));
    }
    void flatten(std::vector<Ciphertext> &in_cts, Ciphertext &o) { core->flatten(pointers(in_cts), core->derived(gk_top), out(o)); }
    void packed_enc_mul(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination) { core->multiply(in(e1), in(e2), out(destination, 3)); }
    void packed_enc_add(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination)
    {
        if (e1.size != e2.size) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        core->add(in(e1, e1.size), in(e2, e1.size), e1.size, out(destination, e1.size));
    }
    void packed_square(Ciphertext &vo, const Ciphertext &vi) { core->square_relinearize(in(vi), core->derived(rk_top), out(vo)); }
    void packed_matMul(Ciphertext &vo, const matrix &M, const Ciphertext &vi)
    {
        core->packed_affine(M, nullptr, use_bsgs, bsgs_n1, bsgs_n2, in(vi), core->derived(gk_top), out(vo));
    }
    void packed_affine(Ciphertext &vo, const matrix &M, const Ciphertext &vi, const vector &b)
    {
        core->packed_affine(M, &b, use_bsgs, bsgs_n1, bsgs_n2, in(vi), core->derived(gk_top), out(vo));
    }
    // Evaluator::relinearize_inplace(encrypted, relin_keys) and sealhelper::encrypted_vec_sum with the key object the call names
    void relinearize_inplace(Ciphertext &encrypted, const RelinKeys &relin_keys)
    {
        core->relinearize(in(encrypted, 3), core->derived(context->keys().relin(detail::words(relin_keys))), out(encrypted));
    }
    void encrypted_vec_sum(const Ciphertext &encrypted_inp, Ciphertext &destination, const GaloisKeys &gal_keys, size_t vec_size)
    {
        core->vec_sum(in(encrypted_inp), core->derived(context->keys().galois(detail::words(gal_keys))), vec_size, out(destination));
    }
    // packed encrypted FC at this level: the handle is made on the level's context from diagonals of this level
    EncMatrix enc_matrix(const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols) { return EncMatrix(context, core, diagonals, rows, cols); }
    void fc_packed(const Ciphertext &vi, const EncMatrix &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply(vi, rk, gal_keys, out);
    }
    // chainable packed FC at this level: open diagonals, one open layer, the FC-square-FC network
    EncMatrix enc_matrix_open(const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols)
    {
        return EncMatrix(context, core, diagonals, rows, cols, true);
    }
    void fc_open(const Ciphertext &vi, const EncMatrix &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        mlp({&mat}, vi, rk, gal_keys, out);
    }
    void mlp(const std::vector<const EncMatrix *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        for (const EncMatrix *m : layers)
            if (m && m->core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
    }
    void fc_packed_hoisted(const Ciphertext &vi, const EncMatrix &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply(vi, rk, gal_keys, out, true);
    }
    void fc_packed_sum(const Ciphertext &vi, const EncMatrix &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out, bool hoisted = false)
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
        mat.apply_sum(vi, rk, gal_keys, out, hoisted);
    }
    // hoisted rotations at this level: out[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys) with the key object the call names
    void rotate_rows_many(const Ciphertext &ct, const std::vector<int> &steps, const GaloisKeys &gal_keys, std::vector<Ciphertext> &o)
    {
        o.resize(steps.size());
        core->rotate_rows_many(in(ct), steps, core->derived(context->keys().galois(detail::words(gal_keys))), [&](size_t i) { return out(o[i])(0); });
    }
    // SEALZpCipher::print_noise / sealhelper::decrypting on the level's context, with the rows of the secret key that level has
    int print_noise(Ciphertext &ciph)
    {
        if (sk_level.empty()) throw std::invalid_argument("invariant_noise_budget: no secret key");
        if (ciph.size < 2) throw std::invalid_argument("encrypted is not at the level of this object");
        const int noise = core->noise_budget({in(ciph, ciph.size)}, ciph.size, 0, sk_level.data())[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }
    std::vector<int64_t> decrypting(const Ciphertext &enc_input, size_t size)
    {
        const size_t n = context->poly_modulus_degree();
        if (sk_level.empty() || size > n) throw std::invalid_argument("decrypting: ciphertext / secret key do not match the context");
        std::vector<uint64_t> u(n);
        core->decrypt(sk_level.data(), in(enc_input), u.data());
        const uint64_t t = context->plain_modulus(), half = (t + 1) >> 1;
        std::vector<int64_t> o(size);
        for (size_t i = 0; i < size; i++) o[i] = u[i] > half ? (int64_t)u[i] - (int64_t)t : (int64_t)u[i];
        return o;
    }
    hhe::AdapterCore &level_core() { return *core; }  // instrumentation (derivations, matrices().uploads())

private:
    std::shared_ptr<HheContext> context;        // the chain's core: its key-set cache holds the sets the level's are derived from
    std::shared_ptr<hhe::AdapterCore> core;     // the level's
    bool use_bsgs;
    size_t bsgs_n1, bsgs_n2;
    std::vector<uint64_t> sk_level;             // [limbs + 1][N]
    hhe::KeySet rk_top, gk_top;                 // the cipher object's sets, kept alive; declared after the contexts
};

class SEALZpCipher {
public:
    typedef std::vector<uint64_t> vector;
    typedef std::vector<std::vector<uint64_t>> matrix;

    SEALZpCipher(ZpCipherParams params, std::shared_ptr<HheContext> con, PublicKey pk, SecretKey sk, RelinKeys rk, GaloisKeys gk)
        : params(params), context(std::move(con)), he_pk(std::move(pk)), he_sk(std::move(sk))
    {
        // the by-value key members of the reference (SEAL_Cipher.h:28-31) become two device key sets, shared with every other cipher
        // object that was built from the same key objects (BaseCSP::decompose builds one per request, CSP.cpp:238-242)
        rk_set = context->keys().relin(detail::words(rk));
        gk_set = context->keys().galois(detail::words(gk));
        mod_degree = context->poly_modulus_degree();
        plain_mod = context->plain_modulus();
    }
    virtual ~SEALZpCipher() = default;

    size_t get_key_size() const { return params.key_size; }
    size_t get_plain_size() const { return params.plain_size; }
    size_t get_cipher_size() const { return params.cipher_size; }
    // SEALZpCipher::get_cipher_size(ct, mod_switch, levels_from_last) (SEAL_Cipher.cpp:363-378): with mod_switch, ct is switched in
    // place (Evaluator::mod_switch_to_inplace) to the level `levels_from_last` steps above last_context_data(), i.e. to
    // 1 + levels_from_last limbs; returns the byte size of the saved object.  Saves here are UNCOMPRESSED (compr_mode_type::none)
    // where the reference's ct.save(s) takes SEAL's default, zstd: the figure is the bound of the reference's.  levels_from_last >= L
    // throws std::invalid_argument (the reference walks off the chain there), and so does a switch to a higher level, as in SEAL.
    size_t get_cipher_size(Ciphertext &ct, bool mod_switch = false, size_t levels_from_last = 0)
    {
        const size_t cur = context->limbs_or_data(ct.limbs);
        if (ct.size < 2 || ct.words.size() != ct.size * cur * context->poly_modulus_degree())
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (mod_switch) {
            const size_t target = context->level_limbs(levels_from_last);
            context->mod_switch(ct.words.data(), ct.size, cur, target, [&](size_t) {
                ct.words.resize(ct.size * target * context->poly_modulus_degree());
                ct.limbs = target;
                return ct.words.data();
            });
        }
        return context->saved_size(ct.size, ct.limbs);
    }
    // Evaluation at a level (no reference counterpart: the reference only measures and ships switched ciphertexts).  The object bound to
    // the level `levels_from_last` steps above last_context_data(), the numbering of get_cipher_size: limbs = 1 + levels_from_last.  It
    // evaluates what get_cipher_size(ct, true, levels_from_last) produced, with this object's keys (their projections, derived on the
    // device) and its BSGS settings as they are now.  This object itself keeps refusing lower-level ciphertexts.
    SEALZpLevel level(size_t levels_from_last)
    {
        return SEALZpLevel(context, context->level_limbs(levels_from_last), he_sk, rk_set, gk_set, use_bsgs, bsgs_n1, bsgs_n2);
    }
    // SEALZpCipher::print_noise (SEAL_Cipher.cpp:71-99): Decryptor::invariant_noise_budget with this object's secret key, on the device
    // (one batched call for the vector), the reference's lines on std::cout and its return values.  An empty vector, where the
    // reference reads ciphs[0], and an object without a secret key throw std::invalid_argument
    int print_noise() { return print_noise(secret_key_encrypted); }
    int print_noise(std::vector<Ciphertext> &ciphs)
    {
        if (ciphs.empty()) throw std::invalid_argument("print_noise: no ciphertext");
        std::vector<const Ciphertext *> p;
        for (auto &ct : ciphs) p.push_back(&ct);
        const std::vector<int> budget = detail::noise_budgets(*context, p, he_sk);
        int min = budget[0], max = min;
        for (int b : budget) {
            if (b > max) max = b;
            if (b < min) min = b;
        }
        std::cout << "min noise budget: " << min << std::endl;
        std::cout << "max noise budget: " << max << std::endl;
        return min;
    }
    int print_noise(Ciphertext &ciph)
    {
        const int noise = detail::noise_budgets(*context, {&ciph}, he_sk)[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }
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

    void activate_bsgs(bool activate) { use_bsgs = activate; }
    void set_bsgs_params(uint64_t n1, uint64_t n2) { bsgs_n1 = n1; bsgs_n2 = n2; }
    void add_some_gk_indices(std::vector<int> &gk_ind) { for (int i : gk_ind) gk_indices.push_back(i); }
    void add_bsgs_indices(uint64_t n1, uint64_t n2) { hhe::bsgs_indices(mod_degree, n1, n2, gk_indices); }   // SEAL_Cipher.cpp:337-346
    void add_diagonal_indices(size_t size) { hhe::diagonal_indices(mod_degree, size, gk_indices); }          // :350-355
    const std::vector<int> &get_gk_indices() const { return gk_indices; }
    // SEALZpCipher::create_gk (SEAL_Cipher.cpp:359): keygen.create_galois_keys(gk_indices, he_gk) with this object's secret key, on the
    // device; the object then rotates with these keys.  get_galois_keys(): what the analyst ships to the CSP
    void create_gk(Seed seed)
    {
        if (he_sk.words.size() != context->key_limbs() * context->poly_modulus_degree()) throw std::invalid_argument("create_gk: no secret key");
        context->generate_galois(he_sk.words.data(), gk_indices, seed, he_gk.keys);
        gk_set = context->keys().galois(detail::words(he_gk));
    }
    const GaloisKeys &get_galois_keys() const { return he_gk; }

    // SEALZpCipher::mask (SEAL_Cipher.cpp:161-166)
    void mask(Ciphertext &cipher, std::vector<uint64_t> &mask_vec)
    {
        context->mask(detail::words(*context, cipher), mask_vec.data(), mask_vec.size(), detail::into(*context, cipher));
    }
    // SEALZpCipher::flatten(in, out, galois_keys) (SEAL_Cipher.cpp:170-181): the rotations use the GaloisKeys object the CALL names
    // (CSP.cpp:271-278 passes csp_he_gk, not the keys the cipher object was built with)
    void flatten(std::vector<Ciphertext> &in, Ciphertext &out, const GaloisKeys &galois_keys)
    {
        context->flatten(pointers(in), detail::words(galois_keys), detail::into(*context, out));
    }
    // convenience: with the Galois keys held by this object
    void flatten(std::vector<Ciphertext> &in, Ciphertext &out) { context->flatten(pointers(in), gk_set, detail::into(*context, out)); }

    // SEALZpCipher::packed_enc_mul / packed_enc_add / packed_square (SEAL_Cipher.cpp:547-566)
    void packed_enc_mul(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination)
    {
        context->multiply(detail::words(*context, e1), detail::words(*context, e2), detail::into(*context, destination, 3));
    }
    void packed_enc_add(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination)
    {
        if (e1.size != e2.size) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        context->add(detail::words(*context, e1, e1.size), detail::words(*context, e2, e1.size), e1.size, detail::into(*context, destination, e1.size));
    }
    void packed_square(Ciphertext &vo, const Ciphertext &vi)  // evaluator.square + relinearize_inplace(he_rk)
    {
        context->square_relinearize(detail::words(*context, vi), rk_set, detail::into(*context, vo));
    }

    // Chainable packed FC (no reference counterpart: hhe_pktnn_2fc_inference stops after fc1): the analyst's open diagonals as a resident
    // matrix, one open layer, and the FC-square-FC network as one device call, with the key objects the call names
    EncMatrix enc_matrix_open(const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols)
    {
        return EncMatrix(context, context, diagonals, rows, cols, true);
    }
    void fc_open(const Ciphertext &vi, const EncMatrix &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        EncMatrix::mlp({&mat}, vi, rk, gal_keys, out);
    }
    void mlp(const std::vector<const EncMatrix *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
    }

    // Hoisted rotations (no reference counterpart: SEAL rotates one step per call): out[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys)
    // with the GaloisKeys object the call names, every rotation from the one set of digit transforms of ct
    void rotate_rows_many(const Ciphertext &ct, const std::vector<int> &steps, const GaloisKeys &gal_keys, std::vector<Ciphertext> &out)
    {
        out.resize(steps.size());
        context->rotate_rows_many(detail::words(*context, ct), steps, detail::words(gal_keys), detail::into(*context, out));
    }

    // SEALZpCipher::packed_matMul / packed_affine (SEAL_Cipher.cpp:522-543): vo = M * vi (+ b), M public, with this object's Galois keys
    void packed_matMul(Ciphertext &vo, const matrix &M, const Ciphertext &vi)
    {
        context->packed_affine(M, nullptr, use_bsgs, bsgs_n1, bsgs_n2, detail::words(*context, vi), gk_set, detail::into(*context, vo));
    }
    void packed_affine(Ciphertext &vo, const matrix &M, const Ciphertext &vi, const vector &b)
    {
        context->packed_affine(M, &b, use_bsgs, bsgs_n1, bsgs_n2, detail::words(*context, vi), gk_set, detail::into(*context, vo));
    }

protected:
    std::vector<const uint64_t *> pointers(const std::vector<Ciphertext> &cts) const
    {
        std::vector<const uint64_t *> p;
        for (auto &ct : cts) p.push_back(detail::words(*context, ct));
        return p;
    }
    ZpCipherParams params;
    uint64_t plain_mod = 0, mod_degree = 0;
    std::vector<Ciphertext> secret_key_encrypted;
    std::shared_ptr<HheContext> context;
    PublicKey he_pk;
    SecretKey he_sk;
    GaloisKeys he_gk;  // filled by create_gk only
    std::vector<int> gk_indices;
    bool use_bsgs = false;
    size_t bsgs_n1 = 0, bsgs_n2 = 0;
    // device key sets of this object's key members, shared with the context's cache and kept alive by this object when the cache
    // evicts them; null for an empty key object.  Declared after `context`: released while their context still exists
    hhe::KeySet rk_set, gk_set;
};

class PASTA_SEAL : public SEALZpCipher {
public:
    PASTA_SEAL(std::shared_ptr<HheContext> con, PublicKey pk, SecretKey sk, RelinKeys rk, GaloisKeys gk)
        : SEALZpCipher(PASTA_PARAMS, std::move(con), std::move(pk), std::move(sk), std::move(rk), std::move(gk)),
          slots(mod_degree), halfslots(mod_degree >> 1) {}

    virtual std::string get_cipher_name() const { return "PASTA-SEAL (n=128,r=3)"; }

    // pasta_3_seal.cpp:190-201
    virtual void add_gk_indices()
    {
        gk_indices.push_back(0);
        gk_indices.push_back(-1);
        if (PASTA_PARAMS.plain_size * 2 != slots) gk_indices.push_back((int)PASTA_PARAMS.plain_size);
        if (use_bsgs)
            for (uint64_t k = 1; k < BSGS_N2; k++) gk_indices.push_back(-(int)(k * BSGS_N1));
    }

    // supply the BFV encryption of the PASTA key that HE_decrypt reads (secret_key_encrypted[0],
    // pasta_3_seal.cpp:58; filled by encrypt_key() on the client side of the reference)
    void set_encrypted_key(const Ciphertext &enc_key) { secret_key_encrypted.assign(1, enc_key); }

    // PASTA_SEAL::encrypt_key_2 (pasta_3_seal.cpp:23-38): the BFV encryption of the 256-word PASTA key ssk under this object's public
    // key, packed as the reference packs it (words 0..127 at slots 0.., words 128..255 at slots N/2..)
    std::vector<Ciphertext> encrypt_key_2(const std::vector<uint64_t> &ssk, Seed seed)
    {
        if (ssk.size() != PASTA_PARAMS.key_size) throw std::runtime_error("Invalid Key length");
        if (he_pk.words.size() != 2 * context->key_limbs() * slots) throw std::invalid_argument("encrypt_key_2: no public key");
        std::vector<uint64_t> key_tmp(halfslots + PASTA_PARAMS.plain_size, 0);
        for (size_t i = 0; i < PASTA_PARAMS.plain_size; i++) {
            key_tmp[i] = ssk[i];
            key_tmp[i + halfslots] = ssk[i + PASTA_PARAMS.plain_size];
        }
        std::vector<Ciphertext> enc_sk(1);
        context->encrypt(he_pk.words.data(), key_tmp.data(), key_tmp.size(), seed, detail::into(*context, enc_sk[0]));
        return enc_sk;
    }

    // PASTA_SEAL::HE_decrypt (pasta_3_seal.cpp:42-104) == decomposition(ciphertexts, secret_key_encrypted)
    virtual std::vector<Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertexts, bool batch_encoder = false)
    {
        if (secret_key_encrypted.empty()) throw std::logic_error("HE_decrypt: encrypted key not set");
        return decomposition(ciphertexts, secret_key_encrypted, batch_encoder);
    }

    // PASTA_SEAL::decomposition (pasta_3_seal.cpp:106-172)
    virtual std::vector<Ciphertext> decomposition(std::vector<uint64_t> &ciphertexts, std::vector<Ciphertext> enc_ssk,
                                                  bool batch_encoder = false)
    {
        (void)batch_encoder;  // ignored by the reference as well (:113)
        if (enc_ssk.empty()) throw std::invalid_argument("decomposition: enc_ssk is empty");
        if (enc_ssk[0].words.size() != context->ct_words()) throw std::invalid_argument("decomposition: enc_ssk is not valid for encryption parameters");
        std::vector<Ciphertext> res(context->blocks_of(ciphertexts.size()));
        context->transcipher(ciphertexts, enc_ssk[0].words.data(), rk_set, gk_set, use_bsgs, detail::into(*context, res));
        return res;
    }
    // ... of a record that was encrypted under `nonce` (PASTA::encrypt with a nonce below): block b runs under the pair (nonce, b).
    // Under one PASTA key a pair encrypts one block, ever (hhe_gfx950.h "PASTA under a caller's nonce"); nobody checks it
    std::vector<Ciphertext> HE_decrypt(std::vector<uint64_t> &ciphertexts, bool batch_encoder, uint64_t nonce)
    {
        if (secret_key_encrypted.empty()) throw std::logic_error("HE_decrypt: encrypted key not set");
        return decomposition(ciphertexts, secret_key_encrypted, batch_encoder, nonce);
    }
    std::vector<Ciphertext> decomposition(std::vector<uint64_t> &ciphertexts, std::vector<Ciphertext> enc_ssk, bool batch_encoder, uint64_t nonce)
    {
        (void)batch_encoder;
        if (enc_ssk.empty()) throw std::invalid_argument("decomposition: enc_ssk is empty");
        if (enc_ssk[0].words.size() != context->ct_words()) throw std::invalid_argument("decomposition: enc_ssk is not valid for encryption parameters");
        std::vector<Ciphertext> res(context->blocks_of(ciphertexts.size()));
        context->transcipher(ciphertexts, enc_ssk[0].words.data(), rk_set, gk_set, use_bsgs, detail::into(*context, res), nonce);
        return res;
    }

    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call: decomposition of every record, the mask of the
    // ragged last block (mask_last: as hhe_pktnn_examples.cpp:620-626; the CSP's own loop masks a copy, i.e. pass false to reproduce
    // that) and flatten with the GaloisKeys object `flatten_gk` -- the blocks never leave HBM.  One flattened ciphertext per record.
    std::vector<Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<Ciphertext> enc_ssk,
                                      const GaloisKeys &flatten_gk, bool mask_last)
    {
        std::vector<Ciphertext> res(records.size());
        if (records.empty()) return res;
        if (enc_ssk.empty()) throw std::invalid_argument("decompose: enc_ssk is empty");
        if (enc_ssk[0].words.size() != context->ct_words()) throw std::invalid_argument("decompose: enc_ssk is not valid for encryption parameters");
        context->decompose(records, enc_ssk[0].words.data(), rk_set, gk_set, detail::words(flatten_gk), mask_last, detail::into(*context, res));
        return res;
    }
    // ... with one nonce per record
    std::vector<Ciphertext> decompose(const std::vector<std::vector<uint64_t>> &records, std::vector<Ciphertext> enc_ssk,
                                      const GaloisKeys &flatten_gk, bool mask_last, const std::vector<uint64_t> &nonces)
    {
        std::vector<Ciphertext> res(records.size());
        if (records.empty()) return res;
        if (enc_ssk.empty()) throw std::invalid_argument("decompose: enc_ssk is empty");
        if (enc_ssk[0].words.size() != context->ct_words()) throw std::invalid_argument("decompose: enc_ssk is not valid for encryption parameters");
        if (nonces.size() != records.size()) throw std::invalid_argument("decompose: one nonce per record");
        context->decompose(records, enc_ssk[0].words.data(), rk_set, gk_set, detail::words(flatten_gk), mask_last, detail::into(*context, res), nonces);
        return res;
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
    const uint64_t t = ctx.plain_modulus(), half = (t + 1) >> 1;
    std::vector<int64_t> out(size);
    for (size_t i = 0; i < size; i++) out[i] = u[i] > half ? (int64_t)u[i] - (int64_t)t : (int64_t)u[i];
    return out;
}

// Decryptor::invariant_noise_budget (seal/decryptor.h:103) of a ciphertext of size 2 or 3 at its level, on the device: what tells whether
// `decrypting` returns the right slots (a budget of 0 means it does not)
inline int invariant_noise_budget(const pasta::Ciphertext &enc_input, const pasta::SecretKey &he_sk, pasta::HheContext &ctx)
{
    return pasta::detail::noise_budgets(ctx, {&enc_input}, he_sk)[0];
}

// sealhelper::packed_enc_multiply, Evaluator::relinearize_inplace(record, csp_rk) and sealhelper::encrypted_vec_sum as
// CSP_hhe_pktnn_1fc::evaluateModel calls them one after the other (sealhelper.cpp:268-274, 379-392; CSP.cpp:296-316), each with the
// key object the call names; the context stands in for the Evaluator argument
inline void packed_enc_multiply(pasta::HheContext &ctx, const pasta::Ciphertext &encrypted1, const pasta::Ciphertext &encrypted2,
                                pasta::Ciphertext &destination)
{
    ctx.multiply(pasta::detail::words(ctx, encrypted1), pasta::detail::words(ctx, encrypted2), pasta::detail::into(ctx, destination, 3));
}
inline void relinearize_inplace(pasta::HheContext &ctx, pasta::Ciphertext &encrypted, const pasta::RelinKeys &relin_keys)
{
    ctx.relinearize(pasta::detail::words(ctx, encrypted, 3), pasta::detail::words(relin_keys), pasta::detail::into(ctx, encrypted));
}
inline void encrypted_vec_sum(pasta::HheContext &ctx, const pasta::Ciphertext &encrypted_inp, pasta::Ciphertext &destination,
                              const pasta::GaloisKeys &gal_keys, const size_t vec_size)
{
    ctx.vec_sum(pasta::detail::words(ctx, encrypted_inp), pasta::detail::words(gal_keys), vec_size, pasta::detail::into(ctx, destination));
}
// the same three calls for one weight row as ONE device call: identical ciphertext words
inline void fc_row(pasta::HheContext &ctx, const pasta::Ciphertext &vi, const pasta::Ciphertext &w_row, const pasta::RelinKeys &csp_rk,
                   const pasta::GaloisKeys &gal_keys, size_t vec_size, pasta::Ciphertext &destination)
{
    ctx.fc_row(pasta::detail::words(ctx, vi), pasta::detail::words(ctx, w_row), pasta::detail::words(csp_rk), pasta::detail::words(gal_keys), vec_size,
               pasta::detail::into(ctx, destination));
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
    EncMatrix::mlp({&mat}, vi, rk, gal_keys, out);
}
inline void mlp(const std::vector<const EncMatrix *> &layers, const pasta::Ciphertext &vi, const pasta::RelinKeys &rk,
                const pasta::GaloisKeys &gal_keys, pasta::Ciphertext &vo)
{
    EncMatrix::mlp(layers, vi, rk, gal_keys, vo);
}
// out[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys), hoisted (hhe_gfx950.h "Hoisted rotations")
inline void rotate_rows_many(pasta::HheContext &ctx, const pasta::Ciphertext &ct, const std::vector<int> &steps, const pasta::GaloisKeys &gal_keys,
                             std::vector<pasta::Ciphertext> &out)
{
    out.resize(steps.size());
    ctx.rotate_rows_many(pasta::detail::words(ctx, ct), steps, pasta::detail::words(gal_keys), pasta::detail::into(ctx, out));
}
}  // namespace sealhelper
