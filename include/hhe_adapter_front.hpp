// hhe_adapter_front.hpp -- the cipher-layer classes of the two C++ adapters, written once over a boundary policy B.
// pasta_seal_gfx950.hpp (word containers; executed by the tests) and pasta_seal_gfx950_seal.hpp (seal:: types; type-checked only)
// each supply a B and instantiate these templates, so the source text the drivers execute is the text the SEAL-typed header compiles.
// Nothing here sees seal:: or the mirror's containers.  B is a struct of typedefs and static functions:
//   Ciphertext, RelinKeys, GaloisKeys, SecretKey   the boundary types
//   Context     the header's context class, derived from hhe::AdapterCore: the core of the chain's data level
//   Binding     what a caller holds to name a context (a cipher object's constructor argument); chain(binding) -> shared_ptr<Context>
//   Level       what names a level of the modulus switching chain at the boundary; top(ctx): the data level's,
//               level_id(ctx, levels_from_last): that of the level so many steps above the last one (the caller has checked the count)
//   in(ctx, level, ct, size)    the words of a coefficient-form ciphertext of `size` polynomials at that level, null if it is not one
//   in_any(ctx, ct)             ... of size >= 2 at any level of the chain (noise budget, get_cipher_size)
//   out(ctx, level, ct, size)   the sink `uint64_t *(size_t)` that makes ct a ciphertext of `size` polynomials at that level
//   size(ct), limbs(ct)         polynomials; data primes as the core's calls take them (0 = the data level)
//   words(RelinKeys), words(GaloisKeys) -> hhe::RelinWords / hhe::GaloisWords; secret(SecretKey) -> (its words, their count)
#pragma once
#include <iostream>
#include "hhe_adapter_core.hpp"

namespace hhe {

// BatchEncoder::decode into signed values: a slot value above (t+1)/2 reads as v - t
inline int64_t centred(uint64_t u, uint64_t t) { return u > ((t + 1) >> 1) ? (int64_t)u - (int64_t)t : (int64_t)u; }

constexpr const char *NOT_VALID = "encrypted is not valid for encryption parameters";   // a cipher object, a free function
constexpr const char *NOT_AT_LEVEL = "encrypted is not at the level of this object";    // a level object, an encrypted matrix
inline const uint64_t *accepted(const uint64_t *words, const char *refusal)
{
    if (!words) throw std::invalid_argument(refusal);
    return words;
}

// Where an object computes: the chain's context (its key-set cache holds the sets the calls name), the core of the level (the chain's own
// at the data level, else AdapterCore::level's) and what names that level at the boundary.  Key sets a call names are the parties'
// ordinary, top-level objects: below the data level the core derives their projections on the device on first use (AdapterCore::derived).
template <class B> struct BoundT {
    typedef typename B::Context Context;
    typedef typename B::Ciphertext Ciphertext;
    typedef typename B::RelinKeys RelinKeys;
    typedef typename B::GaloisKeys GaloisKeys;
    typedef typename B::SecretKey SecretKey;
    typedef typename B::Level Level;

    BoundT() = default;
    BoundT(std::shared_ptr<Context> dev, std::shared_ptr<AdapterCore> at, Level level)
        : device(std::move(dev)), core(at ? std::move(at) : std::shared_ptr<AdapterCore>(device)), id(std::move(level)) {}
    static BoundT at_top(std::shared_ptr<Context> dev)
    {
        Level level = B::top(*dev);
        return BoundT(std::move(dev), nullptr, std::move(level));
    }
    // the level `levels_from_last` steps above last_context_data(), the numbering of get_cipher_size: 1 + levels_from_last data primes
    static BoundT at_level(std::shared_ptr<Context> dev, size_t levels_from_last)
    {
        std::shared_ptr<AdapterCore> at = dev->level(dev->level_limbs(levels_from_last));
        Level level = B::level_id(*dev, levels_from_last);
        return BoundT(std::move(dev), std::move(at), std::move(level));
    }
    bool top() const { return core.get() == device.get(); }
    const uint64_t *in(const Ciphertext &ct, size_t size, const char *refusal) const { return accepted(B::in(*device, id, ct, size), refusal); }
    auto out(Ciphertext &ct, size_t size = 2) const { return B::out(*device, id, ct, size); }
    KeySet held(const KeySet &top_set) const { return top() ? top_set : core->derived(top_set); }
    KeySet relin(const RelinKeys &rk) const { return held(device->keys().relin(B::words(rk))); }
    KeySet galois(const GaloisKeys &gk) const { return held(device->keys().galois(B::words(gk))); }

    std::shared_ptr<Context> device;     // the chain's core
    std::shared_ptr<AdapterCore> core;   // where the calls run: the chain's core, or a level's
    Level id{};                          // the level of the inputs and the results
};

// The analyst's encrypted weight matrix of a packed encrypted FC layer, resident on the device (hhe_gfx950.h "packed encrypted FC";
// no reference counterpart: the reference evaluates one encrypted row per neuron, CSP.cpp:296-316).  diagonals: the r encryptions of the
// generalized diagonals hhe_fc_packed_diagonals lays out, at the data level -- or, made by LevelT::enc_matrix, at that level.  The
// object holds the cores it needs, so it may outlive the cipher objects.
template <class B> struct EncMatrixT : BoundT<B> {
    using typename BoundT<B>::Ciphertext;
    using typename BoundT<B>::RelinKeys;
    using typename BoundT<B>::GaloisKeys;
    using BoundT<B>::core;

    EncMatrixT() = default;
    EncMatrixT(const typename B::Binding &con, const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols)
        : EncMatrixT(BoundT<B>::at_top(B::chain(con)), diagonals, rows, cols) {}
    // open: the diagonals that do not wrap (hhe_fc_open_diagonals) -- the kind fc_open and mlp take; a cyclic one takes the fc_packed forms
    EncMatrixT(BoundT<B> where, const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols, bool open = false)
        : BoundT<B>(std::move(where)), rows(rows), cols(cols), open(open)
    {
        std::vector<const uint64_t *> p;
        for (auto &ct : diagonals) p.push_back(this->in(ct, 2, NOT_AT_LEVEL));
        handle = open ? core->enc_matrix_open(p, rows, cols) : core->enc_matrix(p, rows, cols);
    }
    // the network layers[0], square + relinearize, layers[1], ... on one ciphertext (hhe_mlp_ks); one layer is the open layer alone.
    // Every layer is an open matrix of one core; rk / gal_keys: the parties' ordinary, top-level key objects
    static void mlp(const std::vector<const EncMatrixT *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out)
    {
        if (layers.empty() || !layers[0] || !layers[0]->core) throw std::invalid_argument("mlp: no encrypted matrix");
        const EncMatrixT &first = *layers[0];
        std::vector<hhe::EncMatrix> handles;
        for (const EncMatrixT *m : layers) {
            if (!m || !m->core) throw std::invalid_argument("mlp: no encrypted matrix");
            if (m->core.get() != first.core.get()) throw std::invalid_argument("mlp: the layers are not at one level");
            handles.push_back(m->handle);
        }
        const KeySet r = first.relin(rk), g = first.galois(gal_keys);
        const uint64_t *x = first.in(vi, 2, NOT_AT_LEVEL);
        first.core->mlp(x, handles, r, g, first.out(out));
    }
    void apply_open(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out) const { mlp({this}, vi, rk, gal_keys, out); }
    // slots [0, rows) of the decryption of `out` are (M x) mod t; rk / gal_keys: the parties' ordinary, top-level key objects
    // hoisted: the rotation chain of the layer as rotations of one ciphertext (fc_packed_hoisted)
    // sum: one BEHZ floor over the sum of the layer's r products (fc_packed_sum), with either rotation schedule
    void apply(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out, bool hoisted = false, bool sum = false) const
    {
        if (!core) throw std::invalid_argument("fc_packed: no encrypted matrix");
        const KeySet r = this->relin(rk), g = this->galois(gal_keys);
        const uint64_t *x = this->in(vi, 2, NOT_AT_LEVEL);
        if (sum) core->fc_packed_sum(x, handle, r, g, this->out(out), hoisted);
        else if (hoisted) core->fc_packed_hoisted(x, handle, r, g, this->out(out));
        else core->fc_packed(x, handle, r, g, this->out(out));
    }
    void apply_sum(const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &out, bool hoisted = false) const
    {
        apply(vi, rk, gal_keys, out, hoisted, true);
    }
    hhe::EncMatrix handle;   // declared after the cores (the base): released before them
    size_t rows = 0, cols = 0;
    bool open = false;
};

// The evaluation members a cipher object and a level object share: each takes and produces ciphertexts of exactly the level the object is
// bound to and refuses any other with std::invalid_argument.  rk_set / gk_set are the device key sets of the cipher object's key members
// (top-level sets; a level object names the sets of the cipher object it came from); a key object a call names is looked up per call.
template <class B> class EvalT : protected BoundT<B> {
public:
    typedef std::vector<uint64_t> vector;
    typedef std::vector<std::vector<uint64_t>> matrix;
    using typename BoundT<B>::Ciphertext;
    using typename BoundT<B>::RelinKeys;
    using typename BoundT<B>::GaloisKeys;

protected:
    using BoundT<B>::core;
    using BoundT<B>::out;
    EvalT(BoundT<B> where, KeySet rk, KeySet gk, bool use_bsgs = false, size_t n1 = 0, size_t n2 = 0)
        : BoundT<B>(std::move(where)), use_bsgs(use_bsgs), bsgs_n1(n1), bsgs_n2(n2), rk_set(std::move(rk)), gk_set(std::move(gk)) {}
    const uint64_t *in(const Ciphertext &ct, size_t size = 2) const { return BoundT<B>::in(ct, size, this->top() ? NOT_VALID : NOT_AT_LEVEL); }
    std::vector<const uint64_t *> pointers(const std::vector<Ciphertext> &cts) const
    {
        std::vector<const uint64_t *> p;
        for (auto &ct : cts) p.push_back(in(ct));
        return p;
    }
    auto outs(std::vector<Ciphertext> &cts) const { return [this, &cts](size_t i) { return this->out(cts[i])(0); }; }

public:
    // SEALZpCipher::mask (SEAL_Cipher.cpp:161-166): batch_encoder.encode(mask) + multiply_plain_inplace
    void mask(Ciphertext &cipher, std::vector<uint64_t> &mask_vec) { core->mask(in(cipher), mask_vec.data(), mask_vec.size(), out(cipher)); }
    // SEALZpCipher::flatten(in, out, galois_keys) (SEAL_Cipher.cpp:170-181): out = sum_i rotate_rows(in[i], -i * plain_size, galois_keys);
    // the rotations use the GaloisKeys object the CALL names (CSP.cpp:271-278 passes csp_he_gk, not the keys the cipher object was built with)
    void flatten(std::vector<Ciphertext> &in_cts, Ciphertext &o, const GaloisKeys &galois_keys)
    {
        const std::vector<const uint64_t *> p = pointers(in_cts);
        core->flatten(p, this->galois(galois_keys), out(o));
    }
    // convenience: with the Galois keys held by this object
    void flatten(std::vector<Ciphertext> &in_cts, Ciphertext &o) { core->flatten(pointers(in_cts), this->held(gk_set), out(o)); }

    // SEALZpCipher::packed_enc_mul / packed_enc_add / packed_square (SEAL_Cipher.cpp:547-566)
    void packed_enc_mul(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination) { core->multiply(in(e1), in(e2), out(destination, 3)); }
    void packed_enc_add(const Ciphertext &e1, const Ciphertext &e2, Ciphertext &destination)
    {
        const size_t size = B::size(e1);
        if (size != B::size(e2)) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        core->add(in(e1, size), in(e2, size), size, out(destination, size));
    }
    void packed_square(Ciphertext &vo, const Ciphertext &vi)  // evaluator.square + relinearize_inplace(he_rk)
    {
        core->square_relinearize(in(vi), this->held(rk_set), out(vo));
    }
    // SEALZpCipher::packed_matMul / packed_affine (SEAL_Cipher.cpp:522-543): vo = M * vi (+ b), M public, with this object's Galois keys
    void packed_matMul(Ciphertext &vo, const matrix &M, const Ciphertext &vi)
    {
        core->packed_affine(M, nullptr, use_bsgs, bsgs_n1, bsgs_n2, in(vi), this->held(gk_set), out(vo));
    }
    void packed_affine(Ciphertext &vo, const matrix &M, const Ciphertext &vi, const vector &b)
    {
        core->packed_affine(M, &b, use_bsgs, bsgs_n1, bsgs_n2, in(vi), this->held(gk_set), out(vo));
    }
    // Hoisted rotations (no reference counterpart: SEAL rotates one step per call): o[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys)
    // with the GaloisKeys object the call names, every rotation from the one set of digit transforms of ct
    void rotate_rows_many(const Ciphertext &ct, const std::vector<int> &steps, const GaloisKeys &gal_keys, std::vector<Ciphertext> &o)
    {
        o.resize(steps.size());
        const uint64_t *x = in(ct);
        core->rotate_rows_many(x, steps, this->galois(gal_keys), outs(o));
    }
    // Chainable packed FC (no reference counterpart: hhe_pktnn_2fc_inference stops after fc1): the analyst's open diagonals as a resident
    // matrix, one open layer, and the FC-square-FC network as one device call, with the key objects the call names
    EncMatrixT<B> enc_matrix_open(const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols)
    {
        return EncMatrixT<B>(*this, diagonals, rows, cols, true);
    }
    void fc_open(const Ciphertext &vi, const EncMatrixT<B> &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &o)
    {
        EncMatrixT<B>::mlp({&mat}, vi, rk, gal_keys, o);
    }
    void mlp(const std::vector<const EncMatrixT<B> *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        EncMatrixT<B>::mlp(layers, vi, rk, gal_keys, vo);
    }
    // Plain-weights FC (no reference counterpart: the reference's rectangular layers multiply by encrypted rows): the open layer under a
    // matrix the CSP holds in the clear, vo = M vi + b in slots [0, rows), as ONE key switch with one mod-down plus the tail rotations
    // (hhe_gfx950.h "Plain-weights sum of rotations").  The matrix is found again by content (MatrixCache): plain_fc_open makes it
    // resident ahead of the first request, fc_open_plain uploads it on first use.  b empty: no bias.  gal_keys: the object the call names;
    // every step of hhe_fc_open_galois_steps needs a key of its own in it
    void plain_fc_open(const matrix &M, const vector &b = vector()) { core->plain_fc_open(M, b.empty() ? nullptr : &b); }
    void fc_open_plain(const Ciphertext &vi, const matrix &M, const vector &b, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        const uint64_t *x = in(vi);
        core->fc_open_plain(M, b.empty() ? nullptr : &b, x, this->galois(gal_keys), out(vo));
    }
    // vo = sum_k rotate_rows(ct, steps[k], gal_keys) * encode(plains[k]), the rounding of the key switch taken once over the sum
    void rotate_plain_sum(const Ciphertext &ct, const matrix &plains, const std::vector<int> &steps, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        const uint64_t *x = in(ct);
        core->rotate_plain_sum(x, plains, steps, this->galois(gal_keys), out(vo));
    }

protected:
    bool use_bsgs;
    size_t bsgs_n1, bsgs_n2;
    // shared with the context's cache and kept alive by this object when the cache evicts them; null for an empty key object.  Declared
    // after the cores (the base): released while their context still exists
    KeySet rk_set, gk_set;
};

// What SEALZpCipher::level(levels_from_last) returns: the evaluation members of a cipher object, bound to one level of the modulus
// switching chain.  The object keeps no keys of its own: it names the key sets of the cipher object it came from, with that object's
// BSGS settings as they were, and the core derives their projections on the device on first use (AdapterCore::derived).
template <class B> class LevelT : public EvalT<B> {
protected:
    using BoundT<B>::device;
    using BoundT<B>::core;
    using BoundT<B>::id;
    using EvalT<B>::in;
    using EvalT<B>::out;
    void same_level(const EncMatrixT<B> &mat) const
    {
        if (mat.core.get() != core.get()) throw std::invalid_argument("encrypted matrix is not at the level of this object");
    }

public:
    using typename EvalT<B>::Ciphertext;
    using typename EvalT<B>::RelinKeys;
    using typename EvalT<B>::GaloisKeys;
    LevelT(std::shared_ptr<typename B::Context> con, size_t levels_from_last, const typename B::SecretKey &sk, KeySet rk, KeySet gk, bool use_bsgs, size_t n1,
           size_t n2)
        : EvalT<B>(BoundT<B>::at_level(std::move(con), levels_from_last), std::move(rk), std::move(gk), use_bsgs, n1, n2)
    {
        const auto s = B::secret(sk);
        if (s.second == device->key_limbs() * device->poly_modulus_degree()) sk_level = device->level_rows(s.first, 1, core->data_limbs());
    }

    // Evaluator::relinearize_inplace(encrypted, relin_keys) and sealhelper::encrypted_vec_sum with the key object the call names
    void relinearize_inplace(Ciphertext &encrypted, const RelinKeys &relin_keys)
    {
        const uint64_t *x = in(encrypted, 3);
        core->relinearize(x, this->relin(relin_keys), out(encrypted));
    }
    void encrypted_vec_sum(const Ciphertext &encrypted_inp, Ciphertext &destination, const GaloisKeys &gal_keys, size_t vec_size)
    {
        const uint64_t *x = in(encrypted_inp);
        core->vec_sum(x, this->galois(gal_keys), vec_size, out(destination));
    }
    // packed encrypted FC at this level: the handle is made on the level's context from diagonals of this level
    EncMatrixT<B> enc_matrix(const std::vector<Ciphertext> &diagonals, size_t rows, size_t cols) { return EncMatrixT<B>(*this, diagonals, rows, cols); }
    void fc_packed(const Ciphertext &vi, const EncMatrixT<B> &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &o)
    {
        same_level(mat);
        mat.apply(vi, rk, gal_keys, o);
    }
    void fc_packed_hoisted(const Ciphertext &vi, const EncMatrixT<B> &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &o)
    {
        same_level(mat);
        mat.apply(vi, rk, gal_keys, o, true);
    }
    void fc_packed_sum(const Ciphertext &vi, const EncMatrixT<B> &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &o, bool hoisted = false)
    {
        same_level(mat);
        mat.apply_sum(vi, rk, gal_keys, o, hoisted);
    }
    // chainable packed FC at this level: one open layer, the FC-square-FC network; matrices of another level are refused
    void fc_open(const Ciphertext &vi, const EncMatrixT<B> &mat, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &o)
    {
        mlp({&mat}, vi, rk, gal_keys, o);
    }
    void mlp(const std::vector<const EncMatrixT<B> *> &layers, const Ciphertext &vi, const RelinKeys &rk, const GaloisKeys &gal_keys, Ciphertext &vo)
    {
        for (const EncMatrixT<B> *m : layers)
            if (m) same_level(*m);
        EncMatrixT<B>::mlp(layers, vi, rk, gal_keys, vo);
    }
    // SEALZpCipher::print_noise / sealhelper::decrypting on the level's context, with the rows of the secret key that level has
    int print_noise(Ciphertext &ciph)
    {
        if (sk_level.empty()) throw std::invalid_argument("invariant_noise_budget: no secret key");
        const size_t size = B::size(ciph);
        if (size < 2) throw std::invalid_argument(NOT_AT_LEVEL);
        const int noise = core->noise_budget({in(ciph, size)}, size, 0, sk_level.data())[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }
    std::vector<int64_t> decrypting(const Ciphertext &enc_input, size_t size)
    {
        const size_t n = device->poly_modulus_degree();
        if (sk_level.empty() || size > n) throw std::invalid_argument("decrypting: ciphertext / secret key do not match the context");
        std::vector<uint64_t> u(n);
        core->decrypt(sk_level.data(), in(enc_input), u.data());
        std::vector<int64_t> o(size);
        for (size_t i = 0; i < size; i++) o[i] = centred(u[i], device->plain_modulus());
        return o;
    }
    AdapterCore &level_core() { return *core; }  // instrumentation (derivations, matrices().uploads())

private:
    std::vector<uint64_t> sk_level;   // [limbs + 1][N]
};

// Decryptor::invariant_noise_budget of ciphertexts at any level (size 2 or 3, a switched-down result at its limbs): one device call
// for ciphertexts of one size and level
template <class B>
std::vector<int> noise_budgets(typename B::Context &ctx, const std::vector<const typename B::Ciphertext *> &cts, const typename B::SecretKey &he_sk)
{
    const auto s = B::secret(he_sk);
    if (s.second != ctx.key_limbs() * ctx.poly_modulus_degree()) throw std::invalid_argument("invariant_noise_budget: no secret key");
    std::vector<AdapterCore::NoiseItem> items;
    for (const typename B::Ciphertext *ct : cts) items.push_back({accepted(B::in_any(ctx, *ct), NOT_VALID), B::size(*ct), B::limbs(*ct)});
    return ctx.noise_budget(items, s.first);
}

// The part of pasta::SEALZpCipher (src/pasta/SEAL_Cipher.h:11-129) and the bodies of pasta::PASTA_SEAL (src/pasta/pasta_3_seal.h:8-54) that
// run on the device.  The derived classes keep the reference's constructors and virtual signatures; this object itself refuses
// ciphertexts below the data level, which the object of their level evaluates (level()).
template <class B> class CipherT : public EvalT<B> {
public:
    using typename EvalT<B>::Ciphertext;
    using typename EvalT<B>::RelinKeys;
    using typename EvalT<B>::GaloisKeys;
    typedef typename B::SecretKey SecretKey;

    // the by-value key members of the reference (SEAL_Cipher.h:28-31) become two device key sets, shared with every other cipher
    // object that was built from the same key objects (BaseCSP::decompose builds one per request, CSP.cpp:238-242)
    CipherT(std::shared_ptr<typename B::Context> con, SecretKey sk, const RelinKeys &rk, const GaloisKeys &gk)
        : EvalT<B>(BoundT<B>::at_top(std::move(con)), nullptr, nullptr), he_sk(std::move(sk))
    {
        rk_set = device->keys().relin(B::words(rk));
        gk_set = device->keys().galois(B::words(gk));
    }

    // SEALZpCipher::get_cipher_size(ct, mod_switch, levels_from_last) (SEAL_Cipher.cpp:363-378): with mod_switch, ct is switched in
    // place (Evaluator::mod_switch_to_inplace) to the level `levels_from_last` steps above last_context_data(), i.e. to
    // 1 + levels_from_last limbs; returns the byte size of the saved object.  Saves here are UNCOMPRESSED (compr_mode_type::none)
    // where the reference's ct.save(s) takes SEAL's default, zstd: the figure is the bound of the reference's.  levels_from_last >= L
    // throws std::invalid_argument (the reference walks off the chain there), and so does a switch to a higher level, as in SEAL.
    size_t get_cipher_size(Ciphertext &ct, bool mod_switch = false, size_t levels_from_last = 0)
    {
        const uint64_t *words = accepted(B::in_any(*device, ct), NOT_VALID);
        if (mod_switch) {
            const size_t size = B::size(ct), target = device->level_limbs(levels_from_last);
            device->mod_switch(words, size, device->limbs_or_data(B::limbs(ct)), target, B::out(*device, B::level_id(*device, levels_from_last), ct, size));
        }
        return device->saved_size(B::size(ct), B::limbs(ct));
    }
    // Evaluation at a level (no reference counterpart: the reference only measures and ships switched ciphertexts).  The object bound to
    // the level `levels_from_last` steps above last_context_data(), the numbering of get_cipher_size.  It evaluates what
    // get_cipher_size(ct, true, levels_from_last) produced, with this object's keys (their projections, derived on the device) and its
    // BSGS settings as they are now.
    LevelT<B> level(size_t levels_from_last) { return LevelT<B>(device, levels_from_last, he_sk, rk_set, gk_set, use_bsgs, bsgs_n1, bsgs_n2); }
    // SEALZpCipher::print_noise (SEAL_Cipher.cpp:71-99): Decryptor::invariant_noise_budget with this object's secret key, on the device
    // (one batched call for the vector; a ciphertext below the data level at its own), the reference's lines on std::cout and its return
    // values.  An empty vector, where the reference reads ciphs[0], and an object without a secret key throw std::invalid_argument
    int print_noise() { return print_noise(secret_key_encrypted); }
    int print_noise(std::vector<Ciphertext> &ciphs)
    {
        if (ciphs.empty()) throw std::invalid_argument("print_noise: no ciphertext");
        std::vector<const Ciphertext *> p;
        for (auto &ct : ciphs) p.push_back(&ct);
        const std::vector<int> budget = noise_budgets<B>(*device, p, he_sk);
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
        const int noise = noise_budgets<B>(*device, {&ciph}, he_sk)[0];
        std::cout << "noise budget: " << noise << std::endl;
        return noise;
    }

    void activate_bsgs(bool activate) { use_bsgs = activate; }
    void set_bsgs_params(uint64_t n1, uint64_t n2) { bsgs_n1 = n1; bsgs_n2 = n2; }
    void add_some_gk_indices(std::vector<int> &gk_ind) { for (int i : gk_ind) gk_indices.push_back(i); }
    void add_bsgs_indices(uint64_t n1, uint64_t n2) { bsgs_indices(device->poly_modulus_degree(), n1, n2, gk_indices); }   // SEAL_Cipher.cpp:337-346
    void add_diagonal_indices(size_t size) { diagonal_indices(device->poly_modulus_degree(), size, gk_indices); }          // :350-355
    const std::vector<int> &get_gk_indices() const { return gk_indices; }

protected:
    using BoundT<B>::device;
    using EvalT<B>::use_bsgs;
    using EvalT<B>::bsgs_n1;
    using EvalT<B>::bsgs_n2;
    using EvalT<B>::rk_set;
    using EvalT<B>::gk_set;
    // PASTA_SEAL::add_gk_indices (pasta_3_seal.cpp:190-201)
    void pasta_gk_indices(size_t plain_size, uint64_t n1, uint64_t n2)
    {
        gk_indices.push_back(0);
        gk_indices.push_back(-1);
        if (plain_size * 2 != device->poly_modulus_degree()) gk_indices.push_back((int)plain_size);
        if (use_bsgs)
            for (uint64_t k = 1; k < n2; k++) gk_indices.push_back(-(int)(k * n1));
    }
    // what HE_decrypt reads (secret_key_encrypted[0], pasta_3_seal.cpp:58)
    const std::vector<Ciphertext> &encrypted_key() const
    {
        if (secret_key_encrypted.empty()) throw std::logic_error("HE_decrypt: encrypted key not set");
        return secret_key_encrypted;
    }
    const uint64_t *key_words(const std::vector<Ciphertext> &enc_ssk, const char *who) const
    {
        if (enc_ssk.empty()) throw std::invalid_argument(std::string(who) + ": enc_ssk is empty");
        return accepted(B::in(*device, this->id, enc_ssk[0], 2), (std::string(who) + ": enc_ssk is not valid for encryption parameters").c_str());
    }
    // PASTA_SEAL::decomposition (pasta_3_seal.cpp:106-172): every 128-word block of the record on the device, one batched call; the
    // record was encrypted under `nonce` (block b under the pair (nonce, b)), by default the reference's fixed one
    std::vector<Ciphertext> transcipher(const std::vector<uint64_t> &record, const std::vector<Ciphertext> &enc_ssk, uint64_t nonce = AdapterCore::fixed_nonce)
    {
        const uint64_t *key = key_words(enc_ssk, "decomposition");   // state <- enc_ssk[0] (:126); uploaded when its contents change
        std::vector<Ciphertext> res(AdapterCore::blocks_of(record.size()));
        device->transcipher(record, key, rk_set, gk_set, use_bsgs, this->outs(res), nonce);
        return res;
    }
    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call: decomposition of every record, the mask of the
    // ragged last block and flatten with the GaloisKeys object `flatten_gk` -- the blocks never leave HBM.  One flattened ciphertext per
    // record.  nonces: null = the reference's fixed nonce, else one per record
    std::vector<Ciphertext> decompose_records(const std::vector<std::vector<uint64_t>> &records, const std::vector<Ciphertext> &enc_ssk,
                                              const GaloisKeys &flatten_gk, bool mask_last, const std::vector<uint64_t> *nonces = nullptr)
    {
        std::vector<Ciphertext> res(records.size());
        if (records.empty()) return res;
        const uint64_t *key = key_words(enc_ssk, "decompose");
        if (nonces && nonces->size() != records.size()) throw std::invalid_argument("decompose: one nonce per record");
        device->decompose(records, key, rk_set, gk_set, B::words(flatten_gk), mask_last, this->outs(res), nonces ? *nonces : std::vector<uint64_t>());
        return res;
    }

    SecretKey he_sk;
    std::vector<Ciphertext> secret_key_encrypted;
    std::vector<int> gk_indices;
};

// The sealhelper free functions that name a context: CSP_hhe_pktnn_1fc::evaluateModel's three calls (sealhelper.cpp:268-274, 379-392;
// CSP.cpp:296-316), each with the key object the call names, the same three for one weight row as ONE device call, and hoisted rotations
template <class B> struct FreeT {
    typedef typename B::Context Context;
    typedef typename B::Ciphertext Ciphertext;
    static const uint64_t *in(const Context &ctx, const Ciphertext &ct, size_t size = 2) { return accepted(B::in(ctx, B::top(ctx), ct, size), NOT_VALID); }
    static auto out(const Context &ctx, Ciphertext &ct, size_t size = 2) { return B::out(ctx, B::top(ctx), ct, size); }

    static void packed_enc_multiply(Context &ctx, const Ciphertext &encrypted1, const Ciphertext &encrypted2, Ciphertext &destination)
    {
        ctx.multiply(in(ctx, encrypted1), in(ctx, encrypted2), out(ctx, destination, 3));
    }
    static void relinearize_inplace(Context &ctx, Ciphertext &encrypted, const typename B::RelinKeys &relin_keys)
    {
        ctx.relinearize(in(ctx, encrypted, 3), B::words(relin_keys), out(ctx, encrypted));
    }
    static void encrypted_vec_sum(Context &ctx, const Ciphertext &encrypted_inp, Ciphertext &destination, const typename B::GaloisKeys &gal_keys, size_t vec_size)
    {
        ctx.vec_sum(in(ctx, encrypted_inp), B::words(gal_keys), vec_size, out(ctx, destination));
    }
    // identical ciphertext words to the three calls above
    static void fc_row(Context &ctx, const Ciphertext &vi, const Ciphertext &w_row, const typename B::RelinKeys &csp_rk, const typename B::GaloisKeys &gal_keys,
                       size_t vec_size, Ciphertext &destination)
    {
        ctx.fc_row(in(ctx, vi), in(ctx, w_row), B::words(csp_rk), B::words(gal_keys), vec_size, out(ctx, destination));
    }
    // o[k] = Evaluator::rotate_rows(ct, steps[k], gal_keys), hoisted (hhe_gfx950.h "Hoisted rotations")
    static void rotate_rows_many(Context &ctx, const Ciphertext &ct, const std::vector<int> &steps, const typename B::GaloisKeys &gal_keys, std::vector<Ciphertext> &o)
    {
        o.resize(steps.size());
        ctx.rotate_rows_many(in(ctx, ct), steps, B::words(gal_keys), [&](size_t i) { return out(ctx, o[i])(0); });
    }
    // the open FC layer under plain weights and the primitive under it (hhe_gfx950.h "Plain-weights sum of rotations"); b empty: no bias
    static void fc_open_plain(Context &ctx, const Ciphertext &vi, const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> &b,
                              const typename B::GaloisKeys &gal_keys, Ciphertext &vo)
    {
        ctx.fc_open_plain(M, b.empty() ? nullptr : &b, in(ctx, vi), B::words(gal_keys), out(ctx, vo));
    }
    static void rotate_plain_sum(Context &ctx, const Ciphertext &ct, const std::vector<std::vector<uint64_t>> &plains, const std::vector<int> &steps,
                                 const typename B::GaloisKeys &gal_keys, Ciphertext &vo)
    {
        ctx.rotate_plain_sum(in(ctx, ct), plains, steps, B::words(gal_keys), out(ctx, vo));
    }
};

}  // namespace hhe
