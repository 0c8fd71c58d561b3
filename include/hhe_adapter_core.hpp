// hhe_adapter_core.hpp -- everything the two C++ adapters do that is not type conversion, once, on plain words, over the C ABI of
// libhhe_gfx950.so.  pasta_seal_gfx950.hpp (word containers; executed by the tests) and pasta_seal_gfx950_seal.hpp (seal:: types;
// type-checked only) derive their context class from hhe::AdapterCore and turn their boundary types into `const uint64_t *` and
// output sinks; which buffers, which lock, which key set and which order of C-ABI calls is decided here and nowhere else.
//   KeySetCache  maps every RelinKeys / GaloisKeys OBJECT the caller passes to one device key set (hhe_keyset), recognised by a
//                hash over ALL of its words.  The reference copies its key objects by value into every cipher object and every
//                call (SEAL_Cipher.cpp:9-36, CSP.cpp:238-242), so pointers say nothing; contents do.  An object is uploaded
//                once and stays resident with everything derived from it; beyond `max_sets` (a CSP that serves many analysts) the
//                cache lets go of the least recently used sets.
//   MatrixCache  maps every public matrix (+ bias, + method) a packed affine layer is called with to one device handle (hhe_matrix), by
//                the same kind of content hash: a CSP that applies the same layer per request uploads it once.
//   DeviceArena  grow-only device buffers reused across calls instead of a hipMalloc / hipFree pair per call.
//   AdapterCore  the hhe_ctx, its cache, its arena, the resident encrypted PASTA key and the call bodies; and, per level of its
//                chain that is evaluated at, one further core (level()) whose key sets are derived on the device from this one's.
//
// Ownership and threading, stated once:
//   * A key set is a std::shared_ptr (KeySet).  The cache holds one reference, every cipher object holds one for each key member
//     it was built with, every call holds one for each key object it names.  Eviction drops the cache's reference only: a set is
//     destroyed when its last holder lets go, never under a call or a live cipher object.  Holders declare their KeySet members
//     after their context member, so a set dies before its context.
//   * An empty key object gives a null KeySet.  A cipher object's method then runs with the context's one empty set (and reports
//     the missing key as SEAL would) instead of falling through to the library's default set; a free function that names a key
//     object throws at once.
//   * Every method that touches the arena takes the arena's lock for its whole duration, and looks up the key sets it names under
//     that lock.  Lock order: arena, then cache, then the library's own per-context lock.  The methods on RAII buffers (multiply,
//     add, square_relinearize, relinearize, vec_sum, pasta_crypt, decrypt) take no adapter lock; their key sets are kept alive by
//     the reference the call holds.
//   * Results leave through a sink `uint64_t *dst(size_t item)`: the host destination of item i, asked for after every input has
//     been uploaded (so a destination may alias an input) and written straight from the device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "hhe_gfx950.h"

namespace hhe {

inline void check(int rc)  // return code -> the exception the reference / SEAL throw
{
    if (rc == HHE_OK) return;
    const std::string msg = hhe_last_error();
    switch (rc) {
    case HHE_ERR_NO_GALOIS_KEY:
    case HHE_ERR_NO_RELIN_KEY:
    case HHE_ERR_INVALID: throw std::invalid_argument(msg);  // what SEAL throws for these
    default: throw std::runtime_error(msg);                  // incl. HHE_ERR_TOO_FEW_SLOTS (pasta_3_seal.cpp:376-377)
    }
}

struct DevBuf {  // RAII device buffer
    void *p = nullptr;
    explicit DevBuf(size_t bytes) : p(hhe_malloc(bytes)) { if (!p) throw std::runtime_error("hhe_malloc failed"); }
    ~DevBuf() { hhe_free(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    uint64_t *u64() const { return static_cast<uint64_t *>(p); }
};

// 128 bits over every word (two independent multiply-xorshift lanes) plus the length: a 4-word sample cannot tell two key
// objects of one key generator apart reliably, the whole content can
struct ContentHash {
    uint64_t a = 0x243F6A8885A308D3ULL, b = 0x13198A2E03707344ULL, n = 0;
    void add(const uint64_t *w, size_t count)
    {
        for (size_t i = 0; i < count; i++) {
            a = (a ^ w[i]) * 0x9E3779B97F4A7C15ULL; a ^= a >> 29;
            b = (b + w[i]) * 0xC2B2AE3D27D4EB4FULL; b ^= b >> 31;
        }
        n += count;
    }
    void add_tag(uint64_t t) { add(&t, 1); }
    bool operator<(const ContentHash &o) const { return a != o.a ? a < o.a : b != o.b ? b < o.b : n < o.n; }
    bool operator!=(const ContentHash &o) const { return *this < o || o < *this; }
};

typedef std::shared_ptr<hhe_keyset> KeySet;
// The words of one key object as its adapter holds them; an object without keys is "empty".
// `own`: backing store of an adapter whose key objects are not contiguous in memory.
struct RelinWords {  // RelinKeys::key(2): [L digits][2][K][N], NTT form
    const uint64_t *key = nullptr;
    size_t words = 0;
    std::vector<uint64_t> own;
};
struct GaloisWords {
    std::vector<std::pair<uint32_t, const uint64_t *>> keys;  // (Galois element, its [L][2][K][N] words)
    size_t words = 0;                                         // per key
    std::vector<std::vector<uint64_t>> own;
};

class KeySetCache {
public:
    explicit KeySetCache(hhe_ctx *ctx, size_t max_sets = 16) : ctx_(ctx), max_sets_(max_sets) {}
    KeySet galois(const GaloisWords &g)
    {
        if (g.keys.empty()) return nullptr;
        ContentHash h;
        h.add_tag(0x6b67);  // "gk"
        for (auto &kv : g.keys) { h.add_tag(kv.first); h.add(kv.second, g.words); }
        return lookup(h, [&](hhe_keyset *ks) {
            for (auto &kv : g.keys)
                if (int rc = hhe_keyset_set_galois(ks, kv.first, kv.second)) return rc;
            return (int)HHE_OK;
        });
    }
    KeySet relin(const RelinWords &r)
    {
        if (!r.words) return nullptr;
        ContentHash h;
        h.add_tag(0x726b);  // "rk"
        h.add(r.key, r.words);
        return lookup(h, [&](hhe_keyset *ks) { return hhe_keyset_set_relin(ks, r.key); });
    }
    KeySet new_set() const  // a set without keys, not cached
    {
        hhe_keyset *ks = nullptr;
        check(hhe_keyset_create(ctx_, &ks));
        return KeySet(ks, hhe_keyset_destroy);
    }
    size_t resident() const { return lru_.size(); }
    uint64_t uploads() const { return uploads_; }   // how many objects were sent to the device (a repeated object is not)

private:
    template <typename F> KeySet lookup(const ContentHash &h, F &&fill)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = index_.find(h);
        if (it != index_.end()) {
            lru_.splice(lru_.begin(), lru_, it->second);  // most recently used first
            return it->second->second;
        }
        KeySet ks = new_set();
        check(fill(ks.get()));
        ++uploads_;
        lru_.emplace_front(h, ks);
        index_[h] = lru_.begin();
        while (lru_.size() > max_sets_) {  // the cache's reference goes; whoever still holds the set keeps it alive
            index_.erase(lru_.back().first);
            lru_.pop_back();
        }
        return ks;
    }
    hhe_ctx *ctx_;
    size_t max_sets_;
    std::mutex mu_;
    std::list<std::pair<ContentHash, KeySet>> lru_;
    std::map<ContentHash, std::list<std::pair<ContentHash, KeySet>>::iterator> index_;
    uint64_t uploads_ = 0;
};

// add_diagonal_indices / add_bsgs_indices (SEAL_Cipher.cpp:337-355): the rotation steps of a packed affine layer, appended
inline void diagonal_indices(size_t slot_count, size_t size, std::vector<int> &gk_indices)
{
    if (size * 2 != slot_count) gk_indices.push_back(-((int)size));
    gk_indices.push_back(1);
}
inline void bsgs_indices(size_t slot_count, uint64_t n1, uint64_t n2, std::vector<int> &gk_indices)
{
    diagonal_indices(slot_count, n1 * n2, gk_indices);
    if (n1 == 1 || n2 == 1) return;
    for (uint64_t k = 1; k < n2; k++) gk_indices.push_back((int)(k * n1));
}

// Public matrices of packed affine layers by content: (dim, n1, n2, every word of the matrix and of the bias).  Shared ownership
// like KeySetCache: eviction beyond `max_matrices` drops the cache's reference, a call that still computes with a handle keeps it.
typedef std::shared_ptr<hhe_matrix> Matrix;
// ... and the plain matrices of the open FC layer under plain weights (hhe_plain_fc: rows x cols, + bias) and the plaintext rows of
// rotate_plain_sum (hhe_plain_rows), found again the same way: three kinds of handle, one capacity each, one upload count
typedef std::shared_ptr<hhe_plain_fc> PlainFc;
typedef std::shared_ptr<hhe_plain_rows> PlainRows;
class MatrixCache {
    template <class T> struct Kind {
        std::list<std::pair<ContentHash, std::shared_ptr<T>>> lru;
        std::map<ContentHash, typename std::list<std::pair<ContentHash, std::shared_ptr<T>>>::iterator> index;
    };
    // caller holds mu_.  make() creates the handle on a miss
    template <class T, class Make> std::shared_ptr<T> lookup(Kind<T> &k, const ContentHash &h, Make make)
    {
        auto it = k.index.find(h);
        if (it != k.index.end()) {
            k.lru.splice(k.lru.begin(), k.lru, it->second);
            return it->second->second;
        }
        std::shared_ptr<T> m = make();
        ++uploads_;
        k.lru.emplace_front(h, m);
        k.index[h] = k.lru.begin();
        while (k.lru.size() > max_) {
            k.index.erase(k.lru.back().first);
            k.lru.pop_back();
        }
        return m;
    }

public:
    explicit MatrixCache(hhe_ctx *ctx, size_t max_matrices = 8) : ctx_(ctx), max_(max_matrices) {}
    // M: row-major dim x dim; bias: dim words or null; n1 = n2 = 0: diagonal method
    Matrix get(const uint64_t *M, size_t dim, const uint64_t *bias, size_t n1, size_t n2)
    {
        ContentHash h;
        h.add_tag(0x6d61);  // "ma"
        h.add_tag(dim); h.add_tag(n1); h.add_tag(n2);
        h.add(M, dim * dim);
        h.add_tag(bias ? 1 : 0);
        if (bias) h.add(bias, dim);
        std::lock_guard<std::mutex> lk(mu_);
        return lookup(mats_, h, [&] {
            hhe_matrix *raw = nullptr;
            check(hhe_matrix_create(ctx_, M, dim, bias, n1, n2, &raw));
            return Matrix(raw, hhe_matrix_destroy);
        });
    }
    // M: row-major rows x cols; bias: rows words or null (hhe_plain_fc_create_open)
    PlainFc get_open(const uint64_t *M, size_t rows, size_t cols, const uint64_t *bias)
    {
        ContentHash h;
        h.add_tag(0x7066);  // "pf"
        h.add_tag(rows); h.add_tag(cols);
        h.add(M, rows * cols);
        h.add_tag(bias ? 1 : 0);
        if (bias) h.add(bias, rows);
        std::lock_guard<std::mutex> lk(mu_);
        return lookup(open_, h, [&] {
            hhe_plain_fc *raw = nullptr;
            check(hhe_plain_fc_create_open(ctx_, M, rows, cols, bias, &raw));
            return PlainFc(raw, hhe_plain_fc_destroy);
        });
    }
    // vals: n plaintexts of `count` slot values each (hhe_plain_rows_create)
    PlainRows get_rows(const uint64_t *vals, size_t n, size_t count)
    {
        ContentHash h;
        h.add_tag(0x7072);  // "pr"
        h.add_tag(n); h.add_tag(count);
        h.add(vals, n * count);
        std::lock_guard<std::mutex> lk(mu_);
        return lookup(rows_, h, [&] {
            hhe_plain_rows *raw = nullptr;
            check(hhe_plain_rows_create(ctx_, vals, n, count, &raw));
            return PlainRows(raw, hhe_plain_rows_destroy);
        });
    }
    size_t resident() const { return mats_.lru.size() + open_.lru.size() + rows_.lru.size(); }
    uint64_t uploads() const { return uploads_; }   // how many matrices were sent to the device (a repeated one is not)

private:
    hhe_ctx *ctx_;
    size_t max_;
    std::mutex mu_;
    Kind<hhe_matrix> mats_;
    Kind<hhe_plain_fc> open_;
    Kind<hhe_plain_rows> rows_;
    uint64_t uploads_ = 0;
};

// The encrypted weight matrix of a packed encrypted FC layer as a resident handle (hhe_enc_matrix): shared ownership with
// hhe_enc_matrix_destroy as deleter, as for key sets.  Whoever holds one also holds the core it was made on (the handle names its context).
typedef std::shared_ptr<hhe_enc_matrix> EncMatrix;

// A few grow-only device buffers ("slots"); a call takes the arena's lock for its duration (the library serialises calls on one
// context anyway) and gets buffers that survive the call.
class DeviceArena {
public:
    static constexpr int SLOTS = 6;
    ~DeviceArena() { for (auto &s : buf_) hhe_free(s.first); }
    std::mutex &mutex() { return mu_; }
    uint64_t *get(int slot, size_t bytes)  // caller holds mutex()
    {
        auto &s = buf_[slot];
        if (s.second < bytes) {
            hhe_free(s.first);
            s.first = hhe_malloc(bytes);
            s.second = s.first ? bytes : 0;
            if (!s.first) throw std::runtime_error("hhe_malloc failed");
        }
        return static_cast<uint64_t *>(s.first);
    }
private:
    std::mutex mu_;
    std::pair<void *, size_t> buf_[SLOTS] = {};
};

class AdapterCore {
public:
    // q: coeff_modulus incl. the special prime; max_sets / max_matrices: capacities of the key-set and the matrix cache
    AdapterCore(int logn, const std::vector<uint64_t> &q, uint64_t t, int device = 0, size_t max_sets = 16, size_t max_matrices = 8)
        : n_((size_t)1 << logn), L_(q.size() - 1), t_(t), max_sets_(max_sets), max_matrices_(max_matrices),
          h_(create(logn, q, t, device), hhe_ctx_destroy), keys_(h_.get(), max_sets), empty_(keys_.new_set()), mats_(h_.get(), max_matrices) {}

    size_t poly_modulus_degree() const { return n_; }
    size_t data_limbs() const { return L_; }
    size_t ct_words(size_t size = 2) const { return size * L_ * n_; }
    uint64_t plain_modulus() const { return t_; }
    KeySetCache &keys() { return keys_; }
    MatrixCache &matrices() { return mats_; }
    uint64_t key_uploads = 0;  // instrumentation: how often an encrypted PASTA key was sent to the device

    // SEALZpCipher::mask (SEAL_Cipher.cpp:161-166)
    template <class Sink> void mask(const uint64_t *ct, const uint64_t *vals, size_t count, Sink dst)
    {
        std::lock_guard<std::mutex> lk(arena_.mutex());
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, ct);
        check(hhe_mask(h(), d, vals, count, d, 1));
        download(d, 1, 2, dst);
    }
    // SEALZpCipher::flatten (SEAL_Cipher.cpp:170-181): out = sum_i rotate_rows(in[i], -i * plain_size, gk).  GK: a held KeySet or
    // the GaloisWords of the object the call names
    template <class GK, class Sink> void flatten(const std::vector<const uint64_t *> &in, const GK &gk, Sink dst)
    {
        if (in.empty()) throw std::invalid_argument("flatten: empty input");
        const size_t w = ct_words();
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet g = or_empty(set(gk));
        uint64_t *d = arena_.get(0, in.size() * w * 8), *o = arena_.get(1, w * 8);
        for (size_t i = 0; i < in.size(); i++) upload(d + i * w, in[i]);
        check(hhe_flatten_ks(h(), g.get(), d, in.size(), o, 1));
        download(o, 1, 2, dst);
    }

    // SEALZpCipher::packed_matMul / packed_affine (SEAL_Cipher.cpp:522-543): vo = M * vi (+ b) with the public matrix M, by
    // babystep-giantstep when use_bsgs && n1 != 1 && n2 != 1, else by the diagonal method; bias: null for packed_matMul.  The rotations
    // use the Galois keys the cipher object holds (he_gk).  The reference only warns when n1 * n2 != dim; here that is invalid_argument.
    template <class Sink>
    void packed_affine(const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> *bias, bool use_bsgs, size_t n1, size_t n2,
                       const uint64_t *ct, const KeySet &gk, Sink dst)
    {
        const size_t dim = M.size();
        if (!dim) throw std::invalid_argument("packed_matMul: empty matrix");
        if (bias && bias->size() != dim) throw std::invalid_argument("packed_affine: bias and matrix dimensions differ");
        std::vector<uint64_t> flat(dim * dim);
        for (size_t r = 0; r < dim; r++) {
            if (M[r].size() != dim) throw std::invalid_argument("packed_matMul: matrix is not square");
            std::copy(M[r].begin(), M[r].end(), flat.begin() + r * dim);
        }
        const bool bsgs = use_bsgs && n1 != 1 && n2 != 1;
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const Matrix m = mats_.get(flat.data(), dim, bias ? bias->data() : nullptr, bsgs ? n1 : 0, bsgs ? n2 : 0);
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, ct);
        check(hhe_packed_affine_ks(h(), or_empty(gk).get(), m.get(), d, d, 1));
        download(d, 1, 2, dst);
    }

    // Evaluator::multiply -> size 3; add of two size-`size` ciphertexts; square + relinearize_inplace(rk); relinearize_inplace(rk)
    template <class Sink> void multiply(const uint64_t *e1, const uint64_t *e2, Sink dst)
    {
        DevBuf a(ct_words() * 8), b(ct_words() * 8), o3(ct_words(3) * 8);
        upload(a.u64(), e1);
        upload(b.u64(), e2);
        check(hhe_multiply(h(), a.u64(), b.u64(), o3.u64(), 1));
        download(o3.u64(), 1, 3, dst);
    }
    template <class Sink> void add(const uint64_t *e1, const uint64_t *e2, size_t size, Sink dst)
    {
        DevBuf a(ct_words(size) * 8), b(ct_words(size) * 8);
        upload(a.u64(), e1, size);
        upload(b.u64(), e2, size);
        check(hhe_add(h(), a.u64(), b.u64(), a.u64(), 1, (int)size));
        download(a.u64(), 1, size, dst);
    }
    template <class Sink> void square_relinearize(const uint64_t *vi, const KeySet &rk, Sink dst)
    {
        DevBuf a(ct_words() * 8), o3(ct_words(3) * 8);
        upload(a.u64(), vi);
        check(hhe_square(h(), a.u64(), o3.u64(), 1));  // the words of hhe_multiply(a, a): one operand extension, the squaring kernel
        check(hhe_relinearize_ks(h(), or_empty(rk).get(), o3.u64(), a.u64(), 1));
        download(a.u64(), 1, 2, dst);
    }
    // RK: the RelinWords of the object the call names, or a held KeySet
    template <class RK, class Sink> void relinearize(const uint64_t *e3, const RK &rk, Sink dst)  // CSP.cpp:306
    {
        const KeySet r = named(set(rk), "relin_keys is not valid for encryption parameters");
        DevBuf a3(ct_words(3) * 8), o(ct_words() * 8);
        upload(a3.u64(), e3, 3);
        check(hhe_relinearize_ks(h(), r.get(), a3.u64(), o.u64(), 1));
        download(o.u64(), 1, 2, dst);
    }

    // PASTA_SEAL::decomposition (pasta_3_seal.cpp:106-172): every 128-word block of the record, one batched call; item b of the
    // sink is block b of blocks_of(record.size()).  enc_key: enc_ssk[0], ct_words() words.
    // nonce: the one the record was encrypted under (a (nonce, counter) pair encrypts one block, ever: hhe_gfx950.h "PASTA under a
    // caller's nonce"); the default is the reference's fixed one (:115)
    static constexpr uint64_t fixed_nonce = 123456789;
    static size_t blocks_of(size_t words) { return (words + 127) / 128; }
    template <class Sink>
    void transcipher(const std::vector<uint64_t> &record, const uint64_t *enc_key, const KeySet &rk, const KeySet &gk, bool bsgs, Sink dst,
                     uint64_t nonce = fixed_nonce)
    {
        const size_t nb = blocks_of(record.size());
        if (nb == 0) return;
        std::vector<uint64_t> cw(nb * 128, 0), bidx(nb);
        std::vector<uint32_t> ncw(nb);
        std::copy(record.begin(), record.end(), cw.begin());  // blocks are contiguous; the ragged last one is zero-padded
        for (size_t b = 0; b < nb; b++) {
            ncw[b] = (uint32_t)std::min<size_t>(128, record.size() - b * 128);
            bidx[b] = b;  // pasta.init_shake(nonce, b) (:122)
        }
        std::lock_guard<std::mutex> lk(arena_.mutex());
        uint64_t *key = encrypted_key(enc_key), *out = arena_.get(3, nb * ct_words() * 8);
        if (nonce == fixed_nonce)
            check(hhe_pasta3_transcipher_ks(h(), or_empty(rk).get(), or_empty(gk).get(), key, cw.data(), ncw.data(), bidx.data(), nb, bsgs ? 1 : 0, out));
        else {
            const std::vector<uint64_t> nonces(nb, nonce);
            check(hhe_pasta3_transcipher_nonce_ks(h(), or_empty(rk).get(), or_empty(gk).get(), key, cw.data(), ncw.data(), nonces.data(), bidx.data(), nb,
                                                  bsgs ? 1 : 0, out));
        }
        download(out, nb, 2, dst);
    }
    // BaseCSP::decompose's per-record loop (CSP.cpp:247-278) as ONE device call: decomposition of every record, the mask of the
    // ragged last block (mask_last) and flatten with `flatten_gk`; item s of the sink is record s.  nonces: empty = the reference's
    // fixed nonce for every record, else one per record
    template <class Sink>
    void decompose(const std::vector<std::vector<uint64_t>> &records, const uint64_t *enc_key, const KeySet &rk, const KeySet &gk,
                   const GaloisWords &flatten_gk, bool mask_last, Sink dst, const std::vector<uint64_t> &nonces = {})
    {
        if (records.empty()) return;
        if (!nonces.empty() && nonces.size() != records.size()) throw std::invalid_argument("decompose: one nonce per record");
        const size_t nwords = records[0].size();
        std::vector<uint64_t> flat(records.size() * nwords);
        for (size_t s = 0; s < records.size(); s++) {
            if (records[s].size() != nwords) throw std::invalid_argument("decompose: records of different lengths");
            std::copy(records[s].begin(), records[s].end(), flat.begin() + s * nwords);
        }
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet fgk = or_empty(keys_.galois(flatten_gk));
        uint64_t *key = encrypted_key(enc_key), *out = arena_.get(3, records.size() * ct_words() * 8);
        if (nonces.empty())
            check(hhe_decompose_ks(h(), or_empty(rk).get(), or_empty(gk).get(), fgk.get(), key, flat.data(), records.size(), nwords, mask_last ? 1 : 0, out));
        else
            check(hhe_decompose_nonce_ks(h(), or_empty(rk).get(), or_empty(gk).get(), fgk.get(), key, flat.data(), nonces.data(), records.size(), nwords,
                                         mask_last ? 1 : 0, out));
        download(out, records.size(), 2, dst);
    }

    // sealhelper::encrypted_vec_sum (sealhelper.cpp:385-391), literally:
    // destination = in; for i = -1 .. -(vec_size-1): destination += rotate_rows(in, i, gk)
    template <class GK, class Sink> void vec_sum(const uint64_t *in_words, const GK &gk, size_t vec_size, Sink dst)
    {
        const KeySet g = named(set(gk), "Galois key not present");
        const size_t w = ct_words();
        DevBuf in(w * 8), acc(w * 8), rot(w * 8);
        upload(in.u64(), in_words);
        check(hhe_rotate_rows_ks(h(), g.get(), in.u64(), 0, acc.u64(), 1));  // step 0: a copy, as in SEAL
        for (size_t i = 1; i < vec_size; i++) {
            check(hhe_rotate_rows_ks(h(), g.get(), in.u64(), -(int)i, rot.u64(), 1));
            check(hhe_add(h(), acc.u64(), rot.u64(), acc.u64(), 1, 2));
        }
        download(acc.u64(), 1, 2, dst);
    }
    // packed_enc_multiply + relinearize_inplace(.., rk) + encrypted_vec_sum(.., gk, vec_size) for one weight row (CSP.cpp:296-316)
    // as ONE device call: NAF-trie rotation sum, identical ciphertext words
    template <class Sink>
    void fc_row(const uint64_t *vi, const uint64_t *w_row, const RelinWords &rk, const GaloisWords &gk, size_t vec_size, Sink dst)
    {
        const size_t w = ct_words();
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet r = named(keys_.relin(rk), "fc_row: empty key object"), g = named(keys_.galois(gk), "fc_row: empty key object");
        uint64_t *a = arena_.get(0, w * 8), *b = arena_.get(1, w * 8), *o = arena_.get(3, w * 8);
        upload(a, vi);
        upload(b, w_row);
        check(hhe_fc_row_ks(h(), r.get(), g.get(), a, b, 1, vec_size, o, 1));
        download(o, 1, 2, dst);
    }

    // ---- packed encrypted FC (hhe_gfx950.h "packed encrypted FC"): all rows of the layer in one ciphertext, in place of one fc_row per
    // neuron.  diagonals: the r = fc_packed_shape().first encryptions of the generalized diagonals, ct_words() words each; they are
    // extended and transformed once, here, and are not needed afterwards.
    std::pair<size_t, size_t> fc_packed_shape(size_t rows, size_t cols) const
    {
        size_t r = 0, c = 0;
        check(hhe_fc_packed_shape(n_, rows, cols, &r, &c));
        return {r, c};
    }
    EncMatrix enc_matrix(const std::vector<const uint64_t *> &diagonals, size_t rows, size_t cols)
    {
        if (diagonals.size() != fc_packed_shape(rows, cols).first) throw std::invalid_argument("enc_matrix: one ciphertext per generalized diagonal");
        DevBuf d(diagonals.size() * ct_words() * 8);
        for (size_t i = 0; i < diagonals.size(); i++) upload(d.u64() + i * ct_words(), diagonals[i]);
        hhe_enc_matrix *raw = nullptr;
        check(hhe_enc_matrix_create(h(), d.u64(), rows, cols, &raw));
        return EncMatrix(raw, hhe_enc_matrix_destroy);
    }
    // the layer on one ciphertext: slots [0, rows) of the result are (M x) mod t.  RK / GK: the key objects the call names (their
    // words, or a held KeySet)
    template <class RK, class GK, class Sink> void fc_packed(const uint64_t *vi, const EncMatrix &m, const RK &rk, const GK &gk, Sink dst)
    {
        if (!m) throw std::invalid_argument("fc_packed: no encrypted matrix");
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet r = named(set(rk), "fc_packed: empty key object"), g = named(set(gk), "fc_packed: empty key object");
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, vi);
        check(hhe_fc_packed_ks(h(), r.get(), g.get(), m.get(), d, d, 1));
        download(d, 1, 2, dst);
    }

    // ... with its rotation chain hoisted (hhe_fc_packed_hoisted_ks): rot_i = rotate_rows(x, i, gk); same slots, other words
    template <class RK, class GK, class Sink> void fc_packed_hoisted(const uint64_t *vi, const EncMatrix &m, const RK &rk, const GK &gk, Sink dst)
    {
        if (!m) throw std::invalid_argument("fc_packed: no encrypted matrix");
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet r = named(set(rk), "fc_packed: empty key object"), g = named(set(gk), "fc_packed: empty key object");
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, vi);
        check(hhe_fc_packed_hoisted_ks(h(), r.get(), g.get(), m.get(), d, d, 1));
        download(d, 1, 2, dst);
    }
    // ... with ONE BEHZ floor over the sum of the r products (hhe_fc_packed_sum_ks); hoisted: the rotations of fc_packed_hoisted instead
    // of fc_packed's chain; same slots, other words.  More diagonals than one floor takes ("behz_sum_cap") are refused by the device call.
    template <class RK, class GK, class Sink>
    void fc_packed_sum(const uint64_t *vi, const EncMatrix &m, const RK &rk, const GK &gk, Sink dst, bool hoisted = false)
    {
        if (!m) throw std::invalid_argument("fc_packed: no encrypted matrix");
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet r = named(set(rk), "fc_packed: empty key object"), g = named(set(gk), "fc_packed: empty key object");
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, vi);
        check(hhe_fc_packed_sum_ks(h(), r.get(), g.get(), m.get(), d, d, 1, hoisted ? 1 : 0));
        download(d, 1, 2, dst);
    }
    // ---- chainable packed FC (hhe_gfx950.h "Chainable packed FC"): the diagonals that do not wrap.  An open handle takes fc_open and mlp,
    // a cyclic one the three forms above; the device calls refuse the other kind.
    std::pair<size_t, size_t> fc_open_shape(size_t rows, size_t cols) const
    {
        size_t r = 0, c = 0;
        check(hhe_fc_open_shape(n_, rows, cols, &r, &c));
        return {r, c};
    }
    EncMatrix enc_matrix_open(const std::vector<const uint64_t *> &diagonals, size_t rows, size_t cols)
    {
        if (diagonals.size() != fc_open_shape(rows, cols).first) throw std::invalid_argument("enc_matrix_open: one ciphertext per open diagonal");
        DevBuf d(diagonals.size() * ct_words() * 8);
        for (size_t i = 0; i < diagonals.size(); i++) upload(d.u64() + i * ct_words(), diagonals[i]);
        hhe_enc_matrix *raw = nullptr;
        check(hhe_enc_matrix_create_open(h(), d.u64(), rows, cols, &raw));
        return EncMatrix(raw, hhe_enc_matrix_destroy);
    }
    // the network on one ciphertext: layers[0] open, square + relinearize, layers[1] open, ...; one layer is fc_open.  No slot of the input
    // outside [0, cols) of the first layer needs to be zero
    template <class RK, class GK, class Sink> void mlp(const uint64_t *vi, const std::vector<EncMatrix> &layers, const RK &rk, const GK &gk, Sink dst)
    {
        std::vector<const hhe_enc_matrix *> raw;
        for (const EncMatrix &m : layers) {
            if (!m) throw std::invalid_argument("mlp: no encrypted matrix");
            raw.push_back(m.get());
        }
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet r = named(set(rk), "mlp: empty key object"), g = named(set(gk), "mlp: empty key object");
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, vi);
        check(hhe_mlp_ks(h(), r.get(), g.get(), raw.data(), raw.size(), d, d, 1));
        download(d, 1, 2, dst);
    }
    template <class RK, class GK, class Sink> void fc_open(const uint64_t *vi, const EncMatrix &m, const RK &rk, const GK &gk, Sink dst)
    {
        mlp(vi, std::vector<EncMatrix>{m}, rk, gk, dst);
    }
    // Hoisted rotations (hhe_rotate_rows_many_ks): item k of dst = Evaluator::rotate_rows(in, steps[k], gk), the digit transforms of `in`
    // (and of every node of the steps' NAF trie) computed once.  An empty step list is refused by the device call.
    template <class GK, class Sink> void rotate_rows_many(const uint64_t *in_words, const std::vector<int> &steps, const GK &gk, Sink dst)
    {
        const KeySet g = named(set(gk), "Galois key not present");
        const size_t w = ct_words();
        DevBuf in(w * 8), out((steps.empty() ? 1 : steps.size()) * w * 8);
        upload(in.u64(), in_words);
        check(hhe_rotate_rows_many_ks(h(), g.get(), in.u64(), steps.data(), steps.size(), out.u64(), 1));
        download(out.u64(), steps.size(), 2, dst);
    }

    // ---- plain-weights FC (hhe_gfx950.h "Plain-weights sum of rotations"): a rows x cols matrix the CSP holds in the clear, in the open
    // layout; the handle is found again through the matrix cache, so a CSP that applies the same layer per request uploads it once
    static std::vector<uint64_t> flat_rows(const std::vector<std::vector<uint64_t>> &M, const char *who, size_t &cols)
    {
        if (M.empty() || M[0].empty()) throw std::invalid_argument(std::string(who) + ": empty matrix");
        cols = M[0].size();
        std::vector<uint64_t> flat(M.size() * cols);
        for (size_t r = 0; r < M.size(); r++) {
            if (M[r].size() != cols) throw std::invalid_argument(std::string(who) + ": rows of different lengths");
            std::copy(M[r].begin(), M[r].end(), flat.begin() + r * cols);
        }
        return flat;
    }
    // make the layer resident ahead of its first request; bias: null for none
    PlainFc plain_fc_open(const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> *bias)
    {
        size_t cols = 0;
        const std::vector<uint64_t> flat = flat_rows(M, "plain_fc_open", cols);
        if (bias && bias->size() != M.size()) throw std::invalid_argument("plain_fc_open: bias and matrix dimensions differ");
        return mats_.get_open(flat.data(), M.size(), cols, bias ? bias->data() : nullptr);
    }
    // the layer on one ciphertext (hhe_fc_open_plain_ks): slots [0, rows) of the result are (M x + b) mod t; every step of
    // hhe_fc_open_galois_steps needs a key of its own in gk
    template <class GK, class Sink>
    void fc_open_plain(const std::vector<std::vector<uint64_t>> &M, const std::vector<uint64_t> *bias, const uint64_t *vi, const GK &gk, Sink dst)
    {
        const PlainFc m = plain_fc_open(M, bias);
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet g = named(set(gk), "Galois key not present");
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, vi);
        check(hhe_fc_open_plain_ks(h(), g.get(), m.get(), d, d, 1));
        download(d, 1, 2, dst);
    }
    // sum_k rotate_rows(in, steps[k], gk) * plains[k] under one mod-down (hhe_rotate_plain_sum_ks); plains: one slot vector per step, all of
    // one length.  A step list of all zeros needs no key
    template <class GK, class Sink>
    void rotate_plain_sum(const uint64_t *in_words, const std::vector<std::vector<uint64_t>> &plains, const std::vector<int> &steps, const GK &gk, Sink dst)
    {
        size_t count = 0;
        const std::vector<uint64_t> flat = flat_rows(plains, "rotate_plain_sum", count);
        if (steps.size() != plains.size()) throw std::invalid_argument("rotate_plain_sum: one plaintext per step");
        const PlainRows rows = mats_.get_rows(flat.data(), plains.size(), count);
        std::lock_guard<std::mutex> lk(arena_.mutex());
        const KeySet g = or_empty(set(gk));
        uint64_t *d = arena_.get(0, ct_words() * 8);
        upload(d, in_words);
        check(hhe_rotate_plain_sum_ks(h(), g.get(), rows.get(), steps.data(), steps.size(), d, d, 1));
        download(d, 1, 2, dst);
    }

    // client end: pasta::PASTA::encrypt / decrypt (pasta_3_plain.cpp:9-46) of `count` words in place, key: 256 words
    void pasta_crypt(const uint64_t *key, uint64_t *v, size_t count, bool dec, uint64_t nonce = fixed_nonce)
    {
        if (!count) return;
        DevBuf d(count * 8);
        check(hhe_copy_h2d(h(), d.p, v, count * 8));
        if (nonce == fixed_nonce) check(hhe_pasta3_plain_crypt(h(), key, d.u64(), 1, count, dec ? 1 : 0, d.u64()));
        else check(hhe_pasta3_plain_crypt_nonce(h(), key, &nonce, d.u64(), 1, count, dec ? 1 : 0, d.u64()));
        check(hhe_copy_d2h(h(), v, d.p, count * 8));
    }
    // ---- keys and ciphertexts from a seed, on the device (hhe_gfx950.h "key generation and encryption").  seed: 32 bytes, THE ONLY
    // ENTROPY: fresh from the caller's generator for every call below; the same seed for the same call repeats the randomness.
    size_t key_limbs() const { return L_ + 1; }
    size_t ksk_words() const { return L_ * 2 * (L_ + 1) * n_; }
    // KeyGenerator::secret_key + create_public_key: sk [K][N], pk [2][K][N], NTT form at the key level
    void generate_keys(const uint8_t *seed, std::vector<uint64_t> &sk, std::vector<uint64_t> &pk)
    {
        const size_t kn = key_limbs() * n_;
        DevBuf s(kn * 8), p(2 * kn * 8);
        check(hhe_keygen_secret(h(), seed, s.u64()));
        check(hhe_keygen_public(h(), s.u64(), seed, p.u64()));
        sk.resize(kn);
        pk.resize(2 * kn);
        check(hhe_copy_d2h(h(), sk.data(), s.p, kn * 8));
        check(hhe_copy_d2h(h(), pk.data(), p.p, 2 * kn * 8));
    }
    // KeyGenerator::create_relin_keys: RelinKeys::key(2) words
    void generate_relin(const uint64_t *sk, const uint8_t *seed, std::vector<uint64_t> &key)
    {
        const KeySet ks = keys_.new_set();
        DevBuf s(key_limbs() * n_ * 8);
        check(hhe_copy_h2d(h(), s.p, sk, key_limbs() * n_ * 8));
        check(hhe_keyset_generate_relin(ks.get(), s.u64(), seed));
        key.resize(ksk_words());
        check(hhe_keyset_get_relin(ks.get(), key.data()));
    }
    // KeyGenerator::create_galois_keys(steps, gk) (SEALZpCipher::create_gk, SEAL_Cipher.cpp:359); no steps: create_galois_keys(gk), the
    // default elements.  Words by Galois element.
    void generate_galois(const uint64_t *sk, const std::vector<int> &steps, const uint8_t *seed, std::map<uint32_t, std::vector<uint64_t>> &keys)
    {
        std::vector<uint32_t> elts;
        for (int s : steps) {
            const uint32_t e = (uint32_t)hhe_ctx_query(h(), "galois_elt", s);
            if (!e) throw std::invalid_argument("step count too large");  // GaloisTool::get_elt_from_step
            if (std::find(elts.begin(), elts.end(), e) == elts.end()) elts.push_back(e);
        }
        const KeySet ks = keys_.new_set();
        DevBuf s(key_limbs() * n_ * 8);
        check(hhe_copy_h2d(h(), s.p, sk, key_limbs() * n_ * 8));
        check(hhe_keyset_generate_galois(ks.get(), s.u64(), elts.empty() ? nullptr : elts.data(), elts.size(), seed));
        if (elts.empty())  // the default set: every odd element the set now holds
            for (uint32_t e = 1; e < 2 * n_; e += 2)
                if (hhe_keyset_has_galois(ks.get(), e)) elts.push_back(e);
        keys.clear();
        for (uint32_t e : elts) {
            std::vector<uint64_t> &k = keys[e];
            k.resize(ksk_words());
            check(hhe_keyset_get_galois(ks.get(), e, k.data()));
        }
    }
    // BatchEncoder::encode + Encryptor::encrypt of `count` slot values (the rest are zero) under the public key pk [2][K][N]
    template <class Sink> void encrypt(const uint64_t *pk, const uint64_t *vals, size_t count, const uint8_t *seed, Sink dst)
    {
        if (!count || count > n_) throw std::invalid_argument("encrypt: values do not fit the slots");
        DevBuf p(2 * key_limbs() * n_ * 8), v(count * 8), plain(n_ * 8), ct(ct_words() * 8);
        check(hhe_copy_h2d(h(), p.p, pk, 2 * key_limbs() * n_ * 8));
        check(hhe_copy_h2d(h(), v.p, vals, count * 8));
        check(hhe_encode(h(), v.u64(), 1, count, plain.u64()));
        check(hhe_encrypt(h(), p.u64(), plain.u64(), 0, seed, 1, ct.u64()));
        download(ct.u64(), 1, 2, dst);
    }

    // analyst end: Decryptor::decrypt + BatchEncoder::decode; sk: [K][N] NTT form; vals: N slot values < t.  limbs: the level of the
    // ciphertext ([2][limbs][N] words; 0 = the data level)
    void decrypt(const uint64_t *sk, const uint64_t *ct, uint64_t *vals, size_t limbs = 0)
    {
        const size_t l = limbs_or_data(limbs), words = 2 * l * n_;
        DevBuf c(words * 8), v(n_ * 8);
        check(hhe_copy_h2d(h(), c.p, ct, words * 8));
        check(hhe_decrypt_level(h(), sk, c.u64(), (int)l, 1, v.u64()));
        check(hhe_copy_d2h(h(), vals, v.p, n_ * 8));
    }

    // Decryptor::invariant_noise_budget (seal/decryptor.h:103) of the ciphertexts words[i], all [size][limbs][N] (limbs 0 = the data
    // level), in ONE device call; sk: [K][N] NTT form.  The budgets in the order of `words`
    std::vector<int> noise_budget(const std::vector<const uint64_t *> &words, size_t size, size_t limbs, const uint64_t *sk)
    {
        if (words.empty()) throw std::invalid_argument("noise_budget: no ciphertext");
        const size_t l = limbs_or_data(limbs), w = size * l * n_;
        DevBuf c(words.size() * w * 8);
        for (size_t i = 0; i < words.size(); i++) check(hhe_copy_h2d(h(), c.u64() + i * w, words[i], w * 8));
        std::vector<int32_t> b(words.size());
        check(hhe_noise_budget(h(), sk, c.u64(), (int)size, (int)l, words.size(), b.data(), nullptr));
        return std::vector<int>(b.begin(), b.end());
    }
    // ... of ciphertexts that may differ in size or level: one device call per (size, limbs) among them, i.e. one for what a service holds
    struct NoiseItem { const uint64_t *words; size_t size, limbs; };
    std::vector<int> noise_budget(const std::vector<NoiseItem> &items, const uint64_t *sk)
    {
        if (items.empty()) throw std::invalid_argument("noise_budget: no ciphertext");
        std::vector<int> out(items.size());
        std::vector<char> done(items.size(), 0);
        for (size_t i = 0; i < items.size(); i++) {
            if (done[i]) continue;
            std::vector<const uint64_t *> group;
            std::vector<size_t> at;
            for (size_t j = i; j < items.size(); j++)
                if (!done[j] && items[j].size == items[i].size && limbs_or_data(items[j].limbs) == limbs_or_data(items[i].limbs)) {
                    group.push_back(items[j].words); at.push_back(j); done[j] = 1;
                }
            const std::vector<int> b = noise_budget(group, items[i].size, items[i].limbs, sk);
            for (size_t k = 0; k < at.size(); k++) out[at[k]] = b[k];
        }
        return out;
    }

    // ---- levels (SEALZpCipher::get_cipher_size(ct, mod_switch, levels_from_last), SEAL_Cipher.cpp:363-378).  On THIS core a ciphertext
    // below the data level can be switched further, measured and decrypted, and every evaluation call refuses it; it is evaluated on the
    // core of its level (level() below), whose data level it is.
    size_t limbs_or_data(size_t limbs) const
    {
        if (limbs > L_) throw std::invalid_argument("encrypted is not valid for encryption parameters");
        return limbs ? limbs : L_;
    }
    // limbs of the level `levels_from_last` steps above last_context_data(); the reference walks prev_context_data() off the chain
    // (a null pointer) where this throws
    size_t level_limbs(size_t levels_from_last) const
    {
        if (levels_from_last >= L_) throw std::invalid_argument("levels_from_last is beyond the first level of the modulus switching chain");
        return 1 + levels_from_last;
    }
    // Evaluator::mod_switch_to_inplace: words [size][limbs_in][N] -> the sink's [size][limbs_out][N]; a switch to a higher level throws
    // std::invalid_argument, as SEAL does
    template <class Sink> void mod_switch(const uint64_t *words, size_t size, size_t limbs_in, size_t limbs_out, Sink dst)
    {
        limbs_or_data(limbs_in);
        const size_t win = size * limbs_in * n_, wout = size * limbs_out * n_;
        DevBuf a(win * 8), o((wout ? wout : 1) * 8);
        check(hhe_copy_h2d(h(), a.p, words, win * 8));
        check(hhe_mod_switch(h(), a.u64(), (int)size, 1, (int)limbs_in, (int)limbs_out, o.u64()));
        check(hhe_copy_d2h(h(), dst(0), o.p, wout * 8));
    }
    // bytes of Ciphertext::save(stream, compr_mode_type::none) at that level.  The reference's ct.save(s) takes SEAL's default mode
    // (zstd where SEAL was built with it): its figure is the compressed size, this one the uncompressed size it is bounded by
    size_t saved_size(size_t size, size_t limbs)
    {
        static const uint8_t id[32] = {};
        static const uint64_t none = 0;
        size_t need = 0;
        const int rc = hhe_seal_save_ciphertext_level(h(), &none, size, (int)limbs_or_data(limbs), id, nullptr, 0, &need);  // sizes only: nothing is read
        if (rc != HHE_ERR_CAPACITY) check(rc);
        return need;
    }

    // ---- evaluation at a level.  The core of the level with `limbs` data primes of this chain (hhe_ctx_create_level): made on first
    // use and kept, one per (this core, limbs), with its own context, arena and caches; every call body above runs on it unchanged, on
    // [.][limbs][N].  It holds no keys of its own: the sets its calls name are derived() from this core's.
    std::shared_ptr<AdapterCore> level(size_t limbs)
    {
        if (limbs < 1 || limbs > L_) throw std::invalid_argument("level: the chain has no level with that many data primes");
        std::lock_guard<std::mutex> lk(levels_mu_);
        std::shared_ptr<AdapterCore> &slot = levels_[limbs];
        if (!slot) slot.reset(new AdapterCore(*this, limbs));
        return slot;
    }
    // On a level core: its set that is the projection of `parent_set`, a set of the core higher up the chain -- derived on the device on
    // first use (hhe_keyset_derive_level: nothing is uploaded twice), kept per (parent set, this level), dropped once the parent set is
    // gone (its last holder let go: the parent's cache evicted it and no cipher object holds it).  A null set stays null.
    KeySet derived(const KeySet &parent_set)
    {
        if (!parent_set) return nullptr;
        std::lock_guard<std::mutex> lk(derived_mu_);
        for (auto it = derived_.begin(); it != derived_.end();) it = it->second.first.expired() ? derived_.erase(it) : std::next(it);
        auto it = derived_.find(parent_set.get());
        if (it != derived_.end()) return it->second.second;
        KeySet ks = keys_.new_set();
        check(hhe_keyset_derive_level(ks.get(), parent_set.get()));
        ++derivations;
        derived_[parent_set.get()] = std::make_pair(std::weak_ptr<hhe_keyset>(parent_set), ks);
        return ks;
    }
    uint64_t derivations = 0;  // instrumentation: how many sets were derived (a repeated parent set is not)
    size_t derived_resident()
    {
        std::lock_guard<std::mutex> lk(derived_mu_);
        return derived_.size();
    }
    // rows {0..limbs-1, K-1} of a key-level object [polys][K][N] of this core: the object of that level (sk: polys 1, pk: polys 2)
    std::vector<uint64_t> level_rows(const uint64_t *words, size_t polys, size_t limbs) const
    {
        const size_t K = key_limbs();
        std::vector<uint64_t> out(polys * (limbs + 1) * n_);
        for (size_t p = 0; p < polys; p++)
            for (size_t j = 0; j <= limbs; j++)
                std::copy(words + (p * K + (j == limbs ? K - 1 : j)) * n_, words + (p * K + (j == limbs ? K - 1 : j) + 1) * n_,
                          out.begin() + (p * (limbs + 1) + j) * n_);
        return out;
    }

private:
    AdapterCore(const AdapterCore &parent, size_t limbs)
        : n_(parent.n_), L_(limbs), t_(parent.t_), max_sets_(parent.max_sets_), max_matrices_(parent.max_matrices_),
          h_(create_level(parent.h(), limbs), hhe_ctx_destroy), keys_(h_.get(), max_sets_), empty_(keys_.new_set()), mats_(h_.get(), max_matrices_) {}
    static hhe_ctx *create_level(const hhe_ctx *parent, size_t limbs)
    {
        hhe_ctx *h = nullptr;
        check(hhe_ctx_create_level(parent, (int)limbs, &h));
        return h;
    }
    static hhe_ctx *create(int logn, const std::vector<uint64_t> &q, uint64_t t, int device)
    {
        hhe_ctx *h = nullptr;
        check(hhe_ctx_create(logn, (int)q.size(), q.data(), t, device, &h));
        return h;
    }
    hhe_ctx *h() const { return h_.get(); }
    void upload(uint64_t *d, const uint64_t *src, size_t size = 2) { check(hhe_copy_h2d(h(), d, src, ct_words(size) * 8)); }
    template <class Sink> void download(const uint64_t *d, size_t items, size_t size, Sink &dst)
    {
        for (size_t i = 0; i < items; i++) check(hhe_copy_d2h(h(), dst(i), d + i * ct_words(size), ct_words(size) * 8));
    }
    const KeySet &set(const KeySet &held) { return held; }
    KeySet set(const GaloisWords &g) { return keys_.galois(g); }
    KeySet set(const RelinWords &r) { return keys_.relin(r); }
    const KeySet &or_empty(const KeySet &ks) const { return ks ? ks : empty_; }
    static const KeySet &named(const KeySet &ks, const char *what_if_empty)
    {
        if (!ks) throw std::invalid_argument(what_if_empty);
        return ks;
    }
    // enc_ssk[0] arrives by value with every call (CSP.cpp:249): it crosses PCIe only when its contents change.  Caller holds the
    // arena's lock; the resident copy lives in arena slot 2.
    uint64_t *encrypted_key(const uint64_t *words)
    {
        ContentHash hsh;
        hsh.add(words, ct_words());
        uint64_t *d = arena_.get(2, ct_words() * 8);
        if (!key_resident_ || key_hash_ != hsh) {
            upload(d, words);
            key_hash_ = hsh;
            key_resident_ = true;
            ++key_uploads;
        }
        return d;
    }
    size_t n_, L_;
    uint64_t t_;
    size_t max_sets_, max_matrices_;
    std::unique_ptr<hhe_ctx, void (*)(hhe_ctx *)> h_;  // declared before the key sets: destroyed after every set the core holds
    KeySetCache keys_;
    KeySet empty_;   // what a cipher object built without some key runs with; nothing can put a key into it
    MatrixCache mats_;   // declared after the context, like the key sets: every handle dies before it
    DeviceArena arena_;
    ContentHash key_hash_;
    bool key_resident_ = false;
    // on a level core: parent set -> (the parent set, watched; its projection on this level).  Declared after the context: every set dies before it
    std::mutex derived_mu_;
    std::map<const hhe_keyset *, std::pair<std::weak_ptr<hhe_keyset>, KeySet>> derived_;
    // the cores of this chain's levels, by data primes; independent contexts, released with this core unless a level object still holds one
    std::mutex levels_mu_;
    std::map<size_t, std::shared_ptr<AdapterCore>> levels_;
};

}  // namespace hhe
