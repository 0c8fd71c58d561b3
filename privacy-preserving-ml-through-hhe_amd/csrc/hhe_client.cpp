// hhe_client.cpp -- C ABI of the client / analyst ends: the plain PASTA-3 cipher
// (pasta::PASTA::encrypt / decrypt, pasta::Pasta::keystream -- src/pasta/pasta_3_plain.cpp:9-46,156-178) and batched
// BFV result decryption (sealhelper::decrypting, src/util/sealhelper.cpp:252-266).  Host code only sets up constants and
// launches; the arithmetic is in hhe_client_bodies.h.
#include <algorithm>
#include <cstring>
#include <vector>
#include "hhe_args.h"

namespace {
typedef unsigned __int128 u128;
void barrett_ratio(u64 q, u64 &lo, u64 &hi)
{
    const u128 two64 = (u128)1 << 64;
    hi = (u64)(two64 / q);
    lo = (u64)(((two64 % q) << 64) / q);
}

// nblocks keystream blocks under (nonce, first_block + i), or -- pairs set -- under pairs[i]
int keystream_into(hhe_ctx *c, const uint64_t *key, uint64_t nonce, uint64_t first_block, const PastaPair *pairs, size_t nblocks, u64 *ks, rt_stream st)
{
    for (int i = 0; i < 2 * PASTA_T; ++i)
        if (key[i] >= c->t) return fail(HHE_ERR_INVALID, "PASTA secret key word is not below the plain modulus");
    DevBuf rnd(nblocks * PASTA_RAND_PER_BLOCK * 8), dkey(2 * PASTA_T * 8), dpairs(pairs ? nblocks * sizeof(PastaPair) : 8);
    if (!rnd.p || !dkey.p || !dpairs.p) return dev_fail("hhe_pasta3_plain_keystream");
    if (rt_h2d(dkey.p, key, 2 * PASTA_T * 8, st)) return dev_fail("hhe_pasta3_plain_keystream");
    if (pairs && rt_h2d(dpairs.p, pairs, nblocks * sizeof(PastaPair), st)) return dev_fail("hhe_pasta3_plain_keystream");
    PastaXofArgs x = zeroed<PastaXofArgs>();
    x.mode = XOF_PASTA;
    x.t = c->t; x.nonce = nonce; x.first_block = first_block; x.nblocks = (int)nblocks; x.rand = rnd.w();
    x.pairs = pairs ? (const PastaPair *)dpairs.p : nullptr;
    int bits = 0;
    for (u64 v = c->t; v; v >>= 1) ++bits;
    x.mask = bits >= 64 ? ~(u64)0 : (((u64)1 << bits) - 1);  // Pasta::Pasta(): max_prime_size (pasta_3_plain.cpp:150-153)
    k_pasta_xof(x, st);
    PastaPlainArgs p = zeroed<PastaPlainArgs>();
    p.t = c->t; barrett_ratio(c->t, p.r_lo, p.r_hi);
    p.rand = rnd.w(); p.key = dkey.w(); p.ks = ks; p.nblocks = (int)nblocks;
    k_pasta_plain(p, st);
    if (rt_sync(st)) return dev_fail("hhe_pasta3_plain_keystream");  // temporaries are released on return
    return HHE_OK;
}
}  // namespace

extern "C" int hhe_pasta3_plain_keystream(hhe_ctx *c, const uint64_t *key, uint64_t first_block, size_t nblocks, uint64_t *ks)
{
    HHE_LOCK(c);
    if (!c || !key || !ks || nblocks == 0 || nblocks > ((size_t)1 << 24))
        return fail(HHE_ERR_INVALID, "hhe_pasta3_plain_keystream: bad arguments");
    return keystream_into(c, key, PASTA_NONCE, first_block, nullptr, nblocks, ks, c->lanes[0].stream);
}
extern "C" int hhe_pasta3_plain_keystream_nonce(hhe_ctx *c, const uint64_t *key, uint64_t nonce, uint64_t first_block, size_t nblocks, uint64_t *ks)
{
    HHE_LOCK(c);
    if (!c || !key || !ks || nblocks == 0 || nblocks > ((size_t)1 << 24))
        return fail(HHE_ERR_INVALID, "hhe_pasta3_plain_keystream: bad arguments");
    return keystream_into(c, key, nonce, first_block, nullptr, nblocks, ks, c->lanes[0].stream);
}

// nonces: one per record (each record restarts at block counter 0 under its own nonce), or null: every PASTA::encrypt call of the
// reference restarts at block counter 0 with the fixed nonce, so all records share one keystream
static int plain_crypt(hhe_ctx *c, const uint64_t *key, const uint64_t *nonces, const uint64_t *in, size_t S, size_t nwords, int decrypt, uint64_t *out)
{
    const size_t nb = (nwords + PASTA_T - 1) / PASTA_T;  // ceil(size / plain_size) (pasta_3_plain.cpp:13)
    const size_t nks = nonces ? S * nb : nb;
    if (nks > ((size_t)1 << 24)) return fail(HHE_ERR_INVALID, "hhe_pasta3_plain_crypt: bad arguments");
    rt_stream st = c->lanes[0].stream;
    DevBuf ks(nks * PASTA_T * 8);
    if (!ks.p) return dev_fail("hhe_pasta3_plain_crypt");
    std::vector<PastaPair> pairs(nonces ? nks : 0);
    for (size_t i = 0; i < pairs.size(); ++i) pairs[i] = PastaPair(nonces[i / nb], i % nb);
    int rc = keystream_into(c, key, PASTA_NONCE, 0, nonces ? pairs.data() : nullptr, nks, ks.w(), st);
    if (rc) return rc;
    PastaCryptArgs a;
    u64 lo;
    a.t = c->t; barrett_ratio(c->t, lo, a.r_hi);
    a.in = in; a.ks = ks.w(); a.out = out; a.S = S; a.nwords = nwords; a.decrypt = decrypt != 0;
    a.ks_stride = nonces ? nb * PASTA_T : 0;
    k_pasta_crypt(a, st);
    if (rt_sync(st)) return dev_fail("hhe_pasta3_plain_crypt");
    return HHE_OK;
}
extern "C" int hhe_pasta3_plain_crypt(hhe_ctx *c, const uint64_t *key, const uint64_t *in, size_t S, size_t nwords, int decrypt,
                                      uint64_t *out)
{
    HHE_LOCK(c);
    if (!c || !key || !in || !out || S == 0 || nwords == 0) return fail(HHE_ERR_INVALID, "hhe_pasta3_plain_crypt: bad arguments");
    return plain_crypt(c, key, nullptr, in, S, nwords, decrypt, out);
}
extern "C" int hhe_pasta3_plain_crypt_nonce(hhe_ctx *c, const uint64_t *key, const uint64_t *nonces, const uint64_t *in, size_t S, size_t nwords,
                                            int decrypt, uint64_t *out)
{
    HHE_LOCK(c);
    if (!c || !key || !nonces || !in || !out || S == 0 || nwords == 0) return fail(HHE_ERR_INVALID, "hhe_pasta3_plain_crypt: bad arguments");
    return plain_crypt(c, key, nonces, in, S, nwords, decrypt, out);
}

// The phase of B ciphertexts [B][size][L][N] (coefficient form) under q_0 .. q_{L-1} without its c0: c1s [B][L][N] = c1 s (+ c2 s^2 for
// size 3), coefficient form.  dsk [L][N] = the level's limbs of the key-level secret key on the device; s2 (size 3 only) is scratch:
// [L][N] for s^2, then [B][L][N] for the transform of c2 between its passes (its last pass adds into c1s).  Forward transform of c1
// with the dyadic product fused into the store, for size 3 the transform of c2 multiplied by s^2 and added in its store, one inverse
// transform.  Enqueued on st.
static void phase_c1s(hhe_ctx *c, const u64 *dsk, u64 *s2, const uint64_t *ct, int size, const int L, size_t B, u64 *c1s, rt_stream st)
{
    const size_t ln = (size_t)L * c->n;
    NttArgs a = ntt_args(c, ct + ln, c1s, B * L, 0, L);
    a.L = L;  // the limb count of the call's level, not the context's
    a.src_item_polys = L; a.src_item_stride = (size_t)size * ln; a.store_op = STORE_MUL; a.mul = dsk; a.mul_cycle = L;
    k_ntt(a, false, st);
    if (size == 3) {
        k_elt(elt_args(c, dsk, dsk, s2, L, 0, L), ELT_MUL, st);  // s^2, a dyadic product of the uploaded key (NTT form)
        NttArgs m = a;
        m.src = ct + 2 * ln; m.dst = s2 + ln; m.store_op = STORE_MAC; m.mul = s2; m.acc = c1s;
        k_ntt(m, false, st);
    }
    NttArgs inv = a;
    inv.src = c1s; inv.src_item_polys = 0; inv.src_item_stride = 0; inv.store_op = STORE_PLAIN; inv.mul = nullptr;
    k_ntt(inv, true, st);
}

// Decryption under q_0 .. q_{L-1} for any 1 <= L <= c->L: every constant below is derived from the limb count of the call (a level of
// the modulus chain is the context with its last data primes dropped; gamma and t do not change)
static int decrypt_level(hhe_ctx *c, const uint64_t *sk, const uint64_t *ct, const int L, size_t B, uint64_t *vals)
{
    const size_t n = c->n, ln = (size_t)L * n;
    rt_stream st = c->lanes[0].stream;
    DevBuf dsk(ln * 8), c1s(B * ln * 8), plain(B * n * 8);
    if (!dsk.p || !c1s.p || !plain.p) return dev_fail("hhe_decrypt");
    if (rt_h2d(dsk.p, sk, ln * 8, st)) return dev_fail("hhe_decrypt");  // the level's limbs of the key-level secret key
    phase_c1s(c, dsk.w(), nullptr, ct, 2, L, B, c1s.w(), st);

    DecryptArgs d = zeroed<DecryptArgs>();
    d.mods = c->d_mods; d.ct = ct; d.c1s = c1s.w(); d.plain = plain.w(); d.logn = c->logn; d.L = L; d.B = B;
    d.t = c->t; d.gamma = c->gamma;
    barrett_ratio(c->t, d.t_rlo, d.t_rhi);
    barrett_ratio(c->gamma, d.g_rlo, d.g_rhi);
    const u64 t = c->t, g = c->gamma;
    u64 q_t = 1 % t, q_g = 1 % g;
    for (int j = 0; j < L; ++j) {
        const u64 qj = c->q[j];
        u64 punct_q = 1 % qj, punct_t = 1 % t, punct_g = 1 % g;
        for (int i = 0; i < L; ++i)
            if (i != j) {
                punct_q = nt_mulmod(punct_q, c->q[i] % qj, qj);
                punct_t = nt_mulmod(punct_t, c->q[i] % t, t);
                punct_g = nt_mulmod(punct_g, c->q[i] % g, g);
            }
        const u64 tg = nt_mulmod(t % qj, g % qj, qj);
        d.cj[j] = nt_mulmod(tg, nt_invmod(punct_q, qj), qj);
        d.pt[j] = punct_t;
        d.pg[j] = punct_g;
        q_t = nt_mulmod(q_t, qj % t, t);
        q_g = nt_mulmod(q_g, qj % g, g);
    }
    d.neg_inv_q_t = (t - nt_invmod(q_t, t)) % t;
    d.neg_inv_q_g = (g - nt_invmod(q_g, g)) % g;
    d.inv_g_t = nt_invmod(g % t, t);
    k_decrypt_round(d, st);

    // BatchEncoder::decode: forward NTT mod t, then the slot index map
    NttArgs p = ntt_args(c, plain.w(), plain.w(), B, c->mod_t, 1);
    p.L = L;  // as in phase_c1s
    k_ntt(p, false, st);
    DecodeArgs g2;
    g2.in = plain.w(); g2.vals = vals; g2.slot_map = c->d_slot_map; g2.logn = c->logn; g2.B = B;
    k_decode_gather(g2, st);
    if (rt_sync(st)) return dev_fail("hhe_decrypt");
    return HHE_OK;
}
extern "C" int hhe_decrypt(hhe_ctx *c, const uint64_t *sk, const uint64_t *ct, size_t B, uint64_t *vals)
{
    HHE_LOCK(c);
    if (!c || !sk || !ct || !vals || B == 0) return fail(HHE_ERR_INVALID, "hhe_decrypt: bad arguments");
    return decrypt_level(c, sk, ct, c->L, B, vals);
}
extern "C" int hhe_decrypt_level(hhe_ctx *c, const uint64_t *sk, const uint64_t *ct, int limbs, size_t B, uint64_t *vals)
{
    HHE_LOCK(c);
    if (!c || !sk || !ct || !vals || B == 0 || limbs < 1 || limbs > c->L) return fail(HHE_ERR_INVALID, "hhe_decrypt_level: bad arguments (1 <= limbs <= L)");
    return decrypt_level(c, sk, ct, limbs, B, vals);
}

// Decryptor::invariant_noise_budget (seal/decryptor.h:103) of B ciphertexts at one level: the phase as in decryption, then one launch
// (noise_bits, hhe_client_bodies.h) that leaves the significant bits of the largest centred coefficient of t * phase mod Q per item.
// Q and (Q+1)/2 for the call's level are made here, word by word, and travel in the argument block.
extern "C" int hhe_noise_budget(hhe_ctx *c, const uint64_t *sk, const uint64_t *ct, int size, int limbs, size_t B, int32_t *budget,
                                uint32_t *norm_bits)
{
    HHE_LOCK(c);
    if (!c || !sk || !ct || !budget || B == 0) return fail(HHE_ERR_INVALID, "hhe_noise_budget: bad arguments");
    if (size < 2 || size > 3) return fail(HHE_ERR_INVALID, "hhe_noise_budget: ciphertext size must be 2 or 3");
    if (limbs < 1 || limbs > c->L) return fail(HHE_ERR_INVALID, "hhe_noise_budget: bad arguments (1 <= limbs <= L)");
    const int L = limbs;
    const size_t n = c->n, ln = (size_t)L * n;
    if (B > ((size_t)1 << 30) / L) return fail(HHE_ERR_INVALID, "hhe_noise_budget: batch too large");
    rt_stream st = c->lanes[0].stream;
    DevBuf dsk((size == 3 ? 2 + B : 1) * ln * 8), c1s(B * ln * 8), dbits(B * 4);  // the key | size 3: phase_c1s' scratch
    if (!dsk.p || !c1s.p || !dbits.p) return dev_fail("hhe_noise_budget");
    if (rt_h2d(dsk.p, sk, ln * 8, st) || rt_memset(dbits.p, 0, B * 4, st)) return dev_fail("hhe_noise_budget");
    phase_c1s(c, dsk.w(), dsk.w() + ln, ct, size, L, B, c1s.w(), st);

    DecryptArgs d = zeroed<DecryptArgs>();
    d.mode = DEC_NOISE; d.size = size; d.mods = c->d_mods; d.ct = ct; d.c1s = c1s.w(); d.logn = c->logn; d.L = L; d.B = B;
    d.t = c->t; d.pairs = c->d_moddown; d.bits = (u32 *)dbits.p;
    d.cj[0] = 1;  // Q = q_0 ... q_{L-1} < 2^(64 L): L words
    for (int j = 0; j < L; ++j) {
        u64 carry = 0;
        for (int w = 0; w < L; ++w) {
            const u128 p = (u128)d.cj[w] * c->q[j] + carry;
            d.cj[w] = (u64)p; carry = (u64)(p >> 64);
        }
        d.pg[j] = c->t % c->q[j];
    }
    int q_bits = 0;
    for (int w = 0; w < L; ++w)
        if (d.cj[w]) q_bits = 64 * w + 64 - __builtin_clzll(d.cj[w]);
    {   // (Q+1)/2 = (Q >> 1) + (Q & 1)
        u64 carry = d.cj[0] & 1;
        for (int w = 0; w < L; ++w) {
            const u64 sh = (d.cj[w] >> 1) | (w + 1 < L ? d.cj[w + 1] << 63 : 0);
            d.pt[w] = sh + carry;
            carry = d.pt[w] < sh;
        }
    }
    k_decrypt_round(d, st);
    c->noise_form = L <= NOISE_REGS ? L : 0;
    std::vector<u32> bits(B);
    if (rt_d2h(bits.data(), dbits.p, B * 4, st) || rt_sync(st)) return dev_fail("hhe_noise_budget");
    for (size_t b = 0; b < B; ++b) {
        const int v = q_bits - (int)bits[b] - 1;
        budget[b] = v > 0 ? v : 0;
        if (norm_bits) norm_bits[b] = bits[b];
    }
    return HHE_OK;
}

// ------------------------------------------------------------------ key generation and public-key encryption from a seed
// (KeyGenerator::create_public_key / create_relin_keys / create_galois_keys, Analyst.cpp:38-93, hhe_pktnn_examples.cpp:435-443,
// 615-617; Encryptor::encrypt, pastahelper.cpp:355-377, sealhelper.cpp:123-142).  The randomness is the sampler of
// hhe_keygen_bodies.h; host code only names the positions and launches.
namespace {
enum { PUR_SECRET = 1, PUR_PUBLIC = 2, PUR_RELIN = 3, PUR_GALOIS = 4, PUR_ENCRYPT = 5 };

PastaXofArgs sample_args(const hhe_ctx *c, const uint8_t *seed, u32 purpose, u32 elt, u32 first_index)
{
    PastaXofArgs x = zeroed<PastaXofArgs>();
    x.mode = XOF_SAMPLE;
    for (int w = 0; w < 4; ++w)
        for (int b = 0; b < 8; ++b) x.seed[w] |= (u64)seed[8 * w + b] << (8 * b);
    x.purpose = purpose; x.elt = elt; x.first_index = first_index; x.logn = c->logn; x.mods = c->d_mods;
    return x;
}
void seg_small(SampleSeg &g, int kind, int nidx, int ncomp, int nres, int mod_cycle, u64 *out, size_t idx_stride, size_t comp_stride)
{
    g.kind = kind; g.nidx = nidx; g.ncomp = ncomp; g.nres = nres; g.mod_base = 0; g.mod_cycle = mod_cycle;
    g.out = out; g.idx_stride = idx_stride; g.comp_stride = comp_stride;
}
void seg_uniform(SampleSeg &g, int nidx, int nlimbs, int mod_base, u64 *out, size_t idx_stride, size_t n)
{
    g.kind = SMP_UNIFORM; g.nidx = nidx; g.ncomp = nlimbs; g.nres = 0; g.mod_base = mod_base; g.mod_cycle = nlimbs;
    g.out = out; g.idx_stride = idx_stride; g.comp_stride = n;
}
void sample_launch(const hhe_ctx *c, PastaXofArgs &x, rt_stream st)
{
    const size_t polys = (size_t)x.seg[0].nidx * x.seg[0].ncomp + (size_t)x.seg[1].nidx * x.seg[1].ncomp;
    x.nblocks = (int)(polys << (c->logn - 6));  // one lane per 64-coefficient chunk
    k_pasta_xof(x, st);
}
// in-place transform of `count` polynomials under q_0 .. q_{mod_cycle-1}
NttArgs plain_ntt(const hhe_ctx *c, u64 *polys, size_t count, int mod_cycle) { return ntt_args(c, polys, polys, count, 0, mod_cycle); }
// D encryptions of zero under the secret key at the key level, NTT form, into key [D][2][K][N] (generate_one_kswitch_key; D = 1 without
// new_key: a public key): one sampler launch (a into the c1 slots, e into noise [D][K][N]), one forward transform, one fused launch.
// with_key: new_key [K][N] (NTT form) sits behind the noise, at noise + D * K * N (new_key_of)
u64 *new_key_of(const hhe_ctx *c, u64 *noise, int D) { return noise + (size_t)D * c->K * c->n; }
void gen_enc_zero(hhe_ctx *c, const u64 *sk, bool with_key, const uint8_t *seed, u32 purpose, u32 elt, int D, u64 *key, u64 *noise, rt_stream st)
{
    const int K = c->K;
    const size_t n = c->n;
    PastaXofArgs x = sample_args(c, seed, purpose, elt, 0);
    seg_uniform(x.seg[0], D, K, 0, key + (size_t)K * n, (size_t)2 * K * n, n);
    seg_small(x.seg[1], SMP_NOISE, D, 1, K, K, noise, (size_t)K * n, 0);
    sample_launch(c, x, st);
    k_ntt(plain_ntt(c, noise, (size_t)D * K, K), false, st);
    EltArgs e = elt_args(c, noise, sk, key, (size_t)D * K, 0, K, K);
    e.with_key = with_key ? 1 : 0;
    k_elt(e, ELT_ENCZ, st);
}
int seed_check(const hhe_ctx *c, const char *who)
{
    if (c->logn < 6) return fail(HHE_ERR_INVALID, std::string(who) + ": the sampler needs N >= 64");
    return HHE_OK;
}
}  // namespace

extern "C" int hhe_sample_poly(hhe_ctx *c, const uint8_t *seed, uint32_t purpose, uint32_t elt, uint32_t index, int kind, int mod_base,
                               int mod_count, uint64_t *out)
{
    HHE_LOCK(c);
    if (!c || !seed || !out || purpose > 255 || kind < SMP_TERNARY || kind > SMP_UNIFORM || mod_base < 0 || mod_count < 1 ||
        mod_base + mod_count > c->nmod)
        return fail(HHE_ERR_INVALID, "hhe_sample_poly: bad arguments");
    if (int rc = seed_check(c, "hhe_sample_poly")) return rc;
    rt_stream st = c->lanes[0].stream;
    PastaXofArgs x = sample_args(c, seed, purpose, elt, index);
    if (kind == SMP_UNIFORM) seg_uniform(x.seg[0], 1, mod_count, mod_base, out, 0, c->n);
    else {
        seg_small(x.seg[0], kind, 1, 1, mod_count, mod_count, out, 0, 0);
        x.seg[0].mod_base = mod_base;
    }
    sample_launch(c, x, st);
    if (rt_sync(st)) return dev_fail("hhe_sample_poly");
    return HHE_OK;
}

extern "C" int hhe_keygen_secret(hhe_ctx *c, const uint8_t *seed, uint64_t *sk)
{
    HHE_LOCK(c);
    if (!c || !seed || !sk) return fail(HHE_ERR_INVALID, "hhe_keygen_secret: null argument");
    if (int rc = seed_check(c, "hhe_keygen_secret")) return rc;
    rt_stream st = c->lanes[0].stream;
    PastaXofArgs x = sample_args(c, seed, PUR_SECRET, 0, 0);
    seg_small(x.seg[0], SMP_TERNARY, 1, 1, c->K, c->K, sk, 0, 0);
    sample_launch(c, x, st);
    k_ntt(plain_ntt(c, sk, c->K, c->K), false, st);
    if (rt_sync(st)) return dev_fail("hhe_keygen_secret");
    return HHE_OK;
}

extern "C" int hhe_keygen_public(hhe_ctx *c, const uint64_t *sk, const uint8_t *seed, uint64_t *pk)
{
    HHE_LOCK(c);
    if (!c || !sk || !seed || !pk) return fail(HHE_ERR_INVALID, "hhe_keygen_public: null argument");
    if (int rc = seed_check(c, "hhe_keygen_public")) return rc;
    rt_stream st = c->lanes[0].stream;
    DevBuf noise((size_t)c->K * c->n * 8);
    if (!noise.p) return dev_fail("hhe_keygen_public");
    gen_enc_zero(c, sk, false, seed, PUR_PUBLIC, 0, 1, pk, noise.w(), st);
    if (rt_sync(st)) return dev_fail("hhe_keygen_public");
    return HHE_OK;
}

extern "C" int hhe_keyset_generate_relin(hhe_keyset *ks, const uint64_t *sk, const uint8_t *seed)
{
    if (!ks || !sk || !seed) return fail(HHE_ERR_INVALID, "hhe_keyset_generate_relin: null argument");
    hhe_ctx *c = ks->ctx;
    HHE_LOCK(c);
    if (int rc = seed_check(c, "hhe_keyset_generate_relin")) return rc;
    rt_stream st = c->lanes[0].stream;
    const size_t kn = (size_t)c->K * c->n;
    DevBuf key(c->ksk_words() * 8), noise((size_t)(c->L + 1) * kn * 8);
    if (!key.p || !noise.p) return dev_fail("hhe_keyset_generate_relin");
    k_elt(elt_args(c, sk, sk, new_key_of(c, noise.w(), c->L), c->K, 0, c->K), ELT_MUL, st);  // new_key = s^2 (NTT form)
    gen_enc_zero(c, sk, true, seed, PUR_RELIN, 0, c->L, key.w(), noise.w(), st);
    if (rt_sync(st)) return dev_fail("hhe_keyset_generate_relin");
    keyset_adopt_relin(ks, key.release());
    return HHE_OK;
}

extern "C" int hhe_keyset_generate_galois(hhe_keyset *ks, const uint64_t *sk, const uint32_t *elts, size_t count, const uint8_t *seed)
{
    if (!ks || !sk || !seed || (count == 0) != (elts == nullptr)) return fail(HHE_ERR_INVALID, "hhe_keyset_generate_galois: bad arguments");
    hhe_ctx *c = ks->ctx;
    HHE_LOCK(c);
    if (int rc = seed_check(c, "hhe_keyset_generate_galois")) return rc;
    const size_t n = c->n, kn = (size_t)c->K * n;
    std::vector<u32> list;
    if (count == 0) {  // GaloisTool::get_elts_all (seal/util/galois.h:131): 3^(2^i), 3^-(2^i), then 2N-1
        u64 pos = 3, neg = nt_invmod(3, 2 * n);
        for (int i = 0; i < c->logn - 1; ++i) {
            list.push_back((u32)pos); list.push_back((u32)neg);
            pos = pos * pos % (2 * n); neg = neg * neg % (2 * n);
        }
        list.push_back((u32)(2 * n - 1));
    } else list.assign(elts, elts + count);
    std::vector<u32> uniq;  // one key per element (get_elts_all repeats 3^(N/4))
    for (u32 e : list) {
        if (!(e & 1) || e >= 2 * n) return fail(HHE_ERR_INVALID, "invalid Galois element");  // nothing has been touched
        if (std::find(uniq.begin(), uniq.end(), e) == uniq.end()) uniq.push_back(e);
    }
    rt_stream st = c->lanes[0].stream;
    DevBuf noise((size_t)(c->L + 1) * kn * 8), scoef(kn * 8);
    u64 *const sg = new_key_of(c, noise.w(), c->L);
    std::vector<u64 *> keys;
    auto drop = [&]() { for (u64 *k : keys) rt_free(k); };
    if (!noise.p || !scoef.p) return dev_fail("hhe_keyset_generate_galois");
    if (rt_d2d(scoef.p, sk, kn * 8, st)) return dev_fail("hhe_keyset_generate_galois");
    k_ntt(plain_ntt(c, scoef.w(), c->K, c->K), true, st);  // s in coefficient form, once
    for (u32 e : uniq) {
        u64 *key = (u64 *)rt_malloc(c->ksk_words() * 8);
        if (!key) { rt_sync(st); drop(); return dev_fail("hhe_keyset_generate_galois"); }
        keys.push_back(key);
        GaloisArgs g = galois_args(c, 1, galois_einv(c, e), scoef.w(), kn, sg, kn);  // new_key = sigma_e(s): GaloisTool::apply_galois between the transforms
        g.count = g.L = c->K;  // one item of K limbs: the key level
        k_galois(g, st);
        k_ntt(plain_ntt(c, sg, c->K, c->K), false, st);
        gen_enc_zero(c, sk, true, seed, PUR_GALOIS, e, c->L, key, noise.w(), st);
    }
    if (rt_sync(st)) { drop(); return dev_fail("hhe_keyset_generate_galois"); }
    for (size_t i = 0; i < uniq.size(); ++i) keyset_adopt_galois(ks, uniq[i], keys[i]);
    return HHE_OK;
}

extern "C" int hhe_keyset_get_relin(const hhe_keyset *ks, uint64_t *ksk)
{
    if (!ks || !ksk) return fail(HHE_ERR_INVALID, "hhe_keyset_get_relin: null argument");
    hhe_ctx *c = ks->ctx;
    HHE_LOCK(c);
    if (!ks->rk) return fail(HHE_ERR_NO_RELIN_KEY, "relinearization key not present");
    rt_stream st = c->lanes[0].stream;
    if (rt_d2h(ksk, ks->rk, c->ksk_words() * 8, st) || rt_sync(st)) return dev_fail("hhe_keyset_get_relin");
    return HHE_OK;
}

extern "C" int hhe_keyset_get_galois(const hhe_keyset *ks, uint32_t elt, uint64_t *ksk)
{
    if (!ks || !ksk) return fail(HHE_ERR_INVALID, "hhe_keyset_get_galois: null argument");
    hhe_ctx *c = ks->ctx;
    HHE_LOCK(c);
    auto it = ks->gk.find(elt);
    if (it == ks->gk.end()) return fail(HHE_ERR_NO_GALOIS_KEY, "Galois key not present");
    rt_stream st = c->lanes[0].stream;
    if (rt_d2h(ksk, it->second, c->ksk_words() * 8, st) || rt_sync(st)) return dev_fail("hhe_keyset_get_galois");
    return HHE_OK;
}

extern "C" int hhe_encrypt(hhe_ctx *c, const uint64_t *pk, const uint64_t *plain, int plain_bcast, const uint8_t *seed, size_t B, uint64_t *out)
{
    HHE_LOCK(c);
    if (!c || !pk || !plain || !seed || !out || B == 0) return fail(HHE_ERR_INVALID, "hhe_encrypt: bad arguments");
    if (int rc = seed_check(c, "hhe_encrypt")) return rc;
    const int L = c->L, K = c->K;
    const size_t n = c->n, ln = (size_t)L * n;
    if (B * 3 * (n >> 6) > ((size_t)1 << 30) || B * 2 * L > ((size_t)1 << 30)) return fail(HHE_ERR_INVALID, "hhe_encrypt: batch too large");
    rt_stream st = c->lanes[0].stream;
    DevBuf e(B * 2 * ln * 8), pkd(2 * ln * 8);
    if (!e.p || !pkd.p) return dev_fail("hhe_encrypt");
    // item b: u (ternary) as 2L residue polynomials straight into out [B][2][L][N], e_0 / e_1 (noise) into e [B][2][L][N]
    PastaXofArgs x = sample_args(c, seed, PUR_ENCRYPT, 0, 0);
    seg_small(x.seg[0], SMP_TERNARY, (int)B, 1, 2 * L, L, out, 2 * ln, 0);
    seg_small(x.seg[1], SMP_NOISE, (int)B, 2, L, L, e.w(), 2 * ln, ln);
    sample_launch(c, x, st);
    for (int k = 0; k < 2; ++k)  // the data-level limbs of the key-level public key, contiguous: [2][L][N]
        if (rt_d2d(pkd.w() + k * ln, pk + (size_t)k * K * n, ln * 8, st)) return dev_fail("hhe_encrypt");
    // c_k = INTT(NTT(u) * pk_k) + e_k
    NttArgs a = plain_ntt(c, out, B * 2 * L, L);
    a.store_op = STORE_MUL; a.mul = pkd.w(); a.mul_cycle = 2 * L; a.mul_item_polys = 1;
    k_ntt(a, false, st);
    k_ntt(plain_ntt(c, out, B * 2 * L, L), true, st);
    k_elt(elt_args(c, out, e.w(), out, B * 2 * L, 0, L), ELT_ADD, st);
    // + the scaled plaintext (multiply_add_plain_with_scaling_variant), as hhe_add_plain does
    AddPlainArgs p = c->apl;
    p.ct = out; p.ct_map = nullptr; p.plain = plain; p.plain_ptrs = nullptr; p.plain_shift = 0; p.out = out; p.B = (int)B;
    p.plain_bcast = plain_bcast != 0; p.subtract = 0; p.negate_ct = 0;
    k_add_plain(p, st);
    if (rt_sync(st)) return dev_fail("hhe_encrypt");
    return HHE_OK;
}
