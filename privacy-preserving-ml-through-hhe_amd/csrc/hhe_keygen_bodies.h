// hhe_keygen_bodies.h -- device bodies of BFV key generation and public-key encryption (KeyGenerator::create_public_key /
// create_relin_keys / create_galois_keys, Encryptor::encrypt as the reference's parties call them: Analyst.cpp:38-93,
// pastahelper.cpp:355-377, sealhelper.cpp:123-142).  Included from hhe_client_bodies.h (it needs keccak_f1600 from there).
//
// THE SAMPLER (stated once more in DESIGN.md section 4; tests/keygen_common.py restates it with hashlib).  The seed is the only
// entropy.  Every random word is a function of the caller's 32 seed bytes and a position:
//
//     SHAKE128( seed[32] || u8 purpose || LE32 elt || LE32 index || u8 kind || LE32 limb || LE32 chunk )      (50 bytes, one block)
//
//   purpose  1 secret key, 2 public key, 3 relinearization key, 4 Galois key (elt = the Galois element, else 0),
//            5 encryption (index = the item of the batch); for key-switching keys index = the digit I
//   kind     1 ternary, 2 noise, 3 uniform
//   limb     uniform: the RNS limb (index of the prime in the context's modulus table).  Ternary and noise polynomials are ONE small
//            polynomial written as residues of every requested prime, limb = 0 -- except the two noise polynomials e_0, e_1 of an
//            encryption, which are told apart here: limb = k
//   chunk    one lane owns one chunk of 64 consecutive coefficients: coefficients 64 * chunk .. 64 * chunk + 63
// The output is squeezed as little-endian 64-bit words w, consumed in order:
//   noise    one word per coefficient, popcount(w & 0x1fffff) - popcount((w >> 21) & 0x1fffff): the centred binomial of SEAL 4.0's
//            sample_poly_cbd, values in [-21, 21]
//   ternary  the 32 two-bit fields of a word from the low end; a field equal to 3 is rejected, the value is field - 1; the first 64
//            accepted values are the chunk (the rest of the last word is dropped)
//   uniform  w & (2^bitlen(q) - 1), accepted when below q; the first 64 accepted values are the chunk
// The squeeze loop is unbounded, as pasta_xof_fields_body's is (acceptance is at least 1/2 per word, 3/4 per field).
// Purpose and element separate the domains: a relinearization key and a Galois key made from one seed must not share a and e
// (their difference would be s^2 - sigma(s) in the clear).
#pragma once

enum { SMP_CHUNK_LOG = 6, SMP_CHUNK = 1 << SMP_CHUNK_LOG };

// residues of one small value at coefficient `pos` of the nres output polynomials
HD void sample_store_small(const PastaXofArgs &a, const SampleSeg &sg, u64 *out, int pos, int v)
{
    const size_t n = (size_t)1 << a.logn;
#pragma unroll 1
    for (int r = 0; r < sg.nres; r++) {
        const u64 q = mod_at(a.mods, sg.mod_base + r % sg.mod_cycle).q;
        out[(size_t)r * n + pos] = v < 0 ? q - (u64)(-v) : (u64)v;
    }
}

HD void sample_body(const PastaXofArgs &a, size_t gid)
{
    if (gid >= (size_t)a.nblocks) return;
    const int logc = a.logn - SMP_CHUNK_LOG;  // chunks per polynomial
    size_t p = gid >> logc;
    const u32 chunk = (u32)(gid & (((size_t)1 << logc) - 1));
    const size_t n0 = (size_t)a.seg[0].nidx * a.seg[0].ncomp;
    const SampleSeg sg = p < n0 ? a.seg[0] : a.seg[1];
    if (p >= n0) p -= n0;
    if (p >= (size_t)sg.nidx * sg.ncomp) return;
    const u32 idx = (u32)(p / sg.ncomp), comp = (u32)(p % sg.ncomp);
    const u32 index = a.first_index + idx;
    const u32 limb = sg.kind == SMP_UNIFORM ? (u32)sg.mod_base + comp : comp;
    u64 *out = sg.out + idx * sg.idx_stride + comp * sg.comp_stride + (size_t)chunk * SMP_CHUNK;

    u64 A[25];
#pragma unroll
    for (int i = 0; i < 25; i++) A[i] = 0;
    A[0] = a.seed[0]; A[1] = a.seed[1]; A[2] = a.seed[2]; A[3] = a.seed[3];
    // bytes 32..39: purpose, elt, index[0..2]; 40..47: index[3], kind, limb, chunk[0..1]; 48..50: chunk[2..3], SHAKE suffix 0x1f
    A[4] = (u64)(a.purpose & 0xff) | ((u64)a.elt << 8) | ((u64)(index & 0xffffff) << 40);
    A[5] = (u64)(index >> 24) | ((u64)sg.kind << 8) | ((u64)limb << 16) | ((u64)(chunk & 0xffff) << 48);
    A[6] = (u64)(chunk >> 16) | ((u64)0x1f << 16);
    A[20] = 0x8000000000000000ULL;  // final pad bit of the 168-byte rate
    keccak_f1600(A);

    u64 q = 0, mask = 0;
    if (sg.kind == SMP_UNIFORM) {
        q = mod_at(a.mods, (int)limb).q;
        int bits = 0;
        for (u64 v = q; v; v >>= 1) ++bits;
        mask = (((u64)1 << bits) - 1);  // q < 2^61
    }
    int count = 0;
    for (;;) {
#pragma unroll
        for (int k = 0; k < 21; k++) {  // one squeezed rate block = 21 little-endian 64-bit words
            const u64 w = A[k];
            if (sg.kind == SMP_UNIFORM) {
                const u64 e = w & mask;
                if (count < SMP_CHUNK && e < q) out[count++] = e;
            } else if (sg.kind == SMP_NOISE) {
                if (count < SMP_CHUNK) {
                    const int v = __builtin_popcountll(w & 0x1fffff) - __builtin_popcountll((w >> 21) & 0x1fffff);
                    sample_store_small(a, sg, out, count++, v);
                }
            } else {
#pragma unroll 1
                for (int f = 0; f < 32 && count < SMP_CHUNK; f++) {
                    const int x = (int)((w >> (2 * f)) & 3);
                    if (x != 3) sample_store_small(a, sg, out, count++, x - 1);
                }
            }
        }
        if (count >= SMP_CHUNK) break;
        keccak_f1600(A);
    }
}

// the XOF launch as the tests-only emulator loops it; the device has one kernel per body (k_pasta_xof picks by mode)
HD void pasta_xof_body(const PastaXofArgs &a, size_t gid)
{
    if (a.mode == XOF_SAMPLE) sample_body(a, gid);
    else pasta_xof_fields_body(a, gid);
}

// ------------------------------------------------------------------ fused epilogue of an encryption of zero under the secret key
// ELT_ENCZ (Encryptor::encrypt_zero_symmetric at the key level, NTT form, and the digit term of
// KeyGenerator::generate_one_kswitch_key): gid over [D][K][N], polynomial p = (digit I, limb j); key words [D][2][K][N] at out:
//   out[I][0][j] = -(out[I][1][j] * s[j] + a[I][j])  (+ (q_sp mod q_I) * new_key[I]  where j == I, with_key set)
// out[I][1] = the uniform polynomial the sampler wrote there, a = the transformed noise [D][K][N] followed (with_key) by new_key [K][N],
// b = s [K][N] (all NTT form); mod_cycle = K.  A public key is D = 1 without new_key.
HD void elt_encz_body(const EltArgs &a, size_t gid)
{
    const size_t n = (size_t)1 << a.logn;
    const size_t p = gid >> a.logn;
    if (p >= (size_t)a.count) return;
    const size_t i = gid & (n - 1);
    const int K = a.mod_cycle;
    const size_t I = p / K, j = p % K;
    const ModDev m = mod_at(a.mods, a.mod_base + (int)j);
    const u64 av = a.out[((I * 2 + 1) * K + j) * n + i];
    u64 r = negmod(addmod(mulmod(av, a.b[j * n + i], m), a.a[gid], m.q), m.q);
    if (a.with_key && j == I) {
        const u64 f = reduce64(mod_at(a.mods, a.mod_base + K - 1).q, m);
        r = addmod(r, mulmod(f, a.a[((size_t)a.count + j) * n + i], m), m.q);
    }
    a.out[((I * 2) * K + j) * n + i] = r;
}
