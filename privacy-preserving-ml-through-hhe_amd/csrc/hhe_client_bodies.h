// hhe_client_bodies.h -- client / analyst ends of the protocol on the device.
// (1) The plain PASTA-3 cipher:
// keystream blocks of pasta::Pasta::gen_keystream (src/pasta/pasta_3_plain.cpp:156-173) for many block counters at once,
// and PASTA::encrypt / decrypt (:9-46) over batches of records.  Two kernels:
//   pasta_xof_fields_body  one lane per block counter: SHAKE128(BE64(nonce) || BE64(counter)) squeezed as big-endian 64-bit
//                     words, masked to bitlen(t), rejection-sampled (:56-84) into the 4 x 512 field elements a block
//                     consumes (per affine layer: first row of matrix 1, of matrix 2, rc 1, rc 2 -- the draw order of
//                     linear_layer, :205-211)
//   pasta_plain_phase one workgroup (256 lanes = 2 state halves x 128 columns) per block counter; the sequential
//                     matrix rows (calculate_row, :86-100) are rebuilt on the fly in LDS (two rows live), never stored.
// The server's end draws the same randomness for its public tables (PastaPlainArgs::mode = PP_MODE_EXPAND): the XOF launch then
// reads a (nonce, counter) pair per lane, and the row phases write every row of the eight matrices and the round constants to
// global memory in the layout of hhe_pasta3_block_randomness, where diag_kernel / bsgs_diag_kernel and the encoder read them.
// Bodies are functions of (block, lane, phase) with a workgroup barrier between phases, so the tests-only CPU emulator
// runs the same code.
#pragma once
#include "hhe_common.h"
#include "hhe_modarith.h"

constexpr int PASTA_RAND_PER_BLOCK = (PASTA_R + 1) * 4 * PASTA_T;  // 2048 field elements per block
constexpr int PASTA_PLAIN_THREADS = 2 * PASTA_T;

// The XOF launch has two bodies behind it: the PASTA field elements below, and the seeded BFV sampler of key generation and
// encryption (hhe_keygen_bodies.h).  One segment of a sampler launch = polynomials of one kind: index first_index + i (i < nidx),
// component c (c < ncomp), polynomial p = i * ncomp + c of the segment, written at out + i * idx_stride + c * comp_stride.
enum XofMode { XOF_PASTA = 0, XOF_SAMPLE = 1 };
enum SampleKind { SMP_TERNARY = 1, SMP_NOISE = 2, SMP_UNIFORM = 3 };
struct SampleSeg {
    int kind;
    int nidx, ncomp;
    int nres;                  // ternary / noise: residue r < nres of the one small polynomial goes to out + r * N, modulus mod_base + r % mod_cycle
    int mod_base, mod_cycle;   // uniform: modulus of component c = mod_base + c (one word range per limb), nres unused
    u64 *out;
    size_t idx_stride, comp_stride;
};
struct PastaXofArgs {
    u64 t, mask, nonce, first_block;
    int nblocks;  // lanes: block counters (XOF_PASTA) or 64-coefficient chunks (XOF_SAMPLE)
    u64 *rand;  // [nblocks][4][4][128]
    int mode;     // XofMode
    const PastaPair *pairs;  // XOF_PASTA, optional (device) [nblocks]: lane gid absorbs pairs[gid] instead of (nonce, first_block + gid)
    // XOF_SAMPLE
    u64 seed[4];  // the 32 seed bytes as little-endian words
    u32 purpose, elt, first_index;
    int logn;
    const ModDev *mods;
    SampleSeg seg[2];  // lanes of seg[0] first; an unused segment has nidx = 0
};
struct PastaPlainArgs {
    u64 t, r_lo, r_hi;
    const u64 *rand;  // [nblocks][4][4][128]
    const u64 *key;   // [256] secret key words (device)
    u64 *ks;          // [nblocks][128] keystream blocks
    int nblocks;
    int mode;         // PlainMode
    // PP_MODE_EXPAND: block = one (nonce, counter) pair of the XOF launch; key and ks are unused
    u64 *mats;        // [nblocks][4][2][128][128] rows of get_random_matrix, as DiagArgs::mats / BsgsDiagArgs::mats are read
    u64 *rcs;         // [nblocks][4][2][128] round constants, as op_encode reads them for BlockTables::rc
};
enum PlainMode { PP_MODE_KEYSTREAM = 0, PP_MODE_EXPAND = 1 };
struct PastaCryptArgs {  // records [S][nwords]; word i of a record uses keystream block i / 128, element i % 128
    u64 t, r_hi;  // r_hi = floor(2^64 / t)
    const u64 *in, *ks;
    u64 *out;
    size_t S, nwords;
    int decrypt;
    size_t ks_stride;  // words between the keystreams of two records; 0: one keystream for all (the reference's fixed nonce)
};

// ------------------------------------------------------------------ SHAKE128 (FIPS 202), one sponge per lane
HD u64 pasta_rol(u64 x, int s) { return (x << s) | (x >> (64 - s)); }
HD u64 pasta_bswap(u64 x)
{
    x = ((x & 0x00ff00ff00ff00ffULL) << 8) | ((x >> 8) & 0x00ff00ff00ff00ffULL);
    x = ((x & 0x0000ffff0000ffffULL) << 16) | ((x >> 16) & 0x0000ffff0000ffffULL);
    return (x << 32) | (x >> 32);
}
// Keccak-f[1600] on 25 named lanes (constant indices only, so the state lives in registers)
HD void keccak_f1600(u64 *A)
{
    constexpr u64 RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
                            0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
                            0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
                            0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
                            0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                            0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    for (int round = 0; round < 24; round++) {
        u64 C0 = A[0] ^ A[5] ^ A[10] ^ A[15] ^ A[20], C1 = A[1] ^ A[6] ^ A[11] ^ A[16] ^ A[21];
        u64 C2 = A[2] ^ A[7] ^ A[12] ^ A[17] ^ A[22], C3 = A[3] ^ A[8] ^ A[13] ^ A[18] ^ A[23];
        u64 C4 = A[4] ^ A[9] ^ A[14] ^ A[19] ^ A[24];
        const u64 D0 = C4 ^ pasta_rol(C1, 1), D1 = C0 ^ pasta_rol(C2, 1), D2 = C1 ^ pasta_rol(C3, 1);
        const u64 D3 = C2 ^ pasta_rol(C4, 1), D4 = C3 ^ pasta_rol(C0, 1);
        // theta + rho + pi: B[y + 5*((2x+3y)%5)] = rol(A[x + 5y] ^ D[x], r[x][y])
        const u64 B0 = A[0] ^ D0, B10 = pasta_rol(A[1] ^ D1, 1), B20 = pasta_rol(A[2] ^ D2, 62);
        const u64 B5 = pasta_rol(A[3] ^ D3, 28), B15 = pasta_rol(A[4] ^ D4, 27);
        const u64 B16 = pasta_rol(A[5] ^ D0, 36), B1 = pasta_rol(A[6] ^ D1, 44), B11 = pasta_rol(A[7] ^ D2, 6);
        const u64 B21 = pasta_rol(A[8] ^ D3, 55), B6 = pasta_rol(A[9] ^ D4, 20);
        const u64 B7 = pasta_rol(A[10] ^ D0, 3), B17 = pasta_rol(A[11] ^ D1, 10), B2 = pasta_rol(A[12] ^ D2, 43);
        const u64 B12 = pasta_rol(A[13] ^ D3, 25), B22 = pasta_rol(A[14] ^ D4, 39);
        const u64 B23 = pasta_rol(A[15] ^ D0, 41), B8 = pasta_rol(A[16] ^ D1, 45), B18 = pasta_rol(A[17] ^ D2, 15);
        const u64 B3 = pasta_rol(A[18] ^ D3, 21), B13 = pasta_rol(A[19] ^ D4, 8);
        const u64 B14 = pasta_rol(A[20] ^ D0, 18), B24 = pasta_rol(A[21] ^ D1, 2), B9 = pasta_rol(A[22] ^ D2, 61);
        const u64 B19 = pasta_rol(A[23] ^ D3, 56), B4 = pasta_rol(A[24] ^ D4, 14);
        // chi
        A[0] = B0 ^ (~B1 & B2); A[1] = B1 ^ (~B2 & B3); A[2] = B2 ^ (~B3 & B4); A[3] = B3 ^ (~B4 & B0); A[4] = B4 ^ (~B0 & B1);
        A[5] = B5 ^ (~B6 & B7); A[6] = B6 ^ (~B7 & B8); A[7] = B7 ^ (~B8 & B9); A[8] = B8 ^ (~B9 & B5); A[9] = B9 ^ (~B5 & B6);
        A[10] = B10 ^ (~B11 & B12); A[11] = B11 ^ (~B12 & B13); A[12] = B12 ^ (~B13 & B14); A[13] = B13 ^ (~B14 & B10); A[14] = B14 ^ (~B10 & B11);
        A[15] = B15 ^ (~B16 & B17); A[16] = B16 ^ (~B17 & B18); A[17] = B17 ^ (~B18 & B19); A[18] = B18 ^ (~B19 & B15); A[19] = B19 ^ (~B15 & B16);
        A[20] = B20 ^ (~B21 & B22); A[21] = B21 ^ (~B22 & B23); A[22] = B22 ^ (~B23 & B24); A[23] = B23 ^ (~B24 & B20); A[24] = B24 ^ (~B20 & B21);
        A[0] ^= RC[round];  // iota
    }
}

// Pasta::init_shake + generate_random_field_element (pasta_3_plain.cpp:56-84) for the whole block: element p of the
// block is drawn with "zero allowed" iff it is a round constant (p % 512 >= 256); first-row elements reject zero (:286-295)
HD void pasta_xof_fields_body(const PastaXofArgs &a, size_t gid)
{
    if (gid >= (size_t)a.nblocks) return;
    u64 A[25];
#pragma unroll
    for (int i = 0; i < 25; i++) A[i] = 0;
    // message = BE64(nonce) || BE64(counter); lanes are little-endian, so each lane is the byte swap of its word
    A[0] = pasta_bswap(a.pairs ? a.pairs[gid].nonce : a.nonce);
    A[1] = pasta_bswap(a.pairs ? a.pairs[gid].counter : a.first_block + gid);
    A[2] = 0x1f;                    // SHAKE domain suffix right after the 16 message bytes
    A[20] = 0x8000000000000000ULL;  // final pad bit of the 168-byte rate
    keccak_f1600(A);
    u64 *out = a.rand + gid * PASTA_RAND_PER_BLOCK;
    int count = 0;
    while (count < PASTA_RAND_PER_BLOCK) {
#pragma unroll
        for (int k = 0; k < 21; k++) {  // one squeezed rate block = 21 big-endian 64-bit words
            const u64 e = pasta_bswap(A[k]) & a.mask;
            const bool rc = (count & 511) >= 256;
            if (count < PASTA_RAND_PER_BLOCK && e < a.t && (rc || e != 0)) out[count++] = e;
        }
        keccak_f1600(A);
    }
}

// ------------------------------------------------------------------ keystream block
// LDS words of one workgroup
constexpr int PP_X = 0, PP_ROW0 = 256, PP_ROW = 512, PP_PROD = 1024, PP_PART = 1024 + 8 * 256, PP_Y = PP_PART + 256;
constexpr int PASTA_PLAIN_LDS = PP_Y + 256;
// phases of one affine layer: 0 = first row, 1..127 = next rows, then after every 8th row two reduction phases;
// the schedule below is a flat list so that GPU kernel and emulator walk it identically
constexpr int PP_STEPS_PER_LAYER = PASTA_T + 2 * (PASTA_T / 8) + 3;  // rows + reductions + (affine/mix, sbox a, sbox b)

// One phase of layer `layer` for lane tau of the block's workgroup.  step: 0..127 row i; 128+2g / 129+2g reduction of
// row group g (rows 8g..8g+7) -- issued by the driver loop right after row 8g+7; PP_* finish phases at the end.
enum { PP_ROWSTEP = 0, PP_RED1 = 1, PP_RED2 = 2, PP_AFFINE = 3, PP_SBOX_A = 4, PP_SBOX_B = 5, PP_INIT = 6, PP_OUT = 7 };
// PP_MODE_EXPAND: the phases of the keystream schedule that touch the matrices, with the state left out.  PP_ROWSTEP i rebuilds row i
// of the layer's two matrices exactly as below (two rows live in LDS) and stores it; PP_AFFINE stores the layer's round constants;
// every other phase is empty.  Rows of one matrix depend on each other only through LDS of the same layer, so a layer of a pair is
// a unit of work of its own (the device launches one workgroup per (pair, layer); the emulator walks the layers of a pair in turn).
HD void pasta_expand_phase(const PastaPlainArgs &a, int block, int tau, int layer, int kind, int i, u64 *lds)
{
    const int h = tau >> 7, j = tau & (PASTA_T - 1);
    const u64 *rnd = a.rand + ((size_t)block * (PASTA_R + 1) + layer) * 4 * PASTA_T;
    if (kind == PP_ROWSTEP) {
        ModDev m;
        m.q = a.t; m.r_lo = a.r_lo; m.r_hi = a.r_hi;
        u64 v;
        if (i == 0) {
            v = rnd[h * PASTA_T + j];
            lds[PP_ROW0 + tau] = v;
        } else {  // calculate_row (:86-100)
            const u64 *prev = lds + PP_ROW + ((i - 1) & 1) * 256 + h * PASTA_T;
            v = mulmod(lds[PP_ROW0 + tau], prev[PASTA_T - 1], m);
            if (j) v = addmod(v, prev[j - 1], a.t);
        }
        lds[PP_ROW + (i & 1) * 256 + tau] = v;
        a.mats[((((size_t)block * (PASTA_R + 1) + layer) * 2 + h) * PASTA_T + i) * PASTA_T + j] = v;
    } else if (kind == PP_AFFINE) {
        a.rcs[((size_t)block * (PASTA_R + 1) + layer) * 2 * PASTA_T + tau] = rnd[2 * PASTA_T + tau];
    }
}
HD void pasta_plain_phase(const PastaPlainArgs &a, int block, int tau, int layer, int kind, int i, u64 *lds)
{
    if (a.mode == PP_MODE_EXPAND) { pasta_expand_phase(a, block, tau, layer, kind, i, lds); return; }
    ModDev m;
    m.q = a.t; m.r_lo = a.r_lo; m.r_hi = a.r_hi;
    const u64 t = a.t;
    const int h = tau >> 7, j = tau & (PASTA_T - 1);
    const u64 *rnd = a.rand + ((size_t)block * (PASTA_R + 1) + layer) * 4 * PASTA_T;
    switch (kind) {
    case PP_INIT: lds[PP_X + tau] = a.key[tau]; break;  // state1_ = key[0..128), state2_ = key[128..256) (:160-163)
    case PP_ROWSTEP: {  // Pasta::matmul (:262-279): row i of both matrices and its products with the state
        u64 v;
        if (i == 0) {
            v = rnd[h * PASTA_T + j];
            lds[PP_ROW0 + tau] = v;
        } else {  // calculate_row (:86-100): first_row[j] * prev[127] + prev[j-1]
            const u64 *prev = lds + PP_ROW + ((i - 1) & 1) * 256 + h * PASTA_T;
            v = mulmod(lds[PP_ROW0 + tau], prev[PASTA_T - 1], m);
            if (j) v = addmod(v, prev[j - 1], t);
        }
        lds[PP_ROW + (i & 1) * 256 + tau] = v;
        lds[PP_PROD + (i & 7) * 256 + tau] = mulmod(v, lds[PP_X + tau], m);
        break;
    }
    case PP_RED1: {  // 16 sums (8 rows x 2 halves) of 128 products: 16 lanes per sum, 8 products each
        const int s = tau >> 4, p = tau & 15, r = s >> 1, hh = s & 1;
        const u64 *pr = lds + PP_PROD + r * 256 + hh * PASTA_T + p * 8;
        u64 acc = 0;
        for (int k = 0; k < 8; k++) acc = addmod(acc, pr[k], t);
        lds[PP_PART + tau] = acc;
        break;
    }
    case PP_RED2:
        if (tau < 16) {  // i = index of the group's first row
            const int r = tau >> 1, hh = tau & 1;
            u64 acc = 0;
            for (int k = 0; k < 16; k++) acc = addmod(acc, lds[PP_PART + tau * 16 + k], t);
            lds[PP_Y + hh * PASTA_T + i + r] = acc;
        }
        break;
    case PP_AFFINE: {  // add_rc (:205-211) + mix (:246-257)
        const u64 s1 = addmod(lds[PP_Y + j], rnd[2 * PASTA_T + j], t), s2 = addmod(lds[PP_Y + PASTA_T + j], rnd[3 * PASTA_T + j], t);
        const u64 sum = addmod(s1, s2, t);
        lds[PP_X + tau] = addmod(h ? s2 : s1, sum, t);
        break;
    }
    case PP_SBOX_A:  // sbox_feistel (:229-240) / sbox_cube (:218-225) into Y, copied back by PP_SBOX_B
        if (layer == PASTA_R - 1) {
            const u64 x = lds[PP_X + tau];
            lds[PP_Y + tau] = mulmod(mulmod(x, x, m), x, m);
        } else {
            const u64 x = lds[PP_X + tau];
            lds[PP_Y + tau] = j ? addmod(x, mulmod(lds[PP_X + tau - 1], lds[PP_X + tau - 1], m), t) : x;
        }
        break;
    case PP_SBOX_B: lds[PP_X + tau] = lds[PP_Y + tau]; break;
    case PP_OUT:
        if (tau < PASTA_T) a.ks[(size_t)block * PASTA_T + tau] = lds[PP_X + tau];  // gen_keystream returns state1_ (:172)
        break;
    }
}
// the phase list of one block, shared by the kernel and the emulator: F(kind, layer, i) is called once per phase and
// must run the phase for all 256 lanes followed by a barrier
template <class F> HD void pasta_plain_schedule(F &&f)
{
    f(PP_INIT, 0, 0);
    for (int layer = 0; layer <= PASTA_R; layer++) {
        for (int i = 0; i < PASTA_T; i++) {
            f(PP_ROWSTEP, layer, i);
            if ((i & 7) == 7) { f(PP_RED1, layer, i - 7); f(PP_RED2, layer, i - 7); }
        }
        f(PP_AFFINE, layer, 0);
        if (layer < PASTA_R) { f(PP_SBOX_A, layer, 0); f(PP_SBOX_B, layer, 0); }
    }
    f(PP_OUT, PASTA_R, 0);
}
// the phases of one layer that PP_MODE_EXPAND does anything in: what a device workgroup of that mode walks
template <class F> HD void pasta_expand_schedule(int layer, F &&f)
{
    for (int i = 0; i < PASTA_T; i++) f(PP_ROWSTEP, layer, i);
    f(PP_AFFINE, layer, 0);
}

// PASTA::encrypt / decrypt (pasta_3_plain.cpp:9-46), element-wise over [S][nwords], literally: encrypt
// (v + ks) % t on 64-bit words, decrypt v - ks with one conditional + t (no reduction of an input that is not below t)
HD void pasta_crypt_body(const PastaCryptArgs &a, size_t gid)
{
    if (gid >= a.S * a.nwords) return;
    const size_t i = gid % a.nwords;
    const u64 k = a.ks[(gid / a.nwords) * a.ks_stride + i];
    u64 v = a.in[gid];
    if (a.decrypt) {
        if (k > v) v += a.t;
        a.out[gid] = v - k;
    } else {
        ModDev m;
        m.q = a.t; m.r_hi = a.r_hi;
        a.out[gid] = reduce64(v + k, m);
    }
}

// ------------------------------------------------------------------ analyst side: batched BFV decryption
// Decryptor::bfv_decrypt (seal/decryptor.h:70): phase = c0 + c1*s per data prime (NTT launches with the
// secret key as STORE_MUL operand), then RNSTool::decrypt_scale_and_round (seal/util/rns.h:230-243): multiply by
// t*gamma, fast base conversion q -> {t, gamma}, multiply by -Q^-1, correct by the centred gamma residue, times gamma^-1.
struct DecryptArgs {
    const ModDev *mods;
    const u64 *ct;   // [B][2][L][N]; c0 is read here
    const u64 *c1s;  // [B][L][N]  c1 * s, coefficient form
    u64 *plain;      // [B][N] coefficients mod t
    int logn, L;
    size_t B;
    u64 t, t_rlo, t_rhi, gamma, g_rlo, g_rhi;
    u64 neg_inv_q_t, neg_inv_q_g, inv_g_t;
    u64 cj[HHE_MAXL];  // t*gamma * (Q/q_j)^-1 mod q_j                  | noise mode: the words of Q = q_0 ... q_{L-1}, zero above
    u64 pt[HHE_MAXL];  // Q/q_j mod t                                   | noise mode: the words of (Q+1)/2
    u64 pg[HHE_MAXL];  // Q/q_j mod gamma                               | noise mode: t mod q_j
    // DEC_NOISE (noise_body below): the launch writes no plaintext; size = polynomials per item of ct (c1s then holds c1 s + c2 s^2),
    // pairs = the context's pair table (hhe_ctx::d_moddown: q_m^-1 mod q_j and its Shoup quotient at mod_down_pair(m, j)),
    // bits [B] = the largest significant-bit count of the items' centred noise coefficients (cleared by the caller)
    int mode, size;
    const u64 *pairs;
    u32 *bits;
};
enum DecryptMode { DEC_ROUND = 0, DEC_NOISE = 1 };
HD void decrypt_scale_body(const DecryptArgs &a, size_t gid)
{
    const size_t n = (size_t)1 << a.logn;
    if (gid >= a.B * n) return;
    const size_t b = gid >> a.logn, i = gid & (n - 1);
    ModDev mt, mg;
    mt.q = a.t; mt.r_lo = a.t_rlo; mt.r_hi = a.t_rhi;
    mg.q = a.gamma; mg.r_lo = a.g_rlo; mg.r_hi = a.g_rhi;
    Acc128 st = {0, 0}, sg = {0, 0};
    for (int j = 0; j < a.L; j++) {
        const ModDev m = mod_at(a.mods, j);
        const u64 ph = addmod(a.ct[(b * 2 * a.L + j) * n + i], a.c1s[(b * a.L + j) * n + i], m.q);
        const u64 v = mulmod(ph, a.cj[j], m);
        acc_mac(st, reduce64(v, mt), a.pt[j]);
        acc_mac(sg, reduce64(v, mg), a.pg[j]);
    }
    u64 vt = mulmod(barrett128(st.lo, st.hi, mt), a.neg_inv_q_t, mt);
    const u64 vg = mulmod(barrett128(sg.lo, sg.hi, mg), a.neg_inv_q_g, mg);
    u64 d;
    if (vg > (a.gamma >> 1)) d = addmod(vt, reduce64(a.gamma - vg, mt), a.t);
    else d = submod(vt, reduce64(vg, mt), a.t);
    a.plain[gid] = mulmod(d, a.inv_g_t, mt);
}

// ------------------------------------------------------------------ invariant noise budget (DecryptArgs::mode = DEC_NOISE)
// Decryptor::invariant_noise_budget (seal/decryptor.h:103): the largest centred magnitude of t * (c0 + c1 s [+ c2 s^2]) mod Q over the
// coefficients of an item, as a bit count.  One lane owns one coefficient.  Its column v_j = phase_j * (t mod q_j) is converted to mixed
// radix from the top prime down -- the loop of mod_down_body without the rounding term:
//   e_m = v_m;   v_j <- (v_j - (e_m mod q_j)) * q_m^-1 mod q_j   for j < m        (e_m may be far above q_j: a full reduction)
// so that x = e_{L-1} + q_{L-1} (e_{L-2} + ... + q_1 e_0) is the representative in [0, Q).  Horner from e_0 upward builds it IN the column:
// after step m the integer below q_0 ... q_m < 2^(64 (m + 1)) fills words 0 .. m, whose digits have been used, and the digits above m are
// still there.  x >= (Q+1)/2 is replaced by Q - x, and only the bit count 64 k + 64 - clz(top non-zero word) leaves the lane: the
// largest bit count is the bit count of the largest magnitude.
// LIM > 0: the column in registers, every index a compile-time constant.  LIM = 0: any limb count, the column at col[j * cs] (the
// lane's own words of the workgroup's LDS block, nobody else touches them: no barrier; in the tests-only emulator a local array).
struct NoisePair { u64 inv, inv_s; };
HD NoisePair noise_pair_at(const u64 *tab, int m, int j)
{
    NoisePair c;
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) u64 *p = (const __attribute__((address_space(4))) u64 *)(tab + mod_down_pair(m, j));
#else
    const u64 *p = tab + mod_down_pair(m, j);
#endif
    c.inv = p[0]; c.inv_s = p[1];
    return c;
}
HD u64 noise_word(const DecryptArgs &a, size_t b, size_t i, int j)
{
    const ModDev m = mod_at(a.mods, j);
    const u64 ph = addmod(a.ct[((b * a.size * a.L + j) << a.logn) + i], a.c1s[((b * a.L + j) << a.logn) + i], m.q);
    return mulmod(ph, a.pg[j], m);
}
HD u64 noise_digit_step(u64 vj, u64 e, const ModDev &mj, const NoisePair &c)
{
    return shoup_mul(submod(vj, reduce64(e, mj), mj.q), c.inv, c.inv_s, mj.q);
}
// one word of X * q + carry; the new carry is below q (hi <= q - 1 with the carry-out of the low sum: (2^64 - 1) q + 2^64 - 1 < 2^64 (q + 1))
HD u64 noise_horner_word(u64 &x, u64 q, u64 carry)
{
    const u64 lo = x * q, hi = mulhi64(x, q);
    x = lo + carry;
    return hi + (x < lo);
}
// significant bits of the lane's coefficient; 0 for a lane past the batch
template <int LIM> HD u32 noise_bits(const DecryptArgs &a, size_t gid, u64 *col, int cs)
{
    const size_t n = (size_t)1 << a.logn;
    if (gid >= a.B * n) return 0;
    const size_t b = gid >> a.logn, i = gid & (n - 1);
    u32 bits = 0;
    if constexpr (LIM > 0) {
        u64 x[LIM];
#pragma unroll
        for (int j = 0; j < LIM; j++) x[j] = noise_word(a, b, i, j);
#pragma unroll
        for (int m = LIM - 1; m >= 1; m--)
#pragma unroll
            for (int j = 0; j < m; j++) x[j] = noise_digit_step(x[j], x[m], mod_at(a.mods, j), noise_pair_at(a.pairs, m, j));
#pragma unroll
        for (int m = 1; m < LIM; m++) {
            const u64 qm = mod_at(a.mods, m).q;
            u64 carry = x[m];
#pragma unroll
            for (int w = 0; w < m; w++) carry = noise_horner_word(x[w], qm, carry);
            x[m] = carry;
        }
        bool ge = true, open = true;
#pragma unroll
        for (int w = LIM - 1; w >= 0; w--) {
            const u64 h = a.pt[w];
            if (open && x[w] != h) { ge = x[w] > h; open = false; }
        }
        u64 borrow = 0;
#pragma unroll
        for (int w = 0; w < LIM; w++) {
            const u64 qw = a.cj[w], d = qw - x[w], y = ge ? d - borrow : x[w];
            borrow = (u64)(qw < x[w]) | (u64)(d < borrow);
            if (y) bits = 64u * w + 64u - (u32)__builtin_clzll(y);
        }
    } else {
        const int L = a.L;
        for (int j = 0; j < L; j++) col[j * cs] = noise_word(a, b, i, j);
        for (int m = L - 1; m >= 1; m--) {
            const u64 e = col[m * cs];
            for (int j = 0; j < m; j++) col[j * cs] = noise_digit_step(col[j * cs], e, mod_at(a.mods, j), noise_pair_at(a.pairs, m, j));
        }
        for (int m = 1; m < L; m++) {
            const u64 qm = mod_at(a.mods, m).q;
            u64 carry = col[m * cs];
            for (int w = 0; w < m; w++) {
                u64 x = col[w * cs];
                carry = noise_horner_word(x, qm, carry);
                col[w * cs] = x;
            }
            col[m * cs] = carry;
        }
        bool ge = true;
        for (int w = L - 1; w >= 0; w--) {
            const u64 h = a.pt[w], x = col[w * cs];
            if (x != h) { ge = x > h; break; }
        }
        u64 borrow = 0;
        for (int w = 0; w < L; w++) {
            const u64 qw = a.cj[w], x = col[w * cs], d = qw - x, y = ge ? d - borrow : x;
            borrow = (u64)(qw < x) | (u64)(d < borrow);
            if (y) bits = 64u * w + 64u - (u32)__builtin_clzll(y);
        }
    }
    return bits;
}
// bits[b] = max(bits[b], the lane's count).  On the device the 64 lanes of a wave share an item from N = 64 on (a launch covers B * N lanes
// and a workgroup is a multiple of 64): a wave max, then one 32-bit atomic max per wave.  The tests-only emulator loops the lanes
// under OpenMP: a compare-exchange max on the same word.
HD void noise_commit(const DecryptArgs &a, size_t gid, u32 bits)
{
    const bool live = gid < (a.B << a.logn);
    const size_t b = gid >> a.logn;
#if defined(__HIP_DEVICE_COMPILE__)
    if (a.logn >= 6) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u32 o = (u32)__shfl_xor((int)bits, off, 64);
            bits = o > bits ? o : bits;
        }
        if (live && (threadIdx.x & 63) == 0 && bits) atomicMax(a.bits + b, bits);
    } else if (live && bits) atomicMax(a.bits + b, bits);
#else
    if (!live) return;
    u32 cur = __atomic_load_n(a.bits + b, __ATOMIC_RELAXED);
    while (cur < bits && !__atomic_compare_exchange_n(a.bits + b, &cur, bits, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
#endif
}
constexpr int NOISE_REGS = 8;  // = MOD_DOWN_REGS: the limb counts with a register form
// the form a launch of L limbs takes, as k_decrypt_round picks the kernel on the device
HD void noise_any(const DecryptArgs &a, size_t gid)
{
    u64 col[HHE_MAXL];
    u32 bits;
    switch (a.L <= NOISE_REGS ? a.L : 0) {
    case 1: bits = noise_bits<1>(a, gid, nullptr, 0); break;
    case 2: bits = noise_bits<2>(a, gid, nullptr, 0); break;
    case 3: bits = noise_bits<3>(a, gid, nullptr, 0); break;
    case 4: bits = noise_bits<4>(a, gid, nullptr, 0); break;
    case 5: bits = noise_bits<5>(a, gid, nullptr, 0); break;
    case 6: bits = noise_bits<6>(a, gid, nullptr, 0); break;
    case 7: bits = noise_bits<7>(a, gid, nullptr, 0); break;
    case 8: bits = noise_bits<8>(a, gid, nullptr, 0); break;
    default: bits = noise_bits<0>(a, gid, col, 1); break;
    }
    noise_commit(a, gid, bits);
}
// the launch as the tests-only emulator loops it; on the device every form of either mode is a kernel of its own
HD void decrypt_round_body(const DecryptArgs &a, size_t gid)
{
    if (a.mode == DEC_NOISE) noise_any(a, gid);
    else decrypt_scale_body(a, gid);
}
// BatchEncoder::decode (seal/batchencoder.h:282): after the forward NTT mod t, slot i = ntt[index_map[i]]
struct DecodeArgs {
    const u64 *in;  // [B][N] NTT mod t of the plaintext
    u64 *vals;      // [B][N]
    const u32 *slot_map;
    int logn;
    size_t B;
};
HD void decode_gather_body(const DecodeArgs &a, size_t gid)
{
    const size_t n = (size_t)1 << a.logn;
    if (gid >= a.B * n) return;
    const size_t b = gid >> a.logn, i = gid & (n - 1);
    a.vals[gid] = a.in[b * n + a.slot_map[i]];
}

// the seeded BFV sampler and the dispatch of the XOF launch between its two bodies
#include "hhe_keygen_bodies.h"
