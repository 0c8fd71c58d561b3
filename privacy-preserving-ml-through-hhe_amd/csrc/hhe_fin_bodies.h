// hhe_fin_bodies.h -- the finishing pass res = Enc(c_b) - KS of a transciphering call with ONE workgroup per item
// (fin_item_kernel): the item's plaintext never leaves LDS.  Written like hhe_kernel_bodies.h as per-thread phase functions of
// (item, thread), so a CPU program can loop them (tests/cpp/fin_item_main.cpp); nothing here is a CPU fallback for the product.
//
// The transform is mod t, and where t < 2^30 every value of it fits 32 bits: N words of 4 bytes are 128 KiB at N = 2^15, which
// one workgroup may hold (the CU has 160 KiB).  Phases, a barrier after each:
//   clear    N u32 words of LDS
//   encode   the item's `count` words, reduced mod t and multiplied by N^-1, go to their coefficient slots (BatchEncoder::encode)
//   rounds   the whole inverse negacyclic transform (Gentleman-Sande, SEAL's order: the stages ntt_body_round runs in two passes) in
//            register rounds of radix 8 from stage log N - 1 down, a shorter last round where log N is no multiple of 3
//   store    the add_plain epilogue of the two-pass kernels (fin_store_fetch / fin_store_vals), fed from LDS; in the instantiation
//            with the 32-bit scaling (below) the c0 half only, the c1 half going out in slices in front of the other phases
// The transform is linear, so the N^-1 scaling is applied to the at most 128 words that enter it instead of the N that leave it.
//
// 32-bit arithmetic: Harvey's lazy butterflies with values in [0, 2t).  X' = X + Y < 4t is folded below 2t; Y' = (X + 2t - Y) w
// takes an operand below 4t and leaves the Shoup product in [0, 2t) for ANY 32-bit operand (ws = floor(w 2^32 / t), w < t).  4t must
// not wrap 32 bits: the kernel runs for t < 2^30 (fin_item_ok).  The fully reduced coefficient is unique, so the words written are
// those of the two-pass kernels, bit for bit.
//
// LDS layout: coefficient x lives at word fin_lds_at(x), x with its low five bits XORed by a function of bits 5..7 -- no padding, and
// within an aligned group of 32 words a permutation.  ds_read_b32 / ds_write_b32 serve 32 lanes per cycle from 32 dword banks
// (bank = word index mod 32), so a half-wave must touch 32 distinct values of the low five bits.  Which bits of x vary over 32
// consecutive lanes of a round depends on the round's butterfly distance 2^LO:
//   LO = 0 (8 consecutive points per lane):  bits 3..7      LO = 3:  bits 0..2 and 6..7      LO >= 5:  bits 0..4
// With bank bits (b0..b4) = (x0^x5, x1^x6, x2^x7, x3^x6, x4^x7) each of these sets maps onto all 32 banks; LO takes no other value
// (log N - 3r).  A coefficient pair (x, x + 1), x even, stays in one aligned 8-byte word, swapped where x5 is set.
#pragma once
#include "hhe_kernel_bodies.h"

constexpr int FIN_ITEM_THREADS = 1024;   // 16 waves: at most 128 VGPRs

HD u32 fin_lds_at(u32 x)
{
    const u32 h = x >> 5;
    return x ^ (h & 7) ^ ((h & 6) << 2);
}
HD u32 mulhi32(u32 a, u32 b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (u32)(((u64)a * b) >> 32);
#endif
}
// x*w mod t in [0,2t) for any x < 2^32, with ws = floor(w * 2^32 / t), w < t < 2^31
HD u32 shoup32_lazy(u32 x, u32 w, u32 ws, u32 t) { return x * w - mulhi32(x, ws) * t; }
// x >= c ? x - c : x for x + c < 2^32: a subtraction and an unsigned minimum
HD u32 csub32(u32 x, u32 c)
{
    const u32 d = x - c;
    return d < x ? d : x;
}

struct FinItemConsts { const u32 *itw; u32 t, t2; };
HD FinItemConsts fin_item_consts(const NttArgs &a)
{
    FinItemConsts k;
    k.itw = ld_const(&a.fin->itw);
    k.t = (u32)ld_const(&a.fin->t);
    k.t2 = k.t << 1;
    return k;
}

template <int T> HD void fin_item_clear(const NttArgs &a, int tid, u32 *lds)
{
    const int n = 1 << a.logn;
    for (int i = 4 * tid; i < n; i += 4 * T) { lds[i] = 0; lds[i + 1] = 0; lds[i + 2] = 0; lds[i + 3] = 0; }
}
// word s < count of the item, reduced as encode_scatter_body / ld2_encode reduce it and scaled by N^-1, at coefficient slot_map[s]
template <int T> HD void fin_item_encode(const NttArgs &a, int item, int tid, u32 *lds)
{
    const ModDev mt = mod_at_u(a.mods, a.mod_base);
    const u32 *smap = ld_const(&a.fin->slot_map);
    const int cnt = ld_const(&a.fin->count);
    const u64 t = ld_const(&a.fin->t);
    const u64 *vals = a.src + (size_t)item * a.src_item_stride;
    for (int s = tid; s < cnt; s += T) {
        u64 x = vals[s];
        if (x >= t) x %= t;
        lds[fin_lds_at(smap[s])] = (u32)shoup_mul(x, mt.ninv, mt.ninv_s, t);
    }
}
// one register round: stages S0 .. S0 + RHO - 1 of the 2^LOGN-point inverse transform, highest first (ntt_body_round's inverse
// branch for a tile that is the whole polynomial: M = N, one lane, P = 1)
template <int LOGN, int S0, int RHO, int T> HD void fin_item_round(const NttArgs &a, int tid, u32 *lds)
{
    const FinItemConsts c = fin_item_consts(a);
    const gptr W = as_global(reinterpret_cast<const u64 *>(c.itw));  // (w, ws) with one 8-byte load
    constexpr int LO_BITS = LOGN - S0 - RHO;
    constexpr int RAD = 1 << RHO;
    constexpr int GROUPS = 1 << (LOGN - RHO);
    for (int grp = tid; grp < GROUPS; grp += T) {
        const int hi = grp >> LO_BITS;
        const int lo = grp & ((1 << LO_BITS) - 1);
        const int x0 = (hi << (LOGN - S0)) + lo;
        const int tb = (1 << S0) + hi;
        u32 v[RAD];
#pragma unroll
        for (int k = 0; k < RAD; k++) v[k] = lds[fin_lds_at((u32)(x0 + (k << LO_BITS)))];
#pragma unroll
        for (int u = RHO - 1; u >= 0; u--) {
            const int half = 1 << (RHO - 1 - u);
#pragma unroll
            for (int b = 0; b < (1 << u); b++) {
                const u64 tw = W[(tb << u) + b];
                const u32 w = (u32)tw, ws = (u32)(tw >> 32);
#pragma unroll
                for (int j = 0; j < half; j++) {
                    const int k0 = b * 2 * half + j, k1 = k0 + half;
                    const u32 x = v[k0], y = v[k1];
                    v[k0] = csub32(x + y, c.t2);
                    v[k1] = shoup32_lazy(x + c.t2 - y, w, ws, c.t);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RAD; k++) lds[fin_lds_at((u32)(x0 + (k << LO_BITS)))] = v[k];
    }
}
// all rounds of one thread between two barriers are one call: ROUND counts from 0 (stages LOGN-3 .. LOGN-1) up
template <int LOGN> struct FinItemSched {
    static constexpr int R = (LOGN + 2) / 3;
    static constexpr int s0(int r) { return LOGN - 3 * (r + 1) > 0 ? LOGN - 3 * (r + 1) : 0; }
    static constexpr int rho(int r) { return LOGN - 3 * r >= 3 ? 3 : LOGN - 3 * r; }
};

// The 32-bit scaling (FinArgs::scale32; fin_scale32_ok: t < 2^30 and every data prime above t).  A coefficient m < t is a u32, so the
// two values add_plain derives from it need no 128-bit product:
//   fix = floor((m (Q mod t) + thr) / t):  est = mulhi32(m, q_mod_t_s) is the quotient of m (Q mod t) by t or one below it (Shoup,
//         q_mod_t_s = floor((Q mod t) 2^32 / t)), so m (Q mod t) - est t lies in [0, 2t) and is exact in 32 bits; with thr = (t+1)/2
//         added the sum is below 2.5 t + 1 < 2^32, and each of two conditional subtractions of t that is taken adds 1 to est.
//   (m delta_j + fix) mod q_j:  H = floor(m delta_s / 2^64) with delta_s = floor(delta_j 2^64 / q_j) -- for a 32-bit m that is
//         (m hi32(delta_s) + mulhi32(m, lo32(delta_s))) >> 32, exactly -- leaves m delta_j - H q_j in [0, 2 q_j) (low 64 bits; q_j < 2^61);
//         a conditional subtraction, + fix (fix < t < q_j), and another one give the canonical residue.
// Both are the words plain_fix / plain_scaled return (hhe_kernel_bodies.h), which keep the shared 128-bit definition everywhere else.
struct FinScale32 { u32 t, q_mod_t, q_mod_t_s, thr; };
HD FinScale32 fin_scale32_consts(const FinArgs *f)
{
    const FinScale32 s = {(u32)ld_const(&f->t), (u32)ld_const(&f->q_mod_t), ld_const(&f->q_mod_t_s), (u32)ld_const(&f->thr)};
    return s;
}
HD u32 plain_fix32(const FinScale32 &s, u32 m)
{
    u32 fix = mulhi32(m, s.q_mod_t_s);
    u32 r = m * s.q_mod_t - fix * s.t + s.thr;
#if defined(HHE_RANGE_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    if ((u64)m * s.q_mod_t - (u64)fix * s.t >= 2 * (u64)s.t) hhe_range_violation("32-bit fix: remainder not below 2t");
#endif
    u32 d = r - s.t;
    if (d < r) { r = d; fix++; }
    d = r - s.t;
    if (d < r) { r = d; fix++; }
    return fix;
}
HD u64 plain_scaled32(u32 m, u32 fix, u64 delta, u64 delta_s, u64 q)
{
    const u64 h = ((u64)m * (u32)(delta_s >> 32) + mulhi32(m, (u32)delta_s)) >> 32;
    u64 r = (u64)m * delta - h * q;
#if defined(HHE_RANGE_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    if (r >= 2 * q) hhe_range_violation("32-bit scaling: remainder not below 2q");
#endif
    r = r >= q ? r - q : r;
    r += fix;
    return r >= q ? r - q : r;
}

// the epilogue: coefficient pairs (gi, gi + 1) out of LDS, the operands of G pairs in flight before the first store
#ifndef FIN_ITEM_G
#define FIN_ITEM_G 2
#endif
// In the 32-bit instantiation out[b][1][j] = -c1[j], which needs nothing from LDS, is written by fin_item_c1 in slices ahead of the
// other phases (FIN_ITEM_C1_EARLY 1), and the store phase writes c0 only; 0 leaves both halves to the store phase (A/B builds).
#ifndef FIN_ITEM_C1_EARLY
#define FIN_ITEM_C1_EARLY 1
#endif
// the c0 word as one lazy sum with two conditional subtractions (fin_word32; FIN_ITEM_LAZY 0: negmod, plain_scaled32, addmod: A/B builds)
#ifndef FIN_ITEM_LAZY
#define FIN_ITEM_LAZY 1
#endif
// word `w` of an array whose base is uniform over the workgroup, for w < 2^29: the byte offset is formed in 32 bits, so the access
// takes a scalar base and ONE offset register where a 64-bit index costs a 64-bit vector address per access
HD gptr fin_at(gptr base, u32 w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (gptr)((const __attribute__((address_space(1))) char *)base + (w << 3));
#else
    return base + w;
#endif
}
HD u64 *fin_at(u64 *base, u32 w) { return reinterpret_cast<u64 *>(reinterpret_cast<char *>(base) + (w << 3)); }
// The item's keystream [2][L][N].  The table entry is uniform over the workgroup (the item is the workgroup) and constant while
// the kernel runs, so it is read through the constant address space: one scalar load per kernel, handed to every phase.
HD gptr fin_item_ks(const NttArgs &a, int item)
{
    return as_global(a.mul_ptrs ? ld_const(&a.mul_ptrs[item]) : a.mul + ((size_t)item * 2 * a.L << a.logn));
}
// -c0 + (m delta_j + fix) mod q_j with ONE reduction.  With H as in plain_scaled32, r = m delta_j - H q_j lies in [0, 2 q_j); c0 is
// a residue, so q_j - c0 lies in (0, q_j] and needs no test for zero; fix < t < q_j (fin_scale32_ok).  The sum
//   u = (q_j - c0) + r + fix  lies in (0, 3 q_j + t), below 4 q_j < 2^63 (q_j < 2^61): no 64-bit carry,
// and u - 2 q_j where u >= 2 q_j, then u - q_j where u >= q_j, leave the canonical residue: the word
// addmod(negmod(c0), plain_scaled32(m, fix)) of the three-step form, two conditional subtractions instead of four.
HD u64 fin_word32(u64 c0, u32 m, u32 fix, u64 delta, u64 delta_s, u64 q)
{
    const u64 h = ((u64)m * (u32)(delta_s >> 32) + mulhi32(m, (u32)delta_s)) >> 32;
    const u64 r = (u64)m * delta - h * q;
    u64 u = (q - c0) + r + fix;
#if defined(HHE_RANGE_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    if (r >= 2 * q) hhe_range_violation("fused 32-bit scaling: remainder not below 2q");
    if (c0 >= q || fix >= q || u == 0 || u >= 4 * q) hhe_range_violation("fused 32-bit scaling: lazy sum not in (0, 4q)");
#endif
    const u64 q2 = q << 1;
    u = u >= q2 ? u - q2 : u;
    return u >= q ? u - q : u;
}
// limb j of one pair with the 32-bit scaling: what fin_store_limb writes; C1: the c1 half too.  `o` is the item's output [2][L][N]:
// an address is that base, uniform over the workgroup, plus a 32-bit offset (fin_at; 2 L N <= 2^21 words)
template <bool C1> HD void fin_store_limb32(const NttArgs &a, u64 *o, u32 n, u32 gi, int j, const u32 *mv, const u32 *fix, U2 c0, U2 c1)
{
    const u64 q = mod_at_u(a.mods, j).q;
    const u64 d = ld_const(&a.fin->delta[j]), ds = ld_const(&a.fin->delta_s[j]);
    U2 o0;
#if FIN_ITEM_LAZY
    o0.a = fin_word32(c0.a, mv[0], fix[0], d, ds, q);
    o0.b = fin_word32(c0.b, mv[1], fix[1], d, ds, q);
#else
    o0.a = addmod(negmod(c0.a, q), plain_scaled32(mv[0], fix[0], d, ds, q), q);
    o0.b = addmod(negmod(c0.b, q), plain_scaled32(mv[1], fix[1], d, ds, q), q);
#endif
    st2_stream(fin_at(o, (u32)j * n + gi), o0);
    if (C1) st2_stream(fin_at(o, (u32)(a.L + j) * n + gi), U2{negmod(c1.a, q), negmod(c1.b, q)});
}
// SCALE32 = false (the default) is the shared definition: fin_store_fetch / fin_store_vals, both halves written here.
// kp = fin_item_ks(a, item), which the 32-bit instantiation reads through
template <int T, bool SCALE32 = false, bool C1 = !FIN_ITEM_C1_EARLY>
HD void fin_item_store(const NttArgs &a, int item, int tid, const u32 *lds, gptr kp)
{
    constexpr int G = FIN_ITEM_G;
    NttGeom g = {};
    g.n = 1 << a.logn;
    g.poly = item;
    const u32 t = (u32)ld_const(&a.fin->t);
    const int E2 = g.n >> 1;  // a multiple of T for every N >= 2048; guarded below
    if constexpr (!SCALE32) {
        for (int e0 = tid; e0 < E2; e0 += G * T) {
            FinPre pre[G];
            int gi[G];
#pragma unroll
            for (int k = 0; k < G; k++) {
                if (e0 + k * T >= E2) continue;
                gi[k] = 2 * (e0 + k * T);
                pre[k] = fin_store_fetch(a, g, gi[k]);
            }
#pragma unroll
            for (int k = 0; k < G; k++) {
                if (e0 + k * T >= E2) continue;
                const u32 at = fin_lds_at((u32)gi[k]);
                const u32 p0 = lds[at & ~1u], p1 = lds[at | 1u];
                const bool sw = at & 1;
                const u64 mv[2] = {csub32(sw ? p1 : p0, t), csub32(sw ? p0 : p1, t)};
                fin_store_vals(a, g, gi[k], mv, pre[k]);
            }
        }
    } else {
        const FinScale32 sc = fin_scale32_consts(a.fin);
        const u32 n = (u32)g.n, L = (u32)a.L;
        u64 *o = a.aux_out + ((size_t)item * 2 * L << a.logn);
        for (int e0 = tid; e0 < E2; e0 += G * T) {
            U2 k0[G][FIN_PRE], k1[G][FIN_PRE] = {};
            u32 gi[G];
#pragma unroll
            for (int k = 0; k < G; k++) {
                if (e0 + k * T >= E2) continue;
                gi[k] = 2 * (u32)(e0 + k * T);
#pragma unroll
                for (int j = 0; j < FIN_PRE; j++)
                    if (j < a.L) {
                        k0[k][j] = ld2g(fin_at(kp, (u32)j * n + gi[k]));
                        if (C1) k1[k][j] = ld2g(fin_at(kp, (L + j) * n + gi[k]));
                    }
            }
#pragma unroll
            for (int k = 0; k < G; k++) {
                if (e0 + k * T >= E2) continue;
                const u32 at = fin_lds_at(gi[k]);
                const u32 p0 = lds[at & ~1u], p1 = lds[at | 1u];
                const bool sw = at & 1;
                const u32 mv[2] = {csub32(sw ? p1 : p0, t), csub32(sw ? p0 : p1, t)};
                const u32 fix[2] = {plain_fix32(sc, mv[0]), plain_fix32(sc, mv[1])};
#pragma unroll
                for (int j = 0; j < FIN_PRE; j++)
                    if (j < a.L) fin_store_limb32<C1>(a, o, n, gi[k], j, mv, fix, k0[k][j], k1[k][j]);
                for (int j = FIN_PRE; j < a.L; j++)
                    fin_store_limb32<C1>(a, o, n, gi[k], j, mv, fix, ld2g(fin_at(kp, (u32)j * n + gi[k])),
                                         C1 ? ld2g(fin_at(kp, (L + j) * n + gi[k])) : U2{0, 0});
            }
        }
    }
}
template <int T, bool SCALE32 = false, bool C1 = !FIN_ITEM_C1_EARLY>
HD void fin_item_store(const NttArgs &a, int item, int tid, const u32 *lds)
{
    fin_item_store<T, SCALE32, C1>(a, item, tid, lds, fin_item_ks(a, item));
}

// slice `slice` of `nslices` of the item's c1 half, out[b][1][j] = -c1[j] (L N words as 16-byte pairs, limb j the pairs
// [j N/2, (j+1) N/2)): loads of G pairs, then their stores.  The kernel issues one slice in front of each of its other phases --
// clear, encode, every register round: fin_item_c1_slices -- so that memory drains it while the wave works in LDS.  A barrier
// itself does not wait for the wave's stores (the compiled code waits for LDS and scalar loads in front of it, not for vector
// memory); the next vector load that is waited for does, the counter being one for loads and stores: a round's first twiddle.
// So a slice is sized to one phase and the half is not hoisted whole.  `ks` = fin_item_ks(a, item).
template <int LOGN> constexpr int fin_item_c1_slices() { return 2 + FinItemSched<LOGN>::R; }
#ifndef FIN_ITEM_C1_G
#define FIN_ITEM_C1_G 4
#endif
template <int T> HD void fin_item_c1(const NttArgs &a, int item, int tid, int slice, int nslices, gptr ks)
{
    constexpr int G = FIN_ITEM_C1_G;
    const int half = a.logn - 1;
    const int P = a.L << half;  // at most 2^19 pairs: P * nslices fits an int
    // slice boundaries on multiples of 8 pairs (128 bytes; P is one): no cache line is written in two parts by two phases or two waves
    const int lo = (P * slice / nslices) & ~7, hi = slice + 1 == nslices ? P : (P * (slice + 1) / nslices) & ~7;
    // both bases are uniform over the workgroup; a pair is addressed from them by fin_at (L N <= 2^20 words)
    const gptr kp = ks + ((size_t)a.L << a.logn);
    u64 *o = a.aux_out + (((size_t)item * 2 + 1) * a.L << a.logn);
    for (int j = lo >> half; (j << half) < hi; j++) {  // the limbs the slice touches: the prime is uniform over the workgroup
        const u64 q = mod_at_u(a.mods, j).q;
        const int p_lo = lo > (j << half) ? lo : (j << half), p_hi = hi < ((j + 1) << half) ? hi : ((j + 1) << half);
        for (int p0 = p_lo + tid; p0 < p_hi; p0 += G * T) {
            U2 v[G];
#pragma unroll
            for (int k = 0; k < G; k++)
                if (p0 + k * T < p_hi) v[k] = ld2g(fin_at(kp, 2 * (u32)(p0 + k * T)));
#pragma unroll
            for (int k = 0; k < G; k++)
                if (p0 + k * T < p_hi) st2_stream(fin_at(o, 2 * (u32)(p0 + k * T)), U2{negmod(v[k].a, q), negmod(v[k].b, q)});
        }
    }
}
template <int T> HD void fin_item_c1(const NttArgs &a, int item, int tid, int slice, int nslices)
{
    fin_item_c1<T>(a, item, tid, slice, nslices, fin_item_ks(a, item));
}
