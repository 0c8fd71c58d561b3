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
//   store    the add_plain epilogue of the two-pass kernels (fin_store_fetch / fin_store_vals), fed from LDS
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

// the epilogue: coefficient pairs (gi, gi + 1) out of LDS, the operands of G pairs in flight before the first store
#ifndef FIN_ITEM_G
#define FIN_ITEM_G 2
#endif
template <int T> HD void fin_item_store(const NttArgs &a, int item, int tid, const u32 *lds)
{
    constexpr int G = FIN_ITEM_G;
    NttGeom g = {};
    g.n = 1 << a.logn;
    g.poly = item;
    const u32 t = (u32)ld_const(&a.fin->t);
    const int E2 = g.n >> 1;  // a multiple of T for every N >= 2048; guarded below
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
}
