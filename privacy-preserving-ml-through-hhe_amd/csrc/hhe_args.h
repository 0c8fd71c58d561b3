// hhe_args.h -- host only: where the argument block of a launch is defined.  The kernels' argument structs (hhe_common.h) are plain
// C structs; every block the host driver hands to a launcher starts from one of the builders below, which set what ALL launches of
// that kind share, and the launch site adds what is particular to it (which buffers, which epilogue operands).  A field that every
// schedule must carry is set here, once.  Included by hhe_api.cpp and hhe_client.cpp; never by the kernels or the tests' emulator.
#pragma once
#include <cstring>
#include "hhe_internal.h"

inline int fail(int code, const std::string &msg) { hhe_set_error(msg); return code; }
inline int dev_fail(const char *where) { return fail(HHE_ERR_DEVICE, std::string(where) + ": " + rt_last_error()); }

// an argument block with every byte 0, padding included: a launch copies the block as bytes
template <class T> inline T zeroed()
{
    T a;
    memset(&a, 0, sizeof(a));
    return a;
}

// ------------------------------------------------------------------ transforms and element-wise launches
inline NttArgs ntt_args(const hhe_ctx *c, const u64 *src, u64 *dst, size_t count, int mod_base, int mod_cycle)
{
    NttArgs a = zeroed<NttArgs>();
    a.src = src; a.dst = dst; a.mods = c->d_mods; a.logn = c->logn; a.count = (int)count;
    a.mod_base = mod_base; a.mod_cycle = mod_cycle; a.src_div = 1; a.t = c->t;
    a.load_op = LOAD_PLAIN; a.store_op = STORE_PLAIN; a.mul_cycle = 1; a.mul_item_polys = 1;
    a.L = c->L; a.K = c->K; a.ks = c->ksc;
    a.lazy8 = ntt_lazy8(c, mod_base, mod_cycle);
    return a;
}
inline EltArgs elt_args(const hhe_ctx *c, const u64 *x, const u64 *y, u64 *out, size_t count, int mod_base, int mod_cycle, int b_cycle = 0)
{
    EltArgs a = zeroed<EltArgs>();
    a.a = x; a.b = y; a.out = out; a.mods = c->d_mods; a.logn = c->logn; a.count = (int)count;
    a.mod_base = mod_base; a.mod_cycle = mod_cycle; a.b_cycle = b_cycle;
    return a;
}

// ------------------------------------------------------------------ Galois maps
// the key of `elt` in the set the running entry point named, or null with the error text set (the caller returns HHE_ERR_NO_GALOIS_KEY)
inline const u64 *galois_key(const hhe_ctx *c, u32 elt)
{
    auto it = c->gks->gk.find(elt);
    if (it != c->gks->gk.end()) return it->second;
    hhe_set_error("Galois key not present");
    return nullptr;
}
inline u32 galois_einv(const hhe_ctx *c, u32 elt) { return (u32)nt_invmod(elt, 2 * c->n); }  // elt^-1 mod 2N: apply_galois as a gather

// coefficient-domain map of B items of L limbs: item b at in + b * in_stride -> out + b * out_stride
inline GaloisArgs galois_args(const hhe_ctx *c, size_t B, u32 einv, const u64 *in, size_t in_stride, u64 *out, size_t out_stride)
{
    GaloisArgs g = zeroed<GaloisArgs>();
    g.mods = c->d_mods; g.logn = c->logn; g.count = (int)(B * c->L); g.L = c->L; g.einv = einv;
    g.in = in; g.in_item_stride = in_stride; g.out = out; g.out_item_stride = out_stride;
    return g;
}
// NTT-domain launches over `polys` polynomials (item b, limb j): the index map, the diagonal sums and the babystep-giantstep inner sums
inline PermArgs perm_args(const hhe_ctx *c, size_t polys, const u64 *in, u64 *out, size_t out_item_stride)
{
    PermArgs p = zeroed<PermArgs>();
    p.in = in; p.out = out; p.mods = c->d_mods; p.logn = c->logn; p.count = (int)polys; p.L = c->L;
    p.out_item_stride = out_item_stride;
    return p;
}

// ------------------------------------------------------------------ the stages of one key switch
// digit transforms T[I][J] = NTT_J(d[I] mod q_J) of B items into dst [B][L][K][N], left in the lazy range [0,4q) (the inner product
// reduces); item b's d [L][N] at src + b * src_stride.  load_einv > 0: d is read through that Galois map.  zero_flag: raised where a
// coefficient is 0 (FC shared digits).  sp_only: the transforms modulo the special prime alone, dst [B][L][N]
inline NttArgs ks_digit_args(const hhe_ctx *c, const u64 *src, size_t src_stride, u64 *dst, size_t B, u32 load_einv = 0,
                             u32 *zero_flag = nullptr, bool sp_only = false)
{
    const int L = c->L, K = c->K;
    NttArgs a = sp_only ? ntt_args(c, src, dst, B * L, K - 1, 1) : ntt_args(c, src, dst, B * L * K, 0, K);
    a.src_div = sp_only ? 1 : K; a.src_item_polys = sp_only ? L : L * K; a.src_item_stride = src_stride;
    a.load_op = LOAD_DIGIT; a.digit_reduce = c->digit_reduce; a.store_op = STORE_LAZY;
    a.load_einv = load_einv; a.zero_flag = zero_flag;
    return a;
}
// inner product with the key as its own kernel: S[b][k][J] = sum_I T[b][I][J] * key[I][k][J]
inline KsMacArgs ks_mac_args(const hhe_ctx *c, const u64 *T, const u64 *key, u64 *S, size_t B)
{
    KsMacArgs m = zeroed<KsMacArgs>();
    m.T = T; m.key = key; m.S = S; m.mods = c->d_mods; m.logn = c->logn; m.B = (int)B; m.L = c->L; m.K = c->K;
    return m;
}
// a lane's ws_S [B][2][K][N] holding the sums of a key switch that the fused STORE_KSF pass finishes: data limbs W [B][2][L][N],
// then the special limbs Usp [B][2][N]
struct KsSplit { u64 *W, *Usp; };
inline KsSplit ks_split(const hhe_ctx *c, u64 *ws_S, size_t B) { return KsSplit{ws_S, ws_S + B * 2 * c->L * c->n}; }
// the fused row kernels (ks_row_kernel, ks_perm_row_kernel); with `sp` all 2K sums leave through their inverse row pass into the split
inline KsRowArgs ks_row_args(const hhe_ctx *c, const u64 *key, const u64 *key_s, size_t B, const KsSplit *sp = nullptr)
{
    KsRowArgs x = zeroed<KsRowArgs>();
    x.key = key; x.key_s = key_s; x.B = (int)B; x.L = c->L; x.K = c->K;
    if (sp) { x.U0 = sp->W; x.U1 = sp->W + (size_t)c->L * c->n; x.u_stride = (size_t)2 * c->L * c->n; x.Usp = sp->Usp; }
    return x;
}
// inverse transform of `count` special-limb sums: r = INTT(S[special]) + floor(q_sp/2) mod q_sp (STORE_RSP).  src is [count][N], or
// with `strided` the sums [count][K][N] of an unsplit S, whose special limb is read
inline NttArgs ks_rsp_args(const hhe_ctx *c, const u64 *src, u64 *dst, size_t count, bool strided = false)
{
    NttArgs a = ntt_args(c, strided ? src + (size_t)(c->K - 1) * c->n : src, dst, count, c->K - 1, 1);
    if (strided) { a.src_item_polys = 1; a.src_item_stride = (size_t)c->K * c->n; }
    a.store_op = STORE_RSP;
    return a;
}
// inverse transform of the data-limb sums of a split, in place, with the mod-down in its store (STORE_KSF): out[b] = the key-switched
// pair (+ the polynomials of `base` that base_mask selects; item b at base + b * base_stride, read through the Galois map gal_einv if > 0)
inline NttArgs ks_ksf_args(const hhe_ctx *c, const KsSplit &sp, size_t B, const u64 *base, size_t base_stride, int base_mask, u32 gal_einv, u64 *out)
{
    NttArgs a = ntt_args(c, sp.W, sp.W, B * 2 * c->L, 0, c->L);
    a.store_op = STORE_KSF; a.aux_r = sp.Usp; a.aux_in = base; a.base_stride = base_stride; a.base_mask = base ? base_mask : 0;
    a.gal_einv = base ? gal_einv : 0; a.aux_out = out;
    return a;
}
