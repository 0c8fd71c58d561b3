// hhe_common.h -- shared types for the gfx950 BFV/PASTA-3 kernels and their host driver.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HD __host__ __device__ __forceinline__
#else
#define HD inline
#endif

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int HHE_MAXL = 32;          // data-level RNS limbs supported (the reference's N=65536 chain has 29 primes)
constexpr int HHE_MAXK = HHE_MAXL + 1;
constexpr int PASTA_T = 128;          // pasta_3_plain.h:18,32
constexpr int PASTA_R = 3;            // pasta_3_plain.h:33
constexpr u64 PASTA_NONCE = 123456789ULL;  // pasta_3_seal.cpp:47,115
// What one PASTA block is drawn from: Pasta::init_shake(nonce, block_counter) (pasta_3_plain.cpp:56).  A bare counter is the pair under
// the reference's fixed nonce, so the entry points that take counters and the ones that take pairs name the same cache entries.
// Also the element of the device array a per-pair XOF launch reads (PastaXofArgs::pairs): two words, nonce first.
struct PastaPair {
    u64 nonce, counter;
    PastaPair() = default;
    constexpr PastaPair(u64 counter_) : nonce(PASTA_NONCE), counter(counter_) {}
    constexpr PastaPair(u64 nonce_, u64 counter_) : nonce(nonce_), counter(counter_) {}
    bool operator<(const PastaPair &o) const { return nonce != o.nonce ? nonce < o.nonce : counter < o.counter; }
    bool operator==(const PastaPair &o) const { return nonce == o.nonce && counter == o.counter; }
};

// One RNS modulus as the kernels see it.  Tables live in device memory.
struct ModDev {
    u64 q;
    u64 r_lo, r_hi;        // floor(2^128 / q)
    u64 ninv, ninv_s;      // N^-1 mod q and its Shoup quotient
    u64 ninv_t, ninv_t_s;  // N^-1 * t mod q (INTT fused with the BEHZ "times t")
    const u64 *w, *ws;     // psi^bitrev(k), Shoup quotients [N] each (forward rounds: two 8-byte loads keep the 128-VGPR budget spill-free)
    const u64 *fw;         // [N][2]: the forward powers interleaved with their quotients as well (the row kernel's 8-points-per-lane rounds have the
                           // registers for one 16-byte load per twiddle; half the vector-memory instructions of w / ws)
    const u64 *iw;         // [N][2]: inverse powers interleaved with their Shoup quotients (inverse rounds: one 16-byte load, measured 3 % faster)
    u64 nq;                // 2^64 - q.  Read from the table, so the compiler cannot rewrite "+ h * nq" back into "- h * q": the lazy
                           // product becomes one multiply-add chain and conditional subtractions become add + sign select (no borrow chains)
    // Pseudo-Mersenne form q = 2^b - c (every prime SEAL generates descends from a power of two, seal/util/numth.h:138-139):
    // x mod q = (x mod 2^b) + (x >> b) * c  (mod q), one shift, one mask and one v_mad_u64_u32 -- no compare, no VCC.
    // pm_ok = 1 when 33 <= b <= 60, c < 2^32 and 2^b + 2^(64-b) c <= 2q, i.e. the fold takes ANY 64-bit value below 2q.
    u32 pm_sh;             // b - 32: the quotient x >> b is (high word) >> pm_sh
    u32 pm_mask;           // (1 << (b - 32)) - 1: mask of the high word
    u32 pm_c;              // c
    u32 pm_ok;
};

// The modulus table is written once at context creation.  Kernels read it through the CONSTANT address space: a plain global
// read of a workgroup-uniform entry cannot be proven unclobbered (the kernels store to global memory), so it compiles to a
// vector load that is repeated after every barrier and sits in front of every twiddle address as a second dependent memory
// round trip; from the constant address space it is an s_load into SGPRs (no VGPRs, scalar cache).
HD ModDev mod_at(const ModDev *mods, int i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) ModDev *p = (const __attribute__((address_space(4))) ModDev *)(mods + i);
    ModDev m;
    m.q = p->q; m.r_lo = p->r_lo; m.r_hi = p->r_hi;
    m.ninv = p->ninv; m.ninv_s = p->ninv_s; m.ninv_t = p->ninv_t; m.ninv_t_s = p->ninv_t_s;
    m.w = p->w; m.ws = p->ws; m.fw = p->fw; m.iw = p->iw; m.nq = p->nq;
    m.pm_sh = p->pm_sh; m.pm_mask = p->pm_mask; m.pm_c = p->pm_c; m.pm_ok = p->pm_ok;
    return m;
#else
    return mods[i];
#endif
}

// the same for an index that is uniform over the workgroup (every transform kernel: one modulus per tile): stating the
// uniformity keeps the entry in SGPRs even where the compiler's divergence analysis gives up (inside the strided lane loops)
HD ModDev mod_at_u(const ModDev *mods, int i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    i = __builtin_amdgcn_readfirstlane(i);
    const u64 p = (u64)mods;  // the table pointer too: the compiler sometimes keeps this kernel argument in VGPRs
    mods = (const ModDev *)(((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(p >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)p));
#endif
    return mod_at(mods, i);
}

// Modulus indices inside ModDev[]: 0..K-1 coefficient primes (K-1 = special),
// K..K+L Bsk = {B_0..B_{L-1}, m_sk}, K+L+1 = plain modulus t.

enum NttLoadOp { LOAD_PLAIN = 0, LOAD_DIGIT = 1, LOAD_LIFT = 2, LOAD_RNEG = 3,
                 LOAD_ENCODE = 4 };  // inv, mod t: the tile is gathered from the items' words through FinArgs::slot_inv (BatchEncoder::encode without a plaintext buffer)
enum NttStoreOp {
    STORE_PLAIN = 0, STORE_MUL = 1, STORE_SCALE_T = 2, STORE_MAC = 3,
    STORE_RSP = 5,         // inv (special limb): v + floor(q_sp/2) mod q_sp
    STORE_KS1 = 6,         // inv: (v - r_1 + half) * q_sp^-1, written through the Galois map into aux_out
    STORE_KS0 = 7,         // fwd: NTT-domain key-switch finish of c0 + permuted-frame diagonal MAC
    STORE_KSF = 10,        // inv, polys [B][2][L]: generic key-switch finish (v - r_k + half) * q_sp^-1 (+ base poly k) into aux_out
    STORE_LAZY = 8,        // fwd: leave the result in the lazy range [0,4q) (consumer reduces: key-switch inner product)
    STORE_ADD_PLAIN = 11   // inv, mod t, one polynomial per item: aux_out[b] = scaled plaintext - operand ciphertext of item b (add_plain on a negated operand)
};

// Constants of the fused finishing pass of a transciphering call (LOAD_ENCODE / STORE_ADD_PLAIN), written to device memory once
// per context: NttArgs carries a pointer, not a copy of delta[].
struct FinArgs {
    const u32 *slot_inv;       // [N]: slot_inv[slot_map[s]] = s
    int count;                 // LOAD_ENCODE: words per item placed at slots [0, count); every other coefficient slot is 0
    int L;
    u64 t, q_mod_t, thr;       // as in AddPlainArgs
    u64 t_r_lo, t_r_hi;
    u64 delta[HHE_MAXL];
    // one workgroup per item (fin_item_kernel, hhe_fin_bodies.h); null where the context is not eligible
    const u32 *slot_map;       // [N]: coefficient of slot s
    const u32 *itw;            // [N][2]: the inverse powers mod t in the order of ModDev::iw, each with floor(w * 2^32 / t)
    // the 32-bit scaling of the item kernel (plain_fix32 / plain_scaled32, hhe_fin_bodies.h); zero where fin_scale32_ok does not hold
    u32 q_mod_t_s;             // floor(q_mod_t * 2^32 / t)
    u32 scale32;               // 1: q_mod_t_s and delta_s are set
    u64 delta_s[HHE_MAXL];     // floor(delta[j] * 2^64 / q_j)
};

// where fin_item_kernel runs: N u32 words fit the LDS of one workgroup (4 N <= 128 KiB) and the lazy range [0, 4t) of its 32-bit
// butterflies fits a word
constexpr int FIN_ITEM_MIN_LOGN = 10, FIN_ITEM_MAX_LOGN = 15;
inline bool fin_item_ok(int logn, u64 t) { return logn >= FIN_ITEM_MIN_LOGN && logn <= FIN_ITEM_MAX_LOGN && t < ((u64)1 << 30); }
// where the item kernel scales its plaintext with 32-bit products: the coefficients are below t < 2^30 (fin_item_ok), and the fix
// (below t) is added to a residue with ONE conditional subtraction, so every data prime q[0 .. L) must exceed t
inline bool fin_scale32_ok(int logn, u64 t, const u64 *q, int L)
{
    if (!fin_item_ok(logn, t)) return false;
    for (int j = 0; j < L; ++j)
        if (q[j] <= t) return false;
    return true;
}
// the constants of that scaling from t, q_mod_t and delta[] of `fa` (host only; call where fin_scale32_ok holds)
inline void fin_scale32_fill(FinArgs &fa, const u64 *q, int L)
{
    fa.q_mod_t_s = (u32)((fa.q_mod_t << 32) / fa.t);  // q_mod_t < t < 2^30
    for (int j = 0; j < L; ++j) fa.delta_s[j] = (u64)(((unsigned __int128)fa.delta[j] << 64) / q[j]);  // delta[j] < q[j]
    fa.scale32 = 1;
}

// key-switch mod-down constants, passed by value to the kernels that finish a key switch
struct KsConsts {
    u64 half;                 // floor(q_sp/2)
    u64 half_mod[HHE_MAXL];   // half mod q_j
    u64 qsp_inv[HHE_MAXL];    // q_sp^-1 mod q_j
    u64 qsp_inv_s[HHE_MAXL];
    u64 qsp_mod[HHE_MAXL];    // q_sp mod q_j (FC leaf sums: galois(c0) enters the sum that is later multiplied by q_sp^-1)
    u64 qsp_mod_s[HHE_MAXL];
    // KS1 epilogue in one expression: (v N^-1 - r + half) q_sp^-1 = v (N^-1 q_sp^-1) - r q_sp^-1 + half q_sp^-1  (mod q_j)
    u64 ninv_qinv[HHE_MAXL], ninv_qinv_s[HHE_MAXL];  // N^-1 q_sp^-1 mod q_j and its Shoup quotient
    u64 hq2[HHE_MAXL];                               // 2 q_j + (half q_sp^-1 mod q_j): keeps the lazy difference non-negative
};

struct NttArgs {
    const u64 *src;
    u64 *dst;
    const ModDev *mods;
    int logn;
    int logm;       // log2 of this pass's sub-transform size
    int logc;       // log2 lanes (independent sub-transforms) per tile
    int tiles_log;  // log2 tiles per polynomial in this pass (1-D grid decode)
    int count;      // polynomials in the batch
    int mod_base, mod_cycle;  // modulus of poly p = mod_base + p % mod_cycle
    // source poly of p: src + (p / src_item_polys) * src_item_stride + ((p % src_item_polys) / src_div) * N
    int src_div;          // DIGIT: K, LIFT: L, else 1
    int src_item_polys;   // polys of one batch item in p-space (0 => whole batch is one item)
    size_t src_item_stride;  // words between items in src
    int load_op, store_op;
    u32 load_einv;     // first pass: > 0 => the source is read through a Galois map (apply_galois as a gather): elt^-1 mod 2N;
                       // negation is modulo the SOURCE limb's prime (the digit source d_I lives mod q_I whatever the transform's modulus)
    u32 *zero_flag;    // LOAD_DIGIT: set to 1 when a coefficient equals 0 (the shared-digit FC path then falls back)
    int lazy8;         // every modulus of the launch has the pseudo-Mersenne form (ModDev::pm_ok, q < 2^60): the butterflies use the truncated
                       // Shoup product (results in [0,4q)) and fold with pm_fold once per register round; values stay below 16q <= 2^64
    int digit_reduce;  // DIGIT: 1 if some q_I >= 4*q_J (else the lazy butterflies absorb the unreduced residue)
    u64 t;          // LIFT: plain modulus
    // STORE_MUL / STORE_MAC multiplier (NTT form): (mul_ptrs ? mul_ptrs[p / mul_item_polys] : mul)
    //   + mul_shift + (p % mul_cycle) * N
    const u64 *mul;
    const u64 *const *mul_ptrs;
    size_t mul_shift;
    size_t mul_s_off;   // KS0: > 0 => the Shoup quotients of the multiplier table follow it at this word offset (pdiag of the fused matmul)
    int mul_cycle, mul_item_polys;
    u64 *acc;       // STORE_MAC / DIGIT_DIAG / KS0: accumulator polys
    // fused key-switch epilogues (matmul pipeline)
    int L, K;
    u32 gal_elt;        // KS1: coefficient-domain Galois element (0 = identity); KS0: NTT-domain element
    u32 gal_einv;       // KSF: > 0 => the base is galois(c0) gathered on the fly: elt^-1 mod 2N (aux_in = the un-rotated ciphertexts)
    const u64 *aux_r;   // KS1 / KSF: r [B][2][N] (KS1: poly 1);  KS0: S [B][2][K][N] (poly 0, limb j)
    const u64 *aux_in;  // KS0: c0 (NTT form) of the current state [B][L][N];  KSF: base ciphertexts (item b at aux_in + b * base_stride) or null
    u64 *aux_out;       // KS1: d [B][L][N];  KS0: c0 (NTT form) of the next state [B][L][N];  KSF: out [B][2][L][N]
    size_t base_stride; // KSF: words between the items of aux_in
    int base_mask;      // KSF: bit k set => add base poly k.  Both ops of the finishing pass in one launch (the item kernel): 1 => the
                        // launch takes the instantiation with the 32-bit scaling (FinArgs::scale32 is set); the two-pass kernels ignore it
    KsConsts ks;
    // fused finishing pass.  LOAD_ENCODE: src = the items' words (item b at src + b * src_item_stride, src_item_polys = 1).
    // STORE_ADD_PLAIN: the operand ciphertext of item b is mul_ptrs[b] if mul_ptrs is set, else mul + b * 2LN; aux_out = out [B][2][L][N]
    const FinArgs *fin;
};

enum EltOp { ELT_ADD = 0, ELT_SUB = 1, ELT_NEG = 2, ELT_MUL = 3, ELT_MAC = 4, ELT_COPY = 5, ELT_BCAST = 6, ELT_SHOUP = 7,
             ELT_DIFF = 8,    // ELT_DIFF writes no polynomial: out[0] = 1 when a word of a differs from its word of b (out[0] cleared by the caller)
             ELT_ENCZ = 9,    // key generation: c0 = -(a s + e) (+ f new_key) of an encryption of zero under the secret key (elt_encz_body; a kernel of its own)
             ELT_MODDOWN = 10,  // modulus switching: a [count][mod_cycle][N] -> out [count][b_cycle][N], b = the context's pair table (mod_down_body; kernels of its own)
             ELT_KEYPROJ = 11,  // a key-switch key of a level from one higher up its chain (key_proj_body; a kernel of its own)
             ELT_ADDMANY = 12 };  // out = the sum of b_cycle stacked operands (add_many_body; a kernel of its own)

struct EltArgs {  // element-wise kernels over [count][N] polys, modulus = mod_base + p % mod_cycle
    const u64 *a, *b;
    u64 *out;
    const ModDev *mods;
    int logn, count, mod_base, mod_cycle;
    int b_cycle;  // poly of b = p % b_cycle (broadcast over the batch), 0 => same index
    int with_key;  // ELT_ENCZ: 1 => new_key [K][N] (NTT form) of a key-switching key follows the `count` polynomials of a (fills the
                   // struct's tail padding: the argument block of the older ops keeps its size and offsets)
};

// ELT_MODDOWN (Evaluator::mod_switch_to_inplace on coefficient-form polynomials): `count` polynomials of mod_cycle = limbs_in residues
// each, under q_0 .. q_{limbs_in-1} (mod_base = 0), leave with b_cycle = limbs_out residues; one lane owns one coefficient of one
// polynomial, so the launch covers count << logn lanes like every other op of EltArgs.  b = the per-context table (hhe_ctx::d_moddown):
// for every pair j < m three words at mod_down_pair(m, j) -- q_m^-1 mod q_j, its Shoup quotient, floor(q_m/2) mod q_j.
// Up to MOD_DOWN_REGS input limbs the column lives in registers (one kernel per limb count); longer chains keep it in LDS.
constexpr int MOD_DOWN_REGS = 8;
HD size_t mod_down_pair(int m, int j) { return (size_t)3 * ((size_t)m * (m - 1) / 2 + j); }
inline size_t mod_down_table_words(int L) { return mod_down_pair(L, 0) + 3; }  // never empty (L = 1 has no pair)

// ELT_KEYPROJ (hhe_keyset_derive_level): the key-switch key of the level with l data primes is digits I < l and limbs
// {0 .. l-1, special} of a key higher up the chain.  a = the source key [L_src][2][K_src][N], b_cycle = K_src; out = [l][2][l+1][N],
// mod_cycle = l + 1, count = l * 2 * (l + 1) output polynomials.  Output polynomial p = (I * 2 + k) * (l + 1) + J is source polynomial
// (I * 2 + k) * K_src + (J == l ? K_src - 1 : J).  One lane moves 16 bytes: count << (logn - 1) lanes do the work; the launch
// entry's count << logn covers them, the rest return at the bound.

// ELT_ADDMANY (Evaluator::add_many, seal/evaluator.h:150): a = b_cycle operands stacked [b_cycle][count][N], out [count][N], polynomial p
// under modulus mod_base + p % mod_cycle:  out[p][i] = sum_k a[k][p][i] mod q.  One lane owns two adjacent coefficients (16-byte
// accesses): count << (logn - 1) lanes do the work, the launch entry's count << logn covers them and the rest return at the bound.
// The sum rides in a 128-bit accumulator and is reduced once: any 64-bit input words, any b_cycle an int holds.  A lane reads all
// its operands before it writes, and no other lane touches its words, so out may be one of the operands.

struct CopyItemsArgs {  // dst item (s * dst_stride + dst_off) <- src item (s * src_stride + src_off), `words` words each, s < count
    const u64 *src;
    u64 *dst;
    size_t words, count;
    size_t src_stride, src_off, dst_stride, dst_off;  // in items
};

struct GaloisArgs {  // out[p][k] = +-in[p][k * einv mod 2N]; poly p = (item b, limb j), p = b * L + j
    const u64 *in;
    u64 *out;
    const ModDev *mods;
    int logn, count, L;
    size_t in_item_stride, out_item_stride;  // words between items
    u32 einv;  // elt^-1 mod 2N
    int accumulate;  // 1: out += gathered value (mod q) instead of out = value
};

struct KsMacArgs {  // S[b][k][J][n] = sum_I T[b][I][J][n] * key[I][k][J][n]
    const u64 *T;    // [B][L][K][N]
    const u64 *key;  // [L][2][K][N]
    u64 *S;          // [B][2][K][N]
    const ModDev *mods;
    int logn, B, L, K;
    // optional (FC leaf sums): for J < L the products are added into s_acc[b][k][J][n] instead of being written to S
    u64 *s_acc;
    // optional (fused matmul): acc[b][J][n] += T[b][J][J][n] * mul_ptrs[b][mul_shift + J*N + n] for J < L
    u64 *acc;
    const u64 *const *mul_ptrs;
    size_t mul_shift;
    // optional (FC shared digits): T holds the digit transforms of the UN-rotated c1; the rotation by perm_elt is applied
    // as the NTT-domain index map while reading T, and corr[k][J][n] (KsCorrArgs) is added to the sums
    u32 perm_elt;
    const u64 *corr;  // [2][K][N]
    // optional split output (key switch finished by the fused STORE_KSF pass): the data limbs go to S as [B][2][L][N] and the
    // special limb to S_sp [B][2][N] instead of S [B][2][K][N]
    u64 *S_sp;
};
// one child of a node in a multi-child launch of the key-switch row kernel (ks_perm_row_many_kernel; KsRowArgs::kids)
struct KsKid {
    const u64 *key, *key_s, *corr;   // [L][2][K][N] key and Shoup quotients, [2][K][N] correction table (KsCorrArgs)
    u32 elt, step0;                  // Galois element of the child's rotation; step0 != 0 (plain-weights sum only): the child is step 0, it has no
                                     // key and enters as q_sp * NTT(c0), q_sp * NTT(c1) on the data limbs
};
constexpr int HHE_ROT_GROUP = 16;    // children one launch serves at most (the virtual batch and the lane's sums stay within HHE_CHUNK items)
// Fused key-switch row kernel (ks_row_kernel): for one (item b, key limb J, row tile) it runs the forward ROW pass of the
// L digit transforms T[b][I][J] (their strided pass has already run), multiplies each finished tile with key[I][0..1][J]
// (Shoup products, 64-bit lazy sums kept in registers), and runs the inverse ROW pass on the sums that are
// inverse-transformed next -- so neither T nor S_1 / S_k[special] makes a round trip through memory.
struct KsRowArgs {
    const u64 *key;      // [L][2][K][N]
    const u64 *key_s;    // Shoup quotients floor(key * 2^64 / q_J), same layout
    u64 *S;              // [B][2][K][N]: only S_0[j], j < L, is written (NTT form, canonical) -- the c0 branch reads it; null with U0
    u64 *U0;             // generic key switch: inverse row pass of S_0[j] (item b, limb j at U0 + b * u_stride + j * N); else null
    u64 *U1;             // inverse row pass of S_1[j], j < L (item b, limb j at U1 + b * u_stride + j * N)
    size_t u_stride;     // words between items in U0 / U1
    u64 *Usp;            // [B][2][N]: inverse row pass of S_0[special], S_1[special]
    int B, L, K;
    // fused matmul: acc[b][J][n] += T[b][J][J][n] * mul_ptrs[b][mul_shift + J*N + n] for J < L (the I = J digit)
    u64 *acc;
    const u64 *const *mul_ptrs;
    size_t mul_shift;
    size_t mul_s_off;    // > 0: Shoup quotients of the multiplier table at this word offset behind it
    // FC shared digits (ks_perm_row_kernel; U0 / U1 / Usp as in the generic key switch): T [B][L][K][N] = the COMPLETE digit transforms of the
    // node's un-rotated c1, read through the NTT-domain Galois map of perm_elt; corr [2][K][N] is added to the sums (KsCorrArgs)
    const u64 *T;
    const u64 *corr;
    u32 perm_elt;
    const u64 *c0hat;    // optional [B][L][N]: q_sp * NTT(the node's c0).  Read through the same map it joins S_0[j], so the mod-down
                         // returns galois(c0) + the key-switched part and the KSF epilogue needs no coefficient-domain gather of c0
    // Hoisted rotations (several children of one node in ONE launch, ks_perm_row_many_kernel): B counts VIRTUAL items child * kid_B + b.  Child
    // `ch` takes its key, quotients, correction table and element from kids[ch] (a device table the host wrote; read with wave-uniform
    // loads, never written by a kernel); T and c0hat belong to the node and are indexed by b alone; U0 / U1 / Usp by the virtual item.
    // null / 0 (every single-child caller): key, key_s, corr and perm_elt above serve all B items
    const KsKid *kids;
    int kid_B;
    // Plain-weights sum (hhe_rotate_plain_sum_ks; ks_plain_sum_row_kernel): B counts REAL items and a workgroup loops over the n_kids children
    // of kids itself (kid_B = B).  Child ch's sums, complete with corr and c0hat, are multiplied by limb J of its plaintext -- plain + (ch * K + J) * N,
    // NTT form under all K primes, Shoup quotients plain_s_off words behind -- and added up over the children before the one inverse row
    // pass.  A step-0 child (KsKid::step0) contributes c0hat and c1hat ([B][L][N]: q_sp * NTT(c1)) on the data limbs, nothing on the special one.
    // null (every other caller): one child per workgroup, as above
    const u64 *plain;
    size_t plain_s_off;
    const u64 *c1hat;
    int n_kids;
};
constexpr int PLAIN_SUM_FOLD = 3;    // children between two folds of the outer sums of the plain-weights sum: a fold leaves a sum below 2q, a truncated
                                     // Shoup product adds less than 4q, and 2q + 3 * 4q = 14q fits the 16q <= 2^64 of a pseudo-Mersenne prime where 18q need not

// Correction of the shared-digit key switch (DESIGN.md "FC rotation trie"): the digit d_I of galois_g(c1) differs from
// galois_g applied mod q_J to the digit of c1 by q_I at every sign-flipped, non-zero coefficient, so
//   corr[k][J] = NTT_J(s_g) * sum_{I != J} (q_I mod q_J) * key_g[I][k][J]     (s_g = 0/1 polynomial of the flipped positions)
struct KsCorrArgs {
    const u64 *key;    // [L][2][K][N]
    const u64 *shat;   // [K][N] NTT_J(s_g)
    const u64 *qmod;   // [L][K]  q_I mod q_J
    u64 *corr;         // [2][K][N]
    const ModDev *mods;
    int logn, L, K;
};

struct PermArgs {  // NTT-domain Galois permutation: out[p][x] (op)= in[p][pi_elt(x)] (* mul)
    const u64 *in;
    u64 *out;
    const ModDev *mods;
    int logn, count, L;        // poly p = (item b, limb j)
    size_t out_item_stride;    // words between items in out (in is [count][N])
    u32 elt;
    int mac;                   // 1: out[p][x] += in[p][pi(x)] * mul_ptrs[b][shift + j*N + x]
    const u64 *const *mul_ptrs;
    size_t mul_shift;
    size_t in_item_stride;     // words between items in `in` (0: in is [count][N])
    // steps > 0 -- diagonal sum over shared operands (first affine layer of the fused matmul; diag_sum_body), no index map:
    //   out [b][j][x] (+)= sum_{i < steps} in [i * in_step_stride + j*N + x] * mul_ptrs[b][mul_shift + i * mul_step_stride + j*N + x]
    //   out2[b][j][x] (+)= sum_{i < steps} in2[i * in_step_stride + j*N + x] * (the same multiplier)
    // in / in2 are shared by all items (canonical words); out / out2 use out_item_stride; carry = 1 adds to what out / out2 hold
    int steps, carry;
    const u64 *in2;
    u64 *out2;
    size_t in_step_stride, mul_step_stride;
    // bsgs_n1 > 0 -- babystep-giantstep inner sums of a packed plain-matrix layer (bsgs_inner_sum_body), no index map; poly p = (item b,
    // polynomial pl < 2L), limb j = pl % L, count = B * 2L:
    //   out[k * out_step_stride + b * out_item_stride + pl*N + x] = sum_{i < bsgs_n1} in[i * in_step_stride + b * in_item_stride + pl*N + x]
    //                                                 * mul_ptrs[b][mul_shift + (k * bsgs_n1 + i) * mul_step_stride + j*N + x]   for every k < bsgs_n2
    // in and the multipliers are canonical words in NTT form
    int bsgs_n1, bsgs_n2;
    size_t out_step_stride;
};

struct LeafSumArgs {  // out[b][k][j] += qsp_inv_j * (accS[b][k][j] (INTT'd) + accH[b][k][j])
    const u64 *accS;  // [B][2][L][N] coefficient form (after INTT)
    const u64 *accH;  // [B][2][L][N] rounding terms, and for k = 0 q_sp * galois(c0) of the leaf parents
    u64 *out;         // [B][2][L][N]
    const ModDev *mods;
    int logn, B, L;
    KsConsts ks;
};

constexpr int HHE_LEAF_GROUP = 4;  // leaf key switches of the FC trie handled by one launch (leaves of ANY nodes whose digit transforms are still resident);
                                   // ms per MNIST sample at 1 / 2 / 4 / 8 per launch: 53.3 / 50.6 / 50.3 / 51.6
struct LeafRoundArgs {  // accH[b][k][j] += sum over the m leaves of: half_j - (r_l[b][k] mod q_j) (+ q_sp * galois_l(c0_b of leaf l's parent)[j] for k = 0)
    const u64 *r;      // [B][2][m][N]: INTT(S_k[special]) + floor(q_sp/2) mod q_sp of leaf l (the STORE_RSP result)
    u64 *accH;         // [B][2][L][N]
    const u64 *base[HHE_LEAF_GROUP];  // un-rotated parent ciphertexts of leaf l (item b at base[l] + b * base_stride, c0 limbs first); read through the Galois maps
    size_t base_stride;
    const ModDev *mods;
    int logn, B, L, m;
    u32 gal_einv[HHE_LEAF_GROUP];  // elt_l^-1 mod 2N
    KsConsts ks;
};
// Key-switch inner products of m leaf key switches from the shared digit transforms of their parents (KsMacArgs with perm_elt / corr,
// once per leaf): the data-limb sums of all m leaves go into s_acc with ONE read-modify-write, the special-limb sums of leaf l into
// S_sp[b][k][l].  Leaves of one parent read the same digit transforms back to back (cached).
struct KsMacLeavesArgs {
    u64 *S_sp;         // [B][2][m][N]
    u64 *s_acc;        // [B][2][L][N]
    const ModDev *mods;
    int logn, B, L, K, m;
    const u64 *T[HHE_LEAF_GROUP];     // [B][L][K][N] digit transforms of the un-rotated c1 of leaf l's parent ([B][L][N] when t_polys[l] == 1: special limb only)
    int t_polys[HHE_LEAF_GROUP];      // polynomials per digit in T[l]: K, or 1 for a parent whose children are all leaves
    int sp_only;                      // 1: only the special-limb sums (gid over [B][N/2]); the data-limb sums of the leaves come from the per-element c1 sums (CsumArgs)
    const u64 *key[HHE_LEAF_GROUP];   // [L][2][K][N]
    const u64 *corr[HHE_LEAF_GROUP];  // [2][K][N]
    u32 perm_elt[HHE_LEAF_GROUP];
};

// FC leaves, data limbs.  The inner product of a key switch is linear in the DIGITS as integers, and every leaf with the same Galois
// element g uses the same key: sum_l sum_I NTT_J(d_I(galois_g(c1_l))) key_g[I][k][J] = sum_I NTT_J(D_I) key_g[I][k][J] with D_I = the integer
// sum of the leaves' digits.  A digit of galois_g(c1) is c1_I at the mapped position, or q_I - c1_I where the map flips the sign (c1_I != 0:
// the shared-digit zero flag covers the rest), so D_I = galois_g applied to the integer sum of the UN-rotated limbs with `count` q_I - . at
// the flipped positions.  csum_add: sums[b][I][.] += c1 limbs of up to HHE_CSUM_GROUP parents (64-bit words + a byte counting the wraps);
// csum_digits: out[b][I][J][.] = D_I mod q_J for the K key-level primes -- the digit transforms and ONE inner product per element follow.
// The leaves' q_sp * galois_g(c0) terms are linear mod q_j outright: sums0 collects the un-rotated c0 limbs of the same parents (mod q_j),
// and csum_c0 adds q_sp * galois_g(sums0) into accH once per close -- the per-leaf coefficient-domain gather of c0 (8 bytes per cache
// line) leaves the rounding kernel.
constexpr int HHE_CSUM_GROUP = 8;  // parents per csum_add launch (the sums are read and written once per launch)
struct CsumArgs {
    u64 *sums;          // [B][L][N] integer sums of un-rotated c1 limbs, low 64 bits
    unsigned char *carry;  // [B][L][N] how often a sum wrapped 2^64 (terms below 2^61: 255 wraps cover > 2000 leaves per element)
    u64 *sums0;         // [B][L][N] sums of un-rotated c0 limbs mod q_j (null: not collected)
    const u64 *src[HHE_CSUM_GROUP];  // csum_add: parents' ciphertexts (item b at src[l] + b * src_stride: c0 limbs [L][N], then c1 limbs [L][N])
    size_t src_stride;
    u64 *accH;          // csum_c0: [B][2][L][N]
    u64 qsp_mod[HHE_MAXL], qsp_mod_s[HHE_MAXL];  // csum_c0: q_sp mod q_j and its Shoup quotient
    int m;              // csum_add: parents in this launch
    u64 *out;           // csum_digits: [B][L][K][N]
    const ModDev *mods;
    int logn, B, L, K;
    u32 einv;           // csum_digits: elt^-1 mod 2N
    u32 count;          // csum_digits: leaves summed
};

struct KsFinishArgs {  // SURVEY A.4 mod-down; S already INTT'd (coefficient form)
    const u64 *S;     // [B][2][K][N]
    const u64 *base;  // item b at base + b * base_item_stride, polys [2][L][N]; or null
    size_t base_item_stride;
    u64 *out;         // [B][2][L][N]
    const ModDev *mods;
    int logn, B, L, K;
    int base_mask;    // bit k set => add base poly k
    u64 half;                 // floor(q_sp/2)
    u64 half_mod[HHE_MAXL];   // half mod q_j
    u64 qsp_inv[HHE_MAXL];    // q_sp^-1 mod q_j
    u64 qsp_inv_s[HHE_MAXL];
    u64 qsp_mod[HHE_MAXL];    // q_sp mod q_j (FC leaf sums: galois(c0) enters the sum that is later multiplied by q_sp^-1)
    u64 qsp_mod_s[HHE_MAXL];
    // KS1 epilogue in one expression: (v N^-1 - r + half) q_sp^-1 = v (N^-1 q_sp^-1) - r q_sp^-1 + half q_sp^-1  (mod q_j)
    u64 ninv_qinv[HHE_MAXL], ninv_qinv_s[HHE_MAXL];  // N^-1 q_sp^-1 mod q_j and its Shoup quotient
    u64 hq2[HHE_MAXL];                               // 2 q_j + (half q_sp^-1 mod q_j): keeps the lazy difference non-negative
};

struct AddPlainArgs {
    const u64 *ct;     // [B][2][L][N]
    const u32 *ct_map; // if set: item b reads ciphertext ct_map[b] of `ct` (several items on one operand); out stays [B][2][L][N]
    const u64 *plain;  // [B or 1][N] coefficients mod t
    const u64 *const *plain_ptrs;  // if set: item b reads plain_ptrs[b] + plain_shift
    size_t plain_shift;
    u64 *out;
    const ModDev *mods;
    int logn, B, L;
    int plain_bcast;   // 1: one plain for the whole batch
    int negate_ct;     // 1: out = -ct (+/-) plain
    int subtract;      // 1: sub_plain
    u64 t, q_mod_t, thr;
    u64 t_r_lo, t_r_hi;        // floor(2^128/t)
    u64 delta[HHE_MAXL];
};

struct EncodeArgs {  // slot scatter; INTT mod t follows as an NTT launch
    const u64 *vals;   // [B][stride]
    u64 *out;          // [B][N]
    const u32 *slot_map;
    int logn, B, stride, count;  // count values per item placed at slots [0,count)
    int second_off;    // >=0: values [count, 2*count) go to slots [second_off, second_off+count)
    u64 t;
};

struct DiagArgs {  // PASTA_SEAL::diagonal preparation (pasta_3_seal.cpp:390-401) into slot order
    const u64 *mats;   // [4][2][128][128]
    u64 *out;          // [4*128][N]  (pre-INTT slot image)
    const u32 *slot_map;
    int logn;
};

struct BsgsDiagArgs {  // PASTA_SEAL::babystep_giantstep diagonal preparation (pasta_3_seal.cpp:280-328) into slot order
    const u64 *mats;   // [4][2][128][128]
    u64 *out;          // [4*128][N]
    const u32 *slot_map;
    int logn, n1;      // n1 = BSGS_N1 (16)
};

struct BehzDev {  // SURVEY A.7 constants
    int L;
    u64 inv_punct_q[HHE_MAXL], inv_punct_q_s[HHE_MAXL];
    u64 mt_mod_q[HHE_MAXL];                      // 2^32 mod q_i
    u64 punct_q_bsk[HHE_MAXL][HHE_MAXL + 1];
    u64 punct_q_mt[HHE_MAXL];
    u64 neg_inv_q_mt;
    u64 q_mod_bsk[HHE_MAXL + 1], inv_mt_bsk[HHE_MAXL + 1], inv_q_bsk[HHE_MAXL + 1];
    u64 inv_punct_B[HHE_MAXL];
    u64 punct_B_q[HHE_MAXL][HHE_MAXL];
    u64 punct_B_msk[HHE_MAXL];
    u64 inv_B_msk, msk;
    u64 B_mod_q[HHE_MAXL], neg_B_mod_q[HHE_MAXL];
};

struct BehzExtendArgs {  // x [P][L][N] coeff -> xb [P][L+1][N] coeff (then NTT'd)
    const u64 *x;
    u64 *xb;
    const ModDev *mods;
    const BehzDev *bz;
    int logn, P, L, K;
};

struct TensorArgs {  // d[b][0..2][j] from a[b][0..1][j], b[b][0..1][j]; NTT domain
    const u64 *a, *b;
    u64 *d;
    const ModDev *mods;
    int logn, B, limbs, mod_base;
    int b_div;  // > 0: the second operand of item b is ciphertext b / b_div of `b` (the resident diagonals of a packed encrypted FC layer,
                // each shared by the b_div items of a chunk; a kernel of its own); 0: item b of `b`
    int sum;    // > 0: d[b] = the sum over k < sum of the tensor products of a[k][b] and b[k][b] (b[k][0] when b_div is set), `a` being
                // [sum][B][2][limbs][N] and `b` [sum][B or 1][2][limbs][N] (hhe_multiply_sum; a kernel of its own); 0: one product
    int fold;   // with sum: the addends a 128-bit sum takes between two reductions (tensor_sum_fold of the widest modulus of the launch)
    int square; // != 0: d[b] = the tensor product of a[b] with itself (hhe_square; a kernel of its own); `b`, b_div, sum and fold are not read
};
// Addends between two reductions of tensor_sum_body's sums under a modulus of `bits` bits.  The middle polynomial takes two products
// below 2^(2 bits) per addend on top of a residue below 2^bits, and 2 f (2^bits - 1)^2 + 2^bits < 2^128 holds for f = 2^(127 - 2 bits)
// (32 at 61 bits, 128 at 60).  Capped at 128: past that a reduction is under 1 % of the products, and every interval stays testable.
inline int tensor_sum_fold(int bits) { return bits > 63 ? 1 : 127 - 2 * bits >= 7 ? 128 : 1 << (127 - 2 * bits); }

struct BehzFloorArgs {  // (dq [P][L][N], db [P][L+1][N]) coeff, already *t -> out [P][L][N]
    const u64 *dq, *db;
    u64 *out;
    const ModDev *mods;
    const BehzDev *bz;
    int logn, P, L, K;
};
