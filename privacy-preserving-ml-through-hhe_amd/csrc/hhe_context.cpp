// hhe_context.cpp -- parameter derivation and device-resident tables for one BFV context.
// Follows what SEAL 4.0.0's SEALContext computes for the same (N, coeff_modulus, t):
// NTTTables (seal/util/ntt.h:69-183), BatchEncoder index map (seal/batchencoder.h),
// RNSTool's BEHZ base (seal/util/rns.h:324-399), the BFV scaling-variant constants
// (seal/context.h:350-401).  See SURVEY.md Appendix A for the restated arithmetic.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hhe_internal.h"
#include "../../include/hhe_gfx950.h"

typedef unsigned __int128 u128;

static thread_local std::string g_err;
void hhe_set_error(const std::string &msg) { g_err = msg; }
extern "C" const char *hhe_last_error(void) { return g_err.c_str(); }
extern "C" const char *hhe_backend(void) { return rt_backend_name(); }

// ------------------------------------------------------------------ number theory
u64 nt_mulmod(u64 a, u64 b, u64 m) { return (u64)((u128)a * b % m); }
u64 nt_powmod(u64 a, u64 e, u64 m)
{
    u64 r = 1 % m, x = a % m;
    for (; e; e >>= 1, x = nt_mulmod(x, x, m))
        if (e & 1) r = nt_mulmod(r, x, m);
    return r;
}
u64 nt_invmod(u64 a, u64 m)
{
    __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
    while (r1 != 0) {
        __int128 k = r0 / r1;
        __int128 r2 = r0 - k * r1; r0 = r1; r1 = r2;
        __int128 s2 = s0 - k * s1; s0 = s1; s1 = s2;
    }
    return (u64)(s0 < 0 ? s0 + m : s0);
}
bool nt_is_prime(u64 v)
{
    if (v < 2) return false;
    for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        if (v == p) return true;
        if (v % p == 0) return false;
    }
    u64 d = v - 1;
    int s = 0;
    while ((d & 1) == 0) { d >>= 1; ++s; }
    // bases 2..37 are a deterministic Miller-Rabin certificate below 2^64
    for (u64 base : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        u64 x = nt_powmod(base, d, v);
        if (x == 1 || x == v - 1) continue;
        bool witness = true;
        for (int i = 1; i < s && witness; ++i) {
            x = nt_mulmod(x, x, v);
            if (x == v - 1) witness = false;
        }
        if (witness) return false;
    }
    return true;
}
// util::get_primes (seal/util/numth.h:138-139): descending from the top of the bit size
bool nt_get_primes(u64 factor, int bits, size_t count, std::vector<u64> &out)
{
    out.clear();
    u64 cand = (((u64)1 << bits) - 1) / factor * factor + 1;
    const u64 floor_v = (u64)1 << (bits - 1);
    for (; out.size() < count && cand > floor_v; cand -= factor)
        if (nt_is_prime(cand)) out.push_back(cand);
    return out.size() == count;
}
// util::try_minimal_primitive_root (seal/util/numth.h:155-157)
u64 nt_minimal_primitive_root(u64 degree, u64 q)
{
    const u64 cofactor = (q - 1) / degree;
    u64 root = 0;
    for (u64 g = 2; g < q; ++g) {
        root = nt_powmod(g, cofactor, q);
        if (nt_powmod(root, degree / 2, q) == q - 1) break;
    }
    // all primitive roots are the odd powers of one of them
    const u64 step = nt_mulmod(root, root, q);
    u64 best = root, cur = root;
    for (u64 i = 1; i < degree / 2; ++i) {
        cur = nt_mulmod(cur, step, q);
        if (cur < best) best = cur;
    }
    return best;
}
// util::naf (seal/util/numth.h:22-42)
std::vector<int> nt_naf(int value)
{
    std::vector<int> terms;
    const bool neg = value < 0;
    unsigned v = (unsigned)std::abs(value);
    for (int bit = 0; v; ++bit) {
        int z = (v & 1u) ? 2 - (int)(v & 3u) : 0;
        v = (unsigned)((int)v - z) >> 1;
        if (z) terms.push_back((neg ? -z : z) * (1 << bit));
    }
    return terms;
}
// GaloisTool::get_elt_from_step (seal/util/galois.h:124)
u32 galois_elt_from_step(const hhe_ctx *c, int step)
{
    const u64 m = 2 * (u64)c->n;
    if (step == 0) return (u32)(m - 1);
    const u64 mag = (u64)std::abs(step);
    if (mag >= c->n / 2) return 0;
    const u64 e = step > 0 ? mag : c->n / 2 - mag;
    return (u32)nt_powmod(3, e, m);
}

static u64 bit_reverse(u64 v, int bits)
{
    u64 r = 0;
    for (int i = 0; i < bits; ++i, v >>= 1) r = (r << 1) | (v & 1);
    return r;
}
static u64 shoup_quot(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
static u64 product_mod(const std::vector<u64> &v, int skip, u64 m)
{
    u64 r = 1 % m;
    for (int i = 0; i < (int)v.size(); ++i)
        if (i != skip) r = nt_mulmod(r, v[i] % m, m);
    return r;
}

// ------------------------------------------------------------------ context
static void fill_mod(ModDev &md, u64 q, int logn, u64 t, bool with_tables, u64 *host_tab, const u64 *dev_tab, u64 *root_out)
{
    memset(&md, 0, sizeof(md));
    md.q = q;
    md.nq = 0 - q;
    const u128 two64 = (u128)1 << 64;
    md.r_hi = (u64)(two64 / q);
    md.r_lo = (u64)(((two64 % q) << 64) / q);
    {   // pseudo-Mersenne form q = 2^b - c (hhe_common.h ModDev::pm_*)
        int b = 0;
        while (b < 64 && (q >> b)) ++b;
        const u64 c = b < 64 ? ((u64)1 << b) - q : 0;
        if (b >= 33 && b <= 60 && c < ((u64)1 << 32) && (u128)c * (((u128)1 << (64 - b)) + 2) <= ((u128)1 << b)) {
            md.pm_sh = (u32)(b - 32); md.pm_mask = ((u32)1 << (b - 32)) - 1; md.pm_c = (u32)c; md.pm_ok = 1;
        }
    }
    if (!with_tables) return;
    const size_t n = (size_t)1 << logn;
    const u64 psi = nt_minimal_primitive_root(2 * n, q), ipsi = nt_invmod(psi, q);
    if (root_out) *root_out = psi;
    u64 *w = host_tab, *ws = host_tab + n, *iw = host_tab + 2 * n, *fw = host_tab + 4 * n;
    u64 pw = 1, ipw = 1;
    for (size_t k = 0; k < n; ++k) {
        const size_t r = bit_reverse(k, logn);
        w[r] = pw; ws[r] = shoup_quot(pw, q);
        fw[2 * r] = w[r]; fw[2 * r + 1] = ws[r];
        iw[2 * r] = ipw; iw[2 * r + 1] = shoup_quot(ipw, q);
        pw = nt_mulmod(pw, psi, q);
        ipw = nt_mulmod(ipw, ipsi, q);
    }
    md.ninv = nt_invmod(n % q, q);
    md.ninv_s = shoup_quot(md.ninv, q);
    md.ninv_t = nt_mulmod(md.ninv, t % q, q);
    md.ninv_t_s = shoup_quot(md.ninv_t, q);
    md.w = dev_tab; md.ws = dev_tab + n; md.iw = dev_tab + 2 * n; md.fw = dev_tab + 4 * n;
}

// CoeffModulus::BFVDefault(N) (seal/coeffmodulus via util/globals.cpp, SEAL 4.0.0) as used by
// SEALZpCipher::create_context (src/pasta/SEAL_Cipher.cpp:62-65) and the hard-coded N = 65536 chain (:50-60).
// N = 16384 is pinned by SURVEY A.10; every list is prime, = 1 mod 2N, and sums to the bit count of
// seal/util/hestdparms.h:seal_he_std_parms_128_tc (tests/test_abi.py).
extern "C" int hhe_bfv_default_coeff_modulus(size_t n, uint64_t *out, size_t *count)
{
    static const std::vector<u64> t1024 = {0x7e00001ULL}, t2048 = {0x3fffffff000001ULL},
        t4096 = {0xffffee001ULL, 0xffffc4001ULL, 0x1ffffe0001ULL},
        t8192 = {0x7fffffd8001ULL, 0x7fffffc8001ULL, 0xfffffffc001ULL, 0xffffff6c001ULL, 0xfffffebc001ULL},
        t16384 = {0xfffffffd8001ULL, 0xfffffffa0001ULL, 0xfffffff00001ULL, 0x1fffffff68001ULL, 0x1fffffff50001ULL,
                  0x1ffffffee8001ULL, 0x1ffffffea0001ULL, 0x1ffffffe88001ULL, 0x1ffffffe48001ULL},
        t32768 = {0x7fffffffe90001ULL, 0x7fffffffbf0001ULL, 0x7fffffffbd0001ULL, 0x7fffffffba0001ULL, 0x7fffffffaa0001ULL,
                  0x7fffffffa50001ULL, 0x7fffffff9f0001ULL, 0x7fffffff7e0001ULL, 0x7fffffff770001ULL, 0x7fffffff380001ULL,
                  0x7fffffff330001ULL, 0x7fffffff2d0001ULL, 0x7fffffff170001ULL, 0x7fffffff150001ULL, 0x7ffffffef00001ULL,
                  0xfffffffff70001ULL},
        t65536 = {0xffffffffffc0001ULL, 0xfffffffff840001ULL, 0xfffffffff6a0001ULL, 0xfffffffff5a0001ULL, 0xfffffffff2a0001ULL,
                  0xfffffffff240001ULL, 0xffffffffefe0001ULL, 0xffffffffeca0001ULL, 0xffffffffe9e0001ULL, 0xffffffffe7c0001ULL,
                  0xffffffffe740001ULL, 0xffffffffe520001ULL, 0xffffffffe4c0001ULL, 0xffffffffe440001ULL, 0xffffffffe400001ULL,
                  0xffffffffdda0001ULL, 0xffffffffdd20001ULL, 0xffffffffdbc0001ULL, 0xffffffffdb60001ULL, 0xffffffffd8a0001ULL,
                  0xffffffffd840001ULL, 0xffffffffd6e0001ULL, 0xffffffffd680001ULL, 0xffffffffd2a0001ULL, 0xffffffffd000001ULL,
                  0xffffffffcf00001ULL, 0xffffffffcea0001ULL, 0xffffffffcdc0001ULL, 0xffffffffcc40001ULL};
    const std::vector<u64> *t = nullptr;
    switch (n) {
    case 1024: t = &t1024; break;
    case 2048: t = &t2048; break;
    case 4096: t = &t4096; break;
    case 8192: t = &t8192; break;
    case 16384: t = &t16384; break;
    case 32768: t = &t32768; break;
    case 65536: t = &t65536; break;
    default: hhe_set_error("non-standard poly_modulus_degree"); return HHE_ERR_INVALID;
    }
    if (!count) return HHE_ERR_INVALID;
    if (out && *count >= t->size()) memcpy(out, t->data(), t->size() * 8);
    *count = t->size();
    return HHE_OK;
}

// hhe_ctx_query("behz_sum_cap"): the largest K <= 2^63 - 1 with
//     K N t Q (2^32 + 2L + 1)^2 + 2^65 L  <  2^65 B (floor(m_sk / 2) - L)
// (the condition of hhe_multiply_sum in hhe_gfx950.h, cleared of its fractions), 0 when not even K = 1 meets it.  Found by bisection
// over K with word-by-integer products, so no long division is needed.
static u64 behz_sum_cap(const std::vector<u64> &dq, const std::vector<u64> &Bq, u64 msk, u64 t, size_t n)
{
    typedef std::vector<u64> Big;  // little endian, no leading zero words
    auto mul = [](Big x, u64 m) {
        u64 carry = 0;
        for (u64 &w : x) { const u128 p = (u128)w * m + carry; w = (u64)p; carry = (u64)(p >> 64); }
        if (carry) x.push_back(carry);
        while (!x.empty() && !x.back()) x.pop_back();
        return x;
    };
    auto add = [](Big x, const Big &y) {
        if (x.size() < y.size()) x.resize(y.size(), 0);
        u64 carry = 0;
        for (size_t i = 0; i < x.size(); ++i) { const u128 s = (u128)x[i] + (i < y.size() ? y[i] : 0) + carry; x[i] = (u64)s; carry = (u64)(s >> 64); }
        if (carry) x.push_back(carry);
        return x;
    };
    auto less = [](const Big &x, const Big &y) {
        if (x.size() != y.size()) return x.size() < y.size();
        for (size_t i = x.size(); i-- > 0;)
            if (x[i] != y[i]) return x[i] < y[i];
        return false;
    };
    const u64 L = dq.size();
    if (msk / 2 <= L) return 0;
    Big rhs = {0, 2};  // 2^65
    for (u64 b : Bq) rhs = mul(rhs, b);
    rhs = mul(rhs, msk / 2 - L);
    const Big slack = {0, 2 * L};  // 2^65 L
    Big unit = {(u64)n};
    unit = mul(unit, t);
    for (u64 p : dq) unit = mul(unit, p);
    unit = mul(mul(unit, ((u64)1 << 32) + 2 * L + 1), ((u64)1 << 32) + 2 * L + 1);
    u64 lo = 0, hi = 0x7fffffffffffffffULL;  // lo is admitted (or 0), everything above hi is not
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (less(add(mul(unit, mid), slack), rhs)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

extern "C" int hhe_ctx_create(int logn, int K, const uint64_t *q, uint64_t t, int device, hhe_ctx **out)
{
    if (!out || !q || logn < 10 || logn > 16 || K < 2 || K > HHE_MAXK) {
        hhe_set_error("hhe_ctx_create: invalid arguments (need 10 <= logn <= 16, 2 <= K <= 33)");
        return HHE_ERR_INVALID;
    }
    const size_t n = (size_t)1 << logn;
    for (int i = 0; i < K; ++i)
        if (q[i] >> 61 || (q[i] - 1) % (2 * n) != 0 || !nt_is_prime(q[i])) {
            hhe_set_error("hhe_ctx_create: coeff modulus must be primes < 2^61 congruent to 1 mod 2N");
            return HHE_ERR_INVALID;
        }
    if (t >> 61 || (t - 1) % (2 * n) != 0 || !nt_is_prime(t)) {
        hhe_set_error("hhe_ctx_create: plain modulus must be a prime congruent to 1 mod 2N (batching)");
        return HHE_ERR_INVALID;
    }
    if (rt_set_device(device)) { hhe_set_error(rt_last_error()); return HHE_ERR_DEVICE; }
    hhe_ctx *c = new hhe_ctx();
    c->keys0.ctx = c;
    for (auto &ks : c->rk_slots) ks.ctx = c;
    keyset_new_serial(&c->keys0);
    for (auto &ks : c->rk_slots) keyset_new_serial(&ks);
    c->logn = logn; c->n = n; c->K = K; c->L = K - 1; c->t = t; c->device = device;
    c->q.assign(q, q + K);
    const int L = c->L;
    // BEHZ base (seal/util/rns.h): get_primes(2N, 61, L+2) = m_sk, gamma, B_0..B_{L-1}
    std::vector<u64> aux;
    if (!nt_get_primes(2 * n, 61, (size_t)L + 2, aux)) { delete c; hhe_set_error("no BEHZ primes"); return HHE_ERR_INVALID; }
    c->gamma = aux[1];
    c->bsk.assign(aux.begin() + 2, aux.end());
    c->bsk.push_back(aux[0]);
    c->nmod = K + (L + 1) + 1;
    c->mod_t = K + L + 1;

    std::vector<u64> allq(c->q);
    allq.insert(allq.end(), c->bsk.begin(), c->bsk.end());
    allq.push_back(t);
    std::vector<ModDev> mods(c->nmod);
    c->pm_ok.assign(c->nmod, 0);
    std::vector<u64> host_tab((size_t)c->nmod * 6 * n);
    c->d_tables = (u64 *)rt_malloc(host_tab.size() * 8);
    c->d_mods = (ModDev *)rt_malloc(sizeof(ModDev) * c->nmod);
    c->roots.resize(K);
    for (int i = 0; i < c->nmod; ++i)
        fill_mod(mods[i], allq[i], logn, t, true, host_tab.data() + (size_t)i * 6 * n, c->d_tables + (size_t)i * 6 * n,
                 i < K ? &c->roots[i] : nullptr);
    for (int i = 0; i < c->nmod; ++i) c->pm_ok[i] = (int)mods[i].pm_ok;
    // BatchEncoder matrix_reps_index_map
    c->slot_map.resize(n);
    {
        const u64 m = 2 * n;
        u64 pos = 1;
        for (size_t i = 0; i < n / 2; ++i) {
            c->slot_map[i] = (u32)bit_reverse((pos - 1) >> 1, logn);
            c->slot_map[n / 2 + i] = (u32)bit_reverse((m - pos - 1) >> 1, logn);
            pos = pos * 3 % m;
        }
    }
    c->d_slot_map = (u32 *)rt_malloc(4 * n);
    c->d_slot_inv = (u32 *)rt_malloc(4 * n);
    c->d_fin = (FinArgs *)rt_malloc(sizeof(FinArgs));
    std::vector<u32> slot_inv(n);
    for (size_t i = 0; i < n; ++i) slot_inv[c->slot_map[i]] = (u32)i;

    std::vector<u64> dq(c->q.begin(), c->q.begin() + L), Bq(c->bsk.begin(), c->bsk.begin() + L);
    const u64 msk = c->bsk[L], MT = (u64)1 << 32;
    // hhe_multiply_sum: the most products one floor takes, and the reduction intervals of its sums under the two modulus sets
    c->behz_sum_cap = behz_sum_cap(dq, Bq, msk, t, n);
    auto widest = [](const std::vector<u64> &ps) {
        int bits = 0;
        for (u64 p : ps) bits = std::max(bits, 64 - __builtin_clzll(p));
        return bits;
    };
    c->sum_fold_q = tensor_sum_fold(widest(dq));
    c->sum_fold_bsk = tensor_sum_fold(widest(c->bsk));
    // add_plain scaling variant
    AddPlainArgs &ap = c->apl;
    memset(&ap, 0, sizeof(ap));
    ap.t = t; ap.q_mod_t = product_mod(dq, -1, t); ap.thr = (t + 1) >> 1;
    {
        const u128 two64 = (u128)1 << 64;
        ap.t_r_hi = (u64)(two64 / t);
        ap.t_r_lo = (u64)(((two64 % t) << 64) / t);
    }
    for (int j = 0; j < L; ++j) {
        // floor(Q/t) mod q_j = -(Q mod t) * t^-1 mod q_j  (Q = 0 mod q_j)
        const u64 v = nt_mulmod(ap.q_mod_t % dq[j], nt_invmod(t % dq[j], dq[j]), dq[j]);
        ap.delta[j] = v ? dq[j] - v : 0;
    }
    // key-switch mod-down
    KsFinishArgs &kf = c->ksf;
    memset(&kf, 0, sizeof(kf));
    const u64 qsp = c->q[K - 1];
    kf.half = qsp >> 1;
    for (int j = 0; j < L; ++j) {
        kf.half_mod[j] = kf.half % dq[j];
        kf.qsp_inv[j] = nt_invmod(qsp % dq[j], dq[j]);
        kf.qsp_inv_s[j] = shoup_quot(kf.qsp_inv[j], dq[j]);
    }
    // BEHZ constants
    BehzDev bz;
    memset(&bz, 0, sizeof(bz));
    bz.L = L; bz.msk = msk;
    for (int i = 0; i < L; ++i) {
        bz.inv_punct_q[i] = nt_invmod(product_mod(dq, i, dq[i]), dq[i]);
        bz.inv_punct_q_s[i] = shoup_quot(bz.inv_punct_q[i], dq[i]);
        bz.mt_mod_q[i] = MT % dq[i];
        for (int p = 0; p <= L; ++p) bz.punct_q_bsk[i][p] = product_mod(dq, i, c->bsk[p]);
        bz.punct_q_mt[i] = product_mod(dq, i, MT);
        bz.inv_punct_B[i] = nt_invmod(product_mod(Bq, i, Bq[i]), Bq[i]);
        for (int j = 0; j < L; ++j) bz.punct_B_q[i][j] = product_mod(Bq, i, dq[j]);
        bz.punct_B_msk[i] = product_mod(Bq, i, msk);
        bz.B_mod_q[i] = product_mod(Bq, -1, dq[i]);
        bz.neg_B_mod_q[i] = dq[i] - bz.B_mod_q[i];
    }
    bz.neg_inv_q_mt = (MT - nt_invmod(product_mod(dq, -1, MT), MT)) & (MT - 1);
    for (int p = 0; p <= L; ++p) {
        const u64 P = c->bsk[p];
        bz.q_mod_bsk[p] = product_mod(dq, -1, P);
        bz.inv_mt_bsk[p] = nt_invmod(MT % P, P);
        bz.inv_q_bsk[p] = nt_invmod(bz.q_mod_bsk[p], P);
    }
    bz.inv_B_msk = nt_invmod(product_mod(Bq, -1, msk), msk);
    c->d_behz = (BehzDev *)rt_malloc(sizeof(BehzDev));
    // modulus switching (Evaluator::mod_switch_to_next): dropping q_m rescales every limb j < m by q_m^-1 mod q_j
    std::vector<u64> moddown(mod_down_table_words(L), 0);
    for (int m = 1; m < L; ++m)
        for (int j = 0; j < m; ++j) {
            u64 *e = moddown.data() + mod_down_pair(m, j);
            e[0] = nt_invmod(dq[m] % dq[j], dq[j]);
            e[1] = shoup_quot(e[0], dq[j]);
            e[2] = (dq[m] >> 1) % dq[j];
        }
    c->d_moddown = (u64 *)rt_malloc(moddown.size() * 8);
    // the fused finishing pass of a transciphering call reads the add_plain constants from device memory
    FinArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.slot_inv = c->d_slot_inv; fa.count = PASTA_T; fa.L = L;
    fa.t = ap.t; fa.q_mod_t = ap.q_mod_t; fa.thr = ap.thr; fa.t_r_lo = ap.t_r_lo; fa.t_r_hi = ap.t_r_hi;
    for (int j = 0; j < L; ++j) fa.delta[j] = ap.delta[j];
    // ... and, for the one-workgroup form, the inverse powers mod t as 32-bit words with 32-bit Shoup quotients
    std::vector<u32> itw;
    if (fin_item_ok(logn, t)) {
        const u64 *iw = host_tab.data() + (size_t)c->mod_t * 6 * n + 2 * n;
        itw.resize(2 * n);
        for (size_t k = 0; k < n; ++k) { itw[2 * k] = (u32)iw[2 * k]; itw[2 * k + 1] = (u32)((iw[2 * k] << 32) / t); }
        c->d_fin_itw = (u32 *)rt_malloc(8 * n);
        fa.slot_map = c->d_slot_map; fa.itw = c->d_fin_itw;
        // ... and the quotients of its 32-bit plaintext scaling (HHE_FIN_SCALE32=0: the shared 128-bit definition, as every ineligible context)
        const char *e = getenv("HHE_FIN_SCALE32");
        if (fin_scale32_ok(logn, t, dq.data(), L) && !(e && atoi(e) == 0)) {
            fin_scale32_fill(fa, dq.data(), L);
            c->fin_scale32 = true;
        }
    }

    if (!c->d_tables || !c->d_mods || !c->d_slot_map || !c->d_behz || !c->d_slot_inv || !c->d_fin || !c->d_moddown ||
        rt_h2d(c->d_moddown, moddown.data(), moddown.size() * 8, nullptr) ||
        (!itw.empty() && (!c->d_fin_itw || rt_h2d(c->d_fin_itw, itw.data(), 8 * n, nullptr))) ||
        rt_h2d(c->d_slot_inv, slot_inv.data(), 4 * n, nullptr) || rt_h2d(c->d_fin, &fa, sizeof(fa), nullptr) ||
        rt_h2d(c->d_tables, host_tab.data(), host_tab.size() * 8, nullptr) ||
        rt_h2d(c->d_mods, mods.data(), sizeof(ModDev) * c->nmod, nullptr) ||
        rt_h2d(c->d_slot_map, c->slot_map.data(), 4 * n, nullptr) ||
        rt_h2d(c->d_behz, &bz, sizeof(bz), nullptr) || rt_sync(nullptr)) {
        hhe_set_error(std::string("hhe_ctx_create: device setup failed: ") + rt_last_error());
        hhe_ctx_destroy(c);
        return HHE_ERR_DEVICE;
    }
    c->ksc.half = kf.half;
    for (int j = 0; j < L; ++j) {
        c->ksc.half_mod[j] = kf.half_mod[j]; c->ksc.qsp_inv[j] = kf.qsp_inv[j]; c->ksc.qsp_inv_s[j] = kf.qsp_inv_s[j];
        c->ksc.qsp_mod[j] = qsp % dq[j]; c->ksc.qsp_mod_s[j] = shoup_quot(c->ksc.qsp_mod[j], dq[j]);
        c->ksc.ninv_qinv[j] = nt_mulmod(mods[j].ninv, kf.qsp_inv[j], dq[j]);
        c->ksc.ninv_qinv_s[j] = shoup_quot(c->ksc.ninv_qinv[j], dq[j]);
        c->ksc.hq2[j] = 2 * dq[j] + nt_mulmod(kf.half_mod[j], kf.qsp_inv[j], dq[j]);
    }
    if (const char *mm = getenv("HHE_MATMUL")) c->matmul_mode = atoi(mm);
    if (const char *e = getenv("HHE_SHARED_L0")) c->shared_l0 = std::max(0, atoi(e));
    if (const char *e = getenv("HHE_DEDUP")) c->dedup = atoi(e) != 0;
    if (const char *e = getenv("HHE_PUBLIC_DEVICE")) c->public_device = atoi(e) != 0;
    if (const char *e = getenv("HHE_KS_CACHE")) c->ks_cache.enabled = atoi(e) != 0;
    if (const char *e = getenv("HHE_FIN_FUSED")) c->fin_fused = atoi(e) != 0;
    if (const char *e = getenv("HHE_FIN_ITEM")) c->fin_item = atoi(e) != 0;
    if (const char *e = getenv("HHE_KS_CACHE_MB")) c->ks_cache.budget = (size_t)(std::max(0.0, atof(e)) * (double)(1 << 20));
    c->ks_cache.entry_bytes = c->ct_words() * 8;
    if (const char *e = getenv("HHE_SHARED_L0_MB")) c->l0_budget = (size_t)(std::max(0.0, atof(e)) * (double)(1 << 20));
    if (const char *e = getenv("HHE_BLOCK_CACHE_MB")) c->block_cache_limit = (size_t)std::max(0, atoi(e)) << 20;
    if (const char *e = getenv("HHE_FC_ROWFUSED")) c->fc_row_fused = atoi(e);
    if (const char *e = getenv("HHE_FC_CSUM")) c->fc_csum = atoi(e);
    if (const char *e = getenv("HHE_FC_C0HAT")) c->fc_c0hat = atoi(e);
    if (const char *e = getenv("HHE_FC_CSUMGROUP")) c->fc_csum_group = std::max(1, std::min(HHE_CSUM_GROUP, atoi(e)));
    if (const char *e = getenv("HHE_FC_LEAFSUM")) c->fc_leaf_sums = atoi(e);
    if (const char *e = getenv("HHE_FC_LEAFGROUP")) c->fc_leaf_group = std::max(1, std::min(HHE_LEAF_GROUP, atoi(e)));
    if (const char *e = getenv("HHE_FC_SHARED")) c->fc_shared = atoi(e);
    if (const char *e = getenv("HHE_ROT_HOIST")) c->rot_hoist = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("HHE_FC_CHUNK")) c->fc_chunk = (size_t)std::max(0, atoi(e));
    if (const char *e = getenv("HHE_STREAMS")) c->nstreams = std::max(0, std::min(HHE_MAX_STREAMS, atoi(e)));
    if (const char *e = getenv("HHE_CHUNK")) c->chunk = (size_t)std::max(1, atoi(e));
    for (int s = 1; s <= c->nstreams; ++s) {
        c->lanes[s].stream = rt_stream_create();
        c->lanes[s].own_stream = true;
        c->lanes[s].ev_done = rt_event_create();
    }
    c->ev_fork = rt_event_create();
    c->ev_cmp = rt_event_create();
    {   // a digit d_I < q_I may enter NTT_J unreduced when q_I < 4 q_J (butterfly inputs live in [0,4q))
        u64 qmax = 0, qmin = ~(u64)0;
        for (int i = 0; i < L; ++i) qmax = std::max(qmax, c->q[i]);
        for (int i = 0; i < K; ++i) qmin = std::min(qmin, c->q[i]);
        c->digit_reduce = (qmax / 4 >= qmin) ? 1 : 0;
    }
    kf.mods = c->d_mods; kf.logn = logn; kf.L = L; kf.K = K;
    ap.mods = c->d_mods; ap.logn = logn; ap.L = L;
    *out = c;
    return HHE_OK;
}

// SEAL's level with `limbs` data primes is the BFV context over {q_0 .. q_{limbs-1}, q_sp}: the same derivation on the shorter list.
// get_primes(2N, 61, limbs + 2) is a prefix of the parent's draw, so the level's BEHZ base is a prefix of the parent's with the same
// m_sk and gamma.  Nothing is shared with the parent: the level has its own tables, lock, workspaces, stream and caches.
extern "C" int hhe_ctx_create_level(const hhe_ctx *c, int limbs, hhe_ctx **out)
{
    std::vector<u64> q;
    int logn, device;
    u64 t;
    {
        HHE_LOCK(c);
        if (!c || !out || limbs < 1 || limbs > c->L) {
            hhe_set_error("hhe_ctx_create_level: need a context, 1 <= limbs <= L and an output pointer");
            return HHE_ERR_INVALID;
        }
        q.assign(c->q.begin(), c->q.begin() + limbs);
        q.push_back(c->q[c->K - 1]);
        logn = c->logn; device = c->device; t = c->t;
    }
    return hhe_ctx_create(logn, limbs + 1, q.data(), t, device, out);
}

static void free_lane(Lane &ln)
{
    rt_free(ln.ws_T); rt_free(ln.ws_S); rt_free(ln.ws_d); rt_free(ln.ws_ct3); rt_free(ln.ws_plain); rt_free(ln.ws_vals);
    for (auto &p : ln.ws_ct) { rt_free(p); p = nullptr; }
    ln.ws_rot.release(); ln.ws_aff.release(); ln.ws_fcp.release(); ln.ws_rotm.release(); ln.ws_leaf.release();
    for (auto &sl : ln.fc_slots) { rt_free(sl.tp); rt_free(sl.ct); rt_free(sl.c0hat); }
    ln.fc_slots.clear(); ln.fc_slot_cap = 0;
    for (u64 *p : ln.csum_bufs) rt_free(p);
    ln.csum_bufs.clear();
    rt_free((void *)ln.d_ptrs); ln.d_ptrs = nullptr; ln.ptr_cap = 0;
    for (auto &pr : ln.prof_ev) { rt_event_destroy(pr.first); rt_event_destroy(pr.second); }
    ln.prof_ev.clear(); ln.prof_used = 0;
    rt_free(ln.bz_aq); rt_free(ln.bz_bq); rt_free(ln.bz_ab); rt_free(ln.bz_bb); rt_free(ln.bz_dq); rt_free(ln.bz_db);
    ln.ws_T = ln.ws_S = ln.ws_d = ln.ws_ct3 = ln.ws_plain = ln.ws_vals = nullptr;
    ln.bz_aq = ln.bz_bq = ln.bz_ab = ln.bz_bb = ln.bz_dq = ln.bz_db = nullptr;
    ln.cap = 0;
}
void sync_ctx(hhe_ctx *c)
{
    for (auto &ln : c->lanes) {
        if (&ln == &c->lanes[0] || ln.own_stream) rt_sync(ln.stream);
    }
}

// device block and host staging of the finishing pass of a transciphering call of B items
int fin_reserve(hhe_ctx *c, size_t B)
{
    bool grew;
    int rc = c->fin_dev.reserve(c, fin_tab_words(B) + B * (PASTA_T + c->n), "transciphering: finishing pass", &grew);
    if (grew || rc) c->fin_tab_shadow.clear();  // a new block holds no table
    if (!rc) rc = c->fin_host.reserve(c, KsCache::MAX_SNAPSHOTS + fin_tab_words(B) + B * PASTA_T, "transciphering: finishing pass");
    return rc;
}

int lane_reserve(hhe_ctx *c, Lane &ln, size_t B)
{
    if (B == 0) { hhe_set_error("empty batch"); return HHE_ERR_INVALID; }
    if (B <= ln.cap) return HHE_OK;
    sync_ctx(c);
    free_lane(ln);
    const size_t n = c->n, L = c->L, K = c->K;
    auto alloc = [&](size_t words) { return (u64 *)rt_malloc(words * 8); };
    bool ok = true;
    ok &= !!(ln.ws_T = alloc(B * L * K * n));
    ok &= !!(ln.ws_S = alloc(B * 2 * K * n));
    ok &= !!(ln.ws_d = alloc(B * L * n));
    // the fused matmul loop carves ws_ct[3] into scr [B][L][N] | r [B][2][N] (matmul_diagonal_fused): L + 2 polynomials per item, which
    // is more than a ciphertext's 2 L at L = 1 (a context of two primes, e.g. the last level of a chain)
    for (auto &p : ln.ws_ct) ok &= !!(p = alloc(B * std::max<size_t>(2 * L, L + 2) * n));
    ok &= !!(ln.ws_ct3 = alloc(B * 3 * L * n));
    ok &= !!(ln.ws_plain = alloc(B * n));
    ok &= !!(ln.ws_vals = alloc(B * PASTA_T));
    ok &= !!(ln.bz_aq = alloc(B * 2 * L * n));
    ok &= !!(ln.bz_bq = alloc(B * 2 * L * n));
    ok &= !!(ln.bz_ab = alloc(B * 2 * (L + 1) * n));
    ok &= !!(ln.bz_bb = alloc(B * 2 * (L + 1) * n));
    ok &= !!(ln.bz_dq = alloc(B * 3 * L * n));
    ok &= !!(ln.bz_db = alloc(B * 3 * (L + 1) * n));
    ok &= !!(ln.d_ptrs = (const u64 **)rt_malloc(2 * B * sizeof(u64 *)));
    ln.ptr_cap = B;
    if (!ok) { free_lane(ln); hhe_set_error(std::string("workspace allocation failed: ") + rt_last_error()); return HHE_ERR_DEVICE; }
    ln.cap = B;
    return HHE_OK;
}

extern "C" void hhe_pasta3_clear_block_cache(hhe_ctx *c)
{
    HHE_LOCK(c);
    if (!c) return;
    sync_ctx(c);
    for (auto &kv : c->blocks) { rt_free(kv.second.diag); rt_free(kv.second.pdiag); rt_free(kv.second.rc); rt_free(kv.second.bsgs); }
    c->blocks.clear();
    c->block_bytes = 0;
    c->ks_cache.clear(c);  // a kept keystream belongs to its counter's tables
}
// the keystream ciphertexts kept across transciphering calls, and the copies of the key ciphertexts they belong to; the block tables stay
extern "C" void hhe_pasta3_clear_keystream_cache(hhe_ctx *c)
{
    HHE_LOCK(c);
    if (!c) return;
    c->ks_cache.clear(c);
}

extern "C" void hhe_ctx_destroy(hhe_ctx *c)
{
    if (!c) return;
    sync_ctx(c);
    hhe_pasta3_clear_block_cache(c);
    for (auto &ln : c->lanes) {
        free_lane(ln);
        rt_event_destroy(ln.ev_done);
        rt_event_destroy(ln.ev_stage);
        if (ln.own_stream) rt_stream_destroy(ln.stream);
    }
    rt_event_destroy(c->ev_fork);
    rt_event_destroy(c->ev_cmp);
    keyset_clear(&c->keys0);
    for (auto &ks : c->rk_slots) keyset_clear(&ks);
    for (hhe_keyset *ks : c->sets) { keyset_clear(ks); delete ks; }  // sets the caller did not destroy
    for (hhe_matrix *m : c->mats) matrix_free(m);  // handles the caller did not destroy
    for (hhe_enc_matrix *m : c->enc_mats) enc_matrix_free(m);
    for (hhe_plain_rows *p : c->plain_rows) plain_rows_free(p);
    for (hhe_plain_fc *m : c->plain_fcs) plain_fc_free(m);
    for (auto &kv : c->d_key_shoup) rt_free(kv.second);
    rt_free(c->d_feistel_mask);
    rt_free(c->d_zero_corr);
    rt_free(c->d_qsp_poly);
    c->d_blocks.release(); c->d_flags.release(); c->d_rot_kids.release();
    c->l0_tab.release(); c->l0_ptrs.release();
    c->ks_tab.release(); c->ks_flags.release(); c->fin_dev.release(); c->fin_host.release();
    rt_free(c->d_tables); rt_free(c->d_mods); rt_free(c->d_behz); rt_free(c->d_slot_map); rt_free(c->d_slot_inv); rt_free(c->d_fin); rt_free(c->d_fin_itw);
    rt_free(c->d_moddown);
    delete c;
}

extern "C" int hhe_ctx_set_stream(hhe_ctx *c, void *s)
{
    HHE_LOCK(c);
    if (!c) return HHE_ERR_INVALID;
    c->lanes[0].stream = (rt_stream)s;
    return HHE_OK;
}
extern "C" int hhe_ctx_sync(hhe_ctx *c)
{
    HHE_LOCK(c);
    if (!c) return HHE_ERR_INVALID;
    if (rt_sync(c->lanes[0].stream)) { hhe_set_error(rt_last_error()); return HHE_ERR_DEVICE; }
    return HHE_OK;
}

// Timing of the dominant kernel on the stream it is launched on (bench.py's roofline block): while enabled, every launch
// of ks_row_kernel is bracketed by a pair of timed HIP events.  Results are unaffected.
extern "C" int hhe_ctx_profile(hhe_ctx *c, int enable)
{
    HHE_LOCK(c);
    if (!c) return HHE_ERR_INVALID;
    sync_ctx(c);
    c->profile = enable ? 1 : 0;
    c->prof_items = 0;
    for (auto &ln : c->lanes) ln.prof_used = 0;
    return HHE_OK;
}
extern "C" int hhe_ctx_profile_read(hhe_ctx *c, char *kernel_name, size_t name_cap, uint64_t *launches, double *total_ms, uint64_t *items)
{
    HHE_LOCK(c);
    if (!c || !launches || !total_ms || !items) return HHE_ERR_INVALID;
    sync_ctx(c);
    uint64_t n = 0;
    double ms = 0;
    for (auto &ln : c->lanes) {
        for (size_t i = 0; i < ln.prof_used; ++i) {
            const float t = rt_event_elapsed_ms(ln.prof_ev[i].first, ln.prof_ev[i].second);
            if (t < 0) { hhe_set_error(rt_last_error()); return HHE_ERR_DEVICE; }
            ms += t;
            ++n;
        }
        ln.prof_used = 0;
    }
    *launches = n; *total_ms = ms; *items = c->prof_items;
    c->prof_items = 0;
    if (kernel_name && name_cap) {
        int n1, n2;
        ntt_split(c->logn, n1, n2);
        snprintf(kernel_name, name_cap, "void ks_row_kernel<%d>(NttArgs, KsRowArgs, NttArgs)", n2);  // as rocprofv3 prints it
    }
    return HHE_OK;
}

extern "C" int hhe_ctx_reserve(hhe_ctx *c, size_t B)
{
    HHE_LOCK(c);
    if (!c || B == 0) return HHE_ERR_INVALID;
    if (int rc = fin_reserve(c, B)) return rc;
    // generic ops run whole batches on lane 0; the transciphering path works in chunks on the internal lanes
    if (c->nstreams > 0) {
        const size_t per = std::min(B, c->chunk);
        for (int s = 1; s <= c->nstreams; ++s) {
            int rc = lane_reserve(c, c->lanes[s], per);
            if (rc) return rc;
        }
        return HHE_OK;
    }
    return lane_reserve(c, c->lanes[0], B);
}

extern "C" uint64_t hhe_ctx_query(const hhe_ctx *c, const char *what, int i)
{
    HHE_LOCK(c);
    if (!c || !what) return 0;
    const std::string w(what);
    if (w == "root" && i >= 0 && i < c->K) return c->roots[i];
    if (w == "bsk" && i >= 0 && i <= c->L) return c->bsk[i];
    if (w == "gamma") return c->gamma;
    if (w == "galois_elt") return galois_elt_from_step(c, i);
    if (w == "delta" && i >= 0 && i < c->L) return c->apl.delta[i];
    if (w == "slot_map" && i >= 0 && (size_t)i < c->n) return c->slot_map[i];
    if (w == "fc_fallbacks") return c->fc_fallbacks;
    if (w == "fc_csum_closes") return c->fc_csum_closes;
    if (w == "block_cache_bytes") return c->block_bytes;
    if (w == "block_cache_entries") return c->blocks.size();
    if (w == "row_kernel") return use_row_kernel(c) ? 1 : 0;
    if (w == "shared_l0") return (u64)c->shared_l0;       // smallest batch that takes the shared first layer (0: none)
    if (w == "shared_l0_steps") return c->l0_steps();   // steps per block of the operand table of the last shared first layer (0: none ran)
    if (w == "dedup") return (u64)c->dedup;               // 1: one keystream evaluation per distinct block counter of a call
    if (w == "transcipher_unique") return c->last_unique; // distinct counters of the last transciphering call (its item count when it ran per item)
    if (w == "transcipher_evaluated") return c->last_evaluated;  // keystream chains the last call ran: the counters it found no kept keystream for
    if (w == "fin_fused") return fin_fused_on(c) ? 1 : 0;        // the finishing pass of a transciphering call runs as two fused kernels (HHE_FIN_FUSED)
    if (w == "fin_item") return fin_item_on(c) ? 1 : 0;          // ... or as one kernel with one workgroup per item, from query("fin_item_min") items on (HHE_FIN_ITEM)
    if (w == "fin_item_min") return fin_item_on(c) ? (c->fin_item > 0 ? 1 : (u64)c->fin_item_min) : 0;
    if (w == "fin_item_launches") return c->fin_item_launches;
    if (w == "fin_tab_uploads") return c->fin_tab_uploads;       // uploads of a finishing pass's pointer table or map that were enqueued: one the device already holds is skipped
    if (w == "fin_word_uploads") return c->fin_word_uploads;     // uploads of the items' words: none where the item kernel reads them in the page-locked staging
    if (w == "fin_scale32") return fin_item_on(c) && c->fin_scale32 ? 1 : 0;  // ... with the plaintext scaled by 32-bit products and -c1 written early (HHE_FIN_SCALE32; t < 2^30 below every data prime)
    if (w == "mod_switch_launches") return c->mod_switch_launches;  // kernel launches of hhe_mod_switch: one per call of up to one chunk
    if (w == "key_proj_launches") return c->key_proj_launches;      // kernel launches of hhe_keyset_derive_level into this context's sets: one per key
    if (w == "fc_packed_key_switches") return c->fc_packed_key_switches;  // Galois key switches per item of the last hhe_fc_packed_ks call
    if (w == "rot_hoist") return c->rot_hoist;
    if (w == "rot_many_fallbacks") return c->rot_many_fallbacks;
    if (w == "rot_many_key_switches") return c->rot_many_key_switches;  // of the last hhe_rotate_rows_many_ks / hhe_fc_packed_hoisted_ks call: nodes of its trie
    if (w == "rot_many_launches") return c->rot_many_launches;          // ... and its multi-child launches of ks_perm_row_kernel per chunk
    if (w == "rot_many_group") return HHE_ROT_GROUP;                    // children one such launch serves at most
    if (w == "plain_sum_fold") return PLAIN_SUM_FOLD;                   // children between two folds of the outer sums of ks_plain_sum_row_kernel
    if (w == "plain_sum_fallbacks") return c->plain_sum_fallbacks;      // chunks of the plain-weights sum recomputed from per-child digits
    if (w == "plain_sum_launches") return c->plain_sum_launches;        // of the last such call: launches of ks_plain_sum_row_kernel per chunk (0: separate launches)
    if (w == "plain_sum_mod_downs") return c->plain_sum_mod_downs;      // ... and finish launches of the primitive per chunk
    if (w == "add_many_launches") return c->add_many_launches;            // launches of the sum kernel (hhe_add_many: one per call)
    if (w == "behz_sum_cap") return c->behz_sum_cap;                      // most products hhe_multiply_sum sums under one floor (K = 1 is always served)
    if (w == "multiply_sum_fold_q") return (u64)c->sum_fold_q;            // addends between two reductions of its sums: under the data primes,
    if (w == "multiply_sum_fold_bsk") return (u64)c->sum_fold_bsk;        // ... under the B_sk primes
    if (w == "multiply_sum_launches") return c->multiply_sum_launches;    // launches of the summed tensor kernel: one per modulus set per call or chunk
    if (w == "fc_packed_floors") return c->fc_packed_floors;              // polynomials floored per item of the last packed encrypted FC call
    if (w == "tensor_launches") return c->tensor_launches;                // launches of tensor_kernel / tensor_bcast_kernel: two per BEHZ product of two operands
    if (w == "square_launches") return c->square_launches;                // launches of tensor_square_kernel: two per hhe_square
    if (w == "mlp_layers") return c->mlp_layers;                          // layers of the last hhe_mlp_ks call
    if (w == "mlp_key_switches") return c->mlp_key_switches;              // ... and its Galois key switches per item, summed over the layers
    if (w == "noise_form") return (u64)c->noise_form;  // the last hhe_noise_budget launch: limb count of its register form, 0 = the LDS form
    if (w == "public_device") return (u64)(int64_t)c->public_device;  // HHE_PUBLIC_DEVICE: 0 host, 1 device; unset: (uint64_t)-1, the path is chosen per call
    if (w == "public_device_built") return c->last_public_built;     // pairs whose randomness the last call drew on the device
    if (w == "transcipher_groups") return c->last_groups;            // groups the last transciphering call ran in (1 through the entries without nonces)
    if (w == "ks_cache") return c->ks_cache.enabled ? 1 : 0;      // keystreams are kept across calls (HHE_KS_CACHE)
    if (w == "ks_cache_hits") return c->last_hits;                // counters of the last call served from a kept keystream
    if (w == "ks_cache_entries") return c->ks_cache.entries();
    if (w == "ks_cache_bytes") return c->ks_cache.bytes;
    if (w == "pm_ok" && i >= 0 && i < c->K) return (u64)c->pm_ok[i];
    if (w == "digit_reduce") return (u64)c->digit_reduce;
    return 0;
}

// ------------------------------------------------------------------ key sets
// drop what was derived from the words at `key` (its Shoup table); every stream must be done with them first
static void forget_key(hhe_ctx *c, const u64 *key)
{
    auto sh = c->d_key_shoup.find(key);
    if (sh != c->d_key_shoup.end()) { rt_free(sh->second); c->d_key_shoup.erase(sh); }
}
// The kernels multiply key words through Shoup quotients, which are only right for words below their prime: a key that is not
// reduced is refused (SEAL's safe load does the same, is_data_valid_for).
static int check_key_words(const hhe_ctx *c, const uint64_t *ksk)
{
    const size_t n = c->n;
    for (size_t p = 0; p < (size_t)c->L * 2 * c->K; ++p) {
        const u64 qj = c->q[p % c->K];
        const uint64_t *w = ksk + p * n;
        u64 bad = 0;
        for (size_t i = 0; i < n; ++i) bad |= (u64)(w[i] >= qj);
        if (bad) { hhe_set_error("key-switch key data is not reduced modulo the coefficient primes"); return HHE_ERR_INVALID; }
    }
    return HHE_OK;
}
static int upload_key(hhe_ctx *c, u64 *&slot, const uint64_t *ksk)
{
    int rc = check_key_words(c, ksk);
    if (rc) return rc;
    sync_ctx(c);  // a resident key may still be read by work in flight on any lane
    if (slot) forget_key(c, slot);
    if (!slot) slot = (u64 *)rt_malloc(c->ksk_words() * 8);
    if (!slot || rt_h2d(slot, ksk, c->ksk_words() * 8, c->lanes[0].stream) || rt_sync(c->lanes[0].stream)) {
        hhe_set_error(std::string("key upload failed: ") + rt_last_error());
        return HHE_ERR_DEVICE;
    }
    return HHE_OK;
}
void keyset_new_serial(hhe_keyset *ks)
{
    hhe_ctx *c = ks->ctx;
    if (ks->serial) c->ks_cache.drop_serial(c, ks->serial);
    ks->serial = ++c->next_serial;
}
int keyset_put_relin(hhe_keyset *ks, const u64 *ksk)
{
    keyset_new_serial(ks);
    return upload_key(ks->ctx, ks->rk, ksk);
}
int keyset_put_galois(hhe_keyset *ks, u32 elt, const u64 *ksk)
{
    hhe_ctx *c = ks->ctx;
    if (!(elt & 1) || elt >= 2 * c->n) { hhe_set_error("invalid Galois element"); return HHE_ERR_INVALID; }
    int rc = check_key_words(c, ksk);
    if (rc) return rc;
    auto corr = ks->gk_corr.find(elt);  // derived from the key being replaced
    if (corr != ks->gk_corr.end()) { sync_ctx(c); rt_free(corr->second); ks->gk_corr.erase(corr); }
    auto it = ks->gk.find(elt);
    u64 *slot = it == ks->gk.end() ? nullptr : it->second;
    const bool fresh = slot == nullptr;
    keyset_new_serial(ks);
    rc = upload_key(c, slot, ksk);
    if (rc && fresh) { rt_free(slot); return rc; }  // a key that did not arrive is not registered
    ks->gk[elt] = slot;
    return rc;
}
static void adopt_key(hhe_ctx *c, u64 *&slot, u64 *key)
{
    sync_ctx(c);  // a resident key may still be read by work in flight on any lane
    if (slot) { forget_key(c, slot); rt_free(slot); }
    slot = key;
}
void keyset_adopt_relin(hhe_keyset *ks, u64 *key)
{
    keyset_new_serial(ks);
    adopt_key(ks->ctx, ks->rk, key);
}
void keyset_adopt_galois(hhe_keyset *ks, u32 elt, u64 *key)
{
    hhe_ctx *c = ks->ctx;
    auto corr = ks->gk_corr.find(elt);  // derived from the key being replaced
    if (corr != ks->gk_corr.end()) { sync_ctx(c); rt_free(corr->second); ks->gk_corr.erase(corr); }
    keyset_new_serial(ks);
    u64 *slot = nullptr;
    auto it = ks->gk.find(elt);
    if (it != ks->gk.end()) slot = it->second;
    adopt_key(c, slot, key);
    ks->gk[elt] = slot;
}
void keyset_clear(hhe_keyset *ks)
{
    hhe_ctx *c = ks->ctx;
    keyset_new_serial(ks);
    if (ks->rk) { forget_key(c, ks->rk); rt_free(ks->rk); ks->rk = nullptr; }
    for (auto &kv : ks->gk) { forget_key(c, kv.second); rt_free(kv.second); }
    for (auto &kv : ks->gk_corr) rt_free(kv.second);
    ks->gk.clear();
    ks->gk_corr.clear();
}
extern "C" int hhe_keyset_create(hhe_ctx *c, hhe_keyset **out)
{
    HHE_LOCK(c);
    if (!c || !out) { hhe_set_error("hhe_keyset_create: null argument"); return HHE_ERR_INVALID; }
    hhe_keyset *ks = new hhe_keyset();
    ks->ctx = c;
    keyset_new_serial(ks);
    c->sets.push_back(ks);
    *out = ks;
    return HHE_OK;
}
extern "C" void hhe_keyset_destroy(hhe_keyset *ks)
{
    if (!ks) return;
    hhe_ctx *c = ks->ctx;
    HHE_LOCK(c);
    sync_ctx(c);
    keyset_clear(ks);
    c->sets.erase(std::remove(c->sets.begin(), c->sets.end(), ks), c->sets.end());
    delete ks;
}
extern "C" int hhe_keyset_set_relin(hhe_keyset *ks, const uint64_t *ksk)
{
    if (!ks || !ksk) { hhe_set_error("hhe_keyset_set_relin: null argument"); return HHE_ERR_INVALID; }
    HHE_LOCK(ks->ctx);
    return keyset_put_relin(ks, ksk);
}
extern "C" int hhe_keyset_set_galois(hhe_keyset *ks, uint32_t elt, const uint64_t *ksk)
{
    if (!ks || !ksk) { hhe_set_error("hhe_keyset_set_galois: null argument"); return HHE_ERR_INVALID; }
    HHE_LOCK(ks->ctx);
    return keyset_put_galois(ks, elt, ksk);
}
extern "C" int hhe_keyset_has_galois(const hhe_keyset *ks, uint32_t elt)
{
    if (!ks) return 0;
    HHE_LOCK(ks->ctx);
    return ks->gk.count(elt) ? 1 : 0;
}
extern "C" int hhe_keyset_has_relin(const hhe_keyset *ks)
{
    if (!ks) return 0;
    HHE_LOCK(ks->ctx);
    return ks->rk ? 1 : 0;
}
// the context's default set (the keys PASTA_SEAL was constructed with) and its further relin slots
extern "C" int hhe_set_relin_key_slot(hhe_ctx *c, int slot, const uint64_t *ksk)
{
    HHE_LOCK(c);
    if (!c || !ksk || slot < 0 || slot >= HHE_RELIN_SLOTS) return HHE_ERR_INVALID;
    return keyset_put_relin(c->relin_set(slot), ksk);
}
extern "C" int hhe_set_relin_key(hhe_ctx *c, const uint64_t *ksk) { HHE_LOCK(c); return hhe_set_relin_key_slot(c, 0, ksk); }
extern "C" int hhe_set_galois_key(hhe_ctx *c, uint32_t elt, const uint64_t *ksk)
{
    HHE_LOCK(c);
    if (!c || !ksk) { hhe_set_error("hhe_set_galois_key: null argument"); return HHE_ERR_INVALID; }
    return keyset_put_galois(&c->keys0, elt, ksk);
}
extern "C" int hhe_has_galois_key(const hhe_ctx *c, uint32_t elt) { HHE_LOCK(c); return c && c->keys0.gk.count(elt) ? 1 : 0; }

extern "C" void *hhe_malloc(size_t bytes) { return rt_malloc(bytes); }
extern "C" void hhe_free(void *p) { rt_free(p); }
extern "C" int hhe_copy_h2d(hhe_ctx *c, void *d, const void *h, size_t bytes)
{
    HHE_LOCK(c);
    if (rt_h2d(d, h, bytes, c ? c->lanes[0].stream : nullptr) || rt_sync(c ? c->lanes[0].stream : nullptr)) { hhe_set_error(rt_last_error()); return HHE_ERR_DEVICE; }
    return HHE_OK;
}
extern "C" int hhe_copy_d2h(hhe_ctx *c, void *h, const void *d, size_t bytes)
{
    HHE_LOCK(c);
    if (rt_d2h(h, d, bytes, c ? c->lanes[0].stream : nullptr) || rt_sync(c ? c->lanes[0].stream : nullptr)) { hhe_set_error(rt_last_error()); return HHE_ERR_DEVICE; }
    return HHE_OK;
}
