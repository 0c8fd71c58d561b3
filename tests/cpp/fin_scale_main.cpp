// fin_scale_main.cpp -- the 32-bit plaintext scaling of the item kernel (csrc/hhe_fin_bodies.h: plain_fix32 / plain_scaled32, the
// instantiation fin_item_store<T, true> and the c1 slices of fin_item_c1) against the shared definition, stand-alone on the CPU
// (no GPU, nothing loaded into another process):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHHE_RANGE_CHECK \
//       -Iprivacy-preserving-ml-through-hhe_amd/csrc tests/cpp/fin_scale_main.cpp -o fin_scale
// (a) values: plain_fix32 == plain_fix and plain_scaled32 == plain_scaled == floor((m Q + (t+1)/2) / t) mod q_j, the last evaluated
//     from Q as a multi-word integer divided by t (no delta, no Q mod t), for every m < t at t = 65537 over 60-bit, 50-bit and
//     20-bit primes and, at t = 1073479681, for 0, 1, t - 1, the coefficients at the rounding boundary with their neighbours and
//     10^6 seeded random m.
// (b) phases: the 32-bit instantiation looped over 1024 threads (c1 slices in front of clear, encode and every round, then the
//     store phase) writes the words of the default instantiation and of add_plain_body, at N = 2^10, 2^12, 2^14, counts 0, 1, 128,
//     keystreams by table and by stride, t = 65537 and t = 1073479681, and writes every output word exactly once (counted per
//     phase everywhere, per thread at N = 2^10).
// (c) constants: fin_scale32_fill (the function hhe_ctx_create calls) gives floor(q_mod_t 2^32 / t) and floor(delta_j 2^64 / q_j),
//     checked by multiplying back; fin_scale32_ok refuses a prime at or below t and t >= 2^30.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hhe_fin_bodies.h"

void hhe_range_violation(const char *what)
{
    fprintf(stderr, "range violation: %s\n", what);
    abort();
}

typedef unsigned __int128 u128;
static u64 mulmod_h(u64 a, u64 b, u64 m) { return (u64)((u128)a * b % m); }
static u64 powmod_h(u64 a, u64 e, u64 m)
{
    u64 r = 1;
    for (a %= m; e; e >>= 1, a = mulmod_h(a, a, m))
        if (e & 1) r = mulmod_h(r, a, m);
    return r;
}
static u64 inv_h(u64 a, u64 m) { return powmod_h(a % m, m - 2, m); }  // m prime
static u32 bitrev_h(u32 v, int bits)
{
    u32 r = 0;
    for (int i = 0; i < bits; i++) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}
static void fill_mod(ModDev &md, u64 q)
{
    memset(&md, 0, sizeof(md));
    md.q = q; md.nq = 0 - q;
    const u128 two64 = (u128)1 << 64;
    md.r_hi = (u64)(two64 / q);
    md.r_lo = (u64)(((two64 % q) << 64) / q);
}
static u64 rng_state;
static u64 next_rand() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// Q = q_0 ... q_{L-1} as little-endian 64-bit words (L <= 3 primes of at most 61 bits: 4 words), and floor(Q / t), Q mod t
struct Big { u64 w[4]; };
static Big big_product(const std::vector<u64> &q)
{
    Big r = {{1, 0, 0, 0}};
    for (u64 p : q) {
        u64 carry = 0;
        for (int i = 0; i < 4; i++) { const u128 x = (u128)r.w[i] * p + carry; r.w[i] = (u64)x; carry = (u64)(x >> 64); }
        if (carry) { fprintf(stderr, "big_product overflow\n"); abort(); }
    }
    return r;
}
static Big big_div_small(const Big &a, u64 d, u64 &rem)
{
    Big r;
    rem = 0;
    for (int i = 3; i >= 0; i--) { const u128 x = ((u128)rem << 64) | a.w[i]; r.w[i] = (u64)(x / d); rem = (u64)(x % d); }
    return r;
}
static u64 big_mod(const Big &a, u64 q)  // q < 2^64
{
    u64 r = 0;
    for (int i = 3; i >= 0; i--) r = (u64)((((u128)r << 64) | a.w[i]) % q);
    return r;
}

// the add_plain constants of a context as hhe_ctx_create computes them; delta and q_mod_t are checked against the big integers
static int fill_fin(FinArgs &fa, u64 t, const std::vector<u64> &q)
{
    const int L = (int)q.size();
    memset(&fa, 0, sizeof(fa));
    fa.L = L; fa.t = t; fa.thr = (t + 1) >> 1;
    fa.q_mod_t = 1;
    for (int j = 0; j < L; j++) fa.q_mod_t = mulmod_h(fa.q_mod_t, q[j] % t, t);
    fa.t_r_hi = (u64)(((u128)1 << 64) / t);
    fa.t_r_lo = (u64)((((u128)1 << 64) % t << 64) / t);
    for (int j = 0; j < L; j++) {
        const u64 v = mulmod_h(fa.q_mod_t % q[j], inv_h(t, q[j]), q[j]);
        fa.delta[j] = v ? q[j] - v : 0;
    }
    u64 rem;
    const Big fl = big_div_small(big_product(q), t, rem);
    if (rem != fa.q_mod_t) { fprintf(stderr, "Q mod t differs\n"); return 1; }
    for (int j = 0; j < L; j++)
        if (big_mod(fl, q[j]) != fa.delta[j]) { fprintf(stderr, "delta[%d] differs\n", j); return 1; }
    return 0;
}

// (c)
static int check_consts(const FinArgs &fa, const std::vector<u64> &q)
{
    const u128 a = (u128)fa.q_mod_t << 32, b = (u128)fa.q_mod_t_s * fa.t;
    if (!fa.scale32 || b > a || a - b >= fa.t) { fprintf(stderr, "q_mod_t_s is not floor(q_mod_t 2^32 / t)\n"); return 1; }
    for (size_t j = 0; j < q.size(); j++) {
        const u128 x = (u128)fa.delta[j] << 64, y = (u128)fa.delta_s[j] * q[j];  // delta < q < 2^61: both below 2^125
        if (y > x || x - y >= q[j]) { fprintf(stderr, "delta_s[%zu] is not floor(delta 2^64 / q)\n", j); return 1; }
    }
    for (int j = (int)q.size(); j < HHE_MAXL; j++)
        if (fa.delta_s[j]) { fprintf(stderr, "delta_s[%d] set past L\n", j); return 1; }
    return 0;
}

// (a) for one coefficient
static int check_value(const FinArgs &fa, const std::vector<ModDev> &mods, const Big &Q, u64 m)
{
    const PlainScale sc = {fa.t, fa.q_mod_t, fa.thr, fa.t_r_lo, fa.t_r_hi};
    const FinScale32 s32 = fin_scale32_consts(&fa);
    const u64 fix = plain_fix(sc, m);
    const u32 fix32 = plain_fix32(s32, (u32)m);
    if (fix != fix32 || fix != (u64)(((u128)m * fa.q_mod_t + fa.thr) / fa.t)) {
        fprintf(stderr, "t %llu m %llu: fix %llu, 32-bit %u\n", (unsigned long long)fa.t, (unsigned long long)m, (unsigned long long)fix, fix32);
        return 1;
    }
    // floor((m Q + thr) / t) as a multi-word integer: m < 2^30 and Q < 2^183 leave the top word room
    Big mq = Q;
    u64 carry = fa.thr;
    for (int i = 0; i < 4; i++) { const u128 x = (u128)Q.w[i] * m + carry; mq.w[i] = (u64)x; carry = (u64)(x >> 64); }
    if (carry) { fprintf(stderr, "m Q overflow\n"); abort(); }
    u64 rem;
    const Big fl = big_div_small(mq, fa.t, rem);
    for (int j = 0; j < fa.L; j++) {
        const u64 want = big_mod(fl, mods[j].q);
        const u64 shared = plain_scaled(m, fix, fa.delta[j], mods[j]);
        const u64 got = plain_scaled32((u32)m, fix32, fa.delta[j], fa.delta_s[j], mods[j].q);
        if (got != want || shared != want) {
            fprintf(stderr, "t %llu q %llu m %llu: definition %llx, plain_scaled %llx, 32-bit %llx\n", (unsigned long long)fa.t,
                    (unsigned long long)mods[j].q, (unsigned long long)m, (unsigned long long)want, (unsigned long long)shared, (unsigned long long)got);
            return 1;
        }
    }
    return 0;
}

static const u64 T_SMALL = 65537, T_LARGE = 1073479681;  // both prime and = 1 mod 2^16
static const std::vector<u64> Q60 = {1152921504595968001ULL, 1152921504597016577ULL, 1152921504598720513ULL};
static const std::vector<u64> Q50 = {1125899906738177ULL, 1125899906820097ULL, 0xfffffffd8001ULL};
static const std::vector<u64> Q20 = {786433, 1179649};  // primes just above t = 65537

static int values(u64 t, const std::vector<u64> &q, bool all)
{
    FinArgs fa;
    if (fill_fin(fa, t, q)) return 1;
    if (!fin_scale32_ok(15, t, q.data(), (int)q.size())) { fprintf(stderr, "t %llu: not eligible\n", (unsigned long long)t); return 1; }
    fin_scale32_fill(fa, q.data(), (int)q.size());
    if (check_consts(fa, q)) return 1;
    std::vector<ModDev> mods(q.size());
    for (size_t j = 0; j < q.size(); j++) fill_mod(mods[j], q[j]);
    const Big Q = big_product(q);
    size_t n = 0;
    if (all) {
        for (u64 m = 0; m < t; m++, n++)
            if (check_value(fa, mods, Q, m)) return 1;
    } else {
        // m (Q mod t) mod t = (t - 1) / 2 is the first remainder that rounds up ((t - 1) / 2 + thr = t), (t - 3) / 2 the last that does not
        const u64 qi = inv_h(fa.q_mod_t, t);
        const u64 up = mulmod_h((t - 1) / 2, qi, t), down = mulmod_h((t - 3) / 2, qi, t);
        if (mulmod_h(up, fa.q_mod_t, t) != (t - 1) / 2 || mulmod_h(down, fa.q_mod_t, t) != (t - 3) / 2) { fprintf(stderr, "boundary\n"); return 1; }
        std::vector<u64> ms = {0, 1, 2, t - 2, t - 1, (t - 1) / 2, (t + 1) / 2};
        for (u64 b : {up, down})
            for (u64 d : {t - 1, (u64)0, (u64)1}) ms.push_back((b + d) % t);
        rng_state = 0x2545f4914f6cdd1dULL ^ t ^ q[0];
        for (int i = 0; i < 1000000; i++) ms.push_back(next_rand() % t);
        for (u64 m : ms) {
            n++;
            if (check_value(fa, mods, Q, m)) return 1;
        }
    }
    printf("t = %llu, q_0 = %llu: %zu coefficients scale the same\n", (unsigned long long)t, (unsigned long long)q[0], n);
    return 0;
}

// (b)
template <int LOGN, int R> static void item_rounds(const NttArgs &a, u32 *lds)
{
    if constexpr (R < FinItemSched<LOGN>::R) {
        for (int t = 0; t < FIN_ITEM_THREADS; t++)
            fin_item_round<LOGN, FinItemSched<LOGN>::s0(R), FinItemSched<LOGN>::rho(R), FIN_ITEM_THREADS>(a, t, lds);
        item_rounds<LOGN, R + 1>(a, lds);
    }
}
static const u64 SENTINEL = ~(u64)0;  // no residue: the primes are below 2^61
// what a phase (per_thread: one thread of it) wrote into `scratch` moves to `out`, counted per word
struct Once {
    std::vector<u64> scratch;
    std::vector<unsigned char> cnt;
    u64 *out;
    bool per_thread;
    void merge()
    {
        for (size_t i = 0; i < scratch.size(); i++)
            if (scratch[i] != SENTINEL) { cnt[i]++; out[i] = scratch[i]; scratch[i] = SENTINEL; }
    }
};
// the launch of the 32-bit instantiation as the kernel orders it: slice s of the c1 half in front of phase s, then the c0 half
template <int LOGN> static void item32_launch(NttArgs a, Once &w)
{
    constexpr int NS = fin_item_c1_slices<LOGN>();
    std::vector<u32> lds((size_t)1 << LOGN, 0xdeadbeefu);
    a.aux_out = w.scratch.data();
    for (int item = 0; item < a.count; item++) {
        for (int s = 0; s < NS; s++) {
            for (int t = 0; t < FIN_ITEM_THREADS; t++) {
                fin_item_c1<FIN_ITEM_THREADS>(a, item, t, s, NS);
                if (w.per_thread) w.merge();
            }
            w.merge();
        }
        for (int t = 0; t < FIN_ITEM_THREADS; t++) fin_item_clear<FIN_ITEM_THREADS>(a, t, lds.data());
        for (int t = 0; t < FIN_ITEM_THREADS; t++) fin_item_encode<FIN_ITEM_THREADS>(a, item, t, lds.data());
        item_rounds<LOGN, 0>(a, lds.data());
        for (int t = 0; t < FIN_ITEM_THREADS; t++) {
            fin_item_store<FIN_ITEM_THREADS, true, false>(a, item, t, lds.data());
            if (w.per_thread) w.merge();
        }
        w.merge();
    }
}
template <int LOGN> static void item_launch(const NttArgs &a)
{
    std::vector<u32> lds((size_t)1 << LOGN, 0xdeadbeefu);
    for (int item = 0; item < a.count; item++) {
        for (int t = 0; t < FIN_ITEM_THREADS; t++) fin_item_clear<FIN_ITEM_THREADS>(a, t, lds.data());
        for (int t = 0; t < FIN_ITEM_THREADS; t++) fin_item_encode<FIN_ITEM_THREADS>(a, item, t, lds.data());
        item_rounds<LOGN, 0>(a, lds.data());
        for (int t = 0; t < FIN_ITEM_THREADS; t++) fin_item_store<FIN_ITEM_THREADS>(a, item, t, lds.data());
    }
}

static int phases(int logn, u64 t, const std::vector<u64> &q)
{
    const int L = (int)q.size(), B = logn == 10 ? 2 : 3;
    const size_t n = (size_t)1 << logn, ctw = 2 * L * n;
    FinArgs fa;
    if (fill_fin(fa, t, q)) return 1;
    if (!fin_scale32_ok(logn, t, q.data(), L)) { fprintf(stderr, "N = 2^%d, t = %llu: not eligible\n", logn, (unsigned long long)t); return 1; }
    fin_scale32_fill(fa, q.data(), L);
    std::vector<ModDev> mods(L + 1);
    for (int j = 0; j < L; j++) fill_mod(mods[j], q[j]);
    ModDev &mt = mods[L];
    fill_mod(mt, t);
    std::vector<u64> iw(2 * n);
    std::vector<u32> itw(2 * n);
    {
        u64 psi = 0;  // a primitive 2N-th root of unity: psi^N = -1
        for (u64 g = 2; !psi; g++) {
            const u64 c = powmod_h(g, (t - 1) / (2 * n), t);
            if (powmod_h(c, n, t) == t - 1) psi = c;
        }
        const u64 ipsi = inv_h(psi, t);
        u64 ipw = 1;
        for (size_t k = 0; k < n; k++) {
            const size_t r = bitrev_h((u32)k, logn);
            iw[2 * r] = ipw; iw[2 * r + 1] = (u64)(((u128)ipw << 64) / t);
            itw[2 * r] = (u32)ipw; itw[2 * r + 1] = (u32)((ipw << 32) / t);
            ipw = mulmod_h(ipw, ipsi, t);
        }
        mt.iw = iw.data();
        mt.ninv = inv_h(n, t);
        mt.ninv_s = (u64)(((u128)mt.ninv << 64) / t);
    }
    std::vector<u32> slot_map(n), slot_inv(n);
    {
        const u64 m = 2 * n;
        u64 pos = 1;
        for (size_t i = 0; i < n / 2; i++) {
            slot_map[i] = bitrev_h((u32)((pos - 1) >> 1), logn);
            slot_map[n / 2 + i] = bitrev_h((u32)((m - pos - 1) >> 1), logn);
            pos = pos * 3 % m;
        }
        for (size_t i = 0; i < n; i++) slot_inv[slot_map[i]] = (u32)i;
    }
    fa.slot_inv = slot_inv.data(); fa.slot_map = slot_map.data(); fa.itw = itw.data();
    rng_state = 0x9e3779b97f4a7c15ULL + (u64)logn + t;
    std::vector<u64> words((size_t)B * PASTA_T), ks((size_t)B * ctw);
    for (u64 &w : words) w = next_rand() % t;
    words[0] = t - 1; words[1] = t + 5; words[PASTA_T + 127] = ~(u64)0;
    for (int b = 0; b < B; b++)
        for (int p = 0; p < 2 * L; p++)
            for (size_t i = 0; i < n; i++) ks[(size_t)b * ctw + p * n + i] = next_rand() % q[p % L];
    ks[0] = 0; ks[(size_t)L * n] = 0; ks[(size_t)L * n + 1] = q[0] - 1;  // -0 = 0 in both halves
    std::vector<const u64 *> ptrs(B);
    std::vector<u32> ct_map(B);
    for (int b = 0; b < B; b++) { ct_map[b] = (u32)((b + 1) % B); ptrs[b] = ks.data() + (size_t)ct_map[b] * ctw; }

    std::vector<u64> tmp((size_t)B * n), out_ref((size_t)B * ctw), out_old((size_t)B * ctw), out_new((size_t)B * ctw);
    for (int count : {0, 1, 128})
        for (int by_table = 0; by_table < 2; by_table++) {
            fa.count = count;
            NttArgs a;
            memset(&a, 0, sizeof(a));
            a.src = words.data(); a.mods = mods.data(); a.logn = logn; a.count = B;
            a.mod_base = L; a.mod_cycle = 1; a.src_div = 1; a.src_item_polys = 1; a.src_item_stride = PASTA_T;
            a.load_op = LOAD_ENCODE; a.store_op = STORE_ADD_PLAIN; a.L = L; a.K = L + 1;
            a.mul = ks.data(); a.mul_ptrs = by_table ? ptrs.data() : nullptr; a.fin = &fa;
            std::fill(out_ref.begin(), out_ref.end(), SENTINEL);
            std::fill(out_old.begin(), out_old.end(), SENTINEL);
            std::fill(out_new.begin(), out_new.end(), SENTINEL);
            {   // add_plain_body on the negated keystream, its plaintext from a transform evaluated directly
                std::fill(tmp.begin(), tmp.end(), 0);
                EncodeArgs e;
                memset(&e, 0, sizeof(e));
                e.vals = words.data(); e.out = tmp.data(); e.slot_map = slot_map.data(); e.logn = logn; e.B = B;
                e.stride = PASTA_T; e.count = count; e.second_off = -1; e.t = t;
                for (size_t gid = 0; gid < (size_t)B * count; gid++) encode_scatter_body(e, gid);
                for (int b = 0; b < B; b++) {
                    u64 *x = tmp.data() + (size_t)b * n;
                    for (size_t m = n >> 1, gap = 1; m >= 1; m >>= 1, gap <<= 1)
                        for (size_t blk = 0; blk < m; blk++)
                            for (size_t i = blk * 2 * gap; i < blk * 2 * gap + gap; i++) {
                                const u64 u = x[i], v = x[i + gap];
                                x[i] = (u + v) % t;
                                x[i + gap] = mulmod_h((u + t - v) % t, iw[2 * (m + blk)], t);
                            }
                    for (size_t i = 0; i < n; i++) x[i] = mulmod_h(x[i], mt.ninv, t);
                }
                AddPlainArgs ap;
                memset(&ap, 0, sizeof(ap));
                ap.ct = ks.data(); ap.ct_map = by_table ? ct_map.data() : nullptr; ap.plain = tmp.data(); ap.out = out_ref.data();
                ap.mods = mods.data(); ap.logn = logn; ap.B = B; ap.L = L; ap.negate_ct = 1;
                ap.t = fa.t; ap.q_mod_t = fa.q_mod_t; ap.thr = fa.thr; ap.t_r_lo = fa.t_r_lo; ap.t_r_hi = fa.t_r_hi;
                for (int j = 0; j < L; j++) ap.delta[j] = fa.delta[j];
                for (size_t gid = 0; gid < (size_t)B * n; gid++) add_plain_body(ap, gid);
            }
            a.aux_out = out_old.data();
            Once w;
            w.scratch.assign((size_t)B * ctw, SENTINEL);
            w.cnt.assign((size_t)B * ctw, 0);
            w.out = out_new.data();
            w.per_thread = logn == 10 && count == 128 && !by_table;
            switch (logn) {
            case 10: item_launch<10>(a); item32_launch<10>(a, w); break;
            case 12: item_launch<12>(a); item32_launch<12>(a, w); break;
            case 14: item_launch<14>(a); item32_launch<14>(a, w); break;
            default: return 1;
            }
            for (size_t i = 0; i < w.cnt.size(); i++)
                if (w.cnt[i] != 1) {
                    fprintf(stderr, "N = 2^%d t %llu count %d table %d: word %zu written %d times\n", logn, (unsigned long long)t, count, by_table, i, (int)w.cnt[i]);
                    return 1;
                }
            for (size_t i = 0; i < out_ref.size(); i++)
                if (out_ref[i] != out_new[i] || out_old[i] != out_new[i]) {
                    fprintf(stderr, "N = 2^%d t %llu count %d table %d: word %zu: add_plain_body %llx, default %llx, 32-bit %llx\n", logn,
                            (unsigned long long)t, count, by_table, i, (unsigned long long)out_ref[i], (unsigned long long)out_old[i], (unsigned long long)out_new[i]);
                    return 1;
                }
            if (count == 128 && !by_table) {  // not vacuous: c0 carries a plaintext
                bool any = false;
                for (size_t i = 0; i < n && !any; i++) any = out_ref[i] != (ks[i] ? q[0] - ks[i] : 0);
                if (!any) { fprintf(stderr, "N = 2^%d: the reference added no plaintext\n", logn); return 1; }
            }
        }
    printf("N = 2^%d, t = %llu: same words, each written once\n", logn, (unsigned long long)t);
    return 0;
}

int main()
{
    // (c) what the eligibility refuses
    {
        const u64 below[3] = {268369921, Q50[0], Q50[1]}, equal[1] = {T_SMALL};
        if (fin_scale32_ok(10, T_LARGE, below, 3) || fin_scale32_ok(10, T_SMALL, equal, 1) || fin_scale32_ok(16, T_SMALL, Q60.data(), 3) ||
            fin_scale32_ok(15, (u64)1 << 30, Q60.data(), 3) || !fin_scale32_ok(15, T_SMALL, Q60.data(), 3)) {
            fprintf(stderr, "fin_scale32_ok\n");
            return 1;
        }
    }
    // (a) and (c)
    for (const std::vector<u64> *q : {&Q60, &Q50, &Q20})
        if (values(T_SMALL, *q, true)) return 1;
    for (const std::vector<u64> *q : {&Q60, &Q50})
        if (values(T_LARGE, *q, false)) return 1;
    // (b): primes = 1 mod 2^15 are not needed here (the transform is mod t only)
    for (int logn : {10, 12, 14})
        for (u64 t : {T_SMALL, T_LARGE})
            if (phases(logn, t, logn == 12 ? Q60 : Q50)) return 1;
    printf("fin_scale OK\n");
    return 0;
}
