// Drives the babystep-giantstep inner-sum kernel body (PermArgs::bsgs_n1 > 0) through k_perm at its bounds: every word of the
// baby-step operands and of the multiplier table at q_j - 1.  Links the tests-only emulator, which is built with -DHHE_RANGE_CHECK:
// a lazy sum that wraps aborts the run.  usage: bsgs_inner n1 n2 logn B out.bin q_0 .. q_{L-1}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hhe_launch.h"

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const int n1 = atoi(argv[1]), n2 = atoi(argv[2]), logn = atoi(argv[3]), B = atoi(argv[4]), L = argc - 6;
    const size_t n = (size_t)1 << logn, ln = (size_t)L * n, ctw = 2 * ln;
    std::vector<ModDev> mods(L);
    std::vector<u64> rot((size_t)n1 * B * ctw), tab((size_t)n1 * n2 * ln), out((size_t)n2 * B * ctw, ~(u64)0);
    for (int j = 0; j < L; j++) {
        memset(&mods[j], 0, sizeof(ModDev));
        const u64 q = strtoull(argv[6 + j], nullptr, 10);
        const unsigned __int128 r = ~(unsigned __int128)0 / q;  // floor(2^128 / q): q is odd
        mods[j].q = q; mods[j].r_lo = (u64)r; mods[j].r_hi = (u64)(r >> 64); mods[j].nq = 0 - q;
        for (size_t p = 0; p < (size_t)n1 * B * 2; p++) std::fill_n(&rot[(p * L + j) * n], n, q - 1);
        for (size_t d = 0; d < (size_t)n1 * n2; d++) std::fill_n(&tab[(d * L + j) * n], n, q - 1);
    }
    std::vector<const u64 *> ptrs(B, tab.data());
    PermArgs p;
    memset(&p, 0, sizeof(p));
    p.bsgs_n1 = n1; p.bsgs_n2 = n2;
    p.in = rot.data(); p.in_step_stride = (size_t)B * ctw; p.in_item_stride = ctw;
    p.out = out.data(); p.out_step_stride = (size_t)B * ctw; p.out_item_stride = ctw;
    p.mul_ptrs = ptrs.data(); p.mul_step_stride = ln;
    p.mods = mods.data(); p.logn = logn; p.count = B * 2 * L; p.L = L;
    k_perm(p, nullptr);
    FILE *f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) return 3;
    fclose(f);
    printf("bsgs_inner_sum: %d x %d, %d limbs, %zu words\n", n1, n2, L, out.size());
    return 0;
}
