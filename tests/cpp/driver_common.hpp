// TESTS ONLY -- what the drivers of include/pasta_seal_gfx950.hpp (tests/cpp/*_main.cpp) share: reading the input blob a test wrote,
// writing the output blob it reads, telling a refusal (std::invalid_argument) from any other outcome, and the signed reading of a slot.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

inline std::vector<uint64_t> read_words(FILE *f, size_t n)
{
    std::vector<uint64_t> v(n);
    if (fread(v.data(), 8, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
inline void put(FILE *o, const std::vector<uint64_t> &v) { if (o) fwrite(v.data(), 8, v.size(), o); }   // no output file: nothing is written
template <class F> bool throws_invalid(F &&f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; } catch (...) { return false; }
    return false;
}
inline int64_t centred(uint64_t v, uint64_t t) { return v > (t + 1) / 2 ? (int64_t)v - (int64_t)t : (int64_t)v; }
