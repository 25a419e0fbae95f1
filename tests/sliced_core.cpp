// sliced_interval (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) against brute force, on the
// CPU: tests/test_sliced_core.py builds this with AddressSanitizer and UBSan (a signed overflow in
// the mapping is a failure) and runs it. Exit status 1 at the first failed check, which is printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cubit_program.hpp"

using cubit::SlicedInterval;
using cubit::sliced_bits;
using cubit::sliced_interval;

static uint64_t checks = 0;

static bool direct(int cmp, int64_t v, int64_t c, int64_t c2) {
    switch (cmp) {
    case 0: return v == c;
    case 1: return v != c;
    case 2: return v < c;
    case 3: return v <= c;
    case 4: return v > c;
    case 5: return v >= c;
    default: return v >= c && v < c2;
    }
}

static bool answer(const SlicedInterval& s, uint64_t u) {
    if (s.kind == SlicedInterval::kFalse) return false;
    if (s.kind == SlicedInterval::kAllValid) return true;
    return (u >= s.lo && u <= s.hi) != s.negate;
}

[[noreturn]] static void die(const char* what, int cmp, int64_t c, int64_t c2, int64_t base, uint32_t bits, int64_t key) {
    std::printf("FAILED %s: cmp %d c %" PRId64 " c2 %" PRId64 " base %" PRId64 " bits %u key %" PRId64 "\n", what, cmp, c,
                c2, base, bits, key);
    std::exit(1);
}

// every key of `keys` (all >= base, offsets below 2^bits); whole = keys holds every offset of the range
static void check(int cmp, int64_t c, int64_t c2, int64_t base, uint32_t bits, const std::vector<int64_t>& keys,
                  bool whole) {
    const SlicedInterval s = sliced_interval(cmp, c, c2, base, bits);
    const uint64_t max = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    if (s.kind == SlicedInterval::kInterval && (s.lo > s.hi || s.hi > max || (s.lo == 0 && s.hi == max)))
        die("interval not clamped", cmp, c, c2, base, bits, 0);
    size_t pass = 0;
    for (int64_t k : keys) {
        const uint64_t u = (uint64_t)k - (uint64_t)base;
        const bool want = direct(cmp, k, c, c2);
        if (answer(s, u) != want) die("membership", cmp, c, c2, base, bits, k);
        pass += want;
        ++checks;
    }
    if (whole) {  // a miss is kFalse, a cover kAllValid, anything else an interval
        const SlicedInterval::Kind want = pass == 0             ? SlicedInterval::kFalse
                                          : pass == keys.size() ? SlicedInterval::kAllValid
                                                                : SlicedInterval::kInterval;
        if (s.kind != want) die("kind", cmp, c, c2, base, bits, 0);
    }
}

static void all_forms(const std::vector<int64_t>& consts, int64_t base, uint32_t bits, const std::vector<int64_t>& keys,
                      bool whole) {
    for (int64_t c : consts) {
        for (int cmp = 0; cmp < 6; ++cmp) check(cmp, c, 0, base, bits, keys, whole);
        for (int64_t c2 : consts) check(6, c, c2, base, bits, keys, whole);
    }
}

// v + d when it is an int64
static bool add(int64_t v, __int128 d, int64_t& out) {
    const __int128 r = (__int128)v + d;
    if (r < INT64_MIN || r > INT64_MAX) return false;
    out = (int64_t)r;
    return true;
}

int main() {
    // bits 0 … 6: every key of the range, every constant in [base - 3, base + 2^bits + 2]
    for (uint32_t bits = 0; bits <= 6; ++bits) {
        const int64_t span = (int64_t)((1ull << bits) - 1);
        const int64_t bases[] = {0,         -17,           1000, INT64_MIN, INT64_MIN + 1, INT64_MIN + 3, INT64_MAX - span,
                                 INT64_MAX - span - 1, INT64_MAX - span - 3};
        for (int64_t base : bases) {
            std::vector<int64_t> keys, consts;
            for (int64_t u = 0; u <= span; ++u) keys.push_back(base + u);
            for (int d = -3; d <= span + 3; ++d) {
                int64_t c;
                if (add(base, d, c)) consts.push_back(c);
            }
            consts.push_back(INT64_MIN);
            consts.push_back(INT64_MAX);
            all_forms(consts, base, bits, keys, true);
            if (sliced_bits(base, base + span) != bits) die("sliced_bits", 0, 0, 0, base, bits, 0);
        }
    }
    // wide spans: the keys and constants at both ends of the range and of int64
    for (uint32_t bits : {12u, 31u, 32u, 33u, 62u, 63u, 64u}) {
        const __int128 span = bits >= 64 ? ((__int128)1 << 64) - 1 : ((__int128)1 << bits) - 1;
        std::vector<int64_t> bases = {INT64_MIN};
        int64_t b;
        if (add(INT64_MAX, -span, b)) bases.push_back(b);  // top = INT64_MAX
        if (add(0, -span / 2, b)) bases.push_back(b);
        if (bits < 63) bases.push_back(12345);
        for (int64_t base : bases) {
            std::vector<int64_t> keys, consts;
            for (__int128 d : {(__int128)0, (__int128)1, (__int128)2, span / 2, span / 2 + 1, span - 2, span - 1, span}) {
                int64_t k;
                if (d >= 0 && add(base, d, k)) keys.push_back(k);
            }
            for (__int128 d : {(__int128)-2, (__int128)-1, (__int128)0, (__int128)1, span / 2, span - 1, span, span + 1,
                               span + 2}) {
                int64_t c;
                if (add(base, d, c)) consts.push_back(c);
            }
            for (int64_t c : {INT64_MIN, INT64_MIN + 1, (int64_t)-1, (int64_t)0, (int64_t)1, INT64_MAX - 1, INT64_MAX})
                consts.push_back(c);
            all_forms(consts, base, bits, keys, false);
        }
    }
    if (sliced_bits(INT64_MIN, INT64_MAX) != 64 || sliced_bits(5, 5) != 0 || sliced_bits(-1, 0) != 1)
        die("sliced_bits ends", 0, 0, 0, 0, 0, 0);
    std::printf("sliced ok %" PRIu64 " checks\n", checks);
    return 0;
}
