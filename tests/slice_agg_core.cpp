// The bit-sliced aggregate's host side (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) on the CPU:
// slice_agg_combine against __int128 brute force and the path rule aggregate_from_slices.
// tests/test_slice_agg_core.py builds this with AddressSanitizer and UBSan (a signed overflow in the
// combine step is a failure) and runs it. Exit status 1 at the first failed check, which is printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cubit_program.hpp"

using cubit::aggregate_from_slices;
using cubit::slice_agg_combine;
using cubit::slice_weighted_sum;
using cubit::U128;

static uint64_t checks = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

[[noreturn]] static void die(const char* what, int type, int64_t base, uint32_t bits, uint64_t count) {
    std::printf("FAILED %s: type %d base %" PRId64 " bits %u count %" PRIu64 "\n", what, type, base, bits, count);
    std::exit(1);
}

typedef unsigned __int128 u128;

// One case: `count` valid qualifying rows whose offsets are given as groups (offset, multiplicity).
// The brute force sums the values themselves in 128 bits (signed values sign-extended, UINT64 values
// zero-extended) and takes the extreme keys; the per-slice counts are what the kernel's popcounts give.
struct Group {
    uint64_t off, mult;
};
static void check_case(int type, int64_t base, uint32_t bits, const std::vector<Group>& groups) {
    uint64_t counts[64] = {0};
    uint64_t count = 0, mn = ~0ull, mx = 0;
    u128 want = 0;
    for (const Group& g : groups) {
        if (g.mult == 0) continue;
        if (bits < 64 && (g.off >> bits)) die("test offset out of range", type, base, bits, g.off);
        count += g.mult;
        for (uint32_t s = 0; s < bits; ++s)
            if ((g.off >> s) & 1ull) counts[s] += g.mult;
        mn = g.off < mn ? g.off : mn;
        mx = g.off > mx ? g.off : mx;
        const uint64_t key = (uint64_t)base + g.off;  // modular: the key's bits
        const u128 value = type == CUBIT_TYPE_UINT64 ? (u128)(key ^ 0x8000000000000000ull)
                                                     : (u128)(__int128)(int64_t)key;  // sign-extended
        want += value * (u128)g.mult;
    }
    for (uint32_t ops = 0; ops < 8; ++ops) {
        int64_t out[4] = {-1, -1, -1, -1}, out2[4] = {-1, -1, -1, -1};
        slice_agg_combine(type, base, count, counts, mn, mx, ops, out);
        slice_agg_combine(type, base, count, slice_weighted_sum(counts, bits), mn, mx, ops, out2);
        for (int k = 0; k < 4; ++k)
            if (out[k] != out2[k]) die("counts form != weighted form", type, base, bits, count);
        const u128 got = ((u128)(uint64_t)out[1] << 64) | (uint64_t)out[0];
        if (got != ((ops & 1u) ? want : (u128)0)) die("sum", type, base, bits, count);
        if (count) {
            const int64_t kmin = (int64_t)((uint64_t)base + mn), kmax = (int64_t)((uint64_t)base + mx);
            if (out[2] != ((ops & 2u) ? cubit_fp_value(type, kmin) : 0)) die("min", type, base, bits, count);
            if (out[3] != ((ops & 4u) ? cubit_fp_value(type, kmax) : 0)) die("max", type, base, bits, count);
        } else if (!(ops & 2u) && out[2] != 0) {
            die("min slot not asked for", type, base, bits, count);
        }
        ++checks;
    }
}

static uint64_t max_off(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

static void combine_checks() {
    const uint32_t all_bits[] = {0, 1, 12, 31, 32, 33, 63, 64};
    const uint64_t mults[] = {0, 1, 1ull << 33};
    const int types[] = {CUBIT_TYPE_INT64, CUBIT_TYPE_INT32, CUBIT_TYPE_UINT64, CUBIT_TYPE_VARCHAR};
    for (uint32_t bits : all_bits) {
        const uint64_t top = max_off(bits);
        // bases: 0, -17, near INT64_MIN, and the one that puts the top of the range at INT64_MAX
        std::vector<int64_t> bases;
        for (int64_t b : {(int64_t)0, (int64_t)-17, INT64_MIN, INT64_MIN + 1, INT64_MIN + 5}) {
            // the range [b, b + top] must stay inside int64 keys
            if ((u128)((uint64_t)b ^ 0x8000000000000000ull) + top <= (u128)~0ull) bases.push_back(b);
        }
        bases.push_back((int64_t)((uint64_t)INT64_MAX - top));
        for (int64_t base : bases)
            for (int type : types) {
                if (type == CUBIT_TYPE_INT32 || type == CUBIT_TYPE_VARCHAR) {
                    // 32-bit columns: the keys must be int32 values
                    if (bits > 32 || base < INT32_MIN || (__int128)base + (__int128)top > INT32_MAX) continue;
                }
                // edge offsets with multiplicities 0, 1 and 2^33
                for (uint64_t m0 : mults)
                    for (uint64_t m1 : mults)
                        for (uint64_t m2 : mults)
                            check_case(type, base, bits, {{0, m0}, {top, m1}, {top / 2, m2}});
                // random offsets and multiplicities
                for (int rep = 0; rep < 40; ++rep) {
                    std::vector<Group> groups;
                    const int n = (int)(rnd() % 6);
                    for (int i = 0; i < n; ++i) {
                        const uint64_t off = bits == 0 ? 0 : (bits >= 64 ? rnd() : rnd() & top);
                        const uint64_t mult = (rnd() & 1) ? rnd() % 1000 : rnd() % (1ull << 34);
                        groups.push_back({off, mult});
                    }
                    check_case(type, base, bits, groups);
                }
            }
    }
    // a UINT64 column whose every value is 2^64 - 1: key INT64_MAX, no slices, 2^33 rows
    check_case(CUBIT_TYPE_UINT64, INT64_MAX, 0, {{0, 1ull << 33}});
    check_case(CUBIT_TYPE_UINT64, INT64_MAX, 0, {{0, 1}});
    // … and the full unsigned range from its slices: base = key of 0, 64 bits
    check_case(CUBIT_TYPE_UINT64, INT64_MIN, 64, {{~0ull, 1ull << 33}, {0, 1}, {1ull << 63, 3}});
    // FLOAT / DOUBLE: no SUM, but min / max keys come back as bit patterns (negative keys included)
    for (int type : {CUBIT_TYPE_FLOAT, CUBIT_TYPE_DOUBLE}) {
        const int64_t nan_key = type == CUBIT_TYPE_FLOAT ? 0x7fc00000 : (int64_t)0x7ff8000000000000ull;
        const int64_t base = type == CUBIT_TYPE_FLOAT ? -(int64_t)0x7f800000 : -(int64_t)0x7ff0000000000000ll;  // -inf
        int64_t out[4];
        const uint64_t span = (uint64_t)nan_key - (uint64_t)base;
        slice_agg_combine(type, base, 2, U128{0, 0}, 0, span, 6u, out);
        if (out[0] != 0 || out[1] != 0 || out[2] != cubit_fp_value(type, base) || out[3] != cubit_fp_value(type, nan_key))
            die("floating-point min / max", type, base, 0, 2);
        if (cubit_fp_key(type, out[3]) != nan_key || cubit_fp_key(type, out[2]) != base)
            die("floating-point round trip", type, base, 0, 2);
        ++checks;
    }
}

// The rule as it stood before the three path rules shared one byte count, restated literally:
// aggregate_from_slices gives this answer at every point, ties included.
static bool aggregate_restated(bool force_slices, bool force_column, bool usable, uint32_t bits, uint32_t k_leaves,
                               bool nullable, uint64_t live_rows, uint64_t rows, uint64_t est_rows, uint64_t elem_bytes) {
    if (force_column || !usable) return false;
    if (force_slices) return true;
    const double slices = (double)(bits + k_leaves + (nullable ? 1u : 0u)) / 8.0 * (double)live_rows;
    const double gathered = std::min(128.0 * (double)est_rows, (double)elem_bytes * (double)rows);
    const double column = (double)k_leaves / 8.0 * (double)live_rows + 32.0 * (double)est_rows + gathered;
    return slices <= column;
}
// the least estimate in [0, rows] at which a monotone rule takes the slices (rows + 1: at none)
template <typename F>
static uint64_t crossover(uint64_t rows, const F& rule) {
    if (rule(0)) return 0;
    if (!rule(rows)) return rows + 1;
    uint64_t lo = 0, hi = rows;  // rule(lo) is false, rule(hi) true
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rule(mid)) hi = mid;
        else lo = mid;
    }
    return hi;
}

static void path_rule_checks() {
    const uint64_t rows = 612ull << 20;
    for (uint32_t bits : {0u, 1u, 12u, 24u, 33u, 64u})
        for (uint32_t k : {1u, 3u, 8u})
            for (int nullable = 0; nullable < 2; ++nullable)
                for (uint64_t elem : {4ull, 8ull})
                    for (uint64_t live : {rows, rows / 7}) {
                        // monotone: once the slices are taken at an estimate, they are taken at every larger one
                        bool taken = false;
                        for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1) {
                            const bool s = aggregate_from_slices(false, false, true, bits, k, nullable, live, rows, est, elem);
                            if (taken && !s) die("path rule not monotone", (int)k, (int64_t)est, bits, live);
                            taken = s;
                            // forced either way, whatever the estimate; never the slices without an index
                            if (!aggregate_from_slices(true, false, true, bits, k, nullable, live, rows, est, elem))
                                die("FROM_SLICES not honoured", (int)k, (int64_t)est, bits, live);
                            if (aggregate_from_slices(false, true, true, bits, k, nullable, live, rows, est, elem))
                                die("FROM_COLUMN not honoured", (int)k, (int64_t)est, bits, live);
                            if (aggregate_from_slices(false, false, false, bits, k, nullable, live, rows, est, elem))
                                die("slices without a usable index", (int)k, (int64_t)est, bits, live);
                            checks += 4;
                            for (int f = 0; f < 8; ++f) {
                                if (aggregate_from_slices(f & 1, f & 2, f & 4, bits, k, nullable, live, rows, est, elem) !=
                                    aggregate_restated(f & 1, f & 2, f & 4, bits, k, nullable, live, rows, est, elem))
                                    die("differs from the restated rule", f, (int64_t)est, bits, live);
                                ++checks;
                            }
                        }
                        // just below, at and just above the estimate where the restated rule turns
                        const uint64_t x = crossover(rows, [&](uint64_t est) {
                            return aggregate_restated(false, false, true, bits, k, nullable, live, rows, est, elem);
                        });
                        for (uint64_t est : {x ? x - 1 : 0, x, x + 1}) {
                            if (aggregate_from_slices(false, false, true, bits, k, nullable, live, rows, est, elem) !=
                                aggregate_restated(false, false, true, bits, k, nullable, live, rows, est, elem))
                                die("differs from the restated rule at its crossover", (int)k, (int64_t)est, bits, live);
                            ++checks;
                        }
                    }
    // from the bytes: a 12-bit column keeps its slices for a filter that keeps every row and gathers for one that
    // keeps a millionth of them
    if (!aggregate_from_slices(false, false, true, 12, 1, false, rows, rows, rows, 4)) die("dense 12-bit", 0, 0, 12, rows);
    if (aggregate_from_slices(false, false, true, 12, 1, false, rows, rows, rows / 1000000, 4))
        die("sparse 12-bit", 0, 0, 12, rows);
    checks += 2;
}

int main() {
    combine_checks();
    path_rule_checks();
    std::printf("slice agg ok %" PRIu64 " checks\n", checks);
    return 0;
}
