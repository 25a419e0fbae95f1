// The grouped aggregate's host side (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) on the CPU: the
// slot enumeration, the group numbering, the split into the kernel's rectangular batches, the path
// rule grouped_from_slices, and the per-group combine against __int128 brute force.
// tests/test_group_agg_core.py builds this with AddressSanitizer and UBSan and runs it. Exit status 1
// at the first failed check, which is printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "cubit_program.hpp"

using namespace cubit;

static uint64_t checks = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

[[noreturn]] static void die(const char* what, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
    std::printf("FAILED %s: %" PRId64 " %" PRId64 " %" PRId64 "\n", what, a, b, c);
    std::exit(1);
}
#define CHECK(cond, ...)               \
    do {                               \
        if (!(cond)) die(__VA_ARGS__); \
        ++checks;                      \
    } while (0)

typedef unsigned __int128 u128;

// ---- slots: keys ∪ update values ∪ NULL against a std::set
static void slot_case(const std::vector<int64_t>& keys, const std::vector<int64_t>& upd, bool null_slot) {
    const GroupSlots s = group_slots(keys, upd, null_slot);
    std::set<int64_t> all(keys.begin(), keys.end());
    all.insert(upd.begin(), upd.end());
    CHECK(s.keys.size() == all.size(), "slot count", (int64_t)s.keys.size(), (int64_t)all.size());
    CHECK(s.leaf.size() == s.keys.size(), "leaf list length");
    CHECK(s.size() == all.size() + (null_slot ? 1 : 0), "size with the NULL slot", s.size());
    CHECK(s.has_null == null_slot, "NULL slot flag");
    size_t i = 0;
    for (int64_t k : all) {  // ascending, and each key's leaf is its position in the index (or none)
        CHECK(s.keys[i] == k, "slot order", (int64_t)i, s.keys[i], k);
        const auto it = std::lower_bound(keys.begin(), keys.end(), k);
        const bool is_key = it != keys.end() && *it == k;
        CHECK(s.leaf[i] == (is_key ? (int32_t)(it - keys.begin()) : -1), "slot leaf", (int64_t)i, s.leaf[i]);
        ++i;
    }
}

static void slot_checks() {
    slot_case({}, {}, false);
    slot_case({}, {}, true);
    slot_case({1, 2, 3}, {}, false);
    slot_case({1, 2, 3}, {}, true);
    slot_case({1, 2, 3}, {2}, false);                  // a duplicate between keys and update values
    slot_case({1, 2, 3}, {0, 2, 4}, true);             // update values before, among and after the keys
    slot_case({}, {5, 9}, false);                      // an empty index whose records carry values
    slot_case({INT64_MIN, -1, INT64_MAX}, {INT64_MIN, 0, INT64_MAX}, true);
    for (int rep = 0; rep < 300; ++rep) {
        std::set<int64_t> k, u;
        const int nk = (int)(rnd() % 12), nu = (int)(rnd() % 6);
        for (int i = 0; i < nk; ++i) k.insert((int64_t)(rnd() % 20) - 10);
        for (int i = 0; i < nu; ++i) u.insert((int64_t)(rnd() % 20) - 10);
        slot_case({k.begin(), k.end()}, {u.begin(), u.end()}, (rnd() & 1) != 0);
    }
    // numbering: g = i1·n2 + i2, and back; one column is n2 = 1
    for (uint32_t n1 : {1u, 3u, 16u, 256u})
        for (uint32_t n2 : {1u, 2u, 7u, 16u}) {
            if (group_count(n1, n2) < 0) continue;
            std::vector<int> seen(n1 * n2, 0);
            for (uint32_t i1 = 0; i1 < n1; ++i1)
                for (uint32_t i2 = 0; i2 < n2; ++i2) {
                    const uint32_t g = group_index(i1, i2, n2);
                    uint32_t b1, b2;
                    group_tuple(g, n2, &b1, &b2);
                    CHECK(g < n1 * n2 && b1 == i1 && b2 == i2 && !seen[g]++, "group numbering", g, i1, i2);
                }
        }
    // the 256-group limit on both sides, one and two columns
    CHECK(group_count(256, 1) == 256, "256 groups of one column");
    CHECK(group_count(257, 1) < 0, "257 groups of one column");
    CHECK(group_count(16, 16) == 256, "16 x 16 groups");
    CHECK(group_count(16, 17) < 0, "16 x 17 groups");
    CHECK(group_count(0, 5) == 0, "no slot, no group");
    CHECK(group_count(0xffffffffu, 0xffffffffu) < 0, "the product does not wrap");
    CHECK(CUBIT_AGG_MAX_GROUPS == 256 && CUBIT_AGG_MAX_GROUP_COLS == 2, "limits");
}

// ---- batches: every pair of leaves in exactly one batch, no batch past the kernel's rectangle
static void batch_checks() {
    for (uint32_t limit : {kGroupBatchMinMax, kGroupBatchSum})
        for (int two = 0; two < 2; ++two)
            for (uint32_t n1 = 0; n1 <= 40; ++n1)
                for (uint32_t n2 = 0; n2 <= (two ? 20u : 0u); ++n2)
                    for (uint32_t row_bits : {1u, 13u, 26u, 73u}) {
                        bool swapped = false;
                        const auto bs = split_group_batches(n1, n2, two != 0, limit, row_bits, &swapped);
                        const uint32_t na = swapped ? n2 : n1, nb = swapped ? n1 : n2;
                        CHECK(two || !swapped, "one column never swaps");
                        std::vector<int> seen((size_t)na * (two ? nb : 1), 0);
                        for (const GroupBatch& b : bs) {
                            CHECK(b.na >= 1 && b.na <= (two ? limit / 2 : limit), "batch height", b.na, limit);
                            CHECK(two ? (b.nb >= 1 && b.nb <= 2) : b.nb == 0, "batch width", b.nb);
                            CHECK(b.na * (two ? b.nb : 1) <= limit, "batch size", b.na, b.nb);
                            CHECK(b.a0 + b.na <= na && (!two || b.b0 + b.nb <= nb), "batch range", b.a0, b.b0);
                            for (uint32_t x = 0; x < b.na; ++x)
                                for (uint32_t y = 0; y < (two ? b.nb : 1); ++y)
                                    seen[(size_t)(b.a0 + x) * (two ? nb : 1) + (b.b0 + y)]++;
                        }
                        for (int c : seen) CHECK(c == 1, "a pair of leaves covered once", n1, n2, c);
                        if (two) {  // the orientation taken reads no more than the other
                            const uint64_t other = group_batches_bits(group_batches_of(swapped ? n1 : n2, swapped ? n2 : n1, true, limit), row_bits);
                            CHECK(group_batches_bits(bs, row_bits) <= other, "the cheaper orientation", n1, n2);
                        }
                    }
    // TPC-H Q1's shape, SUM: 3 x 2 leaves are one launch reading b + K + 5 bits per row
    bool swapped = false;
    const auto q1 = split_group_batches(3, 2, true, kGroupBatchSum, 25, &swapped);
    CHECK(q1.size() == 1 && group_batches_bits(q1, 25) == 30, "Q1 is one launch", (int64_t)q1.size());
}

// ---- the path rule
// The rule as it stood before the three path rules shared one byte count, restated literally:
// grouped_from_slices gives this answer at every point, ties included.
static bool grouped_restated(bool force_slices, bool force_column, bool usable, uint64_t slice_bits, uint32_t k_leaves,
                             uint64_t live_rows, uint64_t rows, uint64_t est_rows, const uint64_t* elem_bytes,
                             uint32_t n_probed) {
    if (force_column || !usable) return false;
    if (force_slices) return true;
    const double slices = (double)slice_bits / 8.0 * (double)live_rows;
    double column = (double)k_leaves / 8.0 * (double)live_rows + 16.0 * (double)est_rows;
    for (uint32_t i = 0; i < n_probed; ++i)
        column += 16.0 * (double)est_rows + std::min(128.0 * (double)est_rows, (double)elem_bytes[i] * (double)rows);
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
    const uint64_t eb[3] = {8, 4, 4};
    for (uint32_t bits : {0u, 1u, 12u, 24u, 64u})
        for (uint32_t k : {0u, 1u, 8u})
            for (uint32_t nullable = 0; nullable < 2; ++nullable)
                for (uint64_t live : {rows, rows / 7})
                    for (uint32_t ncols : {1u, 2u}) {
                        const uint32_t row_bits = bits + k + nullable;
                        bool prev_groups = true;  // monotone in the group count: more groups never turn to the slices
                        for (uint32_t groups : {1u, 2u, 6u, 8u, 9u, 25u, 64u, 256u}) {
                            bool sw;
                            const auto bs = split_group_batches(ncols == 1 ? groups : (groups + 1) / 2, ncols == 1 ? 0 : 2,
                                                                ncols == 2, kGroupBatchSum, row_bits, &sw);
                            const uint64_t sb = group_batches_bits(bs, row_bits);
                            bool taken = false;
                            for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1) {
                                const bool s = grouped_from_slices(false, false, true, sb, k, live, rows, est, eb, 1 + ncols);
                                CHECK(!taken || s, "not monotone in the estimated rows", (int64_t)est, bits, groups);
                                taken = s;
                                CHECK(grouped_from_slices(true, false, true, sb, k, live, rows, est, eb, 1 + ncols), "FROM_SLICES");
                                CHECK(!grouped_from_slices(false, true, true, sb, k, live, rows, est, eb, 1 + ncols), "FROM_COLUMN");
                                CHECK(!grouped_from_slices(false, false, false, sb, k, live, rows, est, eb, 1 + ncols),
                                      "slices without a usable index");
                                CHECK(!grouped_from_slices(true, false, false, sb, k, live, rows, est, eb, 1 + ncols),
                                      "forced slices without a usable index");
                                for (int f = 0; f < 8; ++f)
                                    CHECK(grouped_from_slices(f & 1, f & 2, f & 4, sb, k, live, rows, est, eb, 1 + ncols) ==
                                              grouped_restated(f & 1, f & 2, f & 4, sb, k, live, rows, est, eb, 1 + ncols),
                                          "differs from the restated rule", (int64_t)est, bits, groups);
                            }
                            // just below, at and just above the estimate where the restated rule turns
                            const uint64_t x = crossover(rows, [&](uint64_t e) {
                                return grouped_restated(false, false, true, sb, k, live, rows, e, eb, 1 + ncols);
                            });
                            for (uint64_t e : {x ? x - 1 : 0, x, x + 1})
                                CHECK(grouped_from_slices(false, false, true, sb, k, live, rows, e, eb, 1 + ncols) ==
                                          grouped_restated(false, false, true, sb, k, live, rows, e, eb, 1 + ncols),
                                      "differs from the restated rule at its crossover", (int64_t)e, bits, groups);
                            const uint64_t est = rows / 50;
                            const bool s = grouped_from_slices(false, false, true, sb, k, live, rows, est, eb, 1 + ncols);
                            CHECK(prev_groups || !s, "not monotone in the group count", groups, bits, k);
                            prev_groups = s;
                        }
                        // no group leaves, one launch, no group column: aggregate_from_slices itself
                        for (uint64_t elem : {4ull, 8ull})
                            for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1) {
                                const uint64_t e1[1] = {elem};
                                CHECK(grouped_from_slices(false, false, true, row_bits, k, live, rows, est, e1, 1) ==
                                          aggregate_from_slices(false, false, true, bits, k, nullable != 0, live, rows, est, elem),
                                      "differs from aggregate_from_slices", (int64_t)est, bits, k);
                            }
                    }
}

// ---- per-group combine: random rows in random groups, each group's slice counts as the kernel's
// popcounts give them, against the 128-bit sum of the group's values and its extreme keys
static uint64_t max_off(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

static void combine_case(int type, int64_t base, uint32_t bits, uint32_t n_groups) {
    struct Acc {
        uint64_t counts[64] = {0};
        uint64_t cv = 0, mn = ~0ull, mx = 0;
        u128 want = 0;
    };
    std::vector<Acc> acc(n_groups);
    const int n_rows = (int)(rnd() % 64);
    for (int i = 0; i < n_rows; ++i) {
        Acc& a = acc[rnd() % n_groups];
        const uint64_t off = bits == 0 ? 0 : (bits >= 64 ? rnd() : rnd() & max_off(bits));
        const uint64_t mult = (rnd() & 1) ? 1 + rnd() % 1000 : 1 + rnd() % (1ull << 34);
        a.cv += mult;
        for (uint32_t s = 0; s < bits; ++s)
            if ((off >> s) & 1ull) a.counts[s] += mult;
        a.mn = off < a.mn ? off : a.mn;
        a.mx = off > a.mx ? off : a.mx;
        const uint64_t key = (uint64_t)base + off;
        const u128 value = type == CUBIT_TYPE_UINT64 ? (u128)(key ^ 0x8000000000000000ull) : (u128)(__int128)(int64_t)key;
        a.want += value * (u128)mult;
    }
    for (uint32_t g = 0; g < n_groups; ++g) {
        const Acc& a = acc[g];
        int64_t out[4];
        slice_agg_combine(type, base, a.cv, slice_weighted_sum(a.counts, bits), a.mn, a.mx, 7u, out);
        const u128 got = ((u128)(uint64_t)out[1] << 64) | (uint64_t)out[0];
        CHECK(got == a.want, "group sum", type, base, bits);
        if (a.cv) {
            CHECK(out[2] == cubit_fp_value(type, (int64_t)((uint64_t)base + a.mn)), "group min", type, base, bits);
            CHECK(out[3] == cubit_fp_value(type, (int64_t)((uint64_t)base + a.mx)), "group max", type, base, bits);
        }
    }
}

static void combine_checks() {
    const uint32_t all_bits[] = {0, 1, 12, 31, 32, 33, 63, 64};
    const int types[] = {CUBIT_TYPE_INT64, CUBIT_TYPE_INT32, CUBIT_TYPE_UINT64, CUBIT_TYPE_VARCHAR};
    for (uint32_t bits : all_bits) {
        const uint64_t top = max_off(bits);
        std::vector<int64_t> bases;
        for (int64_t b : {(int64_t)0, (int64_t)-17, INT64_MIN, INT64_MIN + 1, INT64_MIN + 5})
            if ((u128)((uint64_t)b ^ 0x8000000000000000ull) + top <= (u128)~0ull) bases.push_back(b);
        bases.push_back((int64_t)((uint64_t)INT64_MAX - top));
        for (int64_t base : bases)
            for (int type : types) {
                if (type == CUBIT_TYPE_INT32 || type == CUBIT_TYPE_VARCHAR)
                    if (bits > 32 || base < INT32_MIN || (__int128)base + (__int128)top > INT32_MAX) continue;
                for (uint32_t n_groups : {1u, 2u, 6u, 9u, 33u})
                    for (int rep = 0; rep < 8; ++rep) combine_case(type, base, bits, n_groups);
            }
    }
}

int main() {
    slot_checks();
    batch_checks();
    path_rule_checks();
    combine_checks();
    std::printf("group agg ok %" PRIu64 " checks\n", checks);
    return 0;
}
