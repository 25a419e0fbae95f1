// The sliced sum(a · b)'s host side (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) on the CPU:
// slice_product_combine against __int128 brute force, and the path rules sum_product_from_slices and
// sum_product_grouped_from_slices against a direct byte count in whole eighths of a byte.
// tests/test_slice_product_core.py builds this with AddressSanitizer and UBSan (a signed overflow in
// the combine step is a failure) and runs it. Exit status 1 at the first failed check, which is printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cubit_program.hpp"

using cubit::kProductGroupBatch;
using cubit::kProductInner;
using cubit::U128;

typedef unsigned __int128 u128;

static uint64_t checks = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

[[noreturn]] static void die(const char* what, int64_t x, int64_t y, uint64_t u, uint64_t v) {
    std::printf("FAILED %s: %" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 "\n", what, x, y, u, v);
    std::exit(1);
}

static uint64_t max_off(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }
static U128 split(u128 x) { return U128{(uint64_t)x, (uint64_t)(x >> 64)}; }

// One case: groups of rows (ua, ub, multiplicity). What the kernel hands the combine step — the
// popcounts of V ∧ A_i ∧ B_j weighted by 2^(i+j), of V ∧ A_i by 2^i, of V ∧ B_j by 2^j, each modulo
// 2^128 — against the products of the values themselves, sign-extended to 128 bits.
struct Rows {
    uint64_t ua, ub, mult;
};
static void check_case(int64_t base_a, uint32_t n_a, int64_t base_b, uint32_t n_b, const std::vector<Rows>& rows) {
    u128 cross = 0, sua = 0, sub = 0, want = 0;
    uint64_t n = 0;
    for (const Rows& r : rows) {
        if ((n_a < 64 && (r.ua >> n_a)) || (n_b < 64 && (r.ub >> n_b))) die("test offset out of range", base_a, base_b, n_a, n_b);
        n += r.mult;
        for (uint32_t i = 0; i < n_a; ++i) {
            if (!((r.ua >> i) & 1ull)) continue;
            sua += (u128)r.mult << i;
            for (uint32_t j = 0; j < n_b; ++j)
                if ((r.ub >> j) & 1ull) cross += (u128)r.mult << (i + j);
        }
        for (uint32_t j = 0; j < n_b; ++j)
            if ((r.ub >> j) & 1ull) sub += (u128)r.mult << j;
        const int64_t a = (int64_t)((uint64_t)base_a + r.ua), b = (int64_t)((uint64_t)base_b + r.ub);
        want += (u128)(__int128)a * (u128)(__int128)b * (u128)r.mult;
    }
    int64_t out[2] = {-1, -1}, swapped[2] = {-1, -1};
    cubit::slice_product_combine(base_a, base_b, n, split(cross), split(sua), split(sub), out);
    cubit::slice_product_combine(base_b, base_a, n, split(cross), split(sub), split(sua), swapped);
    const u128 got = ((u128)(uint64_t)out[1] << 64) | (uint64_t)out[0];
    if (got != want) die("sum", base_a, base_b, n_a, n_b);
    if (out[0] != swapped[0] || out[1] != swapped[1]) die("not symmetric", base_a, base_b, n_a, n_b);
    ++checks;
}

// the bases of an n-slice operand: INT64_MIN, -1, 0 where the range stays inside int64, and the one
// that puts the top of the range at INT64_MAX
static std::vector<int64_t> bases_of(uint32_t bits) {
    const uint64_t top = max_off(bits);
    std::vector<int64_t> out;
    for (int64_t b : {INT64_MIN, (int64_t)-1, (int64_t)0})
        if ((u128)((uint64_t)b ^ 0x8000000000000000ull) + top <= (u128)~0ull) out.push_back(b);
    out.push_back((int64_t)((uint64_t)INT64_MAX - top));
    return out;
}

static void combine_checks() {
    // helpers first: the wide shift and the multiply by a signed 64-bit factor
    for (int rep = 0; rep < 2000; ++rep) {
        const u128 x = ((u128)rnd() << 64) | rnd();
        const int64_t m = rep % 5 == 0 ? INT64_MIN : rep % 5 == 1 ? -1 : (int64_t)rnd();
        const U128 p = cubit::u128_mul_s64(split(x), m);
        if ((((u128)p.hi << 64) | p.lo) != x * (u128)(__int128)m) die("u128_mul_s64", m, 0, (uint64_t)x, 0);
        const uint32_t s = (uint32_t)(rnd() % 128);
        const uint64_t y = rnd();
        const U128 q = cubit::u128_shl_wide(y, s);
        if ((((u128)q.hi << 64) | q.lo) != ((u128)y << s)) die("u128_shl_wide", s, 0, y, 0);
        checks += 2;
    }
    const uint32_t fixed[] = {0, 1, 7, 8, 9, 17, 63, 64};
    for (int rep = 0; rep < 600; ++rep) {
        // slice counts: the edges, then random 0 … 64 per side
        const uint32_t n_a = rep < 64 ? fixed[rep / 8] : (uint32_t)(rnd() % 65);
        const uint32_t n_b = rep < 64 ? fixed[rep % 8] : (uint32_t)(rnd() % 65);
        const uint64_t ta = max_off(n_a), tb = max_off(n_b);
        for (int64_t base_a : bases_of(n_a))
            for (int64_t base_b : bases_of(n_b)) {
                check_case(base_a, n_a, base_b, n_b, {});                    // no row: 0
                check_case(base_a, n_a, base_b, n_b, {{ta, tb, 0}});         // a count of 0
                check_case(base_a, n_a, base_b, n_b, {{0, 0, 1}});           // base_a · base_b alone
                check_case(base_a, n_a, base_b, n_b, {{ta, tb, 1}, {0, tb, 1ull << 33}, {ta, 0, 3}});
                std::vector<Rows> rows;
                const int n = (int)(rnd() % 7);
                for (int i = 0; i < n; ++i)
                    rows.push_back({n_a ? rnd() & ta : 0, n_b ? rnd() & tb : 0,
                                    (rnd() & 1) ? rnd() % 1000 : rnd() % (1ull << 34)});
                check_case(base_a, n_a, base_b, n_b, rows);
            }
    }
    // INT64_MIN · INT64_MIN from 64 slices on both sides, and from no slice at all
    check_case(INT64_MIN, 64, INT64_MIN, 64, {{0, 0, 1}});
    check_case(INT64_MIN, 0, INT64_MIN, 0, {{0, 0, 1ull << 40}});
    check_case(INT64_MIN, 64, INT64_MIN, 64, {{~0ull, ~0ull, 1ull << 40}, {0, ~0ull, 7}});
}

// ---- the path rules against a direct count, in whole eighths of a byte (128-bit integers: exact)

static u128 min128(u128 a, u128 b) { return a < b ? a : b; }
static uint32_t bits_direct(uint32_t n_a, uint32_t n_b, uint32_t k, bool na, bool nb) {
    const uint32_t n_in = n_a < n_b ? n_a : n_b, n_out = n_a < n_b ? n_b : n_a;
    uint32_t passes = (n_in + kProductInner - 1) / kProductInner;
    if (passes < 1) passes = 1;
    return k + (na ? 1 : 0) + (nb ? 1 : 0) + n_in + n_out * passes;
}
static bool plain_direct(bool fs, bool fc, bool usable, uint32_t n_a, uint32_t n_b, uint32_t k, bool na, bool nb,
                         uint64_t live, uint64_t rows, uint64_t est, int b_decode) {
    if (fc || !usable) return false;
    if (fs) return true;
    if ((n_a < n_b ? n_a : n_b) > kProductInner) return false;
    const u128 slices = (u128)bits_direct(n_a, n_b, k, na, nb) * live;
    const u128 gather = min128((u128)1024 * est, (u128)64 * rows);
    const u128 column = (u128)k * live + gather + (b_decode < 0 ? gather : (u128)(uint32_t)b_decode * live);
    return slices <= column;
}
static bool grouped_direct(bool fs, bool fc, bool usable, uint32_t n_a, uint32_t n_b, uint64_t slice_bits, uint32_t k,
                           uint64_t live, uint64_t rows, uint64_t est, const uint64_t* elem, uint32_t n_probed) {
    if (fc || !usable) return false;
    if (fs) return true;
    if ((n_a < n_b ? n_a : n_b) > kProductInner) return false;
    u128 column = (u128)k * live + (u128)128 * est;  // the scan, the ids written and read
    for (uint32_t i = 0; i < n_probed; ++i) column += (u128)128 * est + min128((u128)1024 * est, (u128)8 * elem[i] * rows);
    return (u128)slice_bits * live <= column;
}

static void path_rule_checks() {
    const uint64_t rows = 612ull << 20;
    const uint32_t counts[] = {0, 1, 4, kProductInner, kProductInner + 1, 17, 24, 64};
    for (uint32_t n_a : counts)
        for (uint32_t n_b : counts)
            for (uint32_t k : {0u, 1u, 8u})
                for (int nul = 0; nul < 4; ++nul)
                    for (uint64_t live : {rows, rows / 7})
                        for (int b_decode : {-1, 0, 2, 3})
                            for (uint64_t est = 0; est <= rows; est = est ? est * 4 : 1) {
                                for (int f = 0; f < 8; ++f) {
                                    const bool got = cubit::sum_product_from_slices(f & 1, f & 2, f & 4, n_a, n_b, k, nul & 1,
                                                                                    nul & 2, live, rows, est, b_decode);
                                    if (got != plain_direct(f & 1, f & 2, f & 4, n_a, n_b, k, nul & 1, nul & 2, live, rows, est,
                                                            b_decode))
                                        die("plain rule differs from the direct count", f, b_decode, n_a * 100 + n_b, est);
                                    ++checks;
                                }
                                if (cubit::product_slice_bits(n_a, n_b, k, nul & 1, nul & 2) !=
                                    bits_direct(n_a, n_b, k, nul & 1, nul & 2))
                                    die("slice bits", n_a, n_b, k, (uint64_t)nul);
                            }
    // n_in at kProductInner: auto takes the slices of a filter that keeps every row; one above: auto
    // refuses whatever the bytes say, forced accepts
    if (!cubit::sum_product_from_slices(false, false, true, 24, kProductInner, 1, false, false, rows, rows, rows, -1))
        die("n_in at kProductInner, dense", 0, 0, 24, kProductInner);
    if (cubit::sum_product_from_slices(false, false, true, 24, kProductInner + 1, 1, false, false, rows, rows, rows, -1))
        die("n_in above kProductInner taken automatically", 0, 0, 24, kProductInner + 1);
    if (cubit::sum_product_from_slices(false, false, true, kProductInner + 1, 64, 0, false, false, rows, rows, rows, -1))
        die("n_in above kProductInner taken automatically (swapped)", 0, 0, kProductInner + 1, 64);
    if (!cubit::sum_product_from_slices(true, false, true, 24, kProductInner + 1, 1, false, false, rows, rows, rows, -1))
        die("forced slices refused above kProductInner", 0, 0, 24, kProductInner + 1);
    if (cubit::sum_product_from_slices(true, false, false, 24, 4, 1, false, false, rows, rows, rows, -1))
        die("slices without usable indexes", 0, 0, 24, 4);
    checks += 5;
    // a tie goes to the slices: 8 + 0 slices, no leaf, 8·live eighths against two gathers of 1,024·est
    {
        const uint64_t live = 1ull << 20, est = live / 256;
        if (!cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, est, -1))
            die("tie", 0, 0, live, est);
        if (cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, est - 1, -1))
            die("one row below the tie", 0, 0, live, est - 1);
        // b pinned: one gather; the tie moves to twice the estimate. b decoded from 2 leaves: 2·live more
        if (!cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, 2 * est, 0) ||
            cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, 2 * est - 1, 0))
            die("tie with b pinned", 0, 0, live, est);
        if (!cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, 6 * live / 1024, 2) ||
            cubit::sum_product_from_slices(false, false, true, 8, 0, 0, false, false, live, live, 6 * live / 1024 - 1, 2))
            die("tie with b decoded", 0, 0, live, est);
        checks += 6;
    }
    // the Q1 shape at 612 M rows: 24 × 4 slices, one leaf, 98 % kept: slices; Q6's 2 %: the gather
    if (!cubit::sum_product_from_slices(false, false, true, 24, 4, 1, false, false, rows, rows, rows / 100 * 98, -1))
        die("Q1 shape", 0, 0, 24, 4);
    if (cubit::sum_product_from_slices(false, false, true, 24, 4, 4, false, false, rows, rows, rows / 1000, -1))
        die("sparse filter", 0, 0, 24, 4);
    checks += 2;

    // grouped: one or two group columns, 1 … 17 leaves, the launches split_group_batches makes
    for (uint32_t n_a : {0u, 4u, kProductInner, kProductInner + 1, 24u})
        for (uint32_t n_b : {4u, 24u, 64u})
            for (uint32_t k : {0u, 2u, 8u})
                for (uint32_t g1 : {1u, 3u, 9u, 17u})
                    for (uint32_t g2 : {0u, 2u, 3u}) {
                        const bool two = g2 != 0;
                        const uint32_t row_bits = cubit::product_slice_bits(n_a, n_b, k, true, false);
                        bool swapped = false;
                        const auto batches = cubit::split_group_batches(g1, g2, two, kProductGroupBatch, row_bits, &swapped);
                        uint64_t direct_bits = 0, pairs = 0;
                        for (const auto& b : batches) {
                            if (b.na > (two ? kProductGroupBatch / 2 : kProductGroupBatch) || b.nb > 2) die("batch too wide", b.na, b.nb, g1, g2);
                            direct_bits += row_bits + b.na + b.nb;
                            pairs += (uint64_t)b.na * (two ? b.nb : 1);
                        }
                        if (pairs != (uint64_t)g1 * (two ? g2 : 1)) die("batches miss a group", 0, 0, g1, g2);
                        const uint64_t bits = cubit::group_batches_bits(batches, row_bits);
                        if (bits != direct_bits) die("batch bits", 0, 0, bits, direct_bits);
                        const uint64_t elem[4] = {8, 8, 4, 8};
                        const uint32_t n_probed = 2 + (two ? 2 : 1);
                        for (uint64_t est = 0; est <= rows; est = est ? est * 4 : 1)
                            for (int f = 0; f < 8; ++f) {
                                const bool got = cubit::sum_product_grouped_from_slices(f & 1, f & 2, f & 4, n_a, n_b, bits, k, rows,
                                                                                        rows, est, elem, n_probed);
                                if (got != grouped_direct(f & 1, f & 2, f & 4, n_a, n_b, bits, k, rows, rows, est, elem, n_probed))
                                    die("grouped rule differs from the direct count", f, (int64_t)est, n_a * 100 + n_b, g1 * 100 + g2);
                                ++checks;
                            }
                    }
}

int main() {
    combine_checks();
    path_rule_checks();
    std::printf("slice product ok %" PRIu64 " checks\n", checks);
    return 0;
}
