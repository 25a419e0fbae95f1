// The bit-sliced select's host side (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) on the CPU: the
// quantile_disc index rule, the bucket walk of one radix step, a CPU model of the whole pass sequence
// over random slice sets against std::nth_element, and the path rule select_from_slices.
// tests/test_slice_select_core.py builds this with AddressSanitizer and UBSan and runs it. Exit status 1
// at the first failed check, which is printed.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

#define CHECK(cond, ...)                   \
    do {                                   \
        ++checks;                          \
        if (!(cond)) {                     \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);      \
            std::printf("\n");             \
            std::exit(1);                  \
        }                                  \
    } while (0)

// ---- the index rule against a literal restatement of the reference's formula:
//   scaled_q = (double)(n * q); floored = (idx_t)floor(n - scaled_q); index = max(1, n - floored) - 1
static uint64_t index_restated(uint64_t n, double q) {
    volatile double scaled_q = (double)n * q;  // rounded to double before the subtraction
    volatile double diff = (double)n - scaled_q;
    const uint64_t floored = (uint64_t)std::floor(diff);
    return std::max<uint64_t>(1, n - floored) - 1;
}
static void check_index(uint64_t n, double q) {
    if (!(q >= 0.0 && q <= 1.0)) return;
    const uint64_t got = quantile_disc_index(n, q), want = index_restated(n, q);
    CHECK(got == want, "n %" PRIu64 " q %.17g: %" PRIu64 " != %" PRIu64, n, q, got, want);
    CHECK(n == 0 ? got == 0 : got < n, "n %" PRIu64 " q %.17g: index %" PRIu64 " out of range", n, q, got);
}
static void index_rule() {
    const double grid[] = {0.0, 1.0, 0.5, 1.0 / 3.0, 0.1, 0.9, 0.25, 0.75, 0.99, 1e-9};
    for (uint64_t n = 0; n <= 2000; ++n) {
        for (double q : grid) check_index(n, q);
        const uint64_t js[] = {0, 1, n / 3, n / 2, n ? n - 1 : 0, n};
        for (uint64_t j : js) {
            if (n == 0 || j > n) continue;
            const double q = (double)j / (double)n;
            check_index(n, q);
            check_index(n, std::nextafter(q, 0.0));
            check_index(n, std::nextafter(q, 1.0));
        }
    }
    for (uint64_t big : {1ull << 33, 1ull << 47})
        for (int64_t dn = -3; dn <= 3; ++dn) {
            const uint64_t n = big + (uint64_t)dn;
            for (double q : grid) check_index(n, q);
            for (int r = 0; r < 50; ++r) {
                const double q = (double)(rnd() % n) / (double)n;
                check_index(n, q);
                check_index(n, std::nextafter(q, 0.0));
                check_index(n, std::nextafter(q, 1.0));
            }
        }
    // the ends: q = 0 is the smallest row, q = 1 the largest, the median of an even count the lower one
    CHECK(quantile_disc_index(10, 0.0) == 0 && quantile_disc_index(10, 1.0) == 9 && quantile_disc_index(10, 0.5) == 4,
          "ends");
    CHECK(quantile_disc_index(11, 0.5) == 5 && quantile_disc_index(1, 0.5) == 0, "odd median");
}

// ---- the bucket walk against brute force over the expanded rows
static void check_walk(const std::vector<uint64_t>& counts, bool desc, uint64_t rank) {
    const uint32_t nb = (uint32_t)counts.size();
    std::vector<uint32_t> rows;  // every row's bucket, in the walk's order
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t b = desc ? nb - 1 - i : i;
        for (uint64_t c = 0; c < counts[b]; ++c) rows.push_back(b);
    }
    uint32_t bucket = 9999;
    uint64_t rank_in = ~0ull, out = ~0ull;
    const bool found = select_walk(counts.data(), nb, desc, rank, &bucket, &rank_in, &out);
    CHECK(found == (rank < rows.size()), "nb %u desc %d rank %" PRIu64, nb, (int)desc, rank);
    if (!found) {
        CHECK(bucket == 9999 && rank_in == ~0ull && out == ~0ull, "not found writes nothing");
        return;
    }
    uint64_t before = 0;  // rows of the buckets walked before the rank's bucket
    for (uint32_t r : rows) before += desc ? r > rows[rank] : r < rows[rank];
    CHECK(bucket == rows[rank] && out == before && rank_in == rank - before,
          "nb %u desc %d rank %" PRIu64 ": bucket %u in %" PRIu64 " out %" PRIu64, nb, (int)desc, rank, bucket, rank_in, out);
}
static void bucket_walk() {
    for (uint32_t d = 1; d <= 5; ++d) {
        const uint32_t nb = 1u << d;
        for (int round = 0; round < 60; ++round) {
            std::vector<uint64_t> counts(nb, 0);
            const int shape = round % 4;
            if (shape == 0) counts[rnd() % nb] = 1 + rnd() % 9;  // one non-empty bucket
            else if (shape == 1)
                for (auto& c : counts) c = rnd() % 3 ? 0 : rnd() % 7;  // mostly zero counts
            else if (shape == 2)
                for (auto& c : counts) c = rnd() % 12;
            // shape 3: all zero
            uint64_t total = 0;
            for (uint64_t c : counts) total += c;
            for (bool desc : {false, true}) {
                const uint64_t ranks[] = {0, 1, total / 2, total ? total - 1 : 0, total, total + 5, rnd() % (total + 1)};
                for (uint64_t r : ranks) check_walk(counts, desc, r);
            }
        }
    }
    // counts past 2^32 (ranks are 64-bit)
    const std::vector<uint64_t> big = {1ull << 40, 0, 3ull << 33, 7};
    uint32_t b;
    uint64_t in, out;
    CHECK(select_walk(big.data(), 4, false, (1ull << 40) + 5, &b, &in, &out) && b == 2 && in == 5 && out == (1ull << 40),
          "64-bit ascending");
    CHECK(select_walk(big.data(), 4, true, 7, &b, &in, &out) && b == 2 && in == 0 && out == 7, "64-bit descending");
}

// ---- the whole pass sequence as the kernels run it, on slices held as row bitmaps: pass 0 forms the
// candidates F ∧ valid and histograms the first chunk, every later pass narrows the candidates by the
// bucket the step chose and histograms the next chunk; one select_step after each.
struct Model {
    uint32_t bits;
    std::vector<std::vector<bool>> slice;  // [bits][rows]
    std::vector<bool> valid, filter;
};
static void histogram(const Model& m, const std::vector<bool>& cand, uint32_t cnt, uint32_t low, uint64_t* counts) {
    for (uint32_t i = 0; i < (1u << cnt); ++i) counts[i] = 0;
    for (size_t r = 0; r < cand.size(); ++r) {
        if (!cand[r]) continue;
        uint32_t b = 0;
        for (uint32_t j = 0; j < cnt; ++j) b |= (m.slice[low + j][r] ? 1u : 0u) << j;
        ++counts[b];
    }
}
static void run_model(const Model& m, int type, int64_t base, int mode, uint64_t k, double q, int64_t out[6]) {
    const size_t n = m.valid.size();
    std::vector<bool> cand(n);
    uint64_t count_rows = 0;
    for (size_t r = 0; r < n; ++r) {
        cand[r] = m.filter[r] && m.valid[r];
        count_rows += m.filter[r];
    }
    SelectState s{};
    const uint32_t passes = select_passes(m.bits, kSelectChunk);
    uint64_t counts[1u << kSelectChunk];
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t cnt = select_chunk_bits(m.bits, kSelectChunk, p), low = select_chunk_low(m.bits, kSelectChunk, p);
        if (p > 0 && s.found) {  // narrow by the previous chunk's bucket
            const uint32_t pc = select_chunk_bits(m.bits, kSelectChunk, p - 1), pl = select_chunk_low(m.bits, kSelectChunk, p - 1);
            for (size_t r = 0; r < n; ++r)
                for (uint32_t j = 0; j < pc && cand[r]; ++j)
                    if (m.slice[pl + j][r] != (((s.prefix >> (pl + j)) & 1ull) != 0)) cand[r] = false;
        }
        histogram(m, cand, cnt, low, counts);
        select_step(&s, p == 0, mode, k, q, counts, 1u << cnt, low);
    }
    select_result(s, type, base, count_rows, out);
}
static void check_model(uint32_t bits, size_t n, int ties, bool nulls) {
    Model m;
    m.bits = bits;
    m.slice.assign(bits, std::vector<bool>(n));
    m.valid.assign(n, true);
    m.filter.assign(n, true);
    std::vector<uint64_t> off(n);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    uint64_t pool[3] = {rnd() & mask, rnd() & mask, mask};
    for (size_t r = 0; r < n; ++r) {
        off[r] = ties == 2 ? pool[0] : (ties == 1 ? pool[rnd() % 3] : rnd() & mask);
        if (nulls && rnd() % 5 == 0) m.valid[r] = false;
        m.filter[r] = rnd() % 3 != 0;
        for (uint32_t s = 0; s < bits; ++s) m.slice[s][r] = m.valid[r] && ((off[r] >> s) & 1ull);
    }
    const int64_t base = bits == 64 ? INT64_MIN : (int64_t)(rnd() % 1000) - 500;
    std::vector<uint64_t> sel;
    uint64_t count_rows = 0;
    for (size_t r = 0; r < n; ++r) {
        count_rows += m.filter[r];
        if (m.filter[r] && m.valid[r]) sel.push_back(off[r]);
    }
    const uint64_t cv = sel.size();
    auto expect = [&](bool desc, uint64_t rank, int mode, uint64_t k, double q) {
        int64_t out[6];
        run_model(m, CUBIT_TYPE_INT64, base, mode, k, q, out);
        CHECK(out[4] == (int64_t)cv && out[5] == (int64_t)count_rows, "counts: bits %u n %zu", bits, n);
        if (rank >= cv) {
            CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0, "not found: bits %u n %zu rank %" PRIu64, bits, n, rank);
            return;
        }
        std::vector<uint64_t> v = sel;
        if (desc) std::nth_element(v.begin(), v.begin() + (ptrdiff_t)rank, v.end(), std::greater<uint64_t>());
        else std::nth_element(v.begin(), v.begin() + (ptrdiff_t)rank, v.end());
        const uint64_t want = v[rank];
        uint64_t below = 0, equal = 0;
        for (uint64_t x : sel) {
            below += desc ? x > want : x < want;
            equal += x == want;
        }
        CHECK(out[1] == 1 && (uint64_t)out[0] == (uint64_t)base + want && (uint64_t)out[2] == below && (uint64_t)out[3] == equal,
              "bits %u n %zu mode %d rank %" PRIu64 ": value %" PRId64 " below %" PRId64 " equal %" PRId64, bits, n, mode,
              rank, out[0], out[2], out[3]);
    };
    const uint64_t ranks[] = {0, 1, cv / 2, cv ? cv - 1 : 0, cv, cv + 3, cv ? rnd() % cv : 0};
    for (uint64_t r : ranks) {
        expect(false, r, kSelectRank, r, 0.0);
        expect(true, r, kSelectRankDesc, r, 0.0);
    }
    for (double q : {0.0, 0.1, 0.25, 0.5, 1.0}) expect(false, cv ? index_restated(cv, q) : 0, kSelectQuantile, 0, q);
}
static void pass_sequence() {
    for (uint32_t bits = 0; bits <= 64; ++bits)
        for (int ties = 0; ties < 3; ++ties) {
            const size_t n = bits % 7 == 0 ? 1 + rnd() % 3000 : rnd() % 300;
            check_model(bits, n, ties, (bits + ties) % 2 == 0);
        }
    // the chunking: every slice lies in exactly one chunk, most significant first, later chunks whole
    for (uint32_t bits = 0; bits <= 64; ++bits) {
        const uint32_t passes = select_passes(bits, kSelectChunk);
        uint32_t next = bits;
        for (uint32_t p = 0; p < passes; ++p) {
            const uint32_t cnt = select_chunk_bits(bits, kSelectChunk, p), low = select_chunk_low(bits, kSelectChunk, p);
            CHECK(low + cnt == next && cnt <= kSelectChunk && (p == 0 || cnt == kSelectChunk), "chunks of %u bits", bits);
            next = low;
        }
        CHECK(next == 0, "chunks of %u bits end at 0", bits);
    }
}

// ---- the path rule
// The rule as it stood before the three path rules shared one byte count, restated literally:
// select_from_slices gives this answer at every point, ties included.
static bool select_restated(bool force_slices, bool force_column, bool usable, uint32_t bits, uint32_t k_leaves,
                            bool nullable, uint64_t live_rows, uint64_t rows, uint64_t est_rows, uint64_t elem_bytes) {
    if (force_column || !usable) return false;
    if (force_slices) return true;
    const uint32_t passes = select_passes(bits, kSelectChunk);
    const uint32_t last = select_chunk_bits(bits, kSelectChunk, passes - 1);
    const double per_row = (double)(k_leaves + (nullable ? 1u : 0u) + 1u + 2u * bits - last + 2u * (passes - 1));
    const double slices = per_row / 8.0 * (double)live_rows;
    const double gathered = std::min(128.0 * (double)est_rows, (double)elem_bytes * (double)rows);
    const double column = (double)k_leaves / 8.0 * (double)live_rows + 32.0 * (double)est_rows + gathered +
                          8.0 * (double)(64 / kSelectArrayBits) * (double)est_rows;
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

static void path_rule() {
    for (uint32_t bits : {0u, 1u, 4u, 12u, 24u, 64u})
        for (uint32_t k : {0u, 1u, 4u, 8u})
            for (bool nullable : {false, true})
                for (uint64_t rows : {1ull, 1000ull, 131072ull, 612000000ull}) {
                    const uint64_t live = rows;
                    bool prev = false;
                    for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1) {
                        const bool s = select_from_slices(false, false, true, bits, k, nullable, live, rows, est, 8);
                        CHECK(!prev || s, "monotone: bits %u k %u rows %" PRIu64 " est %" PRIu64, bits, k, rows, est);
                        prev = s;
                        CHECK(select_from_slices(true, false, true, bits, k, nullable, live, rows, est, 8), "forced slices");
                        CHECK(!select_from_slices(false, true, true, bits, k, nullable, live, rows, est, 8), "forced column");
                        CHECK(!select_from_slices(false, false, false, bits, k, nullable, live, rows, est, 8), "no index");
                        CHECK(!select_from_slices(true, false, false, bits, k, nullable, live, rows, est, 8), "no index, forced");
                        for (int f = 0; f < 8; ++f)
                            CHECK(select_from_slices(f & 1, f & 2, f & 4, bits, k, nullable, live, rows, est, 8) ==
                                      select_restated(f & 1, f & 2, f & 4, bits, k, nullable, live, rows, est, 8),
                                  "restated: bits %u k %u rows %" PRIu64 " est %" PRIu64 " flags %d", bits, k, rows, est, f);
                    }
                    // just below, at and just above the estimate where the restated rule turns
                    const uint64_t x = crossover(rows, [&](uint64_t est) {
                        return select_restated(false, false, true, bits, k, nullable, live, rows, est, 8);
                    });
                    for (uint64_t est : {x ? x - 1 : 0, x, x + 1})
                        CHECK(select_from_slices(false, false, true, bits, k, nullable, live, rows, est, 8) ==
                                  select_restated(false, false, true, bits, k, nullable, live, rows, est, 8),
                              "restated at the crossover: bits %u k %u rows %" PRIu64 " est %" PRIu64, bits, k, rows, est);
                }
    // every row of a large partition: the slices; a handful of rows: the column
    CHECK(select_from_slices(false, false, true, 24, 2, true, 612000000, 612000000, 306000000, 4), "dense takes the slices");
    CHECK(!select_from_slices(false, false, true, 24, 2, true, 612000000, 612000000, 100, 4), "sparse takes the column");
}

int main() {
    index_rule();
    bucket_walk();
    pass_sequence();
    path_rule();
    std::printf("slice select ok %" PRIu64 " checks\n", checks);
    return 0;
}
