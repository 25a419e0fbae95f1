// The grouped bit-sliced select's host side (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) on the
// CPU: a model of the grouped pass sequence as the kernels run it — one shared candidate set, a
// histogram per group, select_step per group, narrowing by each group's own bucket, batches of groups —
// over random slice sets against std::nth_element per group, and the path rule
// select_grouped_from_slices. tests/test_slice_select_grouped_core.py builds this with AddressSanitizer
// and UBSan and runs it. Exit status 1 at the first failed check, which is printed.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cubit_program.hpp"

using namespace cubit;

static uint64_t checks = 0;
static uint64_t rng_state = 0x2545f4914f6cdd1dull;
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

// ---- the grouped pass sequence on slices held as row bitmaps
struct Model {
    uint32_t bits;
    std::vector<std::vector<bool>> slice;  // [bits][rows]
    std::vector<bool> valid, filter;
    std::vector<int> group;  // the row's group, -1: in none (the group bitvectors are disjoint)
    uint32_t n_groups;
};
// One batch [g0, g0 + ng) through all its passes over the shared candidate set `cand`, which pass 0
// rewrites whole. out: 6 slots per group of the call.
static void run_batch(const Model& m, std::vector<bool>& cand, uint32_t g0, uint32_t ng, int type, int64_t base, int mode,
                      uint64_t k, double q, int64_t* out) {
    const size_t n = m.valid.size();
    constexpr uint32_t NB = 1u << kSelectChunk;
    std::vector<SelectState> st(ng);
    std::vector<uint64_t> rows(ng, 0);
    std::vector<uint64_t> counts((size_t)ng * NB);
    auto slot_of = [&](size_t r) -> int {
        const int g = m.group[r];
        return g >= (int)g0 && g < (int)(g0 + ng) ? g - (int)g0 : -1;
    };
    // pass 0: C = ∪_g F ∧ E_g ∧ valid, count_rows_g = |F ∧ E_g|
    for (size_t r = 0; r < n; ++r) {
        const int s = slot_of(r);
        cand[r] = s >= 0 && m.filter[r] && m.valid[r];
        if (s >= 0 && m.filter[r]) ++rows[(size_t)s];
    }
    const uint32_t passes = select_passes(m.bits, kSelectChunk);
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t cnt = select_chunk_bits(m.bits, kSelectChunk, p), low = select_chunk_low(m.bits, kSelectChunk, p);
        if (p > 0) {  // C' = C ∧ ∪_g (E_g ∧ [previous chunk = group g's bucket]); a group not found keeps nothing
            const uint32_t pc = select_chunk_bits(m.bits, kSelectChunk, p - 1), pl = select_chunk_low(m.bits, kSelectChunk, p - 1);
            bool any = false;
            for (uint32_t s = 0; s < ng; ++s) any |= st[s].found != 0;
            if (any) {  // (a batch without a found group leaves the candidates alone)
                for (size_t r = 0; r < n; ++r) {
                    if (!cand[r]) continue;
                    const int s = slot_of(r);
                    bool keep = s >= 0 && st[(size_t)s].found;
                    for (uint32_t j = 0; j < pc && keep; ++j)
                        if (m.slice[pl + j][r] != (((st[(size_t)s].prefix >> (pl + j)) & 1ull) != 0)) keep = false;
                    cand[r] = keep;
                }
            }
        }
        std::fill(counts.begin(), counts.end(), 0);
        bool any = p == 0;
        for (uint32_t s = 0; s < ng; ++s) any |= st[s].found != 0;
        if (any)
            for (size_t r = 0; r < n; ++r) {
                if (!cand[r]) continue;
                const int s = slot_of(r);
                if (s < 0 || (p > 0 && !st[(size_t)s].found)) continue;
                uint32_t b = 0;
                for (uint32_t j = 0; j < cnt; ++j) b |= (m.slice[low + j][r] ? 1u : 0u) << j;
                ++counts[(size_t)s * NB + b];
            }
        // (the partials hold 2^kSelectChunk counters per slot whatever the chunk; those past 2^cnt are zero)
        for (uint32_t s = 0; s < ng; ++s) select_step(&st[s], p == 0, mode, k, q, &counts[(size_t)s * NB], NB, low);
    }
    for (uint32_t s = 0; s < ng; ++s) select_result(st[s], type, base, rows[s], out + 6 * (size_t)(g0 + s));
}
static void run_model(const Model& m, uint32_t batch, int type, int64_t base, int mode, uint64_t k, double q,
                      std::vector<int64_t>& out) {
    out.assign((size_t)m.n_groups * 6, -1);
    std::vector<bool> cand(m.valid.size());  // the one scratch candidate set, shared by the batches
    for (uint32_t g0 = 0; g0 < m.n_groups; g0 += batch)
        run_batch(m, cand, g0, std::min(batch, m.n_groups - g0), type, base, mode, k, q, out.data());
}

static uint64_t index_restated(uint64_t n, double q) {
    volatile double scaled_q = (double)n * q;
    volatile double diff = (double)n - scaled_q;
    const uint64_t floored = (uint64_t)std::floor(diff);
    return std::max<uint64_t>(1, n - floored) - 1;
}

static void check_model(uint32_t bits, size_t n, uint32_t n_groups, int ties, bool nulls) {
    Model m;
    m.bits = bits;
    m.n_groups = n_groups;
    m.slice.assign(bits, std::vector<bool>(n));
    m.valid.assign(n, true);
    m.filter.assign(n, true);
    m.group.assign(n, -1);
    std::vector<uint64_t> off(n);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    const uint64_t pool[3] = {rnd() & mask, rnd() & mask, mask};
    // some groups stay empty, group 0 holds one value only, about a tenth of the rows are in no group
    const uint32_t empty_a = n_groups > 2 ? (uint32_t)(rnd() % n_groups) : n_groups;
    const uint32_t empty_b = n_groups > 5 ? (uint32_t)(rnd() % n_groups) : n_groups;
    const uint64_t one_value = rnd() & mask;
    for (size_t r = 0; r < n; ++r) {
        off[r] = ties == 2 ? pool[0] : (ties == 1 ? pool[rnd() % 3] : rnd() & mask);
        if (nulls && rnd() % 5 == 0) m.valid[r] = false;
        m.filter[r] = rnd() % 3 != 0;
        if (rnd() % 10 != 0) {
            // skewed sizes: a rank found in the large groups lies past the end of the small ones
            uint32_t g = (uint32_t)(rnd() % n_groups);
            if (rnd() % 2) g = (uint32_t)(rnd() % (g + 1));
            if (g != empty_a && g != empty_b) m.group[r] = (int)g;
        }
        if (m.group[r] == 0 && n_groups > 1) off[r] = one_value;
        for (uint32_t s = 0; s < bits; ++s) m.slice[s][r] = m.valid[r] && ((off[r] >> s) & 1ull);
    }
    const int64_t base = bits == 64 ? INT64_MIN : (int64_t)(rnd() % 1000) - 500;
    std::vector<std::vector<uint64_t>> sel(n_groups);
    std::vector<uint64_t> count_rows(n_groups, 0);
    uint64_t largest = 0;
    for (size_t r = 0; r < n; ++r) {
        if (m.group[r] < 0 || !m.filter[r]) continue;
        ++count_rows[(size_t)m.group[r]];
        if (m.valid[r]) sel[(size_t)m.group[r]].push_back(off[r]);
    }
    for (const auto& v : sel) largest = std::max<uint64_t>(largest, v.size());

    auto expect = [&](int mode, uint64_t k, double q) {
        std::vector<int64_t> ref_out, out;
        for (uint32_t batch = 1; batch <= 8; ++batch) {  // the result is the same at every batch size
            run_model(m, batch, CUBIT_TYPE_INT64, base, mode, k, q, out);
            if (batch == 1) ref_out = out;
            CHECK(out == ref_out, "batch %u differs: bits %u n %zu groups %u", batch, bits, n, n_groups);
        }
        run_model(m, kGroupBatchSelect, CUBIT_TYPE_INT64, base, mode, k, q, out);
        CHECK(out == ref_out, "kGroupBatchSelect differs: bits %u n %zu groups %u", bits, n, n_groups);
        const bool desc = mode == kSelectRankDesc;
        for (uint32_t g = 0; g < n_groups; ++g) {
            const int64_t* o = &out[(size_t)g * 6];
            const uint64_t cv = sel[g].size();
            const uint64_t rank = mode == kSelectQuantile ? (cv ? index_restated(cv, q) : 0) : k;
            CHECK(o[4] == (int64_t)cv && o[5] == (int64_t)count_rows[g], "counts: bits %u n %zu group %u", bits, n, g);
            if (count_rows[g] == 0) CHECK(std::all_of(o, o + 6, [](int64_t x) { return x == 0; }), "six zeros: group %u", g);
            if (rank >= cv) {
                CHECK(o[0] == 0 && o[1] == 0 && o[2] == 0 && o[3] == 0, "not found: bits %u n %zu group %u rank %" PRIu64, bits, n,
                      g, rank);
                continue;
            }
            std::vector<uint64_t> v = sel[g];
            if (desc) std::nth_element(v.begin(), v.begin() + (ptrdiff_t)rank, v.end(), std::greater<uint64_t>());
            else std::nth_element(v.begin(), v.begin() + (ptrdiff_t)rank, v.end());
            const uint64_t want = v[rank];
            uint64_t below = 0, equal = 0;
            for (uint64_t x : sel[g]) {
                below += desc ? x > want : x < want;
                equal += x == want;
            }
            CHECK(o[1] == 1 && (uint64_t)o[0] == (uint64_t)base + want && (uint64_t)o[2] == below && (uint64_t)o[3] == equal,
                  "bits %u n %zu groups %u group %u mode %d rank %" PRIu64 ": value %" PRId64 " below %" PRId64 " equal %" PRId64,
                  bits, n, n_groups, g, mode, rank, o[0], o[2], o[3]);
        }
    };
    // ranks of the largest group: found there, past the end in the smaller ones
    const uint64_t ranks[] = {0, 1, largest / 2, largest ? largest - 1 : 0, largest, largest ? rnd() % largest : 0};
    for (uint64_t r : ranks) {
        expect(kSelectRank, r, 0.0);
        expect(kSelectRankDesc, r, 0.0);
    }
    for (double q : {0.0, 0.5, 1.0}) expect(kSelectQuantile, 0, q);
}
static void pass_sequence() {
    for (uint32_t bits = 0; bits <= 64; ++bits)
        for (int ties = 0; ties < 3; ++ties) {
            const size_t n = bits % 7 == 0 ? 1 + rnd() % 3000 : rnd() % 300;
            const uint32_t n_groups = 1 + (uint32_t)(rnd() % 20);
            check_model(bits, n, n_groups, ties, (bits + ties) % 2 == 0);
        }
    for (uint32_t n_groups = 1; n_groups <= 20; ++n_groups) check_model(12, 1 + rnd() % 3000, n_groups, (int)(n_groups % 3), true);
}

// ---- the path rule
// slice_bits restated literally over the batches
static uint64_t slice_bits_restated(const std::vector<GroupBatch>& bs, uint32_t bits, uint32_t k_leaves, bool nullable) {
    const uint32_t passes = bits ? (bits + 3) / 4 : 1;
    const uint32_t d_last = bits ? 4 : 0;  // every later chunk is whole, so the last one is unless it is the first
    const uint32_t last = passes == 1 ? bits : d_last;
    uint64_t sum = 0;
    const size_t launches = bs.empty() ? 1 : bs.size();
    for (size_t i = 0; i < launches; ++i) {
        const uint64_t leaves = bs.empty() ? 0 : bs[i].na + bs[i].nb;
        sum += k_leaves + (nullable ? 1 : 0) + 1 + 2 * bits - last + 2 * (passes - 1) + leaves * passes;
    }
    return sum;
}
static void path_rule() {
    static_assert(kSelectChunk == 4, "the restatement spells the chunk out");
    const std::vector<GroupBatch> none;
    for (uint32_t bits : {0u, 1u, 4u, 5u, 12u, 24u, 64u})
        for (uint32_t k : {0u, 1u, 4u, 8u})
            for (bool nullable : {false, true})
                for (uint64_t rows : {1ull, 1000ull, 131072ull, 612000000ull})
                    for (uint64_t eb : {4ull, 8ull}) {
                        const uint64_t live = rows;
                        // no group leaf, one launch: select_from_slices at every grid point
                        const uint64_t sb0 = select_grouped_slice_bits(none, bits, k, nullable);
                        for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1)
                            for (int f = 0; f < 8; ++f)
                                CHECK(select_grouped_from_slices(f & 1, f & 2, f & 4, sb0, k, live, rows, est, &eb, 1) ==
                                          select_from_slices(f & 1, f & 2, f & 4, bits, k, nullable, live, rows, est, eb),
                                      "ungrouped: bits %u k %u rows %" PRIu64 " est %" PRIu64 " flags %d", bits, k, rows, est, f);
                        for (uint32_t n1 : {1u, 3u, 7u, 9u, 25u})
                            for (uint32_t n2 : {0u, 2u, 3u}) {
                                bool swapped = false;
                                const std::vector<GroupBatch> bs = split_group_batches(
                                    n1, n2, n2 != 0, kGroupBatchSelect, bits + k + (nullable ? 1u : 0u), &swapped);
                                const uint64_t sb = select_grouped_slice_bits(bs, bits, k, nullable);
                                CHECK(sb == slice_bits_restated(bs, bits, k, nullable), "slice_bits: bits %u k %u %u x %u", bits, k,
                                      n1, n2);
                                const uint64_t ebs[3] = {eb, 4, 8};
                                const uint32_t np = n2 ? 3 : 2;
                                bool prev = false;
                                for (uint64_t est = 0; est <= rows; est = est ? est * 2 : 1) {
                                    const bool s = select_grouped_from_slices(false, false, true, sb, k, live, rows, est, ebs, np);
                                    CHECK(!prev || s, "monotone: bits %u k %u rows %" PRIu64 " est %" PRIu64, bits, k, rows, est);
                                    prev = s;
                                    CHECK(select_grouped_from_slices(true, false, true, sb, k, live, rows, est, ebs, np), "forced slices");
                                    CHECK(!select_grouped_from_slices(false, true, true, sb, k, live, rows, est, ebs, np), "forced column");
                                    CHECK(!select_grouped_from_slices(false, false, false, sb, k, live, rows, est, ebs, np), "no index");
                                    CHECK(!select_grouped_from_slices(true, false, false, sb, k, live, rows, est, ebs, np),
                                          "no index, forced");
                                }
                            }
                    }
    // every batch holds at most kGroupBatchSelect groups, and every group lands in exactly one
    for (uint32_t n1 = 1; n1 <= 40; ++n1) {
        bool swapped = false;
        const std::vector<GroupBatch> bs = split_group_batches(n1, 0, false, kGroupBatchSelect, 13, &swapped);
        uint32_t next = 0;
        for (const GroupBatch& b : bs) {
            CHECK(b.a0 == next && b.na >= 1 && b.na <= kGroupBatchSelect && b.nb == 0, "batches of %u groups", n1);
            next += b.na;
        }
        CHECK(next == n1 && bs.size() == (n1 + kGroupBatchSelect - 1) / kGroupBatchSelect, "batches of %u groups cover them", n1);
    }
    const uint64_t ebs[2] = {4, 4};
    bool swapped = false;
    const std::vector<GroupBatch> b7 = split_group_batches(7, 0, false, kGroupBatchSelect, 14, &swapped);
    const uint64_t sb7 = select_grouped_slice_bits(b7, 12, 1, true);
    CHECK(select_grouped_from_slices(false, false, true, sb7, 1, 612000000, 612000000, 306000000, ebs, 2), "dense takes the slices");
    CHECK(!select_grouped_from_slices(false, false, true, sb7, 1, 612000000, 612000000, 100, ebs, 2), "sparse takes the column");
}

int main() {
    pass_sequence();
    path_rule();
    std::printf("slice select grouped ok %" PRIu64 " checks\n", checks);
    return 0;
}
