// The filter-program compiler, free of HIP so a CPU program can run it (tests/program_core.cpp): the
// EvalProgram encoding the eval kernels decode, an integer comparison as a range, the walk of a pushed
// filter tree, the expression algebra over bitvector leaves, the emitter that writes an expression as
// a program and picks its form, and the postfix parser. What touches a table or the device: cubit_capi.hip.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/cubit_gpu.h"

namespace cubit {

constexpr int kMaxLeaves = 8;
constexpr int kMaxOps = 16;  // 2 bits each in EvalProgram::ops
// registers of the kernels' postfix stack: a program whose Emitter::max_depth exceeds it is not run
constexpr int kMaxDepth = 4;

enum : uint32_t { OP_AND = 1, OP_OR = 2, OP_ANDNOT = 3 };

// A postfix program whose leaves appear in order 0..n_leaves-1: leaf k is pushed
// (complemented if bit k of `negate`), then nops(k) binary ops are applied. The op counts
// (4 bits per leaf) and opcodes (2 bits per op) are packed into words so the kernel decodes
// them with scalar shifts (a runtime-indexed byte array in the kernel arguments compiles to
// vector loads, each followed by an s_waitcnt vmcnt(0) that drains every outstanding load).
// Evaluation forms: the general postfix interpreter, or a branch-free two-level form chosen
// by the emitter (leaves ordered by group, gstart bit k = leaf k opens a group).
enum : uint32_t { FORM_POSTFIX = 0, FORM_CONJ = 1, FORM_DNF = 2, FORM_CNF = 3 };

struct EvalProgram {
    const uint64_t* leaf[kMaxLeaves];
    uint32_t negate;
    uint32_t n_leaves;
    uint32_t nops;    // 4 bits per leaf
    uint32_t ops;     // 2 bits per op
    uint32_t form;    // FORM_*; FORM_POSTFIX runs the postfix program (is_conjunction upgrades)
    uint32_t gstart;  // FORM_DNF / FORM_CNF group starts
};

inline uint32_t prog_nops(const EvalProgram& p, int k) { return (p.nops >> (4 * k)) & 15u; }

// A left-deep chain of ANDs (nops = 0,1,1,…; every op AND) evaluates as a plain conjunction.
inline bool is_conjunction(const EvalProgram& p) {
    if (p.n_leaves == 0 || prog_nops(p, 0) != 0) return false;
    for (uint32_t k = 1; k < p.n_leaves; ++k)
        if (prog_nops(p, (int)k) != 1 || ((p.ops >> (2 * (k - 1))) & 3u) != OP_AND) return false;
    return true;
}

// the kernel template a program runs (dispatch_k_form, cubit_kernels.hip)
inline uint32_t eval_form(const EvalProgram& p) {
    if (p.form == FORM_DNF || p.form == FORM_CNF || p.form == FORM_CONJ) return p.form;
    return is_conjunction(p) ? FORM_CONJ : FORM_POSTFIX;
}

// A comparison (CUBIT_CMP_* or the between form c <= v < c2) as the inclusive range [lo, hi] of
// passing values, complemented when neg (!=); empty: lo > hi. clamp32 narrows it to INT32 values.
struct CmpRange {
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    int neg = 0;
    bool empty() const { return lo > hi; }
    bool contains(int64_t v) const { return (v >= lo && v <= hi) != (neg != 0); }
    // the values both ranges hold (neither complemented)
    CmpRange intersect(const CmpRange& o) const { return {std::max(lo, o.lo), std::min(hi, o.hi), 0}; }
    void clamp32(int32_t& lo32, int32_t& hi32) const {
        const bool none = lo > hi || lo > INT32_MAX || hi < INT32_MIN;
        lo32 = none ? 1 : (int32_t)std::max<int64_t>(lo, INT32_MIN);
        hi32 = none ? 0 : (int32_t)std::min<int64_t>(hi, INT32_MAX);
    }
};
inline CmpRange cmp_range(int cmp, int64_t constant, int64_t constant2) {
    CmpRange r;
    switch (cmp) {
    case 0: r.lo = r.hi = constant; break;                                            // =
    case 1: r.lo = r.hi = constant; r.neg = 1; break;                                 // !=
    case 2: if (constant == INT64_MIN) { r.lo = 1; r.hi = 0; } else r.hi = constant - 1; break;  // <
    case 3: r.hi = constant; break;                                                   // <=
    case 4: if (constant == INT64_MAX) { r.lo = 1; r.hi = 0; } else r.lo = constant + 1; break;  // >
    case 5: r.lo = constant; break;                                                   // >=
    default:                                                                          // c <= v < c2
        r.lo = constant;
        if (constant2 == INT64_MIN) { r.lo = 1; r.hi = 0; } else r.hi = constant2 - 1;
        break;
    }
    return r;
}

// A comparison against a key constant as a bit-sliced index (CUBIT_INDEX_SLICED) answers it. The
// index holds `bits` slices of u = (uint64)key - (uint64)base, so its valid rows' keys lie in
// [base, base + 2^bits - 1]. cmp is CUBIT_CMP_* (0 … 5, c2 unused) or 6, the half-open c <= v < c2.
// kInterval: the passing keys are those with lo <= u <= hi, or with negate set (!=) the others;
// kFalse / kAllValid: no key of that range passes / every one does. All arithmetic is unsigned:
// k ↦ (uint64)k ^ 2^63 keeps the signed order, so offsets of INT64_MIN / INT64_MAX constants and a
// 64-bit span never overflow.
struct SlicedInterval {
    enum Kind { kFalse, kAllValid, kInterval } kind = kFalse;
    uint64_t lo = 0, hi = 0;
    bool negate = false;
};
// the bit length of top - base (0: one value, 64: INT64_MIN … INT64_MAX)
inline uint32_t sliced_bits(int64_t base, int64_t top) {
    const uint64_t span = (uint64_t)top - (uint64_t)base;
    return span ? 64u - (uint32_t)__builtin_clzll(span) : 0u;
}
inline SlicedInterval sliced_interval(int cmp_or_between, int64_t c, int64_t c2, int64_t base, uint32_t bits) {
    const CmpRange r = cmp_range(cmp_or_between, c, c2);
    const bool neg = r.neg != 0;
    SlicedInterval none, all;
    none.kind = neg ? SlicedInterval::kAllValid : SlicedInterval::kFalse;
    all.kind = neg ? SlicedInterval::kFalse : SlicedInterval::kAllValid;
    if (r.empty() || r.hi < base) return none;
    constexpr uint64_t kBias = 0x8000000000000000ull;
    const uint64_t ub = (uint64_t)base ^ kBias;
    const uint64_t max = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    const uint64_t lo = r.lo <= base ? 0 : ((uint64_t)r.lo ^ kBias) - ub;
    uint64_t hi = ((uint64_t)r.hi ^ kBias) - ub;  // r.hi >= base
    if (lo > max) return none;
    if (hi > max) hi = max;
    if (lo == 0 && hi == max) return all;
    SlicedInterval s;
    s.kind = SlicedInterval::kInterval;
    s.lo = lo;
    s.hi = hi;
    s.negate = neg;
    return s;
}

// ---- aggregates from a bit-sliced index (O'Neil & Quass 1997 §3; Rinfret et al. 2001)
//
// With F the filter's rows, v the column's validity and c_s = popcount(F ∧ v ∧ slice s),
// SUM = count(F ∧ v)·base + Σ_s 2^s·c_s, and MIN / MAX are base plus the smallest / largest offset.
// The combine step below runs on the device (the finishing kernel, cubit_kernels.hip) and on the
// CPU (tests/slice_agg_core.cpp): every operation is unsigned and modular, so base = INT64_MIN with
// 64 slices overflows nothing signed. Type codes as CUBIT_TYPE_*.
#ifdef __HIPCC__
#define CUBIT_HD __host__ __device__
#else
#define CUBIT_HD
#endif

struct U128 {
    uint64_t lo, hi;
};
CUBIT_HD inline U128 u128_add(U128 a, U128 b) {
    const uint64_t lo = a.lo + b.lo;
    return {lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}
// x·2^s mod 2^128, s < 64
CUBIT_HD inline U128 u128_shl(uint64_t x, uint32_t s) { return {x << s, s ? x >> (64 - s) : 0}; }
// a·b as 128 bits, both unsigned
CUBIT_HD inline U128 u128_mul(uint64_t a, uint64_t b) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    return {(uint64_t)p, (uint64_t)(p >> 64)};
}
// Σ_s 2^s·counts[s] over the first n_slices (≤ 64) per-slice counts
CUBIT_HD inline U128 slice_weighted_sum(const uint64_t* counts, uint32_t n_slices) {
    U128 w{0, 0};
    for (uint32_t s = 0; s < n_slices && s < 64; ++s) w = u128_add(w, u128_shl(counts[s], s));
    return w;
}
// a comparison key as cubit_table_column_statistics hands it out (cubit_fp_value, restated so the
// device can call it): FLOAT / DOUBLE keys → bit patterns, UINT64 keys → the value's bits
CUBIT_HD inline int64_t agg_key_value(int type, int64_t key) {
    if (type == CUBIT_TYPE_UINT64) return (int64_t)((uint64_t)key ^ 0x8000000000000000ull);
    if (type == CUBIT_TYPE_FLOAT) return key < 0 ? (int64_t)(0x80000000u | (uint32_t)(0 - (uint64_t)key)) : key;
    if (type == CUBIT_TYPE_DOUBLE) return key < 0 ? (int64_t)(0x8000000000000000ull | (0 - (uint64_t)key)) : key;
    return key;
}
constexpr uint32_t kAggSum = 1u, kAggMin = 2u, kAggMax = 4u;  // CUBIT_AGG_SUM / _MIN / _MAX
// The aggregate's first four result slots {sum_lo, sum_hi, min, max} (slots of ops not asked for: 0).
// `weighted` = Σ_s 2^s·c_s, count_valid = count(F ∧ v), min_off / max_off = the smallest / largest
// offset among those rows (anything when there is none), base = the slices' base key. The values of a
// UINT64 column are (key ^ 2^63) = (base ^ 2^63) + offset, summed unsigned; every other type's value
// is its key, summed signed: count·base in two's complement is the unsigned product less count·2^64
// when base is negative.
CUBIT_HD inline void slice_agg_combine(int type, int64_t base, uint64_t count_valid, U128 weighted, uint64_t min_off,
                                       uint64_t max_off, uint32_t ops, int64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ops & kAggSum) {
        const bool uns = type == CUBIT_TYPE_UINT64;
        const uint64_t b = uns ? (uint64_t)base ^ 0x8000000000000000ull : (uint64_t)base;
        U128 s = u128_mul(count_valid, b);
        if (!uns && base < 0) s.hi -= count_valid;
        s = u128_add(s, weighted);
        out[0] = (int64_t)s.lo;
        out[1] = (int64_t)s.hi;
    }
    if (ops & kAggMin) out[2] = agg_key_value(type, (int64_t)((uint64_t)base + min_off));
    if (ops & kAggMax) out[3] = agg_key_value(type, (int64_t)((uint64_t)base + max_off));
}
// the same from the 64 per-slice counts (counts past the index's slices are 0)
CUBIT_HD inline void slice_agg_combine(int type, int64_t base, uint64_t count_valid, const uint64_t counts[64],
                                       uint64_t min_off, uint64_t max_off, uint32_t ops, int64_t out[4]) {
    slice_agg_combine(type, base, count_valid, slice_weighted_sum(counts, 64), min_off, max_off, ops, out);
}

// The one byte count behind the path rules below: the slices (true) or scan + probe + reduce over
// the column. force_slices / force_column: the caller's FROM_SLICES / FROM_COLUMN flag (it has
// refused both together, and FROM_SLICES without a usable index). Otherwise the path that moves
// fewer bytes:
//   slices: slice_bits/8 bytes per live row — the bits of a row the slice path reads, summed over
//           its launches or passes (each rule below counts its own);
//   column: the scan reads K/8 bytes per live row; per estimated qualifying row the id is written and
//           read (16 bytes), for each probed column the value and its validity are written and read
//           (16 bytes) and the gather moves one 128-byte line, but never more lines than that column
//           has (elem_bytes: the probed columns' element sizes), and the reduction reads column_extra
//           bytes more.
// Every term is a whole number of eighths of a byte, and below 2^53 eighths (a partition of 2^36 rows
// is far inside) the double sums are exact: the order of the terms cannot move a tie.
// Correctness never depends on the choice.
inline bool path_from_slices(bool force_slices, bool force_column, bool usable, uint64_t slice_bits, uint32_t k_leaves,
                             uint64_t live_rows, uint64_t rows, uint64_t est_rows, const uint64_t* elem_bytes,
                             uint32_t n_probed, double column_extra) {
    if (force_column || !usable) return false;
    if (force_slices) return true;
    const double slices = (double)slice_bits / 8.0 * (double)live_rows;
    double column = (double)k_leaves / 8.0 * (double)live_rows + (16.0 + column_extra) * (double)est_rows;
    for (uint32_t i = 0; i < n_probed; ++i)
        column += 16.0 * (double)est_rows + std::min(128.0 * (double)est_rows, (double)elem_bytes[i] * (double)rows);
    return slices <= column;
}

// Which path cubit_table_aggregate takes (path_from_slices, one probed column):
//   slices: every live row reads its bit of the b slices, the K program leaves and, when the column
//           is nullable, its validity: (b + K + nullable)/8 bytes per live row.
// The constants are derived from bytes alone and stay so: at 612 M rows the measured crossover
// (scripts/slice_agg_timing.py, interpolated between its 1e-3 and 2 % points: about 0.9 % of the rows
// for 12 slices, 1.6 % for 24) lies where this rule puts it (0.94 %, 1.9 %), DESIGN.md §3.
inline bool aggregate_from_slices(bool force_slices, bool force_column, bool usable, uint32_t bits, uint32_t k_leaves,
                                  bool nullable, uint64_t live_rows, uint64_t rows, uint64_t est_rows,
                                  uint64_t elem_bytes) {
    return path_from_slices(force_slices, force_column, usable, bits + k_leaves + (nullable ? 1u : 0u), k_leaves, live_rows,
                            rows, est_rows, &elem_bytes, 1, 0.0);
}

// ---- grouped aggregates (cubit_table_aggregate_grouped): GROUP BY one or two columns that carry an
// every-value EQUALITY index, so each group is the AND of one bitvector per group column.
//
// The slots of a group column, ascending: the index's keys, the values its update records carry that
// are no key (an MVCC update may move a row to a value the index has never seen; such a slot has no
// bitvector and can have rows on the column path only), then one NULL slot when the column is
// nullable or a record sets it NULL. Keys are comparison keys (value_key), as Index::keys holds them.
struct GroupSlots {
    std::vector<int64_t> keys;  // the non-NULL slots' keys, ascending and distinct
    std::vector<int32_t> leaf;  // parallel: the key's position in the index (its bitvector), -1 = none
    bool has_null = false;      // the NULL slot, last
    uint32_t size() const { return (uint32_t)keys.size() + (has_null ? 1u : 0u); }
};
// index_keys and update_values: ascending and distinct, each on its own
inline GroupSlots group_slots(const std::vector<int64_t>& index_keys, const std::vector<int64_t>& update_values,
                              bool null_slot) {
    GroupSlots s;
    s.has_null = null_slot;
    size_t i = 0, j = 0;
    while (i < index_keys.size() || j < update_values.size()) {
        if (j == update_values.size() || (i < index_keys.size() && index_keys[i] <= update_values[j])) {
            if (j < update_values.size() && update_values[j] == index_keys[i]) ++j;
            s.keys.push_back(index_keys[i]);
            s.leaf.push_back((int32_t)i++);
        } else {
            s.keys.push_back(update_values[j++]);
            s.leaf.push_back(-1);
        }
    }
    return s;
}
// Group g = i1·n2 + i2 over the slots of the two columns (n2 = 1 with one column).
inline uint32_t group_index(uint32_t i1, uint32_t i2, uint32_t n2) { return i1 * n2 + i2; }
inline void group_tuple(uint32_t g, uint32_t n2, uint32_t* i1, uint32_t* i2) {
    *i1 = g / n2;
    *i2 = g % n2;
}
// n1·n2 when it is at most CUBIT_AGG_MAX_GROUPS, else -1 (n2 = 1 with one column)
inline int64_t group_count(uint32_t n1, uint32_t n2) {
    const uint64_t n = (uint64_t)n1 * n2;
    return n <= CUBIT_AGG_MAX_GROUPS ? (int64_t)n : -1;
}

// One launch of eval_slice_aggregate_grouped takes a rectangle of groups: na leaves of the first
// list from a0 on × nb leaves of the second from b0 on (nb = 0: one group column, nothing loaded for
// a second). The kernel's rectangles are `limit` × 1 for one column and limit/2 × 2 for two, either
// column on the side of 2 (`swapped`: the first list is the second group column's).
constexpr uint32_t kGroupBatchSum = 8;     // groups per launch, SUM and the counts
constexpr uint32_t kGroupBatchMinMax = 4;  // with MIN / MAX (the ripple state is per group)
struct GroupBatch {
    uint32_t a0, na, b0, nb;
};
inline std::vector<GroupBatch> group_batches_of(uint32_t na_all, uint32_t nb_all, bool two, uint32_t limit) {
    std::vector<GroupBatch> out;
    const uint32_t A = two ? limit / 2 : limit, B = two ? 2u : 0u;
    if (!two) {
        for (uint32_t a = 0; a < na_all; a += A) out.push_back({a, std::min(A, na_all - a), 0u, 0u});
        return out;
    }
    for (uint32_t a = 0; a < na_all; a += A)
        for (uint32_t b = 0; b < nb_all; b += B) out.push_back({a, std::min(A, na_all - a), b, std::min(B, nb_all - b)});
    return out;
}
// bytes per row of a set of launches, in eighths: each reads the row's bits (the slices, the program
// leaves, the validity) and its own group leaves
inline uint64_t group_batches_bits(const std::vector<GroupBatch>& bs, uint32_t row_bits) {
    uint64_t bits = 0;
    for (const GroupBatch& b : bs) bits += (uint64_t)row_bits + b.na + b.nb;
    return bits;
}
// The split that reads fewer bytes (n1 / n2: the leaves of the first / second group column, n2 = 0
// with one column; row_bits = b + K + nullable). Every pair of leaves lands in exactly one batch.
inline std::vector<GroupBatch> split_group_batches(uint32_t n1, uint32_t n2, bool two, uint32_t limit, uint32_t row_bits,
                                                   bool* swapped) {
    *swapped = false;
    if (!two) return group_batches_of(n1, 0, false, limit);
    std::vector<GroupBatch> plain = group_batches_of(n1, n2, true, limit);
    std::vector<GroupBatch> swap = group_batches_of(n2, n1, true, limit);
    if (group_batches_bits(swap, row_bits) < group_batches_bits(plain, row_bits)) {
        *swapped = true;
        return swap;
    }
    return plain;
}

// Which path cubit_table_aggregate_grouped takes (path_from_slices; the value column and each group
// column are probed: elem_bytes holds the value column's size, then each group column's):
//   slices: each launch reads (b + K + nullable + its group leaves)/8 bytes per live row:
//           slice_bits = that sum over the launches (group_batches_bits).
// With no group column and one launch without group leaves this is aggregate_from_slices.
inline bool grouped_from_slices(bool force_slices, bool force_column, bool usable, uint64_t slice_bits, uint32_t k_leaves,
                                uint64_t live_rows, uint64_t rows, uint64_t est_rows, const uint64_t* elem_bytes,
                                uint32_t n_probed) {
    return path_from_slices(force_slices, force_column, usable, slice_bits, k_leaves, live_rows, rows, est_rows, elem_bytes,
                            n_probed, 0.0);
}

// ---- sum(a · b) from the bit slices of two columns (cubit_table_sum_product's slice path,
// cubit_bitslice_sum_product; Rinfret et al. 2001)
//
// With ua = a - base_a and ub = b - base_b the offsets the slices hold, A_i / B_j their slices,
// V = F ∧ valid_a ∧ valid_b and n = |V|:
//   Σ a·b  = n·base_a·base_b + base_a·Σub + base_b·Σua + Σ ua·ub
//   Σua    = Σ_i 2^i·popc(V ∧ A_i)   (Σub likewise)
//   Σua·ub = Σ_i Σ_j 2^(i+j)·popc(V ∧ A_i ∧ B_j)
// all modulo 2^128 with the bases sign-extended: the exact two's-complement 128-bit sum for any slice
// counts 0 … 64, INT64_MIN … INT64_MAX included. The kernel keeps a group of up to kProductInner
// slices of the operand with fewer slices (the inner one) masked in registers and streams the other's
// (the outer one's) past them; a wider inner operand takes further groups, each streaming the outer
// slices again.
constexpr uint32_t kProductInner = 8;  // inner slices held in registers per pass over the outer slices

// x·2^s mod 2^128, s < 128
CUBIT_HD inline U128 u128_shl_wide(uint64_t x, uint32_t s) { return s < 64 ? u128_shl(x, s) : U128{0, x << (s - 64)}; }
// x·m mod 2^128, m sign-extended: the unsigned product less x·2^64 when m is negative
CUBIT_HD inline U128 u128_mul_s64(U128 x, int64_t m) {
    U128 p = u128_mul(x.lo, (uint64_t)m);
    p.hi += x.hi * (uint64_t)m;
    if (m < 0) p.hi -= x.lo;
    return p;
}
// {sum_lo, sum_hi} of Σ a·b from cross = Σ ua·ub, sum_ua, sum_ub (each mod 2^128) and n
CUBIT_HD inline void slice_product_combine(int64_t base_a, int64_t base_b, uint64_t n, U128 cross, U128 sum_ua,
                                           U128 sum_ub, int64_t out[2]) {
    U128 s = u128_mul_s64(u128_mul_s64(U128{n, 0}, base_a), base_b);
    s = u128_add(s, u128_mul_s64(sum_ub, base_a));
    s = u128_add(s, u128_mul_s64(sum_ua, base_b));
    s = u128_add(s, cross);
    out[0] = (int64_t)s.lo;
    out[1] = (int64_t)s.hi;
}

// passes over the outer slices: one per group of kProductInner inner slices (one with no inner slice)
inline uint32_t product_passes(uint32_t n_in) { return std::max(1u, (n_in + kProductInner - 1) / kProductInner); }
// the bits of a live row the slice path reads: the K leaves, the validities, each inner slice once and
// the outer slices once per pass
inline uint32_t product_slice_bits(uint32_t n_a, uint32_t n_b, uint32_t k_leaves, bool nullable_a, bool nullable_b) {
    const uint32_t n_in = std::min(n_a, n_b), n_out = std::max(n_a, n_b);
    return k_leaves + (nullable_a ? 1u : 0u) + (nullable_b ? 1u : 0u) + n_in + n_out * product_passes(n_in);
}
// Which path cubit_table_sum_product takes, by bytes alone:
//   slices: product_slice_bits/8 bytes per live row, whatever the filter keeps;
//   column: the fused kernel (eval_sum_product) reads K/8 bytes per live row and per operand one
//           128-byte line per estimated qualifying row, never more than the 8·rows bytes the column
//           has; b decoded from b_decode index leaves costs b_decode/8 bytes per live row instead, and
//           nothing when the filter pins it to one value (b_decode = 0; -1: b is gathered).
// Without a force flag the slices are taken only when usable, in one streaming pass
// (n_in ≤ kProductInner) and their bytes are not more; a wider inner operand runs from slices only
// when forced. Every term is a whole number of eighths of a byte, as path_from_slices'. The constants
// are derived from bytes alone: at 612 M rows, 24 × 4 slices and K = 1 the rule's crossover is 1.37 % of
// the rows, and scripts/slice_product_timing.py measured the column faster at 1 % and the slices
// faster from 10 % up.
inline bool sum_product_from_slices(bool force_slices, bool force_column, bool usable, uint32_t n_a, uint32_t n_b,
                                    uint32_t k_leaves, bool nullable_a, bool nullable_b, uint64_t live_rows, uint64_t rows,
                                    uint64_t est_rows, int b_decode) {
    if (force_column || !usable) return false;
    if (force_slices) return true;
    if (std::min(n_a, n_b) > kProductInner) return false;
    const double slices = (double)product_slice_bits(n_a, n_b, k_leaves, nullable_a, nullable_b) / 8.0 * (double)live_rows;
    const double gather = std::min(128.0 * (double)est_rows, 8.0 * (double)rows);
    double column = (double)k_leaves / 8.0 * (double)live_rows + gather;
    column += b_decode < 0 ? gather : (double)b_decode / 8.0 * (double)live_rows;
    return slices <= column;
}
// Which path cubit_table_sum_product_grouped takes (path_from_slices; both operands and each group
// column are probed: elem_bytes holds a's size, b's, then each group column's):
//   slices: each launch of eval_slice_sum_product_grouped reads product_slice_bits and its own group
//           leaves per live row: slice_bits = that sum over the launches (group_batches_bits).
// The structural condition is the ungrouped rule's: without a force flag, one streaming pass.
constexpr uint32_t kProductGroupBatch = 4;  // groups per launch of the grouped kernel
inline bool sum_product_grouped_from_slices(bool force_slices, bool force_column, bool usable, uint32_t n_a, uint32_t n_b,
                                            uint64_t slice_bits, uint32_t k_leaves, uint64_t live_rows, uint64_t rows,
                                            uint64_t est_rows, const uint64_t* elem_bytes, uint32_t n_probed) {
    if (!force_slices && std::min(n_a, n_b) > kProductInner) return false;
    return path_from_slices(force_slices, force_column, usable, slice_bits, k_leaves, live_rows, rows, est_rows, elem_bytes,
                            n_probed, 0.0);
}

// ---- selection by rank from a bit-sliced index (cubit_table_select; O'Neil & Quass 1997 §3)
//
// A radix select over the offsets u = key - base, most significant slices first. A step histograms
// one chunk of slices over the candidate rows (the filter's non-NULL rows whose higher bits equal the
// prefix chosen so far), walks the buckets to the one that holds the rank still sought, and appends
// that bucket to the prefix. The step logic below runs on the device (select_step_kernel,
// cubit_kernels.hip) and on the CPU (tests/slice_select_core.cpp).
constexpr int kSelectRank = CUBIT_SELECT_RANK, kSelectRankDesc = CUBIT_SELECT_RANK_DESC, kSelectQuantile = CUBIT_SELECT_QUANTILE;
// slices per pass of the slice select (2^d buckets per thread) and bits per pass of the array select
constexpr uint32_t kSelectChunk = 4;
constexpr uint32_t kSelectArrayBits = 8;

// The 0-based ascending rank quantile_disc(col, q) returns among n values, q a double in [0, 1]
// (the reference's Interpolator<true>::Index for a non-DECIMAL q,
// src/include/duckdb/core_functions/aggregate/quantile_sort_tree.hpp:166-188), in the same double
// arithmetic on the device as on the host: the product is rounded before the subtraction (no fused
// multiply-add). n = 0 gives 0, which is no row.
CUBIT_HD inline uint64_t quantile_disc_index(uint64_t n, double q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scaled_q = (double)n * q;
    const uint64_t floored = (uint64_t)floor((double)n - scaled_q);
    const uint64_t left = n - floored;
    return (left > 1 ? left : 1) - 1;
}

// The chunks of a select over `bits` slices, most significant first: the first takes bits mod d
// slices when that is non-zero, so every later chunk is whole. With no slice one pass still runs
// (it counts the rows; its single bucket is the base).
CUBIT_HD inline uint32_t select_passes(uint32_t bits, uint32_t d) { return bits ? (bits + d - 1) / d : 1; }
CUBIT_HD inline uint32_t select_first_chunk(uint32_t bits, uint32_t d) { return bits % d ? bits % d : (bits ? d : 0); }
// the slices of chunk p (0-based): count and lowest slice
CUBIT_HD inline uint32_t select_chunk_bits(uint32_t bits, uint32_t d, uint32_t p) {
    return p == 0 ? select_first_chunk(bits, d) : d;
}
CUBIT_HD inline uint32_t select_chunk_low(uint32_t bits, uint32_t d, uint32_t p) {
    return bits ? bits - select_first_chunk(bits, d) - p * d : 0;
}

// The bucket walk of one radix step. counts: nb bucket counts, bucket i = the rows whose chunk bits
// are i; desc walks them from the top. rank: the 0-based rank still sought among those rows in the
// walk's direction. Finds the bucket that holds it, the rank inside that bucket and the rows the
// step ruled out before it (the buckets walked past). False — nothing written — when rank is at or
// past the total.
CUBIT_HD inline bool select_walk(const uint64_t* counts, uint32_t nb, bool desc, uint64_t rank, uint32_t* bucket,
                                 uint64_t* rank_in, uint64_t* ruled_out) {
    uint64_t before = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t b = desc ? nb - 1 - i : i;
        if (rank - before < counts[b]) {
            *bucket = b;
            *rank_in = rank - before;
            *ruled_out = before;
            return true;
        }
        before += counts[b];
    }
    return false;
}

// The select's device state, carried from step to step on the stream.
struct SelectState {
    uint64_t prefix;       // the offset's bits chosen so far, at their place in the offset
    uint64_t rank;         // the rank still sought inside the prefix's rows
    uint64_t below;        // rows ruled out before the value in the direction asked
    uint64_t equal;        // rows inside the prefix
    uint64_t found;        // 0: no such row (every later step leaves the state alone)
    uint64_t count_valid;  // the filter's non-NULL rows
};
// One step: `first` turns mode / k / q and the first histogram's total into the rank; low = the
// chunk's lowest bit in the offset.
CUBIT_HD inline void select_step(SelectState* s, bool first, int mode, uint64_t k, double q, const uint64_t* counts,
                                 uint32_t nb, uint32_t low) {
    if (first) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < nb; ++i) total += counts[i];
        s->prefix = s->below = s->equal = 0;
        s->count_valid = total;
        s->rank = mode == kSelectQuantile ? quantile_disc_index(total, q) : k;
        s->found = s->rank < total ? 1 : 0;
    }
    if (!s->found) return;
    uint32_t bucket = 0;
    uint64_t rank_in = 0, out = 0;
    if (!select_walk(counts, nb, mode == kSelectRankDesc, s->rank, &bucket, &rank_in, &out)) {
        s->found = 0;  // (the histograms of one select always hold the rank: not reached)
        return;
    }
    s->prefix |= (uint64_t)bucket << low;
    s->rank = rank_in;
    s->below += out;
    s->equal = counts[bucket];
}
// the six result slots {value, found, count_below, count_equal, count_valid, count_rows}: the value
// mapped from the offset as slice_agg_combine maps MIN / MAX
CUBIT_HD inline void select_result(const SelectState& s, int type, int64_t base, uint64_t count_rows, int64_t out[6]) {
    out[0] = s.found ? agg_key_value(type, (int64_t)((uint64_t)base + s.prefix)) : 0;
    out[1] = (int64_t)s.found;
    out[2] = s.found ? (int64_t)s.below : 0;
    out[3] = s.found ? (int64_t)s.equal : 0;
    out[4] = (int64_t)s.count_valid;
    out[5] = (int64_t)count_rows;
}

// Which path cubit_table_select takes (path_from_slices, one probed column):
//   slices: pass 0 reads the K leaves, the validity and its chunk and writes the candidates; each
//           later pass reads and writes the candidates, reads the previous chunk again and the next:
//           (K + nullable + 1 + 2b - d + 2·(passes - 1))/8 bytes per live row, d = the last chunk;
//   column: the aggregate's scan + probe, then 64/kSelectArrayBits passes over the probed values
//           (8 bytes each).
// The constants are derived from bytes alone and marked so: at 612 M rows (scripts/slice_select_timing.py,
// DESIGN.md §3) the rule's crossover is 1.4 % of the rows for 12 slices and 3.1 % for 24, while the
// slices measured faster from 1 % up (and slower at 1e-3): the array passes run well below the memory
// rate the model charges them.
inline bool select_from_slices(bool force_slices, bool force_column, bool usable, uint32_t bits, uint32_t k_leaves,
                               bool nullable, uint64_t live_rows, uint64_t rows, uint64_t est_rows, uint64_t elem_bytes) {
    const uint32_t passes = select_passes(bits, kSelectChunk);
    const uint32_t last = select_chunk_bits(bits, kSelectChunk, passes - 1);
    const uint32_t per_row = k_leaves + (nullable ? 1u : 0u) + 1u + 2u * bits - last + 2u * (passes - 1);
    return path_from_slices(force_slices, force_column, usable, per_row, k_leaves, live_rows, rows, est_rows, &elem_bytes, 1,
                            8.0 * (double)(64 / kSelectArrayBits));
}

// ---- selection by rank per group (cubit_table_select_grouped): the select above over the groups of
// cubit_table_aggregate_grouped. The groups of one call are pairwise disjoint row sets, so one
// candidate bitvector carries the radix selects of a whole batch of groups: a batch runs through all
// its passes (each group narrowed by its own chosen bucket) before the next batch starts.
constexpr uint32_t kGroupBatchSelect = 8;  // groups per launch (the resource table is in DESIGN.md §3)
static_assert(kGroupBatchSelect <= kGroupBatchSum, "GroupAggArgs holds the batch");
// bits per pass of the grouped array select: 2^4 buckets × CUBIT_AGG_MAX_GROUPS groups of 64-bit LDS counters
constexpr uint32_t kSelectGroupArrayBits = 4;
// the bits a live row costs the slice path, summed over the launches: the ungrouped select's, plus
// the launch's group leaves in each of its passes. No batch (no group leaf): one launch without leaves.
inline uint64_t select_grouped_slice_bits(const std::vector<GroupBatch>& bs, uint32_t bits, uint32_t k_leaves,
                                          bool nullable) {
    const uint32_t passes = select_passes(bits, kSelectChunk);
    const uint32_t last = select_chunk_bits(bits, kSelectChunk, passes - 1);
    const uint64_t per_row = k_leaves + (nullable ? 1u : 0u) + 1u + 2u * bits - last + 2u * (passes - 1);
    if (bs.empty()) return per_row;
    uint64_t sum = 0;
    for (const GroupBatch& b : bs) sum += per_row + (uint64_t)(b.na + b.nb) * passes;
    return sum;
}
// Which path cubit_table_select_grouped takes (path_from_slices; the value column and each group
// column are probed: elem_bytes holds the value column's size, then each group column's):
//   slices: slice_bits = select_grouped_slice_bits over the launches;
//   column: the grouped aggregate's scan + probes, then the array passes, each reading the 8-byte
//           probed value of every probed column: 64/kSelectGroupArrayBits passes with a group column,
//           the ungrouped array select's 64/kSelectArrayBits with none.
// The constants are derived from bytes alone and marked so. With no group leaf and one launch this is
// select_from_slices.
inline bool select_grouped_from_slices(bool force_slices, bool force_column, bool usable, uint64_t slice_bits,
                                       uint32_t k_leaves, uint64_t live_rows, uint64_t rows, uint64_t est_rows,
                                       const uint64_t* elem_bytes, uint32_t n_probed) {
    const uint32_t array_passes = 64 / (n_probed > 1 ? kSelectGroupArrayBits : kSelectArrayBits);
    return path_from_slices(force_slices, force_column, usable, slice_bits, k_leaves, live_rows, rows, est_rows, elem_bytes,
                            n_probed, 8.0 * (double)array_passes * (double)n_probed);
}

// One past the last node of the subtree rooted at node i of a prefix-order node array, or -1 when
// the array ends inside it. A negative child count reads as none.
inline int filter_subtree_end(const cubit_filter_node* nodes, uint32_t n_nodes, uint32_t i) {
    int64_t open = 1;  // subtrees begun and not yet walked
    uint32_t j = i;
    for (; open > 0; ++j) {
        if (j >= n_nodes) return -1;
        open += std::max<int32_t>(nodes[j].n_children, 0) - 1;
    }
    return (int)j;
}

// What a node may hold whatever the table: a kind in range, and cmp in 0…5 on a constant filter.
enum class NodeCheck { kOk, kBadKind, kBadCmp };
inline NodeCheck check_filter_node(const cubit_filter_node& f) {
    if (f.kind < CUBIT_FILTER_CONSTANT || f.kind > CUBIT_FILTER_AND) return NodeCheck::kBadKind;
    if (f.kind == CUBIT_FILTER_CONSTANT && (f.cmp < 0 || f.cmp > 5)) return NodeCheck::kBadCmp;
    return NodeCheck::kOk;
}

// Expression over bitvectors. Leaves carry the row predicate they encode so that MVCC
// update patches can recompute a row's bit from its visible value.
struct Leaf {
    const uint64_t* bv = nullptr;
    int column = -1;  // -1: not derived from a column value (visibility, temp)
    // 0 = cmp (v CMP c), 1 = valid (NN), 2 = bin (c <= v < constant2), 3 = a kept combination of
    // the column's bitvectors that is no single interval (a derived leaf; never patched)
    int pred = 0;
    int cmp = 0;
    int64_t constant = 0;
    int64_t constant2 = 0;
    // where its zone classes (zonemaps) come from: kZoneBits = bv is a table-owned index leaf or
    // validity bitvector, classified from its own bits; kZoneStats = bv holds exactly the valid
    // rows whose base value passes (cmp, constant) — a K0 or candidate-check leaf — classified
    // from the column's per-zone min / max like a ConstantFilter's CheckStatistics; kZoneNone
    // = visibility and materialised leaves (mixed everywhere)
    int zsrc = 0;
    // a leaf patched with MVCC updates keeps the classes of the base leaf it was copied from
    // (zbv: that bitvector, for kZoneBits) except in the zones that hold an update record of
    // column zdirty (there: mixed)
    const uint64_t* zbv = nullptr;
    int zdirty = -1;
    // pred 3: the estimated fraction of rows it keeps, from the literals it replaced (< 0: none)
    double sel = -1.0;
};
enum { kZoneNone = 0, kZoneBits = 1, kZoneStats = 2 };

struct Expr;
using ExprP = std::shared_ptr<Expr>;
struct Expr {
    enum Kind { LEAF, AND, OR, ANDNOT, CONST_TRUE, CONST_FALSE } kind = CONST_FALSE;
    Leaf leaf;
    bool neg = false;  // LEAF only
    ExprP a, b;
};

inline ExprP mk_node(Expr::Kind k) {
    auto e = std::make_shared<Expr>();
    e->kind = k;
    return e;
}
inline ExprP mk_true() { return mk_node(Expr::CONST_TRUE); }
inline ExprP mk_false() { return mk_node(Expr::CONST_FALSE); }
inline ExprP mk_leaf(const Leaf& l, bool neg = false) {
    auto e = mk_node(Expr::LEAF);
    e->leaf = l;
    e->neg = neg;
    return e;
}
inline ExprP mk_not(const ExprP& x);
inline ExprP mk_bin(Expr::Kind k, ExprP a, ExprP b) {
    using K = Expr::Kind;
    const bool at = a->kind == K::CONST_TRUE, af = a->kind == K::CONST_FALSE;
    const bool bt = b->kind == K::CONST_TRUE, bf = b->kind == K::CONST_FALSE;
    switch (k) {
    case K::AND:
        if (af || bf) return mk_false();
        if (at) return b;
        if (bt) return a;
        break;
    case K::OR:
        if (at || bt) return mk_true();
        if (af) return b;
        if (bf) return a;
        break;
    case K::ANDNOT:
        if (af || bt) return mk_false();
        if (bf) return a;
        if (at) return mk_not(b);
        break;
    default:
        break;
    }
    auto e = mk_node(k);
    e->a = std::move(a);
    e->b = std::move(b);
    return e;
}
// NOT pushed to the leaves (De Morgan); ANDNOT(a,b) = a & ~b → ~a | b
inline ExprP mk_not(const ExprP& x) {
    using K = Expr::Kind;
    switch (x->kind) {
    case K::CONST_TRUE: return mk_false();
    case K::CONST_FALSE: return mk_true();
    case K::LEAF: return mk_leaf(x->leaf, !x->neg);
    case K::AND: return mk_bin(K::OR, mk_not(x->a), mk_not(x->b));
    case K::OR: return mk_bin(K::AND, mk_not(x->a), mk_not(x->b));
    case K::ANDNOT: return mk_bin(K::OR, mk_not(x->a), x->b);
    }
    return mk_false();
}

inline int count_leaves(const ExprP& e) {
    if (e->kind == Expr::LEAF) return 1;
    if (e->kind == Expr::CONST_TRUE || e->kind == Expr::CONST_FALSE) return 0;
    return count_leaves(e->a) + count_leaves(e->b);
}

// registers the expression needs (Sethi–Ullman / Strahler number)
inline int need(const ExprP& e) {
    if (e->kind == Expr::LEAF) return 1;
    const int l = need(e->a), r = need(e->b);
    return l == r ? l + 1 : std::max(l, r);
}

// top-level conjuncts of e (a & ~leaf contributes the complemented leaf as a conjunct)
inline void conj_parts(const ExprP& e, std::vector<ExprP>& out) {
    if (e->kind == Expr::AND) {
        conj_parts(e->a, out);
        conj_parts(e->b, out);
    } else if (e->kind == Expr::ANDNOT && e->b->kind == Expr::LEAF) {
        conj_parts(e->a, out);
        out.push_back(mk_leaf(e->b->leaf, !e->b->neg));
    } else if (e->kind != Expr::CONST_TRUE) {
        out.push_back(e);
    }
}
inline void leaves_of(const ExprP& e, std::vector<const uint64_t*>& out) {
    if (e->kind == Expr::LEAF) out.push_back(e->leaf.bv);
    else if (e->a) {
        leaves_of(e->a, out);
        if (e->b) leaves_of(e->b, out);
    }
}

// Emit postfix: the heavier child of an AND / OR first (Sethi–Ullman); a & ~b in that order (a heavier
// b that is a leaf would go first, complemented, under an AND). ok: the program holds the expression;
// max_depth: the stack it needs (fits checks both).
struct Emitter {
    EvalProgram prog{};
    int n_ops = 0;
    int depth = 0, max_depth = 0;
    bool ok = true;
    void leaf(const Leaf& l, bool neg) {
        if (prog.n_leaves >= (uint32_t)kMaxLeaves) {
            ok = false;
            return;
        }
        const uint32_t k = prog.n_leaves++;
        prog.leaf[k] = l.bv;
        if (neg) prog.negate |= 1u << k;
        max_depth = std::max(max_depth, ++depth);
    }
    void op(uint32_t o) {
        const uint32_t k = prog.n_leaves - 1;
        if (prog.n_leaves == 0 || n_ops >= kMaxOps || prog_nops(prog, (int)k) == 15) {
            ok = false;
            return;
        }
        prog.ops |= o << (2 * n_ops++);
        prog.nops += 1u << (4 * k);
        --depth;
    }
    // a conjunction of (possibly complemented) leaves: AND nodes, ANDNOT with a leaf on the right
    static bool conj_leaves(const ExprP& e, std::vector<std::pair<Leaf, bool>>& out) {
        switch (e->kind) {
        case Expr::LEAF: out.push_back({e->leaf, e->neg}); return true;
        case Expr::AND: return conj_leaves(e->a, out) && conj_leaves(e->b, out);
        case Expr::ANDNOT:
            if (e->b->kind != Expr::LEAF) return false;
            if (!conj_leaves(e->a, out)) return false;
            out.push_back({e->b->leaf, !e->b->neg});
            return true;
        default: return false;
        }
    }
    using Lits = std::vector<std::pair<Leaf, bool>>;
    static bool or_literals(const ExprP& e, Lits& out) {
        if (e->kind == Expr::LEAF) {
            out.push_back({e->leaf, e->neg});
            return true;
        }
        if (e->kind == Expr::OR) return or_literals(e->a, out) && or_literals(e->b, out);
        return false;
    }
    static void or_parts(const ExprP& e, std::vector<ExprP>& out) {
        if (e->kind == Expr::OR) {
            or_parts(e->a, out);
            or_parts(e->b, out);
        } else {
            out.push_back(e);
        }
    }
    // AND-ed parts; a & ~leaf contributes the complemented leaf as a part of its own
    static bool and_parts(const ExprP& e, std::vector<Lits>& groups) {
        if (e->kind == Expr::AND) return and_parts(e->a, groups) && and_parts(e->b, groups);
        if (e->kind == Expr::ANDNOT) {
            if (e->b->kind != Expr::LEAF) return false;
            if (!and_parts(e->a, groups)) return false;
            groups.push_back({{e->b->leaf, !e->b->neg}});
            return true;
        }
        Lits g;
        if (!or_literals(e, g)) return false;
        groups.push_back(std::move(g));
        return true;
    }
    // two-level program: groups of literals combined by `inner`, groups combined by `outer`;
    // the postfix encoding of the same program is emitted alongside (interpreter fallback)
    bool emit_groups(const std::vector<Lits>& groups, uint32_t inner, uint32_t outer, uint32_t form) {
        size_t total = 0;
        for (const auto& g : groups) total += g.size();
        if (groups.empty() || total > (size_t)kMaxLeaves) return false;
        uint32_t gstart = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            gstart |= 1u << prog.n_leaves;
            for (size_t i = 0; i < groups[gi].size(); ++i) {
                leaf(groups[gi][i].first, groups[gi][i].second);
                if (i) op(inner);
            }
            if (gi) op(outer);
        }
        prog.form = form;
        prog.gstart = gstart;
        return ok;
    }
    // top level: a pure conjunction is emitted as a left-deep AND chain (branch-free CONJ
    // form, is_conjunction above); an OR of conjunctions (DNF) or an AND of ORs of literals
    // (CNF) as a branch-free two-level program; anything else as postfix
    void emit_top(const ExprP& e) {
        Lits c;
        if (e->kind != Expr::LEAF && conj_leaves(e, c)) {
            leaf(c[0].first, c[0].second);
            for (size_t i = 1; i < c.size(); ++i) {
                leaf(c[i].first, c[i].second);
                op(OP_AND);
            }
            return;
        }
        if (e->kind == Expr::OR) {
            std::vector<ExprP> parts;
            or_parts(e, parts);
            std::vector<Lits> groups;
            bool dnf = true;
            for (const auto& p : parts) {
                Lits g;
                if (!conj_leaves(p, g)) {
                    dnf = false;
                    break;
                }
                groups.push_back(std::move(g));
            }
            if (dnf) {
                Emitter trial;
                if (trial.emit_groups(groups, OP_AND, OP_OR, FORM_DNF)) {
                    *this = trial;
                    return;
                }
            }
        }
        if (e->kind == Expr::AND || e->kind == Expr::ANDNOT) {
            std::vector<Lits> groups;
            if (and_parts(e, groups)) {
                Emitter trial;
                if (trial.emit_groups(groups, OP_OR, OP_AND, FORM_CNF)) {
                    *this = trial;
                    return;
                }
            }
        }
        emit(e);
    }
    void emit(const ExprP& e) {
        switch (e->kind) {
        case Expr::LEAF: leaf(e->leaf, e->neg); return;
        case Expr::AND:
        case Expr::OR: {
            const uint32_t o = e->kind == Expr::AND ? OP_AND : OP_OR;
            if (need(e->b) > need(e->a)) {
                emit(e->b);
                emit(e->a);
            } else {
                emit(e->a);
                emit(e->b);
            }
            op(o);
            return;
        }
        case Expr::ANDNOT: {
            if (need(e->b) > need(e->a) && e->b->kind == Expr::LEAF) {
                // a & ~b == (~b) & a with b a leaf: emit complemented leaf first
                leaf(e->b->leaf, !e->b->neg);
                emit(e->a);
                op(OP_AND);
            } else {
                emit(e->a);
                emit(e->b);
                op(OP_ANDNOT);
            }
            return;
        }
        default: ok = false; return;
        }
    }
};

// one kernel pass evaluates e: its program holds it and the kernels' stack is deep enough
inline bool fits(const ExprP& e) {
    Emitter em;
    em.emit_top(e);
    return em.ok && em.max_depth <= kMaxDepth;
}

// A caller's postfix program (cubit_bitvector_eval: an entry >= 0 pushes that leaf, a CUBIT_OP_*
// pops two values and pushes one) as an expression, or the first check it fails.
struct PostfixParse {
    enum Error { kNone, kLeafRange, kUnderflow, kBadOpcode, kEmpty, kLeftOver } error;
    ExprP expr;     // kNone
    uint32_t at;    // kLeafRange, kUnderflow, kBadOpcode: the failing entry's index …
    int32_t value;  // … and the entry
    size_t left;    // kEmpty, kLeftOver: the values the program leaves on the stack
};
inline PostfixParse parse_postfix(const uint64_t* const* leaves, uint32_t n_leaves, uint32_t leaf_negate,
                                  const int32_t* prog, uint32_t n_prog) {
    using P = PostfixParse;
    std::vector<ExprP> st;
    for (uint32_t i = 0; i < n_prog; ++i) {
        const int32_t x = prog[i];
        if (x >= 0) {
            if ((uint32_t)x >= n_leaves) return {P::kLeafRange, nullptr, i, x, 0};
            Leaf l;
            l.bv = leaves[x];
            st.push_back(mk_leaf(l, x < 32 && ((leaf_negate >> x) & 1u) != 0));
        } else {
            if (st.size() < 2) return {P::kUnderflow, nullptr, i, x, 0};
            if (x != CUBIT_OP_AND && x != CUBIT_OP_OR && x != CUBIT_OP_ANDNOT) return {P::kBadOpcode, nullptr, i, x, 0};
            const ExprP b = st.back(), a = st[st.size() - 2];
            st.resize(st.size() - 2);
            st.push_back(mk_bin(x == CUBIT_OP_AND ? Expr::AND : x == CUBIT_OP_OR ? Expr::OR : Expr::ANDNOT, a, b));
        }
    }
    if (st.size() != 1) return {st.empty() ? P::kEmpty : P::kLeftOver, nullptr, 0, 0, st.size()};
    return {P::kNone, st[0], 0, 0, 0};
}

}  // namespace cubit
