// Internal interfaces shared by the HIP kernels (cubit_kernels.hip) and the C ABI /
// planner (cubit_capi.hip). Not installed; the public surface is include/cubit_gpu.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cubit_program.hpp"
#include "cubit_row_list.hpp"
#include "cubit_segments.hpp"

namespace cubit {

// DuckDB storage geometry (src/include/duckdb/common/vector_size.hpp:16-20,
// src/include/duckdb/storage/storage_info.hpp:20). Both are whole 64-bit words, so vector
// and row-group boundaries never split a bitvector word.
constexpr uint64_t kVectorSize = 2048;
constexpr uint64_t kRowGroupSize = 122880;
static_assert(kVectorSize % 64 == 0 && kVectorSize / 64 == 32, "vector must be 32 words");
static_assert(kRowGroupSize % 64 == 0 && kRowGroupSize / 64 == 1920, "row group must be 1920 words");

// Filter kernel geometry: 256-thread workgroups; each thread owns PAIRS 16-byte word pairs
// per leaf (one dwordx4 load per pair; a wave-instruction moves 1 KiB). Bitvectors are padded
// to kPadWords so every tile shape reads in bounds.
constexpr int kThreads = 256;
constexpr uint64_t kPadWords = 16384;  // 1,048,576 rows
// kMaxLeaves, EvalProgram and the evaluation forms: cubit_program.hpp

// Column value types as the kernels see them: INT32 / INT64 values, or FLOAT / DOUBLE bit patterns
// (4 / 8 bytes) compared through their order key (cubit_fp_key, include/cubit_gpu.h: NaN one key
// above +inf, -x → -pattern(x), so -0.0 == +0.0 — DuckDB's floating-point operators,
// comparison_operators.hpp:100-146). Type codes as in cubit_gpu.h.
// VARCHAR columns hold int32 codes of an order-preserving dictionary (cubit_dict): compared as
// INT32 values, the codes order as the strings do.
// UBIGINT (UINT64) columns hold the unsigned values' bits, compared through the key v ^ 2^63 (the
// unsigned order as a signed one).
constexpr int kTypeInt32 = 0, kTypeInt64 = 1, kTypeUInt64 = 7, kTypeFloat = 8, kTypeDouble = 9, kTypeVarchar = 10;
__host__ __device__ __forceinline__ bool type_is32(int type) {
    return type == kTypeInt32 || type == kTypeFloat || type == kTypeVarchar;
}
__host__ __device__ __forceinline__ bool type_is_fp(int type) { return type == kTypeFloat || type == kTypeDouble; }
// the type a table's compare kernels see for a column: FLOAT / DOUBLE columns keep their keys as an
// INT32 / INT64 column beside the patterns
__host__ __device__ __forceinline__ int key_type(int type) {
    return type == kTypeFloat ? kTypeInt32 : type == kTypeDouble ? kTypeInt64 : type;
}
// values compared through a key other than themselves (FLOAT, DOUBLE, UBIGINT)
__host__ __device__ __forceinline__ bool type_is_keyed(int type) { return type_is_fp(type) || type == kTypeUInt64; }
__host__ __device__ __forceinline__ int32_t fp_key32(uint32_t u) {
    const uint32_t mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u) return 0x7fc00000;
    return (u >> 31) ? -(int32_t)mag : (int32_t)mag;
}
__host__ __device__ __forceinline__ int64_t fp_key64(uint64_t u) {
    const uint64_t mag = u & 0x7fffffffffffffffull;
    if (mag > 0x7ff0000000000000ull) return (int64_t)0x7ff8000000000000ull;
    return (u >> 63) ? -(int64_t)mag : (int64_t)mag;
}
// the comparison key of a value as the ABI carries it (FLOAT: the zero-extended 32-bit pattern)
__host__ __device__ __forceinline__ int64_t value_key(int type, int64_t v) {
    if (type == kTypeFloat) return fp_key32((uint32_t)v);
    if (type == kTypeDouble) return fp_key64((uint64_t)v);
    if (type == kTypeUInt64) return (int64_t)((uint64_t)v ^ 0x8000000000000000ull);
    return v;
}
// kernels templated on the key kind FK (0: the value itself, 1: FLOAT pattern, 2: DOUBLE pattern,
// 3: UBIGINT bits)
template <int FK, typename T>
__host__ __device__ __forceinline__ T key_of(T raw) {
    if constexpr (FK == 1) return (T)fp_key32((uint32_t)raw);
    else if constexpr (FK == 2) return (T)fp_key64((uint64_t)raw);
    else if constexpr (FK == 3) return (T)((uint64_t)raw ^ 0x8000000000000000ull);
    else return raw;
}

inline uint64_t padded_words(uint64_t n_rows) {
    const uint64_t w = (n_rows + 63) / 64;
    return ((w + kPadWords - 1) / kPadWords) * kPadWords;
}

struct EvalArgs {
    EvalProgram prog;
    uint64_t n_rows;
    uint64_t n_words;  // ceil(n_rows / 64)
    int64_t row_base;
    int64_t* rowids;
    uint64_t capacity;
    uint64_t* count;         // result: the number of qualifying rows (written at kernel end)
    uint64_t* result_words;  // optional evaluated bitvector
    uint32_t num_tiles;
    // claim ticket (context-owned, kTicketWords words, zero between launches): running claim
    // counter + arrival counters. The last workgroup to finish publishes *count and re-zeroes
    // the ticket, so no memset launch precedes a scan (finish_ticket, cubit_kernels.hip).
    uint64_t* ticket;
    // zonemap skip (device, ascending): the tiles to evaluate, num_tiles entries; null = every
    // tile 0 … num_tiles-1. The planner leaves out the tiles whose zone classes prove the program
    // false on every row (RowGroup::CheckZonemap, row_group.cpp:361-371, over bitvector zones).
    const uint32_t* live;
    // eval_decode_lookback: context-owned flag words (kLookbackMaxTiles, zeroed once) and the
    // launch's epoch (> 0, one per launch on the context), which tags every flag it publishes
    uint64_t* flags;
    uint64_t epoch;
    // polls of one flag before the polling thread counts that tile itself (0 = the kernel's
    // default; cubit_ctx_set_lookback_spins forces the recount path in tests)
    uint32_t spin_limit;
    // eval_decode_lookback: exclusive prefix of every tile's qualifying rows, known before the
    // launch (a program of one index bitvector: its per-zone counts, a zone being one decode
    // tile), or null. With it no workgroup publishes or waits, at any tile count.
    const uint64_t* tile_prefix;
    // the prefixed decode's side output (both or neither; cubit_row_list.hpp): the low 16 bits of
    // every qualifying row's tile-local offset at list_off[tile_prefix[tile] + i], whatever the
    // capacity, and the tile's rows below 65,536 at list_lo[tile]
    uint16_t* list_off;
    uint32_t* list_lo;
};
// decode_row_list_kernel: a bitvector's row list (cubit_row_list.hpp) into what the prefixed decode
// of the bitvector writes
struct RowListArgs {
    const uint64_t* prefix;  // tiles + 1 entries
    const uint16_t* off;
    const uint32_t* lo_cnt;
    uint32_t tiles;
    int64_t row_base;
    int64_t* rowids;
    uint64_t capacity;
    uint64_t* count;
};
// eval_decode_lookback: one workgroup per tile, at most this many tiles per launch (6.0e8 rows).
// Every workgroup reads the counts of all earlier tiles, so the flag reads grow with the square
// of the tile count: at 4,578 tiles (SF100) the kernel takes 68.5 µs against 64.7 µs for the
// run-claimed decode; larger launches are not measured, so ordered scans past this size keep the
// run-claimed decode + ordering pass.
constexpr uint32_t kLookbackMaxTiles = 4608;
// Zonemaps: one zone = one decode tile (2,048 words = 131,072 rows). Class byte per zone:
// bit 0 = no row of the zone is set, bit 1 = every row of the zone is set (a zone past the
// last row has both).
constexpr uint64_t kZoneWords = 2048;
constexpr uint64_t kZoneRows = kZoneWords * 64;
constexpr uint32_t kTicketStride = 64;  // words (512 B) between ticket counters
constexpr uint32_t kTicketGroups = 8;
constexpr uint32_t kTicketWords = kTicketStride * (kTicketGroups + 2);

// launchers (cubit_kernels.hip); all asynchronous on `stream`
// what a tile-walking launch used (cubit_ctx_last_grid): the workgroups of its persistent grid and
// the tiles they walked between them. The slice launchers fill `shape` (optional) from the grid they
// launch, for a select from pass 0's
struct LaunchShape {
    uint32_t workgroups = 0;
    uint32_t tiles = 0;
};
uint64_t decode_tile_words();  // words per eval_decode_tiles tile
uint64_t count_tile_words(uint32_t n_leaves);  // words per eval_count_kernel tile
int decode_block_threads();
// evaluate + decode into per-tile runs; dir (optional) gets {start, length} per tile
// ev0 / ev1 (optional): events stamped by the kernel dispatch itself (hipExtLaunchKernel), so
// their elapsed time is the kernel's execution, as rocprofv3's kernel trace reports it
// kernel: 0 = by the measured policy (launch_decode_kf), 1 = pair-claimed, 2 = run-claimed,
// 3 = look-back (one tile per workgroup, runs in tile order: small partitions by policy —
// lookback_max_tiles — and ordered scans up to kLookbackMaxTiles); decode_kernel_for resolves
// it for a launch
int decode_kernel_for(uint32_t n_leaves, uint32_t num_tiles, unsigned grid, int kernel, bool live = false,
                      int n_cus = 256, bool prefixed = false);
// the largest tile count the measured policy decodes with the look-back kernel (grid = tiles)
uint32_t lookback_max_tiles(uint32_t n_leaves, int n_cus);
hipError_t launch_eval_decode(const EvalArgs& a, uint64_t* dir, unsigned grid, hipStream_t stream,
                              hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int kernel = 0, int n_cus = 256);
// row ids, tile directory and count from a row list: one workgroup per tile, no bitvector read
hipError_t launch_decode_row_list(const RowListArgs& a, uint64_t* dir, hipStream_t stream, hipEvent_t ev0 = nullptr,
                                  hipEvent_t ev1 = nullptr);
// zone classes of a bitvector (class byte per zone, see kZoneWords) for zones [z0, z0 + nz),
// and (cnt non-null) each zone's set rows
hipError_t launch_zone_classes(const uint64_t* bv, uint64_t n_rows, uint32_t z0, uint32_t nz, uint8_t* out,
                               hipStream_t stream, uint32_t* cnt = nullptr);
// per-zone min / max of a raw column's valid rows; fl bit 0 = some row valid, bit 1 = every row
hipError_t launch_column_zone_stats(const void* col, int type, const uint64_t* validity, uint64_t n_rows, uint32_t nz,
                                    int64_t* mn, int64_t* mx, uint8_t* fl, hipStream_t stream);
// evaluate + count (and/or write the result bitvector)
hipError_t launch_eval_count(const EvalArgs& a, hipStream_t stream, hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr);
// lay per-tile runs out in row order: dst[dst_off[i] ...] = src[dir run i]
hipError_t launch_order_runs(const uint64_t* dir, uint32_t n_tiles, uint64_t* dst_off, const int64_t* src,
                             uint64_t capacity, int64_t* dst, hipStream_t stream);
// cmp = CUBIT_CMP_* (0..5) or kCmpBetween (constant <= v < constant2)
constexpr int kCmpBetween = 6;
hipError_t launch_compare_bitvector(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int cmp,
                                    int64_t constant, uint64_t* out_words, hipStream_t stream, int64_t constant2 = 0);
// candidate check of a constant inside one bin [k_lo, k_hi) of a range index: cand =
// hi_bv \ lo_bv (lo_bv null = ∅, hi_bv null = every valid row); out = (cmp LT: lo_bv ∪)
// {r ∈ cand : v[r] cmp constant}; cmp ∈ {CUBIT_CMP_EQ, CUBIT_CMP_LT}
hipError_t launch_candidate_check(const void* col, int type, const uint64_t* validity, const uint64_t* lo_bv,
                                  const uint64_t* hi_bv, uint64_t n_rows, int cmp, int64_t constant,
                                  uint64_t* out_words, hipStream_t stream);
// selection narrowing: out = mask ∩ valid ∩ {v cmp constant}, the column read at mask rows only
hipError_t launch_masked_compare(const void* col, int type, const uint64_t* validity, const uint64_t* mask,
                                 uint64_t n_rows, int cmp, int64_t constant, uint64_t* out, hipStream_t stream);
// K0 over several keys in one pass of the column (index build): out[k] = cmp(v, c[k], c2[k]),
// cmp ∈ {EQ, LT, between}
constexpr int kMultiKeys = 16;
struct MultiKeyArgs {
    int64_t c[kMultiKeys];
    int64_t c2[kMultiKeys];
    uint64_t* out[kMultiKeys];
    uint32_t m;
};
hipError_t launch_compare_bitvectors(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int cmp,
                                     const MultiKeyArgs& a, hipStream_t stream);
// Bit-sliced index (CUBIT_INDEX_SLICED): slice s holds bit s of u = (uint64)key - (uint64)base of
// every valid row (NULL rows and padding 0); each slice is padded_words(n_rows) words.
constexpr uint32_t kMaxSlices = 64;
struct SliceSet {
    uint64_t* s[kMaxSlices];  // least significant first
};
// the column → its n_slices slices, one pass of the column per kMultiKeys slices (every word of
// every slice written). ev0 / ev1 (optional) are stamped by the first / last dispatch.
hipError_t launch_bitslice_build(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t base,
                                 uint32_t n_slices, const SliceSet& out, hipStream_t stream, hipEvent_t ev0 = nullptr,
                                 hipEvent_t ev1 = nullptr);
// out = valid ∧ (lo <= u <= hi), complemented under valid when negate; validity null = every row
// below n_rows (read only below ceil(n_rows / 64) words; 16-byte aligned, as are the slices and out)
hipError_t launch_bitslice_compare(const SliceSet& slices, uint32_t n_slices, const uint64_t* validity, uint64_t n_rows,
                                   uint64_t lo, uint64_t hi, int negate, uint64_t* out, hipStream_t stream,
                                   hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// Aggregates of a column over a program's rows, read from the column's slices (fused evaluate +
// aggregate, eval_slice_aggregate) or reduced from probed values (aggregate_arrays_kernel). Either
// kernel leaves kAggPartial int64 per workgroup in `partials` — {Σ lo, Σ hi, smallest offset, largest
// offset, valid rows} — and one finishing wave combines them on the device (slice_agg_combine,
// cubit_program.hpp) into out[0..5] = {sum_lo, sum_hi, min, max, count_valid, count_rows}, so the
// result is ready on the stream with no host round trip, in exact integers whatever the grid and
// the arrival order. The workspace holds kAggWorkspace int64: the partials of up to kAggMaxGrid
// workgroups, then the qualifying-row count the kernels publish (agg_count_slot).
constexpr int kAggPartial = 5;
constexpr unsigned kAggMaxGrid = 1024;
constexpr uint64_t kAggWorkspace = (uint64_t)kAggPartial * kAggMaxGrid + 2;
__host__ __device__ inline uint64_t* agg_count_slot(int64_t* workspace) {
    return reinterpret_cast<uint64_t*>(workspace + (uint64_t)kAggPartial * kAggMaxGrid);
}
struct SliceAggArgs {
    SliceSet slices;
    uint32_t n_slices;
    // the aggregated column's validity: null = every row valid; read only below ceil(n_rows / 64)
    // words (16-byte aligned, as the slices are)
    const uint64_t* validity;
    int64_t* workspace;
};
// words per tile of eval_slice_aggregate: one zone
constexpr uint64_t kAggTileWords = 2048;
// a.prog may hold no leaf (n_leaves = 0: every row below n_rows qualifies); a.count is set by the
// launcher; a.num_tiles tiles of kAggTileWords words (a.live: the zones to evaluate); ops =
// CUBIT_AGG_SUM | _MIN | _MAX; type / base: the column's type and the slices' base key
hipError_t launch_eval_slice_aggregate(EvalArgs a, const SliceAggArgs& g, uint32_t ops, int type, int64_t base,
                                       int n_cus, LaunchShape* shape,
                                       int64_t* out, hipStream_t stream, hipEvent_t ev0 = nullptr,
                                       hipEvent_t ev1 = nullptr);
// the same result from x[i] (the probed values as the ABI carries them, 0 at NULL rows) and valid
// (bit i, null = all valid), i < min(*d_count, max_n)
hipError_t launch_aggregate_arrays(const int64_t* x, const uint64_t* valid, const uint64_t* d_count, uint64_t max_n,
                                   uint32_t ops, int type, int64_t* workspace, int64_t* out, hipStream_t stream);
// Σ a·b over a program's rows from the slices of both columns (eval_slice_sum_product). `outer` is
// the operand with at least as many slices as `inner` (the sum is symmetric, so either column may be
// either). The kernel leaves kProductPartial int64 per workgroup in the aggregate workspace —
// {cross lo, hi, Σ outer offsets lo, hi, Σ inner offsets lo, hi, valid rows} — and one finishing wave
// combines them (slice_product_combine, cubit_program.hpp) into out[0..1] = {sum_lo, sum_hi}, with
// out_slots = 4 also out[2..3] = {count_valid, count_rows}; count_out (optional) gets count_rows too.
constexpr int kProductPartial = 7;
constexpr unsigned kProductMaxGrid = (unsigned)((uint64_t)kAggPartial * kAggMaxGrid / kProductPartial);
struct SliceProductArgs {
    SliceSet outer, inner;
    uint32_t n_outer, n_inner;
    // the operands' validities: null = every row valid; read only below ceil(n_rows / 64) words
    const uint64_t* valid_a;
    const uint64_t* valid_b;
    int64_t* workspace;  // kAggWorkspace int64
};
// a as launch_eval_slice_aggregate's (a.count is set by the launcher)
hipError_t launch_eval_slice_sum_product(EvalArgs a, const SliceProductArgs& g, int64_t base_outer, int64_t base_inner,
                                         int n_cus, LaunchShape* shape,
                                         int64_t* out, int out_slots, uint64_t* count_out, hipStream_t stream,
                                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// Selection by rank (cubit_table_select): a radix select over the column's slices (eval_slice_select,
// slice_select_narrow: kSelectChunk slices per pass) or over probed values (select_arrays_kernel:
// kSelectArrayBits bits per pass), one workgroup after each pass summing and walking the histogram
// (select_step_kernel; the step logic is cubit_program.hpp's). The workspace (kSelectWorkspace int64,
// allocated on the context by the first select) holds the workgroups' partial histograms — up to
// kAggMaxGrid × 2^kSelectChunk or kSelectArrayGrid × 2^kSelectArrayBits counters — then the device
// state and the qualifying-row count. out[0..5] = {value, found, count_below, count_equal,
// count_valid, count_rows}, ready on the stream with no host round trip.
constexpr unsigned kSelectArrayGrid = 256;
constexpr uint64_t kSelectPartials = (uint64_t)kSelectArrayGrid << kSelectArrayBits;
static_assert(((uint64_t)kAggMaxGrid << kSelectChunk) <= kSelectPartials, "the slice path's partials fit");
constexpr uint64_t kSelectWorkspace = kSelectPartials + sizeof(SelectState) / sizeof(int64_t) + 2;
__host__ __device__ inline SelectState* select_state(int64_t* workspace) {
    return reinterpret_cast<SelectState*>(workspace + kSelectPartials);
}
__host__ __device__ inline uint64_t* select_count_slot(int64_t* workspace) {
    return reinterpret_cast<uint64_t*>(workspace + kSelectPartials + sizeof(SelectState) / sizeof(int64_t));
}
struct SliceSelectArgs {
    SliceSet slices;
    uint32_t n_slices;
    const uint64_t* validity;  // as SliceAggArgs'
    // the candidate bitvector: padded_words(n_rows) words of scratch, 16-byte aligned; the evaluated
    // tiles' words are written by pass 0 and narrowed in place by the later passes
    uint64_t* cand;
    int64_t* workspace;
};
// a as launch_eval_slice_aggregate's (a.count is set by the launcher); mode / k / q: CUBIT_SELECT_*, the
// rank, the quantile; *n_passes (optional) = the passes over the slices
hipError_t launch_slice_select(EvalArgs a, const SliceSelectArgs& g, int mode, uint64_t k, double q, int type,
                               int64_t base, int n_cus, LaunchShape* shape,
                               int64_t* out, hipStream_t stream, uint32_t* n_passes = nullptr,
                               hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the same result from x[i] / valid as launch_aggregate_arrays takes them
hipError_t launch_select_arrays(const int64_t* x, const uint64_t* valid, const uint64_t* d_count, uint64_t max_n,
                                int mode, uint64_t k, double q, int type, int64_t* workspace, int64_t* out,
                                hipStream_t stream, uint32_t* n_passes = nullptr);
// out[0 … na + nb) = the ascending merge of two ascending runs of distinct row ids (cubit_table_top_n);
// *count = na + nb
hipError_t launch_merge_ids(const int64_t* a, uint64_t na, const int64_t* b, uint64_t nb, int64_t* out, uint64_t* count,
                            hipStream_t stream);
// The grouped forms (cubit_table_aggregate_grouped). Either kernel leaves kGroupPartial int64 per
// group and workgroup in `partials`, group-major ([slot][workgroup]) — {Σ lo, Σ hi, smallest offset,
// largest offset, valid rows, rows} — and one finishing wave per group combines them as above
// (six zeros for a group without a row). The workspace (kGroupWorkspace int64, allocated on the
// context when the first grouped call needs it) holds the column path's CUBIT_AGG_MAX_GROUPS groups ×
// kGroupColGrid workgroups; the slice path's kGroupBatchSum slots × kAggMaxGrid workgroups fit in it.
constexpr int kGroupPartial = 6;
constexpr unsigned kGroupColGrid = 512;
constexpr uint64_t kGroupWorkspace = (uint64_t)kGroupPartial * CUBIT_AGG_MAX_GROUPS * kGroupColGrid;
static_assert((uint64_t)kGroupPartial * kGroupBatchSum * kAggMaxGrid <= kGroupWorkspace, "the slice path's partials fit");
constexpr uint32_t kNoGroup = 0xffffffffu;
// One launch's rectangle of groups: slot j = a (one group column, n2 = 0) or 2·a + b (two), its
// rows F ∧ v ∧ e1[a] ∧ e2[b]. A leaf with its neg bit set is a group column's validity, complemented
// in the kernel (the NULL slot); it is read only below ceil(n_rows / 64) words, as every leaf is.
struct GroupAggArgs {
    const uint64_t* e1[kGroupBatchSum];
    const uint64_t* e2[2];
    uint32_t n1, n2;
    uint32_t neg1, neg2;
    uint32_t group[kGroupBatchSum];  // the group each slot's result goes to (kNoGroup: none)
    int64_t* partials;
};
// a as launch_eval_slice_aggregate's (a.count and a.ticket are not used: each group's rows are
// counted in its partials); g.workspace is not used. q.n1 ≤ kGroupBatchSum (kGroupBatchMinMax when
// ops holds MIN or MAX) with one group column, half that with two. out: the whole result, 6 int64
// per group.
hipError_t launch_eval_slice_aggregate_grouped(const EvalArgs& a, const SliceAggArgs& g, const GroupAggArgs& q,
                                               uint32_t ops, int type, int64_t base, int n_cus, LaunchShape* shape,
                                               int64_t* out,
                                               hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// The column path's reduction per group: x / xvalid as launch_aggregate_arrays', and per group column
// its probed values, their validity words, its type, the ascending keys of its non-NULL slots
// (device) and its NULL slot (-1: none). A row whose group value is in no slot counts nowhere.
struct GroupColArgs {
    const int64_t* v[2];
    const uint64_t* valid[2];
    const int64_t* keys[2];
    uint32_t n_keys[2];
    int32_t null_slot[2];
    int type[2];
    uint32_t n_cols;
    uint32_t n2;  // slots of the second column (1 with one column)
};
hipError_t launch_aggregate_arrays_grouped(const int64_t* x, const uint64_t* valid, const GroupColArgs& gc,
                                           uint32_t n_groups, const uint64_t* d_count, uint64_t max_n, uint32_t ops,
                                           int type, int64_t* partials, int64_t* out, hipStream_t stream);
// Σ a·b per group (cubit_table_sum_product_grouped). Either kernel leaves kProductGroupPartial int64
// per group and workgroup in `partials`, group-major — the ungrouped seven words, then the rows — and
// one finishing wave per group writes out[4·group …] = {sum_lo, sum_hi, count_valid, count_rows}.
// The slice kernel takes q as launch_eval_slice_aggregate_grouped does, q.n1 ≤ kProductGroupBatch with
// one group column, half that with two; the grouped workspace (kGroupWorkspace) holds both paths'.
constexpr int kProductGroupPartial = 8;
static_assert((uint64_t)kProductGroupPartial * kProductGroupBatch * kAggMaxGrid <= kGroupWorkspace, "the slice path's partials fit");
constexpr unsigned kProductColGrid = (unsigned)(kGroupWorkspace / ((uint64_t)kProductGroupPartial * CUBIT_AGG_MAX_GROUPS));
hipError_t launch_eval_slice_sum_product_grouped(const EvalArgs& a, const SliceProductArgs& g, const GroupAggArgs& q,
                                                 int64_t base_outer, int64_t base_inner, int n_cus, LaunchShape* shape,
                                                 int64_t* out,
                                                 hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the column path's reduction: xa / xb the probed operands (0 at NULL rows) with their validity words
// (null: all valid), gc as launch_aggregate_arrays_grouped's
hipError_t launch_sum_product_arrays_grouped(const int64_t* xa, const uint64_t* va, const int64_t* xb, const uint64_t* vb,
                                             const GroupColArgs& gc, uint32_t n_groups, const uint64_t* d_count,
                                             uint64_t max_n, int64_t* partials, int64_t* out, hipStream_t stream);
// Selection by rank per group (cubit_table_select_grouped). The slice path runs a batch of up to
// kGroupBatchSelect groups through all its passes over one candidate bitvector
// (eval_slice_select_grouped, then slice_select_narrow_grouped per later chunk); the column path runs
// every group at once over the probed values (select_arrays_grouped_kernel, kSelectGroupArrayBits bits
// per pass). Either leaves, per workgroup and slot, kSelectSlotCols counters — the chunk's 2^4 buckets,
// then the slot's rows (pass 0 only) — workgroup-major with a stride of n_slots · kSelectSlotCols, and
// one workgroup after each pass (select_step_grouped_kernel) sums them and applies select_step to each
// slot's SelectState. The workspace (kSelectGroupWorkspace int64, allocated on the context when the
// first grouped select needs it): the partials, then CUBIT_AGG_MAX_GROUPS states, then as many
// count_rows slots. out + 6·group = the six slots of launch_slice_select.
static_assert(kSelectGroupArrayBits == kSelectChunk, "both paths' passes have the same buckets per slot");
constexpr uint32_t kSelectSlotCols = (1u << kSelectChunk) + 1;
constexpr uint64_t kSelectGroupSlotBlocks = (uint64_t)kAggMaxGrid * kGroupBatchSelect;  // slots × workgroups
constexpr uint64_t kSelectGroupPartials = kSelectGroupSlotBlocks * kSelectSlotCols;
constexpr unsigned kSelectGroupColGrid = 256;  // the column path's grid at most, and no more than fits:
__host__ __device__ inline unsigned select_group_col_grid(uint32_t n_groups) {
    const unsigned fit = (unsigned)(kSelectGroupSlotBlocks / (n_groups ? n_groups : 1));
    return fit < kSelectGroupColGrid ? fit : kSelectGroupColGrid;
}
static_assert((uint64_t)kAggMaxGrid * kGroupBatchSelect * kSelectSlotCols <= kSelectGroupPartials, "the slice path's partials fit");
static_assert(kSelectGroupSlotBlocks / CUBIT_AGG_MAX_GROUPS >= 1, "the column path's partials fit at any group count");
constexpr uint64_t kSelectStateWords = sizeof(SelectState) / sizeof(int64_t);
static_assert(sizeof(SelectState) % sizeof(int64_t) == 0, "a state is whole words");
constexpr uint64_t kSelectGroupWorkspace =
    kSelectGroupPartials + (uint64_t)CUBIT_AGG_MAX_GROUPS * kSelectStateWords + CUBIT_AGG_MAX_GROUPS;
static_assert(kGroupBatchSelect <= CUBIT_AGG_MAX_GROUPS, "a batch's states and count_rows slots fit");
__host__ __device__ inline SelectState* select_group_state(int64_t* workspace, uint32_t slot) {
    return reinterpret_cast<SelectState*>(workspace + kSelectGroupPartials) + slot;
}
__host__ __device__ inline uint64_t* select_group_rows(int64_t* workspace, uint32_t slot) {
    return reinterpret_cast<uint64_t*>(workspace + kSelectGroupPartials + (uint64_t)CUBIT_AGG_MAX_GROUPS * kSelectStateWords) +
           slot;
}
// a / g as launch_slice_select's (no ticket: each group's rows are counted in its partials); q as
// launch_eval_slice_aggregate_grouped's with q.n1 ≤ kGroupBatchSelect (half that with two group
// columns; q.partials is not used). The same k / q for every group.
hipError_t launch_slice_select_grouped(const EvalArgs& a, const SliceSelectArgs& g, const GroupAggArgs& q, int mode,
                                       uint64_t k, double quantile, int type, int64_t base,
                                       int n_cus, LaunchShape* shape, int64_t* out,
                                       hipStream_t stream, uint32_t* n_passes = nullptr, hipEvent_t ev0 = nullptr,
                                       hipEvent_t ev1 = nullptr);
// the same result for every group from x / valid and gc as launch_aggregate_arrays_grouped takes them
hipError_t launch_select_arrays_grouped(const int64_t* x, const uint64_t* valid, const GroupColArgs& gc, uint32_t n_groups,
                                        const uint64_t* d_count, uint64_t max_n, int mode, uint64_t k, double quantile,
                                        int type, int64_t* workspace, int64_t* out, hipStream_t stream,
                                        uint32_t* n_passes = nullptr);
// after a merge: every 64-row word holding one of the m merged rows (ascending) sliced again from
// the column as it stands
hipError_t launch_bitslice_reslice(const int64_t* rows, uint64_t m, const void* col, int type, const uint64_t* validity,
                                   uint64_t n_rows, int64_t base, uint32_t n_slices, const SliceSet& slices,
                                   hipStream_t stream);
// index-build statistics (out3 = {min, max, valid count}, pre-set by the caller) and the
// presence bitmap of the valid values (bit v - vmin, `range` bits, zeroed by the caller)
hipError_t launch_column_minmax(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t* out3,
                                hipStream_t stream);
hipError_t launch_presence(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t vmin,
                           uint64_t range, uint64_t* bits, hipStream_t stream);
// Quantile edges (index build): one pass of a multi-target radix select over the normalised key
// u = (uint64)(key - vmin), which has `bits` significant bits. Pass 0 (consumed = 0) counts the top
// d bits of u over every valid row into counts[0 … 2^d). A later pass is given the active prefixes
// (n_active distinct values of u >> (bits - consumed), ascending, on the device) and counts the
// next d bits of the rows under prefix i into counts[i·2^d … (i + 1)·2^d); every other row is
// ignored. The counters are 64-bit, zeroed by the caller. A workgroup counts in LDS (32-bit
// counters, kQuantileCounters of them, beside the prefix table) and adds its non-zero counters to
// `counts` once at its end, so the caller picks d with n_active · 2^d ≤ kQuantileCounters
// (quantile_pass_bits); pass 0 counts kQuantileD0 bits (fewer when u has fewer).
constexpr uint32_t kQuantileCounters = 16384;  // 64 KiB of LDS
constexpr uint32_t kQuantileD0 = 12;
constexpr uint32_t kQuantileMaxActive = 1023;  // n_bins ≤ 1,024
struct QuantileHistArgs {
    int64_t vmin;
    uint32_t bits;      // 0 … 64
    uint32_t consumed;  // bits the earlier passes resolved: 0, or ≥ kQuantileD0
    uint32_t d;         // bits this pass counts: consumed + d ≤ bits (pass 0 of a single-valued column: 0)
    uint32_t n_active;  // pass > 0: 1 … kQuantileMaxActive
    const uint64_t* prefixes;
    uint64_t* counts;
};
// the bits a pass after the first counts: the most that keep every active prefix's counters in LDS
inline uint32_t quantile_pass_bits(uint32_t n_active, uint32_t bits_left) {
    uint32_t d = 0;
    while (d < bits_left && ((uint64_t)n_active << (d + 1)) <= kQuantileCounters) ++d;
    return d;
}
// grid: four (pass 0) or two workgroups per CU, grid-strided. ev0 / ev1 (optional) are stamped by the dispatch, as
// for launch_eval_decode. wave_agg: a wave whose rows share one counter adds once (the kept form;
// false is the plain form scripts/quantile_timing.py times it against).
hipError_t launch_quantile_hist(const void* col, int type, const uint64_t* validity, uint64_t n_rows,
                                const QuantileHistArgs& a, int n_cus, hipStream_t stream, hipEvent_t ev0 = nullptr,
                                hipEvent_t ev1 = nullptr, bool wave_agg = true);
// K5: DuckDB BITPACKING groups (BpGroup, cubit_segments.hpp) → plain values
hipError_t launch_bitunpack(const uint8_t* bytes, const BpGroup* groups, uint64_t n_groups, int type, void* out,
                            hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// strings → codes of a sorted dictionary, all on the device (NULL rows 0; a missing string -1,
// counted into *missing)
hipError_t launch_dict_encode(const uint8_t* bytes, const uint64_t* offs, uint64_t n, const uint64_t* validity,
                              const uint8_t* dbytes, const uint64_t* doffs, uint64_t dn, int32_t* codes,
                              unsigned long long* missing, hipStream_t stream);
// DuckDB RLE segments parsed into runs (values of the column's type, cumulative exclusive run
// ends) expanded into the column (type 0: INT32, else INT64); tile_first: scratch of
// (n_rows + 2047) / 2048 + 1 words
hipError_t launch_rle_expand(const void* vals, const uint64_t* ends, uint64_t n_runs, uint64_t n_rows, int type,
                             uint64_t* tile_first, void* out, hipStream_t stream, hipEvent_t start, hipEvent_t stop);
// K5 + K0 fused: {valid rows whose value cmp constant} straight from the BITPACKING groups
// (cmp = CUBIT_CMP_* or kCmpBetween); out must be zero (words shared by two groups are OR-ed)
// simple_width > 0: every group is FOR of ≤ 32 bits, CONSTANT or CONSTANT_DELTA, and the widest
// FOR group has ≤ simple_width bits (bitpacked_compare_waves); 0: the LDS kernel
hipError_t launch_bitpacked_compare(const uint8_t* bytes, const BpGroup* groups, uint64_t n_groups, int type,
                                    const uint64_t* validity, int cmp, int64_t constant, int64_t constant2,
                                    uint64_t* out, hipStream_t stream, int simple_width = 0);
// out[i] = (int32)(in[i] - offset), i < min(*d_count, max_n) (transfer compaction of a column)
// out[i] = (unsigned width-byte)(in[i] - offset), width 1 / 2 / 4; *overflow = 1 when a value
// falls outside [offset, offset + 2^(8·width))
hipError_t launch_narrow_unsigned(const int64_t* in, const uint64_t* d_count, uint64_t max_n, int64_t offset, int width,
                                  void* out, uint32_t* overflow, hipStream_t stream);
// a narrower / unsigned column (CUBIT_TYPE_INT8 … UINT64) widened to its INT32 / INT64 storage
hipError_t launch_widen(const void* in, int src_type, uint64_t n, void* out, hipStream_t stream);
hipError_t launch_narrow_i32(const int64_t* in, const uint64_t* d_count, uint64_t max_n, int64_t offset, int32_t* out,
                             hipStream_t stream, uint32_t* overflow = nullptr);
// FLOAT / DOUBLE columns: keys[i] = the comparison key of pattern raw[i] (the column the compare
// kernels read); out[i] = value_key(type, v[i]); raw[rows[i]] = v[i] (0 where valids[i] = 0)
hipError_t launch_fp_keys(const void* raw, int type, uint64_t n, void* keys, hipStream_t stream);
hipError_t launch_value_keys(const int64_t* v, uint64_t n, int type, int64_t* out, hipStream_t stream);
hipError_t launch_scatter_raw(const int64_t* rows, const int64_t* v, const uint8_t* valids, uint64_t m, int type,
                              void* raw, hipStream_t stream);
hipError_t launch_gather(const void* col, int type, const int64_t* rowids, const uint64_t* d_count, uint64_t max_n,
                         int64_t row_base, int64_t* out, hipStream_t stream);
// the probe with NULL-ness: values (0 at NULL rows) and out_valid bit i = row rowids[i] valid
// (⌈min(*d_count, max_n) / 64⌉ words written; validity nullptr = every row valid)
hipError_t launch_gather_valid(const void* col, int type, const uint64_t* validity, const int64_t* rowids,
                               const uint64_t* d_count, uint64_t max_n, int64_t row_base, int64_t* out,
                               uint64_t* out_valid, hipStream_t stream);
hipError_t launch_gather_sum_product(const int64_t* a, const int64_t* b, const int64_t* rowids,
                                     const uint64_t* d_count, uint64_t max_n, int64_t row_base, int64_t* partials,
                                     int64_t* out, hipStream_t stream);
constexpr int kSumBlocks = 1024;  // partials buffer holds 2 * kSumBlocks int64

// Fused filter + probe + reduce: sum(a[r] * b[r]) over the qualifying rows r (K1+K3).
// b = nullptr: b is decoded from its range index, b = v0 + Σ_j delta[j]·[r ∉ dleaf[j]]
// (dleaf[j] = L(v_j), the filter pins b to v0 < v1 < … ≤ kMaxDecode+1 values).
constexpr int kMaxDecode = 3;
struct SumArgs {
    const int64_t* a;
    const uint64_t* a_valid;  // optional
    const int64_t* b;         // nullptr → decode
    const uint64_t* b_valid;  // optional (gather mode)
    const uint64_t* dleaf[kMaxDecode];
    int64_t delta[kMaxDecode];
    int64_t v0;
    uint32_t n_decode;
    int64_t* partials;  // 2 int64 (lo, hi) per workgroup
    // a read from its DuckDB BITPACKING segments instead of the plain column (null = plain):
    // the packed bytes, the group records (BpGroup, row order) and per 2,048-row vector the
    // index of the group holding its first row. CONSTANT / CONSTANT_DELTA / FOR groups are
    // random-accessible (value i = base (+ aux·i | + its w bits at bit i·w)); a row of a
    // DELTA_FOR group is read from a_plain (the unpacked column), as its value needs the prefix
    // of its group.
    const uint8_t* a_bytes;
    const BpGroup* a_groups;
    const uint32_t* a_vgroup;
    const int64_t* a_plain;
    uint64_t a_n_groups;
};
// grid = persistent workgroups; partials must hold 2·grid int64; out = {lo, hi}
hipError_t launch_eval_sum_product(const EvalArgs& a, const SumArgs& s, unsigned grid, int64_t* out, hipStream_t stream);
unsigned sum_product_grid(unsigned n_cus);
// sum over i < *d_count of x[i]·y[i] (MVCC fallback of the fused path)
hipError_t launch_sum_product_arrays(const int64_t* x, const int64_t* y, const uint64_t* d_count, uint64_t max_n,
                                     int64_t* partials, int64_t* out, hipStream_t stream);

// MVCC (K4)
// visibility: words = valid-row mask, then clear rows whose delete is visible to txn
hipError_t launch_visibility(const int64_t* del_rows, const uint64_t* del_ids, uint64_t n_del, uint64_t n_rows,
                             uint64_t start_time, uint64_t transaction_id, uint64_t* words, hipStream_t stream,
                             const int64_t* hidden_ranges = nullptr, uint32_t n_hidden = 0);
// mark rows with an update visible to txn into `mask` (atomicOr)
hipError_t launch_update_mask(const int64_t* upd_rows, const uint64_t* upd_versions, uint64_t n_upd,
                              uint64_t start_time, uint64_t transaction_id, uint64_t* mask, hipStream_t stream);
hipError_t launch_fill_valid(uint64_t* words, uint64_t n_rows, hipStream_t stream);

// Index maintenance. Append: splice n_bits bits of src (bit 0 = first appended row) into dst
// at bit offset bit_off (dst words outside the splice untouched). Merge: base values of the
// merged rows replaced (rows become valid) and the bits of every index bitvector whose
// predicate changes for a row flipped. encoding: 0 range L(k) = {v < k}, 1 equality, 2 bins
// (keys = edges, n_keys - 1 bitvectors); bvs = nullptr: no index.
struct MergeIndex {
    const int64_t* keys;  // device, sorted
    uint64_t* const* bvs; // device array of bitvector pointers
    uint32_t n_keys;
    int32_t encoding;
};
hipError_t launch_splice_bits(uint64_t* dst, const uint64_t* src, uint64_t bit_off, uint64_t n_bits,
                              hipStream_t stream);
// merge by 64-row words: the m merged records' rows ascend, each row once; valids: per record
// 1 = the value, 0 = NULL (nullptr: every row valid; a NULL needs `validity`)
hipError_t launch_merge_words(const int64_t* rows, const int64_t* values, const uint8_t* valids, uint64_t m,
                              uint64_t n_rows, void* col, int type, uint64_t* validity, MergeIndex ix0, MergeIndex ix1,
                              hipStream_t stream);
// Column sync: changed[w] = the rows of word w whose NULL-ness differs between the old and the new
// column, or that are valid on both sides with different stored bits (`type` gives the element
// size only; FLOAT / DOUBLE callers pass the pattern column). changed holds padded_words(n_rows)
// words, all written (0 past the rows); the changed rows are added into *counter (zeroed by the
// caller). The validities may be null (all valid) and are read only below ceil(n_rows / 64) words.
// ev0 / ev1 (optional) are stamped by the dispatch, as for launch_eval_decode.
hipError_t launch_column_diff(const void* old_col, const uint64_t* old_valid, const void* new_col,
                              const uint64_t* new_valid, int type, uint64_t n_rows, uint64_t* changed,
                              uint64_t* counter, hipStream_t stream, hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr);
// the records of m changed rows (ascending local ids) as launch_merge_words takes them: values[i] =
// the new column at rows[i] (INT32 / codes sign-extended, FLOAT zero-extended, 0 for NULL), valids[i]
hipError_t launch_sync_gather(const void* new_col, const uint64_t* new_valid, int type, const int64_t* rows, uint64_t m,
                              int64_t* values, uint8_t* valids, hipStream_t stream);
}  // namespace cubit
