/*
 * cubit_gpu.h — C ABI of the MI355X bitmap-indexed table-scan filter (libcubitgpu.so).
 *
 * The reference (DuckDB v1.1.2, /root/reference) has no C ABI for this path: its drop-in
 * boundary is the C++ `TableFunction` callback struct
 * (src/include/duckdb/function/table_function.hpp:184-301) whose `seq_scan` implementation
 * (src/function/table/table_scan.cpp:119-146, 405-442) drives
 * RowGroup::TemplatedScan (src/storage/table/row_group.cpp:447-604). The entry points below
 * are what a C++ DuckDB extension calls from its replacement table
 * function; each cites the reference function whose work it takes over.
 *
 * Conventions: every call returns an int status (CUBIT_OK = 0), never
 * throws across the ABI, and records a message readable with cubit_last_error() (thread
 * local). Output buffers are caller-owned device buffers. A context owns one HIP stream
 * (cubit_ctx_set_stream), a claim ticket and a tile directory; every call on a context or on
 * its tables holds the context's mutex, so DuckDB's pipeline threads may share it (calls
 * serialise; GPU work stays asynchronous on the stream). Once cubit_ctx_create has returned, the
 * library issues every kernel, copy and memset on the context's stream (or on a copy stream made
 * from it) and nothing on the null stream, so a context bound to a hipStreamNonBlocking stream
 * orders its work behind whatever the caller has pending there. Results named "last" belong to the
 * context's most recent call: threads that need their own give themselves a context each.
 * Row ids are int64 (DuckDB ROW_TYPE). Bitvectors are LSB-first 64-bit words, the layout
 * of DuckDB's ValidityMask (src/include/duckdb/common/types/validity_mask.hpp:22,164-168).
 */
#ifndef CUBIT_GPU_H
#define CUBIT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes */
#define CUBIT_OK 0
#define CUBIT_ERR_INVALID 1      /* bad argument */
#define CUBIT_ERR_HIP 2          /* HIP runtime error */
#define CUBIT_ERR_OOM 3          /* device allocation failed */
#define CUBIT_ERR_UNSUPPORTED 4  /* predicate shape / type not supported */
#define CUBIT_ERR_CAPACITY 5     /* output buffer too small (count still reported) */
#define CUBIT_ERR_DEVICE 6       /* device-side failure (stream event creation, …) */

/* ---- physical types (DuckDB PhysicalType subset on the path: DATE = INT32,
 *      DECIMAL(15,2) = INT64, BIGINT = INT64, INTEGER = INT32). A column holds INT32 or INT64
 *      values; the narrower and unsigned codes name the T of BITPACKING segments
 *      (cubit_table_add_bitpacked_column; bitpacking.cpp:953-977 GetFunction: BOOL and INT8
 *      as int8_t, …, UINT64 and LIST offsets as uint64_t), unpacked into an INT32 column
 *      (INT8, INT16, UINT8, UINT16) or an INT64 column (UINT32). A UINT64 (UBIGINT) column
 *      holds the unsigned values' 64 bits and compares them unsigned, through the key
 *      v ^ 2^63 (cubit_fp_key): its constants, keys, update values, statistics and probed values
 *      are those bits in an int64. */
#define CUBIT_TYPE_INT32 0
#define CUBIT_TYPE_INT64 1
#define CUBIT_TYPE_INT8 2
#define CUBIT_TYPE_INT16 3
#define CUBIT_TYPE_UINT8 4
#define CUBIT_TYPE_UINT16 5
#define CUBIT_TYPE_UINT32 6
#define CUBIT_TYPE_UINT64 7
/* FLOAT / DOUBLE (PhysicalType::FLOAT / DOUBLE): the column holds the IEEE bit patterns as DuckDB's
 * vectors do, and every value crossing the ABI — filter constants, index keys, update values,
 * statistics, probed values — is a bit pattern carried in an int64 (FLOAT: the 32-bit pattern,
 * zero-extended). Comparisons follow DuckDB's floating-point operators
 * (src/common/vector_operations/comparison_operators.cpp:17-88, src/include/duckdb/common/
 * operator/comparison_operators.hpp:100-146): NaN equals NaN and is greater than every other value,
 * -0.0 equals +0.0. The library compares through cubit_fp_key below, an order-preserving map of the
 * patterns onto signed integers under which those operators are plain integer comparisons. */
#define CUBIT_TYPE_FLOAT 8
#define CUBIT_TYPE_DOUBLE 9
/* VARCHAR (PhysicalType::VARCHAR, string_t): the column holds int32 codes of an order-preserving
 * dictionary (cubit_dict: the distinct strings sorted as DuckDB compares them —
 * src/include/duckdb/common/types/string_type.hpp:143-206: the bytes as unsigned, then the length),
 * so a code comparison is the string comparison and every index, zonemap and kernel works on the
 * codes. A CONSTANT filter node on a VARCHAR column carries the ADDRESS of a cubit_string in
 * `constant` (the planner maps it to a code bound; strings absent from the dictionary included);
 * index keys (cubit_table_build_index `values`) likewise. Update values, appended values, probed
 * values and statistics are codes. */
#define CUBIT_TYPE_VARCHAR 10
/* HUGEINT / UHUGEINT (PhysicalType::INT128 / UINT128: hugeint_t / uhugeint_t, {lower, upper}) have
 * no column storage of their own: such a column is a dictionary column (cubit_table_add_dict_column)
 * over its values' 16-byte ORDER KEYS (cubit_key128: the 128 bits big-endian, HUGEINT's sign bit
 * flipped), whose unsigned byte order — the dictionary's order — is the values' order (hugeint_t's
 * and uhugeint_t's comparison operators). Its codes are the values' ranks, so every index, zonemap
 * and kernel works on them as on a VARCHAR column's; filter constants and index keys cross as
 * cubit_strings over their keys, probed codes map back through cubit_dict_entry + cubit_value128.
 * The type codes name the key encoding only (a column of more than 2^31 - 1 distinct values does
 * not fit the INT32 codes and stays on the caller's CPU path). */
#define CUBIT_TYPE_INT128 11
#define CUBIT_TYPE_UINT128 12
static inline void cubit_key128(int type, uint64_t lower, uint64_t upper, unsigned char key[16]) {
    if (type == CUBIT_TYPE_INT128) upper ^= 0x8000000000000000ull; /* signed order as unsigned bytes */
    for (int i = 0; i < 8; i++) {
        key[i] = (unsigned char)(upper >> (56 - 8 * i));
        key[8 + i] = (unsigned char)(lower >> (56 - 8 * i));
    }
}
static inline void cubit_value128(int type, const unsigned char key[16], uint64_t *lower, uint64_t *upper) {
    uint64_t hi = 0, lo = 0;
    for (int i = 0; i < 8; i++) {
        hi = (hi << 8) | key[i];
        lo = (lo << 8) | key[8 + i];
    }
    *lower = lo;
    *upper = type == CUBIT_TYPE_INT128 ? hi ^ 0x8000000000000000ull : hi;
}

/* The comparison key of a FLOAT / DOUBLE bit pattern or UINT64 value (any other type: the value
 * itself): UINT64 → v ^ 2^63; FLOAT / DOUBLE: every
 * NaN → one key above +inf's, -x → -(pattern of x) (so -0.0 and +0.0 share key 0), +x → its pattern.
 * cubit_fp_value is its inverse on keys (a NaN key → the positive quiet NaN, key 0 → +0.0). */
static inline int64_t cubit_fp_key(int type, int64_t bits) {
    if (type == CUBIT_TYPE_UINT64) return (int64_t)((uint64_t)bits ^ 0x8000000000000000ull);  /* unsigned order */
    if (type == CUBIT_TYPE_FLOAT) {
        const uint32_t u = (uint32_t)bits, mag = u & 0x7fffffffu;
        if (mag > 0x7f800000u) return 0x7fc00000;
        return (u >> 31) ? -(int64_t)mag : (int64_t)mag;
    }
    if (type == CUBIT_TYPE_DOUBLE) {
        const uint64_t u = (uint64_t)bits, mag = u & 0x7fffffffffffffffull;
        if (mag > 0x7ff0000000000000ull) return (int64_t)0x7ff8000000000000ull;
        return (u >> 63) ? -(int64_t)mag : (int64_t)mag;
    }
    return bits;
}
static inline int64_t cubit_fp_value(int type, int64_t key) {
    if (type == CUBIT_TYPE_UINT64) return (int64_t)((uint64_t)key ^ 0x8000000000000000ull);
    if (type == CUBIT_TYPE_FLOAT) return key < 0 ? (int64_t)(0x80000000u | (uint32_t)(-key)) : key;
    if (type == CUBIT_TYPE_DOUBLE) return key < 0 ? (int64_t)(0x8000000000000000ull | (uint64_t)(-key)) : key;
    return key;
}

/* ---- comparison (ExpressionType COMPARE_* used by ConstantFilter,
 *      src/planner/filter/constant_filter.cpp) */
#define CUBIT_CMP_EQ 0
#define CUBIT_CMP_NE 1
#define CUBIT_CMP_LT 2
#define CUBIT_CMP_LE 3
#define CUBIT_CMP_GT 4
#define CUBIT_CMP_GE 5

/* ---- filter node kinds: mirror TableFilterType (src/include/duckdb/planner/table_filter.hpp:20-27) */
#define CUBIT_FILTER_CONSTANT 0    /* ConstantFilter(cmp, constant) on `column` */
#define CUBIT_FILTER_IS_NULL 1
#define CUBIT_FILTER_IS_NOT_NULL 2
#define CUBIT_FILTER_OR 3          /* ConjunctionOrFilter, n_children follow (prefix order) */
#define CUBIT_FILTER_AND 4         /* ConjunctionAndFilter */

/* ---- bitmap index encodings */
#define CUBIT_INDEX_RANGE 0     /* L_j = {valid rows with v < edge_j}; exact for constants on edges */
#define CUBIT_INDEX_EQUALITY 1  /* E_k = {rows with v == value_k} (CUBIT's equality encoding) */
#define CUBIT_INDEX_BINS 2      /* B_i = {valid rows with edge_i <= v < edge_i+1}: kept beside a range or
                                   equality index on the same column; a range whose bounds are bin
                                   edges reads its bins instead of two range bitvectors when fewer */
/* A bit-sliced index (O'Neil & Quass, SIGMOD 1997; Rinfret, O'Neil & O'Neil, SIGMOD 2001): a secondary
 * index kept beside a column's RANGE / EQUALITY index and its BINS index. With k_r the comparison
 * key of row r (cubit_fp_key of the stored value; a dictionary column's code), base / top the
 * smallest / largest key over the valid rows and b the bit length of (uint64)top - (uint64)base (0
 * when one value is present, 64 for INT64_MIN ... INT64_MAX): slice s (0 <= s < b) is a table-owned
 * bitvector whose bit r = valid(r) && ((((uint64)k_r - (uint64)base) >> s) & 1). NULL rows are 0 in
 * every slice, padding is 0; a column with no valid row, or an empty partition, gets an empty index
 * with no slices. Any comparison with a constant is a ripple of AND / OR / ANDNOT over the slices'
 * 64-row words from the top slice down, exact for every constant: it answers what would otherwise be
 * a whole-column K0 pass, reading b/8 bytes per row. Memory: b * n_rows / 8 bytes. */
#define CUBIT_INDEX_SLICED 3

/* ---- bitvector program opcodes (operands >= 0 are leaf indices, postfix order) */
#define CUBIT_OP_AND (-1)
#define CUBIT_OP_OR (-2)
#define CUBIT_OP_ANDNOT (-3) /* a AND NOT b */

/* ---- scan flags
 * Default output order ("tile runs"): the row ids of each 131,072-row tile form one
 * ascending run, and runs appear in the order tiles finished — the shape of DuckDB's
 * parallel table scan, whose morsels reach the sink in nondeterministic order with a batch
 * index (src/function/table/table_scan.cpp:179-189). cubit_ctx_last_tiles() returns the
 * tile directory ({start, length} per tile) that restores row order for free.
 * CUBIT_SCAN_ORDERED lays the runs out ascending: the look-back decode places each tile's run at
 * the sum of the earlier tiles' counts, so no extra pass (partitions up to 4,608 tiles = 6.0e8
 * rows; larger ones take one extra device pass). The small partitions that AUTO decodes with the
 * look-back kernel are ascending without the flag, too.
 * Capacity: *d_count is always the full number of qualifying rows. When it exceeds
 * `capacity` the calls still return CUBIT_OK (they do not wait for the kernel) and the
 * buffer holds an unspecified subset of the ids (runs are claimed in nondeterministic order;
 * with CUBIT_SCAN_ORDERED the ordered array has holes) — compare *d_count with capacity, or
 * pass CUBIT_SCAN_CHECK_CAPACITY, which waits for the scan and returns CUBIT_ERR_CAPACITY. */
#define CUBIT_SCAN_COUNT_ONLY 1u     /* do not materialise row ids */
#define CUBIT_SCAN_ORDERED 2u        /* one globally ascending array */
#define CUBIT_SCAN_CHECK_CAPACITY 4u /* synchronise; CUBIT_ERR_CAPACITY when *d_count > capacity */
/* Zonemaps (RowGroup::CheckZonemap / CheckZonemapSegments, src/storage/table/row_group.cpp:361-371,
 * 407-445): every index and validity bitvector carries, per zone of 131,072 rows, whether no row
 * or every row of the zone is set. A scan evaluates its filter over these classes (three-valued
 * logic) and skips the zones where it is false on every row — as the reference skips row groups
 * whose min/max statistics fail a filter. Results are identical either way; this flag turns the
 * skip off. */
#define CUBIT_SCAN_NO_ZONEMAP 8u

typedef struct cubit_ctx cubit_ctx;
typedef struct cubit_table cubit_table;
typedef struct cubit_dict cubit_dict;

/* a string constant or key of a VARCHAR column (string_t's data and size) */
typedef struct {
    const char *data;
    uint64_t size;
} cubit_string;

/* One node of a predicate tree in prefix order. A TableFilterSet (per-column AND,
 * table_filter.hpp:67-101) is an AND root whose children each reference one column; a
 * cross-column OR tree (the residual PhysicalFilter, execute_conjunction.cpp:56-142) uses
 * the same nodes. */
typedef struct {
    int32_t kind;       /* CUBIT_FILTER_* */
    int32_t cmp;        /* CUBIT_CMP_* (CONSTANT only) */
    int32_t column;     /* table column index (leaf kinds) */
    int32_t n_children; /* AND / OR */
    int64_t constant;   /* CONSTANT: value in the column's physical representation */
} cubit_filter_node;

/* DuckDB TransactionData{start_time, transaction_id} (src/include/duckdb/transaction/transaction_data.hpp) */
typedef struct {
    uint64_t start_time;
    uint64_t transaction_id;
} cubit_txn;

/* ------------------------------------------------------------------ context */
/* devices visible to the process (one context per device for a table held as partitions) */
int cubit_device_count(int *n);
int cubit_ctx_create(int device, cubit_ctx **out);
int cubit_ctx_destroy(cubit_ctx *ctx);
/* stream is a hipStream_t (NULL = the null stream). */
int cubit_ctx_set_stream(cubit_ctx *ctx, void *stream);
const char *cubit_last_error(void);
/* Which evaluate + decode kernel the context's scans launch: AUTO (the measured policy: the
 * look-back kernel — one workgroup per 131,072-row tile, output offsets by look-back over the
 * earlier tiles' counts — when the partition's tiles fit the co-resident grid; else the
 * run-claimed kernel when a workgroup walks three or more tiles, else the pair-claimed one),
 * or one of them always (tests and benchmarks; LOOKBACK up to 4,608 tiles). Results are
 * identical. Under AUTO a CUBIT_SCAN_ORDERED scan takes the look-back kernel at any size up to
 * 4,608 tiles (its runs land in tile order). */
#define CUBIT_DECODE_AUTO 0
#define CUBIT_DECODE_PAIRS 1
#define CUBIT_DECODE_RUNS 2
#define CUBIT_DECODE_LOOKBACK 3
/* reported by cubit_ctx_last_decode_kernel only: a program of one index bitvector as it stands
 * decodes with its offsets known up front (the bitvector's per-zone counts, kept with its zone
 * map): the look-back kernel without its walk, at any tile count; taken under AUTO and LOOKBACK */
#define CUBIT_DECODE_PREFIXED 4
int cubit_ctx_set_decode_kernel(cubit_ctx *ctx, int kernel);
/* Look-back decode: polls of an earlier tile's flag before the polling thread counts that tile
 * from its bitvectors itself (0 = the library default, 2^22). The expiry path is part of every
 * launch — no workgroup waits without bound and the count is always exact — and a small limit
 * forces it (tests). */
int cubit_ctx_set_lookback_spins(cubit_ctx *ctx, uint32_t spins);
/* The compute units the context's launchers size their persistent grids by: 0 = the device's own
 * count (the default), 1 … the device's count = that many; anything else is CUBIT_ERR_INVALID. The
 * setting only ever lowers a count, so a grid only shrinks and the look-back kernel is admitted to
 * no more tiles than before. With a small count a table of a few tiles runs the loops of a table of
 * hundreds — several tiles per workgroup, uneven shares (tests). Results are identical under any
 * setting. cubit_ctx_compute_units reads the device's count and the one in use. */
int cubit_ctx_set_compute_units(cubit_ctx *ctx, int n);
int cubit_ctx_compute_units(cubit_ctx *ctx, int *device, int *in_use);
/* The workgroups the context's last tile-walking launch used and the tiles they walked between them
 * (the live tiles, under a zonemap skip), as its launcher set them: the slice-answered aggregates,
 * selects (the first pass) and sums of products, the fused filter+SUM, and the decode. Zeros before
 * the first such launch; a call answered without a launch leaves the earlier values. */
int cubit_ctx_last_grid(cubit_ctx *ctx, uint32_t *workgroups, uint32_t *tiles);
/* The kernel the context's last decode launched (CUBIT_DECODE_PAIRS, _RUNS, _LOOKBACK or _PREFIXED; 0 when
 * the partition had no row and nothing was launched). */
int cubit_ctx_last_decode_kernel(cubit_ctx *ctx, int *kernel);
/* Whether the last decode read the bitvector's row list (cubit_table_row_list_stats) in the
 * bitvector's place. Such a decode reports CUBIT_DECODE_PREFIXED above: its offsets are known up
 * front all the same, and it writes what the prefixed kernel writes. */
int cubit_ctx_last_decode_from_list(cubit_ctx *ctx, int *from_list);
/* Filter-kernel durations measured with HIP events recorded around each launch on the
 * context stream (ms); requires cubit_ctx_enable_timing(ctx, 1). */
int cubit_ctx_enable_timing(cubit_ctx *ctx, int on);
int cubit_last_kernel_ms(cubit_ctx *ctx, float *ms);
/* Every timed filter-kernel launch since the last reset: ms[i] for i < min(cap, *n). */
int cubit_ctx_timing_reset(cubit_ctx *ctx);
int cubit_ctx_kernel_times(cubit_ctx *ctx, float *ms, uint32_t cap, uint32_t *n);
/* Steady-state decode time: the context's next decode launch is issued `reps` times back to
 * back on its stream between two stream events (reps <= 100000; 0 disarms). Every repeat
 * rewrites the same outputs from the same inputs, so results are unchanged. Afterwards
 * cubit_ctx_repeat_time gives the mean ms per launch and the number of launches bracketed.
 * A dispatch-stamped pair (cubit_ctx_enable_timing) puts a marker and its gap inside each
 * sample, which matters for kernels of a few microseconds. */
int cubit_ctx_set_repeat(cubit_ctx *ctx, uint32_t reps);
int cubit_ctx_repeat_time(cubit_ctx *ctx, double *ms_per_launch, uint32_t *launches);
/* Compile-time contract checks (vector 2048 = 32 words, row group 122880 = 1920 words). */
int cubit_abi_version(void);
int cubit_vector_size(void);
int cubit_row_group_size(void);

/* ------------------------------------------------------------------ device memory helpers */
int cubit_dev_alloc(cubit_ctx *ctx, uint64_t bytes, void **dptr);
int cubit_dev_free(cubit_ctx *ctx, void *dptr);
/* Page-locked host memory: device ↔ host copies into it run at the link's rate (the
 * table-function mirror stages its DataChunk columns here). cubit_host_free accepts a NULL
 * context (the memory outlives contexts). */
int cubit_host_alloc(cubit_ctx *ctx, uint64_t bytes, void **hptr);
int cubit_host_free(cubit_ctx *ctx, void *hptr);
int cubit_memcpy_h2d(cubit_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int cubit_memcpy_d2h(cubit_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int cubit_memset_d(cubit_ctx *ctx, void *dst, int value, uint64_t bytes);
/* Device → device copy enqueued on the context stream (not waited for): the table-function
 * mirror packs a group's 8-byte row ids into its staging block with it. */
int cubit_memcpy_d2d(cubit_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int cubit_sync(cubit_ctx *ctx);
/* Copy streams: a stream of the context's device whose work starts after everything enqueued
 * on the context stream before the call (one pipeline task of the table-function mirror copies
 * its windows on its own, so the tasks' copies overlap instead of queueing on one stream).
 * cubit_memcpy_d2h_stream copies on it and waits for the copy; cubit_memcpy_d2h_async only
 * enqueues it, and cubit_copy_stream_sync waits for everything enqueued on the stream (the
 * copies of one window's columns, one wait). Destroyed streams go back to a pool of the context
 * (creating a HIP stream costs milliseconds) and are freed with it. */
int cubit_copy_stream_create(cubit_ctx *ctx, void **stream);
int cubit_copy_stream_destroy(cubit_ctx *ctx, void *stream);
int cubit_memcpy_d2h_stream(cubit_ctx *ctx, void *stream, void *dst, const void *src, uint64_t bytes);
int cubit_memcpy_d2h_async(cubit_ctx *ctx, void *stream, void *dst, const void *src, uint64_t bytes);
int cubit_copy_stream_sync(cubit_ctx *ctx, void *stream);
/* An event marking everything enqueued so far on a copy stream, or on the context stream when
 * `stream` is NULL (pooled per context): cubit_copy_event_sync waits for it on the host — a
 * consumer thread waits for one staged group of copies, not for the whole stream;
 * cubit_copy_stream_wait_event makes a copy stream wait for it on the device — the copies of a
 * group start when that group's probes are done; cubit_copy_event_destroy waits too and returns
 * it to the pool. */
int cubit_copy_event_record(cubit_ctx *ctx, void *stream, void **event);
int cubit_copy_event_sync(cubit_ctx *ctx, void *event);
int cubit_copy_stream_wait_event(cubit_ctx *ctx, void *stream, void *event);
int cubit_copy_event_destroy(cubit_ctx *ctx, void *event);
/* Synchronise the context stream and report any pending HIP error. */
int cubit_ctx_check(cubit_ctx *ctx);
/* Tile directory of the last row-id materialisation on this context (device pointer, valid
 * until the next scan): d_dir[2i] = start of tile i's run in the output, d_dir[2i+1] = its
 * length; tile i covers rows [i*rows_per_tile, (i+1)*rows_per_tile) of the partition. */
int cubit_ctx_last_tiles(cubit_ctx *ctx, const uint64_t **d_dir, uint32_t *n_tiles, uint64_t *rows_per_tile);

/* ------------------------------------------------------------------ low level (kernels) */

/* K0 — predicate → bitvector over a raw column (TemplatedFilterSelection compare,
 * column_segment.cpp:261-349; NULL never passes). words must hold
 * cubit_padded_words(n_rows) words; padding is zeroed. */
int cubit_build_bitvector(cubit_ctx *ctx, const void *d_col, int type, const uint64_t *d_validity, uint64_t n_rows,
                          int cmp, int64_t constant, uint64_t *d_words);
/* words per bitvector including tile padding */
uint64_t cubit_padded_words(uint64_t n_rows);
/* The kernels of a bit-sliced index (CUBIT_INDEX_SLICED), as cubit_build_bitvector is K0's. d_slices
 * is a host array of n_slices (0 ... 64) device pointers, least significant slice first, each
 * cubit_padded_words(n_rows) words, every word written (padding zeroed).
 * cubit_bitslice_build: slice s gets bit s of (uint64)key - (uint64)base of every valid row, `base`
 * given as a comparison key (cubit_fp_key of a FLOAT / DOUBLE pattern, value ^ 2^63 for UINT64). A
 * row whose key - base does not fit n_slices bits is the caller's error: its high bits are dropped
 * (a table's index never holds one). One pass of the column per 16 slices.
 * cubit_bitslice_compare: d_words = valid AND (lo <= u <= hi), u the row's offset read from the
 * slices, lo / hi unsigned offsets from the base; negate != 0 gives valid AND NOT (lo <= u <= hi).
 * lo > hi is the empty interval. d_validity NULL = every row below n_rows is valid; it is read only
 * below ceil(n_rows / 64) words. Slices, validity and d_words must be 16-byte aligned.
 * Both run on the context's stream; with timing on each call is one timed launch. */
int cubit_bitslice_build(cubit_ctx *ctx, const void *d_col, int type, const uint64_t *d_validity, uint64_t n_rows,
                         int64_t base, uint32_t n_slices, uint64_t *const *d_slices);
int cubit_bitslice_compare(cubit_ctx *ctx, const uint64_t *const *d_slices, uint32_t n_slices,
                           const uint64_t *d_validity, uint64_t n_rows, uint64_t lo, uint64_t hi, int negate,
                           uint64_t *d_words);

/* K1+K2 — evaluate a postfix program over `n_leaves` device bitvectors (each
 * cubit_padded_words(n_rows) words; leaf_negate bit k complements leaf k before use) and
 * write the int64 row ids row_base + r of the set rows into d_rowids (capacity `capacity`;
 * tile-run order unless CUBIT_SCAN_ORDERED), the count into *d_count (device). d_rowids may be NULL with
 * CUBIT_SCAN_COUNT_ONLY; d_result_words (optional) receives the evaluated bitvector.
 * Replaces the per-vector sel narrowing + row-id synthesis of RowGroup::TemplatedScan
 * (row_group.cpp:537-580). */
int cubit_bitvector_eval(cubit_ctx *ctx, const uint64_t *const *d_leaves, uint32_t n_leaves, uint32_t leaf_negate,
                         const int32_t *prog, uint32_t n_prog, uint64_t n_rows, int64_t row_base, int64_t *d_rowids,
                         uint64_t capacity, uint64_t *d_count, uint64_t *d_result_words, uint32_t flags);

/* K3 — gather a column at row ids: out[i] = col[rowids[i] - row_base] as int64
 * (ColumnData::FetchRow / FilterScan+Slice, column_data.cpp:305-309, 452-461). The number
 * of ids is read from *d_count (device), at most max_n. */
int cubit_gather(cubit_ctx *ctx, const void *d_col, int type, const int64_t *d_rowids, const uint64_t *d_count,
                 uint64_t max_n, int64_t row_base, int64_t *d_out);
/* Transfer compaction of a DataChunk column: d_out[i] = (int32)(d_in[i] - offset) for
 * i < min(*d_count, max_n). A caller whose column values all lie within [offset - 2^31,
 * offset + 2^31) (row ids of a partition below 2^31 rows with offset = row_base; DATE, or
 * DECIMAL / BIGINT whose statistics fit) moves 4 instead of 8 bytes per row to the host and
 * widens while it fills the vector (the table-function mirror's windows). */
int cubit_narrow_i32(cubit_ctx *ctx, const int64_t *d_in, const uint64_t *d_count, uint64_t max_n, int64_t offset,
                     int32_t *d_out);
/* cubit_narrow_i32 that checks the bound instead of trusting it: *d_overflow (device; the caller
 * zeroes it) becomes 1 when some value lies outside [offset - 2^31, offset + 2^31), and the
 * compacted copy must then not be used. */
int cubit_narrow_i32_checked(cubit_ctx *ctx, const int64_t *d_in, const uint64_t *d_count, uint64_t max_n,
                             int64_t offset, int32_t *d_out, uint32_t *d_overflow);
/* Transfer compaction to the width a column's statistics allow: d_out[i] = (unsigned, `width` =
 * 1, 2, 3 or 4 bytes, little-endian, packed)(d_in[i] - offset) for i < min(*d_count, max_n), for
 * values in [offset, offset + 2^(8·width)) — e.g. l_discount's 0 … 10 as one byte,
 * l_extendedprice's cents as three, a partition's row ids as four. *d_overflow
 * (device; the caller zeroes it) becomes 1 when a value lies outside, and the copy must then not
 * be used. */
int cubit_narrow_checked(cubit_ctx *ctx, const int64_t *d_in, const uint64_t *d_count, uint64_t max_n, int64_t offset,
                         int width, void *d_out, uint32_t *d_overflow);
/* Fused probe + reduce: sum over ids of a[r]*b[r] as a 128-bit integer (lo, hi int64 at
 * d_out[0..1]) — Q6's sum(l_extendedprice*l_discount) (DECIMAL(38,4) storage). */
int cubit_gather_sum_product(cubit_ctx *ctx, const int64_t *d_a, const int64_t *d_b, const int64_t *d_rowids,
                             const uint64_t *d_count, uint64_t max_n, int64_t row_base, int64_t *d_out);

/* ------------------------------------------------------------------ table partition API */

/* A row-range partition of a table resident on one device: rows [row_base, row_base+n_rows). */
int cubit_table_create(cubit_ctx *ctx, uint64_t n_rows, int64_t row_base, cubit_table **out);
int cubit_table_destroy(cubit_table *t);
/* rows, row base and owning context of a partition */
int cubit_table_info(cubit_table *t, uint64_t *n_rows, int64_t *row_base, cubit_ctx **ctx);
/* Device pointer (read-only, owned by the table or the caller that registered it) and type
 * of column `col`'s values — e.g. a column unpacked by K5 (ColumnData's decoded vectors,
 * src/storage/table/column_data.cpp:135-188). */
int cubit_table_column_data(cubit_table *t, int col, const void **data, int *type);
/* Register column `col`. data/validity are host pointers unless on_device = 1 (then the
 * table only references them). validity may be NULL (no NULLs). A caller-owned (on_device = 1)
 * buffer must not change while registered unless the caller says so with
 * cubit_table_column_changed: the table caches per-zone statistics of the values (zonemaps,
 * column statistics, selectivity estimates) and would otherwise skip zones by stale bounds.
 * Index bitvectors are not rebuilt by it (rebuild with cubit_table_build_index). `type` may be
 * any CUBIT_TYPE_* code: an 8- / 16-bit or unsigned column is widened on the device into an
 * owned INT32 / INT64 column (even from on_device data) — TINYINT … UINTEGER vectors as DuckDB
 * holds them; a UINT64 (UBIGINT) column keeps its values' bits and compares them unsigned; a FLOAT
 * or DOUBLE column is copied into the table (even from on_device data) as its bit patterns plus
 * their comparison keys (see the type codes) — widened and FP copies are the table's own, so a
 * later change to the caller's buffer is not seen: register the column again; a VARCHAR column is registered with its dictionary
 * (cubit_table_add_dict_column). Appends, updates and probes then use the stored values
 * (cubit_table_column_data reports the type held). */
int cubit_table_add_column(cubit_table *t, int col, int type, const void *data, const uint64_t *validity,
                           int on_device);
/* ---- VARCHAR dictionaries. A dictionary is built once per table (every partition of a table
 * encodes its rows against the same one, so codes are global) from any list of strings: n strings,
 * string i = bytes[offsets[i], offsets[i+1]) — duplicates and order do not matter; it keeps the
 * distinct ones sorted in DuckDB's string order (at most 2^31 - 1). Immutable once built: a table
 * that gains a string its dictionary lacks is re-registered with a new one (cubit_dict_encode
 * says so). cubit_dict_destroy drops the caller's reference; columns registered with the
 * dictionary hold their own until they go. Host-only: no context, no device memory. */
int cubit_dict_create(const char *bytes, const uint64_t *offsets, uint64_t n, cubit_dict **out);
int cubit_dict_destroy(cubit_dict *d);
int cubit_dict_size(const cubit_dict *d, uint64_t *n);
/* the string of a code (pointers into the dictionary, valid while it lives) */
int cubit_dict_entry(const cubit_dict *d, uint64_t code, const char **data, uint64_t *size);
/* codes[i] = the code of string i (layout as cubit_dict_create); a row whose validity bit is 0
 * (validity may be NULL) gets code 0 and its string is not read. CUBIT_ERR_UNSUPPORTED when a
 * valid string is not in the dictionary (codes are then unspecified). */
int cubit_dict_encode(const cubit_dict *d, const char *bytes, const uint64_t *offsets, uint64_t n,
                      const uint64_t *validity, int32_t *codes);
/* *lower_bound = the first code whose string is >= s (the size when none), *present = s is in it */
int cubit_dict_lookup(const cubit_dict *d, const char *data, uint64_t size, uint64_t *lower_bound, int *present);
/* cubit_dict_encode with every array in the context's device memory (the strings, their offsets,
 * the validity, the codes): one GPU lane per string searches the dictionary's entries (copied to
 * the device for the call). A valid string the dictionary lacks gets code -1 and makes the call
 * return CUBIT_ERR_UNSUPPORTED after the launch. */
int cubit_dict_encode_device(cubit_ctx *ctx, const cubit_dict *d, const char *d_bytes, const uint64_t *d_offsets,
                             uint64_t n, const uint64_t *d_validity, int32_t *d_codes);
/* Register a VARCHAR column: codes (host, or device with on_device = 1 as cubit_table_add_column)
 * of the table's rows against `d`, validity as for cubit_table_add_column. Every valid code must
 * lie in [0, size of d) (CUBIT_ERR_INVALID otherwise). The column holds a reference to d. */
int cubit_table_add_dict_column(cubit_table *t, int col, cubit_dict *d, const int32_t *codes, const uint64_t *validity,
                                int on_device);

/* The values of a caller-owned column changed: drop what the table derived from them. */
int cubit_table_column_changed(cubit_table *t, int col);
/* Register a column given as DuckDB BITPACKING segments (K5; the reference's persistent
 * integer storage, src/storage/compression/bitpacking.cpp): `bytes` holds the segment images
 * (each: 8-byte header = end of its metadata words, group data, metadata words of the
 * 2,048-row groups growing down), segment i at seg_offsets[i] (8-aligned) with seg_rows[i]
 * rows; the segments cover the partition in row order. The GPU unpacks every group
 * (CONSTANT, CONSTANT_DELTA, FOR, DELTA_FOR) into the column; NULLs come from `validity`
 * (host words; DuckDB keeps them in a separate validity segment). `type` is the segments' T,
 * any CUBIT_TYPE_* (header fields of T's size, T's wrap-around arithmetic); the column holds
 * the values widened to INT32 or INT64, or (UINT64) as their 64 bits, compared unsigned (see the
 * type codes). Malformed segments are
 * refused before anything is launched. With timing on, the unpack kernel is a timed launch
 * (cubit_last_kernel_ms). */
int cubit_table_add_bitpacked_column(cubit_table *t, int col, int type, const uint8_t *bytes, uint64_t n_bytes,
                                     const uint64_t *seg_offsets, const uint64_t *seg_rows, uint32_t n_segments,
                                     const uint64_t *validity);
/* Register a column given as DuckDB RLE segments (src/storage/compression/rle.cpp, the
 * reference's run-length codec for numeric columns): segment i at seg_offsets[i] with seg_rows[i]
 * rows, each as RLECompressState::FlushSegment writes it (8-byte header = offset of the uint16
 * run lengths, the run values as T from byte 8, the lengths after them; runs of at most 65,535
 * rows, zero-length runs allowed); the segments cover the partition in row order. The host reads
 * the runs (a segment whose runs do not cover its rows is refused before anything is launched),
 * only the runs cross to the device, and the GPU expands them into the column. `type` and the
 * column held are as for cubit_table_add_bitpacked_column; NULLs come from `validity` (a NULL
 * row's run value is whatever run it fell in, as in the reference). With timing on, the expand
 * kernel is a timed launch. */
int cubit_table_add_rle_column(cubit_table *t, int col, int type, const uint8_t *bytes, uint64_t n_bytes,
                               const uint64_t *seg_offsets, const uint64_t *seg_rows, uint32_t n_segments,
                               const uint64_t *validity);
/* Register a column given as DuckDB segments whose codecs differ from row group to row group, as
 * DuckDB's checkpoint picks one per segment (ColumnDataCheckpointer): seg_codecs[i] is
 * CUBIT_CODEC_UNCOMPRESSED (rows × T, the segment as FixedSizeAppend writes it),
 * CUBIT_CODEC_CONSTANT (no bytes; every row is seg_constants[i], the value as T widened to int64 —
 * a CONSTANT segment's value lives in its statistics), CUBIT_CODEC_RLE or CUBIT_CODEC_BITPACKING
 * (the layouts above); seg_offsets[i] is ignored for CONSTANT segments and seg_constants may be
 * NULL when there are none. The GPU writes every segment's rows; `type`, the column held and
 * `validity` as for cubit_table_add_bitpacked_column (the packed segments are not kept: the
 * packed filter does not apply). */
#define CUBIT_CODEC_UNCOMPRESSED 0
#define CUBIT_CODEC_CONSTANT 1
#define CUBIT_CODEC_RLE 2
#define CUBIT_CODEC_BITPACKING 3
int cubit_table_add_segment_column(cubit_table *t, int col, int type, const uint8_t *bytes, uint64_t n_bytes,
                                   const uint64_t *seg_offsets, const uint64_t *seg_rows, const int32_t *seg_codecs,
                                   const int64_t *seg_constants, uint32_t n_segments, const uint64_t *validity);
/* A column registered with cubit_table_add_bitpacked_column keeps its segments on the device:
 * a constant comparison the index cannot answer (K0) then unpacks and compares in one pass over
 * the packed bytes (w/8 bytes per row — the reference's ColumnSegment::Scan →
 * BitpackingScanPartial → FilterSelection, column_segment.cpp:378-522) instead of reading the
 * plain column. Off by default: on MI355X it measured 0.41–0.45 ms against K0's 0.43–0.44 ms
 * for a 600 M-row 12-bit date column (2.6x fewer bytes, but the unpack is instruction-bound, so
 * it does not win). Results are identical either way. Appends and merges drop the segments (the
 * plain column stays). cubit_table_last_packed: leaves the last scan built so. */
int cubit_table_use_packed_filter(cubit_table *t, int on);
int cubit_table_last_packed(cubit_table *t, uint32_t *n_leaves);
/* A column with a bit-sliced index (cubit_table_build_index(t, col, CUBIT_INDEX_SLICED, NULL, 0))
 * answers a constant comparison that would otherwise be a whole-column K0 pass from its slices,
 * when they move fewer bytes: (b + 2) / 8 per row against the column's 4 or 8. The leaf is bit for
 * bit K0's, so zonemaps, narrowing estimates and MVCC patches are unchanged; index leaves,
 * candidate checks, equality unions, bins and narrowed (masked) compares stay as they are. On a
 * column whose only index is bit-sliced, the constant bounds of a conjunction (a <= x AND x < b)
 * fold into one leaf, one pass over the slices. On by default; results are identical either way.
 * cubit_table_last_sliced: leaves the last scan / sum_product / aggregate built from slices, plus
 * one when the aggregate itself read its column's slices (cubit_table_aggregate). Off, it also
 * sends cubit_table_aggregate to the column path. */
int cubit_table_use_sliced(cubit_table *t, int on);
int cubit_table_last_sliced(cubit_table *t, uint32_t *n_leaves);
/* Selection narrowing (on by default): in a conjunction, a constant comparison on a column the
 * index cannot answer (K0) reads its column only at the rows the rest of the conjunction keeps,
 * when that is at most one row in 32 — the reference's filter loop reading each later filter
 * column through the selection of the earlier ones (RowGroup::TemplatedScan, row_group.cpp:
 * 537-550). Results are identical either way. cubit_table_last_narrowed: K0 leaves the last
 * scan built so. */
int cubit_table_use_narrowing(cubit_table *t, int on);
int cubit_table_last_narrowed(cubit_table *t, uint32_t *n_leaves);
/* The columns of the K0 comparisons the last scan built, in build order (cols[i] for i <
 * min(cap, *n)). Narrowing orders them by estimated selectivity — every literal's fraction of
 * kept rows from its column's per-zone min / max, the reference's AdaptiveFilter ordering
 * (src/execution/adaptive_filter.cpp:21-88) decided up front — most selective first, so the
 * order does not depend on the order of the filters; the estimate also decides whether to
 * narrow, without waiting for the device. */
int cubit_table_last_k0_order(cubit_table *t, int32_t *cols, uint32_t cap, uint32_t *n);
/* Build a bitmap index on `col` (K0). edges/values sorted ascending; n = 0 means "all
 * distinct values of the column" (exact for every constant). RANGE / EQUALITY replace the
 * column's primary index; BINS (n >= 2 edges) adds a secondary binned index; SLICED (n must be 0:
 * CUBIT_ERR_INVALID otherwise) adds the secondary bit-sliced index. Like every index it is
 * maintained in place: an append slices the new rows and splices them in (a key above the top adds
 * all-zero high slices first; a key below the base rebuilds the slices in one build), merges and
 * syncs re-slice the 64-row words that hold a changed row, and re-registering the column drops it. */
int cubit_table_build_index(cubit_table *t, int col, int encoding, const int64_t *values, uint32_t n);
/* Build a RANGE or BINS index on `col` whose edges are the column's equi-depth quantiles, chosen
 * on the GPU by a radix select over the column where it lies (a few streaming histogram passes; the
 * column is not copied to the host): for columns with too many distinct values for the n = 0 form
 * above (dates, prices, TIMESTAMPs, ids, DOUBLE measures). With k the comparison keys of the m valid
 * rows in ascending order and q_j = k[(j * m) / n_bins] (integer division), j = 1 ... n_bins - 1:
 *   CUBIT_INDEX_RANGE: the keys are the distinct q_j above k[0] (L(min) is empty). A column with one
 *     distinct value, or with no valid row, gets an index with no bitvector, as with n = 0 above.
 *   CUBIT_INDEX_BINS: the edges are the distinct values of {k[0]} + {q_j} + {k[m-1] + 1}; where
 *     k[m-1] + 1 is not a key (k[m-1] is INT64_MAX, UINT64_MAX or a FLOAT / DOUBLE NaN), k[m-1]
 *     itself (one past a FLOAT / DOUBLE +inf is the NaN key). Fewer than two edges, or m = 0:
 *     CUBIT_ERR_INVALID.
 *   CUBIT_INDEX_EQUALITY (quantile keys are not the values an equality index wants), n_bins outside
 *   2 ... 1,024 and an unregistered column: CUBIT_ERR_INVALID.
 * Each bin then holds about the same share of the rows, so a constant that is not a key costs the
 * same candidate check wherever it falls. The result is an ordinary index with explicit keys: it is
 * saved, loaded, appended to, merged into and synced like one from cubit_table_build_index.
 * keys / cap / n_keys (each optional, as cubit_table_last_k0_order's): *n_keys = the number of keys
 * chosen, keys[i] for i < min(cap, *n_keys) the keys in the form cubit_table_build_index takes them:
 * bit patterns for FLOAT / DOUBLE (cubit_fp_value of the key), the bits of UINT64 values. For a
 * dictionary column (VARCHAR) they are codes, where cubit_table_build_index takes addresses of
 * cubit_strings.
 * Memory: up to n_bins bitvectors of n_rows / 8 bytes each (64 bins over 600 M rows: 4.8 GB). Each
 * partition of a multi-device table chooses its own edges from its own rows. With timing on, each
 * histogram pass is a timed launch. */
int cubit_table_build_index_quantiles(cubit_table *t, int col, int encoding, uint32_t n_bins, int64_t *keys,
                                      uint32_t cap, uint32_t *n_keys);
/* Number of bitvectors and bytes held by the indexes on col, all encodings (0 if none). */
int cubit_table_index_info(cubit_table *t, int col, uint32_t *n_bitvectors, uint64_t *bytes);
/* Index persistence (the reference persists index state through IndexStorageInfo,
 * bound_index.hpp:117-118): write a column's RANGE / EQUALITY / BINS / SLICED index (keys,
 * statistics, bitvectors) to one file, and load it back into a partition of the same size
 * (it replaces that encoding's index on the column). The file does not carry the column
 * data: load it only beside the column it was built from. It names the column's type and, for a
 * dictionary column (VARCHAR, HUGEINT / UHUGEINT), its dictionary (a fingerprint of the entries):
 * a load onto a column of another type or against another dictionary is refused
 * (CUBIT_ERR_INVALID). A version-1 file names neither and holds raw values as keys: it loads onto
 * an INT32 / INT64 column only (UBIGINT, FLOAT and DOUBLE indexes are keyed by comparison keys).
 * A SLICED index is saved with no keys and one bitvector per slice; a file whose bitvector count is
 * not the bit length of vmax - vmin is refused. */
int cubit_table_save_index(cubit_table *t, int col, int encoding, const char *path);
int cubit_table_load_index(cubit_table *t, int col, const char *path);

/* MVCC delta. Deletes: rows with their delete ids (ChunkVectorInfo::deleted,
 * chunk_info.cpp:181-202). Updates on `col`: rows, new values and version ids
 * (UpdateSegment::Update, update_segment.cpp:1074-1199), chronological. Host arrays. */
int cubit_table_set_deletes(cubit_table *t, const int64_t *rows, const uint64_t *ids, uint64_t n);
int cubit_table_set_updates(cubit_table *t, int col, const int64_t *rows, const int64_t *values,
                            const uint64_t *versions, uint64_t n);
/* Updates that may set NULL (UPDATE … SET x = NULL, or a NULL row given a value): as
 * cubit_table_set_updates, plus valid[i] (1 = values[i], 0 = NULL; valid = NULL: every record
 * carries its value). DuckDB keeps these as the validity column's update chain beside the value
 * chain (InitializeUpdateValidity, src/storage/table/update_segment.cpp:588-600) and merges the
 * newest visible record into the vector's mask (UpdateMergeValidity :94-99, FetchRowValidity
 * :357-370). A reader that sees a SET NULL record finds the row in IS NULL and in no comparison,
 * and its probe reports NULL; cubit_table_column_statistics reports has_null. A column
 * registered without validity gets an all-valid one on the first SET NULL record. */
int cubit_table_set_updates_nullable(cubit_table *t, int col, const int64_t *rows, const int64_t *values,
                                     const uint8_t *valid, const uint64_t *versions, uint64_t n);
/* Inserts: n disjoint row ranges [row_begin[i], row_end[i]) appended by one transaction each,
 * with its insert id (ChunkConstantInfo::insert_id / ChunkVectorInfo::inserted,
 * src/storage/table/chunk_info.cpp:36-53, 123-161); a reader sees a range when
 * UseInsertedVersion(start_time, transaction_id, id) holds (chunk_info.cpp:11-19). Rows
 * outside every range were inserted before any snapshot. Replaces the previous set. */
int cubit_table_set_inserts(cubit_table *t, const int64_t *row_begin, const int64_t *row_end, const uint64_t *ids,
                            uint64_t n);

/* Index maintenance. Append n_new rows to the partition
 * (RowGroupCollection::Append, src/storage/table/row_group_collection.cpp, with every index's
 * BoundIndex::Append, src/include/duckdb/execution/index/bound_index.hpp:67-70): data[i] /
 * validity[i] are host arrays for column cols[i], one entry per registered column; validity[i]
 * = NULL (or validity = NULL) means all valid, else LSB-first words with bit 0 = the first
 * appended row. The new rows get local ids n_rows … n_rows+n_new-1; every index on every column
 * is maintained in place (bitvectors of the appended slice spliced in at bit n_rows; statistics
 * widened; an every-distinct-value index gains keys for values it has not seen). insert_id != 0
 * records [n_rows, n_rows+n_new) as an insert range of that transaction (see set_inserts);
 * 0 = visible to every snapshot. Storage grows geometrically when the padding runs out.
 * Columns registered as caller-owned device memory (add_column on_device = 1) are copied into
 * table-owned storage on the first append or merge; the caller's buffer is no longer read.
 * On an error the partition keeps its previous rows: scans and counts are those of the state
 * before the call (a later append overwrites the slice). What the failed call already did to
 * the indexes stays but never changes a result: bits spliced past the last row (masked by every
 * scan), statistics widened (bounds the values still lie within) and keys added to an
 * every-distinct-value index (exact leaves of values no row holds). */
int cubit_table_append(cubit_table *t, uint64_t n_new, const int *cols, const void *const *data,
                       const uint64_t *const *validity, uint32_t n_cols, uint64_t insert_id);
/* Merge the update records of `col` with version < horizon into the base values and the
 * column's indexes (the checkpoint of update chains, UpdateSegment, update_segment.cpp;
 * CUBIT's merge of its update bitvectors): each row takes its newest merged record — its value
 * (the row becomes valid) or NULL (the row's validity bit clears and it leaves every index
 * bitvector) — and the index bitvectors flip the rows whose predicate changed. Only snapshots with
 * start_time >= horizon may be served afterwards (as the reference folds versions only below
 * the lowest active start). Records at or past horizon stay. *n_merged = rows merged. */
int cubit_table_merge_updates(cubit_table *t, int col, uint64_t horizon, uint64_t *n_merged);
/* Bring `col` to new contents given whole — what a host engine holds after committed UPDATEs:
 * the column's values, with no list of the rows that changed. values = n_rows entries in the
 * element type the column was registered with (as data[i] of cubit_table_append: 4 bytes for
 * INT32 / FLOAT columns and dictionary codes, 8 bytes for every other type; FLOAT / DOUBLE as bit
 * patterns); validity = LSB-first words, NULL = every row valid. Host pointers, or with
 * on_device = 1 device pointers read in place (nothing is copied). The changed rows are found on
 * the device in one pass over the old and the new column: a row changed when its NULL-ness
 * differs, or when it is valid on both sides and the stored value differs (FLOAT / DOUBLE: the bit
 * pattern, so -0.0 -> +0.0 is a change and the probe returns what the host holds); two NULLs are
 * equal whatever their slots hold. *n_changed is written whenever the call succeeds. With
 * *n_changed > max_changed nothing is changed and *applied = 0 (the caller rebuilds the column);
 * else *applied = 1 and the base values, the validity and the column's RANGE / EQUALITY / BINS
 * indexes stand exactly as after cubit_table_merge_updates of one record per changed row (SET
 * NULL and NULL -> value included: a column registered without validity gets one, statistics
 * widen, an every-distinct-value index gains keys). *n_changed = 0 invalidates nothing: zone maps
 * and patched leaves stay. Refused (CUBIT_ERR_INVALID): an unregistered column, a column with
 * update records outstanding (merge or clear them first), a changed code outside the dictionary.
 * Extra device memory while the call runs: n_rows x element size + the validity words for host
 * input (none with on_device), one bitvector, and 17 bytes per changed row (25 for FLOAT /
 * DOUBLE); an allocation failure returns CUBIT_ERR_OOM. On an error before the records are applied
 * (every refusal, CUBIT_ERR_OOM of the staging) the table is as it was before the call. */
int cubit_table_sync_column(cubit_table *t, int col, const void *values, const uint64_t *validity,
                            int on_device, uint64_t max_changed, uint64_t *n_changed, int *applied);

/* The scan: evaluate a predicate tree (prefix nodes) for transaction `txn` (NULL = see
 * every committed row, no MVCC delta applied) and write the qualifying row ids into
 * d_rowids (tile runs, or ascending with CUBIT_SCAN_ORDERED), the count into *d_count. Replaces TableScanFunc → DataTable::Scan →
 * RowGroup::TemplatedScan's filter + row-id materialisation (table_scan.cpp:119-146). */
int cubit_table_scan(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                     int64_t *d_rowids, uint64_t capacity, uint64_t *d_count, uint32_t flags);
/* cubit_table_scan plus this scan's tile directory (as cubit_ctx_last_tiles describes it),
 * copied into d_dir (room for dir_cap tiles, 2 words each) on the context's stream within the
 * same call: safe when several threads scan on one context, where a cubit_ctx_last_tiles read
 * after the scan may already describe another thread's scan. *n_tiles = 0: no run (the filter
 * folded away or nothing to decode). Not with CUBIT_SCAN_COUNT_ONLY; CUBIT_ERR_CAPACITY when
 * dir_cap is too small (a partition has ⌈n_rows / 131,072⌉ tiles). */
int cubit_table_scan_tiles(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                           int64_t *d_rowids, uint64_t capacity, uint64_t *d_count, uint32_t flags, uint64_t *d_dir,
                           uint32_t dir_cap, uint32_t *n_tiles, uint64_t *rows_per_tile);
/* Probe column `col` at the scan's row ids (visible values for txn; a NULL row's slot as stored). */
int cubit_table_probe(cubit_table *t, int col, const cubit_txn *txn, const int64_t *d_rowids, const uint64_t *d_count,
                      uint64_t max_n, int64_t *d_out);
/* The probe with NULL-ness — ColumnData::FilterScan + Vector::Slice (column_data.cpp:305-309,
 * vector.cpp:223-258) and FetchRow (column_data.cpp:452-461) hand back the vector's validity with
 * its values: d_out[i] = the visible value of row d_rowids[i], 0 when it is NULL, and bit i of
 * d_validity (LSB-first 64-bit words, DuckDB's ValidityMask layout; room for ⌈max_n / 64⌉ words,
 * the first ⌈min(*d_count, max_n) / 64⌉ written, bits past the count 0) = the row is valid for
 * txn, with its visible SET NULL / value records applied. */
int cubit_table_probe_validity(cubit_table *t, int col, const cubit_txn *txn, const int64_t *d_rowids,
                               const uint64_t *d_count, uint64_t max_n, int64_t *d_out, uint64_t *d_validity);
/* Estimated qualifying rows of a filter tree (the nodes cubit_table_scan takes), from the
 * per-zone min / max statistics the zonemaps use (values uniform within a zone, columns
 * independent) — the cardinality estimate a caller sizes its row-id buffer by, as DuckDB's
 * TableScanInitGlobal sizes nothing but the planner estimates a filtered scan's rows from column
 * statistics (table_scan.cpp:88-106, TableFilter::CheckStatistics). No kernel beyond the zone
 * statistics (computed once per table version); exactness never depends on it. */
int cubit_table_estimate_rows(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, uint64_t *rows);
/* Bitvectors the last cubit_table_scan read per 64-row word (K) — for roofline bytes. */
int cubit_table_last_plan(cubit_table *t, uint32_t *n_leaves, uint32_t *n_passes);
/* The evaluation form of the last planned program, the kernel template its n_leaves run in:
 * 0 = POSTFIX (the general interpreter), 1 = CONJ (an AND of literals), 2 = DNF (an OR of ANDs of
 * literals), 3 = CNF (an AND of ORs of literals). 0 as well when the filter folded to FALSE or the
 * partition is empty (n_leaves is 0 then). With cubit_table_last_plan it names the (leaf count,
 * form) instantiation that ran — for tests; results never depend on it. */
int cubit_table_last_form(cubit_table *t, uint32_t *form);
/* Derived leaves. A combination of one column's index / validity bitvectors that scans keep asking
 * for — a RANGE interval's L(hi) AND NOT L(lo), the union behind an IN-list on an EQUALITY index or
 * a range over BINS — is evaluated once and kept as one table-owned bitvector, which later plans
 * read in the combination's place (K falls by k - 1 for a group of k). A combination is kept on
 * the first request before which uses * (k - 1) >= k + 1 (an interval: the fourth request); that
 * scan runs one extra bits-only pass, counted in cubit_table_last_plan's n_passes. Results never
 * change: entries are dropped whenever a table-owned bitvector is written, grown or freed, and a
 * column whose MVCC updates the reader sees is read through its own (patched) leaves.
 * `bytes` bounds what the kept bitvectors may hold (default: a quarter of the table's index
 * bitvectors), the least recently used going first; 0 turns the feature off and frees them. */
int cubit_table_set_derived_budget(cubit_table *t, uint64_t bytes);
/* Kept combinations, the bytes they hold, and the groups that plans replaced by one so far
 * (any pointer may be NULL). */
int cubit_table_derived_stats(cubit_table *t, uint32_t *leaves, uint64_t *bytes, uint64_t *hits);
/* Chains: the derivable literals of one AND chain that lie on two or more columns (a repeated WHERE
 * clause, such as TPC-H Q6's three columns) are kept as one bitvector too, under the same budget and
 * LRU. A chain is bought by cost: on the first request before which
 * uses * (k - 1) * B >= (k + 1) * B + fixed_bytes, B the bytes of one bitvector, k the bitvectors the
 * plan reads in the chain's place, fixed_bytes the fixed cost of an admitting scan expressed in bytes
 * (default: measured, cubit_derived.hpp). A small table needs thousands of requests, so a one-off
 * query pays nothing. 0 makes it the count rule of the column groups; UINT64_MAX never keeps a
 * chain (kept ones stay until evicted or invalidated).
 * There are two such costs, and this call sets both to fixed_bytes: that of an admitting scan which
 * allocates the chain's block (a table's first admission; a table whose budget holds one block), and
 * that of one which takes a block waiting in the table's free list (cubit_table_derived_pool_stats:
 * every later admission, and every re-admission after a write to the table). A request is priced by
 * whether a block is waiting at that moment; its counter is the same under either cost. */
int cubit_table_set_derived_chain_cost(cubit_table *t, uint64_t fixed_bytes);
/* The cost of an admitting scan that takes a waiting block, alone (default: measured, about a tenth of
 * the allocating scan's; cubit_derived.hpp). The allocating cost stays as it is; a later
 * cubit_table_set_derived_chain_cost replaces both again. 0 and UINT64_MAX mean what they mean there. */
int cubit_table_set_derived_chain_cost_pooled(cubit_table *t, uint64_t fixed_bytes);
/* Kept chains (counted in cubit_table_derived_stats' leaves and bytes too) and the chains that plans
 * replaced by one leaf so far (counted in its hits too). Any pointer may be NULL. */
int cubit_table_derived_chain_stats(cubit_table *t, uint32_t *chains, uint64_t *hits);
/* The blocks of kept combinations that were dropped (every write to the table drops them all; the
 * budget evicts) wait in a table-owned free list, bounded by the derived budget, and the next
 * admission takes one instead of allocating inside its scan. The table's first admission allocates
 * up to four blocks, as far as the budget goes. free_blocks: blocks waiting; device_allocs: device
 * allocations of such blocks since the table was created. The list is emptied when the budget is
 * set to 0, when the table's bitvectors grow, and with the table. */
int cubit_table_derived_pool_stats(cubit_table *t, uint32_t *free_blocks, uint64_t *device_allocs);
/* Row lists. A table-owned bitvector that a scan decodes alone (one index leaf, a kept group or
 * chain) and that is sparse enough is also kept as a list of its set rows: 2 bytes per row and 4 per
 * 131,072-row tile, wanted only when that is at most half the bitvector's bytes. The first such
 * decode of a bitvector pays nothing, the second writes the list beside its row ids, later ones read
 * the list and not the bitvector; row ids, tile directory and count are the same. A list's bytes
 * count against the derived budget: it is built only into room nothing else uses (a budget of 0:
 * never), goes before any kept bitvector does, and with its bitvector's zone map on every write to
 * the table. Forced PAIRS / RUNS decodes never read one. on = 0 stops building and reading (lists
 * held stay until dropped); default on. */
int cubit_table_use_row_lists(cubit_table *t, int on);
/* Lists held, their bytes (not part of cubit_table_derived_stats' bytes), and the decodes answered
 * from a list so far. Any pointer may be NULL. */
int cubit_table_row_list_stats(cubit_table *t, uint32_t *lists, uint64_t *bytes, uint64_t *scans_from_lists);
/* Column statistics — DataTable::GetStatistics behind seq_scan's `statistics` callback
 * (TableScanStatistics, src/function/table/table_scan.cpp:108-117): min / max of the valid
 * values (widened by the column's update records, as UpdateSegment merges updates into the
 * segment statistics) and whether any row is NULL / non-NULL. min = max = 0 when no row is
 * valid. */
int cubit_table_column_statistics(cubit_table *t, int col, int64_t *min, int64_t *max, int *has_null,
                                  int *has_no_null);
/* Zones (131,072 rows each) the last scan or sum_product evaluated, out of the partition's
 * zones; fewer when the zonemaps skipped some (0 when the filter folded to FALSE). */
int cubit_table_last_zones(cubit_table *t, uint32_t *evaluated, uint32_t *zones);

/* SELECT sum(a * b) WHERE <filter> as one fused pass (K1 + K3): evaluate the program,
 * gather a (and b) for the qualifying rows only, accumulate in 128 bits — no row ids are
 * materialised. Replaces the scan → FilterScan/Slice probe (column_data.cpp:305-309) → SUM
 * chain of a query like TPC-H Q6 (sum(l_extendedprice * l_discount)). a and b are INT64
 * columns (DECIMAL storage); rows where a or b is NULL do not contribute. When the filter
 * pins b to at most 4 values of an exact range index, b is decoded from that index instead
 * of gathered (CUBIT_SUM_GATHER_B forces the gather). d_out[0..1] = {lo, hi} of the 128-bit
 * sum; d_count (optional) = qualifying rows. Visible MVCC updates on a or b fall back to
 * scan + probe (with validity when a column is nullable: NULL rows add nothing) + sum. */
#define CUBIT_SUM_GATHER_B 1u
#define CUBIT_SUM_NO_ZONEMAP 2u /* as CUBIT_SCAN_NO_ZONEMAP */
/* When a was registered as DuckDB BITPACKING segments (cubit_table_add_bitpacked_column), the
 * fused pass reads it at the qualifying rows straight from them: BitpackingScanPartial +
 * ColumnData::FilterScan (src/storage/compression/bitpacking.cpp:779-868, column_data.cpp:305-309)
 * as one pass that touches only the packed lines holding a qualifying row (a FOR value is its
 * group's base + w bits at bit i·w; rows of DELTA_FOR groups come from the unpacked column). The
 * gathers move whole 128-byte lines, so w-bit values touch fewer lines than 8-byte ones (SF100 Q6,
 * 24-bit l_extendedprice: 0.223 vs 0.245 ms). CUBIT_SUM_PLAIN_A reads the unpacked column instead;
 * CUBIT_SUM_PACKED_A names the default. */
#define CUBIT_SUM_PACKED_A 4u
#define CUBIT_SUM_PLAIN_A 8u
/* A second path answers the same sum from the operands' bit slices without reading either column
 * (Rinfret et al. 2001): with ua = a - base_a, ub = b - base_b the offsets the slices hold and
 * V = F AND valid_a AND valid_b, sum(a * b) = |V| * base_a * base_b + base_a * sum(ub) + base_b * sum(ua)
 * + sum over i, j of 2^(i+j) * popcount(V AND A_i AND B_j), carried modulo 2^128: the same exact
 * two's-complement sum. It is usable when both columns carry a non-empty bit-sliced index
 * (CUBIT_INDEX_SLICED), cubit_table_use_sliced is on and no update record of either is visible to txn;
 * it reads (K + validities + n_in + n_out * passes) / 8 bytes per row of the evaluated zones whatever
 * the filter keeps (n_in <= n_out the slice counts, passes = max(1, ceil(n_in / 8))). Without a force
 * flag it runs when usable, n_in <= 8 (one pass over the outer slices) and its bytes are not more than
 * the fused gather's estimate. CUBIT_SUM_FROM_SLICES forces it (CUBIT_ERR_INVALID when not usable),
 * CUBIT_SUM_FROM_COLUMN forces the fused gather; both together are CUBIT_ERR_INVALID.
 * cubit_table_last_sum_product tells which ran and the slice kernel's launches (0 from the column;
 * either pointer may be NULL); cubit_table_last_sliced counts one more leaf per operand read from
 * its slices. */
#define CUBIT_SUM_FROM_SLICES 16u /* as CUBIT_AGG_FROM_SLICES */
#define CUBIT_SUM_FROM_COLUMN 32u /* as CUBIT_AGG_FROM_COLUMN */
int cubit_table_sum_product(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                            int col_a, int col_b, int64_t *d_out, uint64_t *d_count, uint32_t flags);
int cubit_table_last_sum_product(cubit_table *t, int *from_slices, uint32_t *n_launches);
/* SELECT g1 [, g2], sum(a * b), count(*) WHERE <filter> GROUP BY g1 [, g2] (the shape of TPC-H Q1's
 * sum(l_extendedprice * l_discount) per l_returnflag, l_linestatus). Groups and their numbering are
 * exactly cubit_table_aggregate_groups', with cubit_table_aggregate_grouped's refusals (an every-value
 * EQUALITY index on each group column, CUBIT_AGG_MAX_GROUPS, cap_groups below the group count is
 * CUBIT_ERR_CAPACITY). For group g, d_out + 4 * g (device, cap_groups * 4 int64) =
 * {sum_lo, sum_hi, count_valid, count_rows}: count_rows = the group's qualifying rows, count_valid =
 * those where neither a nor b is NULL (only they add to the sum). A group with no qualifying row has
 * four zeros; so has every group of an empty partition or under a filter that folds to FALSE.
 *   From the slices (both operands usable as above, and no update record of a, b or a group column
 * visible to txn): the fused kernel takes 4 groups per launch (4 x 1 bitvectors of one group column,
 * 2 x 2 of two), each launch reading the ungrouped bytes and its group bitvectors; more groups run as
 * further launches. From the column: scan into scratch, probe a, b and each group column with
 * validity (visible MVCC updates applied), reduce per group in 128 bits. flags: CUBIT_SUM_FROM_SLICES |
 * _FROM_COLUMN | _NO_ZONEMAP (anything else is CUBIT_ERR_INVALID); without a force flag the slices run
 * when usable, n_in <= 8 and estimated to move no more bytes. cubit_table_last_sum_product reports the
 * path and the fused kernel's launches. */
int cubit_table_sum_product_grouped(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes,
                                    const cubit_txn *txn, int col_a, int col_b, const int *group_cols,
                                    uint32_t n_group_cols, uint32_t flags, int64_t *d_out, uint32_t cap_groups);
/* The slice path's kernel on a caller's slices, with the conventions of cubit_bitslice_aggregate: each
 * operand's slices (0 ... 64 device pointers, each cubit_padded_words(n_rows) words, 16-byte aligned),
 * its validity (NULL = every row valid) and the base key its offsets count from; d_filter as there.
 * d_out (device, 4 int64) = {sum_lo, sum_hi, count_valid, count_rows}: count_valid = the qualifying
 * rows where neither operand is NULL. */
int cubit_bitslice_sum_product(cubit_ctx *ctx, const uint64_t *const *d_a_slices, uint32_t n_a,
                               const uint64_t *d_a_validity, int64_t base_a, const uint64_t *const *d_b_slices,
                               uint32_t n_b, const uint64_t *d_b_validity, int64_t base_b, const uint64_t *d_filter,
                               uint64_t n_rows, int64_t *d_out);
/* How the last sum_product read b: number of values decoded from the index (0 = gathered;
 * 1 = the filter pins b to one value, which is multiplied in as a constant: no leaf is read). */
int cubit_table_last_sum_decode(cubit_table *t, uint32_t *n_values);
/* Whether the last sum_product read a from its BITPACKING segments. */
int cubit_table_last_sum_packed(cubit_table *t, int *packed);

/* SELECT sum(col), min(col), max(col), count(col), count(*) WHERE <filter> of one column, ready on
 * the context's stream with no host round trip. d_out (device, 6 int64) =
 * {sum_lo, sum_hi, min, max, count_valid, count_rows}; ops = CUBIT_AGG_SUM | _MIN | _MAX names the
 * aggregates wanted, the two counts are always written and the slots of ops not asked for are 0.
 *   The aggregates run over the qualifying rows where col is not NULL: SUM, MIN and MAX ignore NULLs
 * (the reference's BaseSumOperation and MinMaxBase answer IgnoreNull() true,
 * src/include/duckdb/core_functions/aggregate/sum_helpers.hpp:170,
 * src/core_functions/aggregate/distributive/minmax.cpp:84, so AggregateExecutor::UnaryFlatLoop skips
 * the rows its validity mask clears, common/vector_operations/aggregate_executor.hpp:53-90),
 * count_valid is COUNT(col) (CountFunction::CountFlatLoop counts the valid rows only,
 * src/function/aggregate/distributive/count.cpp:60-106) and count_rows is COUNT(*) (CountStarFunction,
 * count.cpp:25). With count_valid = 0 the reference's SUM / MIN / MAX are NULL: sum is 0 and
 * min / max are unspecified here, SQL NULL is the caller's to emit.
 *   sum is the exact 128-bit two's-complement sum of the values (a UINT64 column's values are summed
 * unsigned); min / max are in the form cubit_table_column_statistics reports them (FLOAT / DOUBLE bit
 * patterns: the key order is DuckDB's value order, NaN above +inf, -0.0 = +0.0 reported as +0.0;
 * UINT64 bits; a dictionary column's codes). An empty partition, or a filter that folds to FALSE,
 * gives zero counts.
 *   CUBIT_ERR_UNSUPPORTED: SUM on a FLOAT / DOUBLE / VARCHAR / dictionary column (its keys are not
 * linear in the value; MIN / MAX on them work). CUBIT_ERR_INVALID: an unregistered column, ops or
 * flags outside the bits below, both force flags together.
 *   Two paths give the same result. From the slices: with a non-empty bit-sliced index
 * (CUBIT_INDEX_SLICED) on col, cubit_table_use_sliced on and no update record of col visible to
 * txn, one fused kernel evaluates the filter program (visibility and zonemap skip included) and
 * aggregates from the slices: SUM = count_valid * base + sum over s of 2^s * popcount(F AND valid AND
 * slice s), MIN / MAX a ripple from the top slice down (O'Neil & Quass 1997), (b + K [+ 1]) / 8 bytes
 * per row of the evaluated zones. From the column: scan into scratch, probe with validity (visible
 * MVCC updates applied), reduce. Without a force flag the path estimated to move fewer bytes is
 * taken. CUBIT_AGG_FROM_SLICES forces the first (CUBIT_ERR_INVALID when the conditions above do
 * not hold), CUBIT_AGG_FROM_COLUMN the second; cubit_table_last_aggregate tells which ran
 * (cubit_table_last_sliced counts the slice path as one more sliced leaf; cubit_table_last_zones
 * reports the evaluated zones). */
#define CUBIT_AGG_SUM 1u
#define CUBIT_AGG_MIN 2u
#define CUBIT_AGG_MAX 4u            /* the two counts are always written */
#define CUBIT_AGG_FROM_SLICES 16u   /* force the slice path (CUBIT_ERR_INVALID if the column has no usable bit-sliced index) */
#define CUBIT_AGG_FROM_COLUMN 32u   /* force the column path */
#define CUBIT_AGG_NO_ZONEMAP 64u    /* as CUBIT_SCAN_NO_ZONEMAP */
int cubit_table_aggregate(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                          int col, uint32_t ops, int64_t *d_out);
int cubit_table_last_aggregate(cubit_table *t, int *from_slices);

/* SELECT g1 [, g2], sum(col), min(col), max(col), count(col), count(*) WHERE <filter> GROUP BY g1 [, g2]:
 * cubit_table_aggregate per group, in one pass. Each of the one or two group columns carries a primary
 * CUBIT_INDEX_EQUALITY index over every distinct value (built with n = 0, or kept so by appends and
 * merges); anything else is CUBIT_ERR_UNSUPPORTED, naming the column. VARCHAR and HUGEINT / UHUGEINT
 * group columns work: their equality indexes are over dictionary codes.
 *   The slots of a group column, ascending: the index's keys; the values that one of the column's
 * update records carries and that are no key (an MVCC update may move a row to a value the index has
 * never seen); and one NULL slot, last, when the column is nullable or an update record sets it NULL
 * (GROUP BY makes NULL a group of its own: the reference's hash and perfect-hash aggregates group NULL
 * keys like any other, src/execution/operator/aggregate/physical_hash_aggregate.cpp,
 * physical_perfecthash_aggregate.cpp). Group g = i1 * n2 + i2 over the slots of the two columns
 * (n2 = 1 with one column); n1 * n2 above CUBIT_AGG_MAX_GROUPS is CUBIT_ERR_UNSUPPORTED.
 *   cubit_table_aggregate_groups (host only) reports the numbering: *n_groups = n1 * n2, and for
 * g < min(cap, *n_groups) keys[g * n_group_cols + c] = the slot's key of group column c in the form
 * cubit_table_build_index_quantiles reports keys (FLOAT / DOUBLE bit patterns, UINT64 bits, a dictionary
 * column's codes; 0 at a NULL slot) and key_is_null[g * n_group_cols + c] = 1 at a NULL slot. keys and
 * key_is_null may be NULL. The numbering holds until a group column's index or update records change
 * (build, append, merge, sync, set_updates).
 *   cubit_table_aggregate_grouped writes, for group g at d_out + 6 * g (device, cap_groups * 6 int64),
 * the six slots of cubit_table_aggregate: {sum_lo, sum_hi, min, max, count_valid, count_rows}, with its
 * NULL handling, type rules, SUM refusal and ops (CUBIT_AGG_FROM_SLICES, _FROM_COLUMN and _NO_ZONEMAP
 * included). A group with no qualifying row has six zeros (the caller omits it, as SQL does); so has
 * every group of an empty partition or under a filter that folds to FALSE. cap_groups below the
 * group count is CUBIT_ERR_CAPACITY. The result is ready on the context's stream with no host round
 * trip.
 *   From the slices (a usable bit-sliced index on col, and no update record of col or of a group
 * column visible to txn): one fused kernel evaluates the filter program and aggregates a batch of
 * groups per launch, each group's rows formed in registers as F AND E1 AND E2 of the group columns'
 * equality bitvectors (the NULL slot: the complement of the column's validity), reading
 * (b + K [+ 1] + the launch's group bitvectors) / 8 bytes per row of the evaluated zones; more groups
 * than one launch takes run as further launches on the stream. A slot that exists only because of an
 * update value has no bitvector and no rows on this path. From the column: scan into scratch, probe
 * col and each group column with validity (visible MVCC updates applied), reduce per group. Without
 * a force flag the path estimated to move fewer bytes runs; both give the same numbers.
 * cubit_table_last_grouped tells which ran, the group count and the fused kernel's launches (0 on
 * the column path); any of its pointers may be NULL. */
#define CUBIT_AGG_MAX_GROUP_COLS 2
#define CUBIT_AGG_MAX_GROUPS 256
int cubit_table_aggregate_groups(cubit_table *t, const int *group_cols, uint32_t n_group_cols, int64_t *keys,
                                 uint8_t *key_is_null, uint32_t cap, uint32_t *n_groups);
int cubit_table_aggregate_grouped(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes,
                                  const cubit_txn *txn, int col, const int *group_cols, uint32_t n_group_cols,
                                  uint32_t ops, int64_t *d_out, uint32_t cap_groups);
int cubit_table_last_grouped(cubit_table *t, int *from_slices, uint32_t *n_groups, uint32_t *n_launches);
/* The slice path's kernel on a caller's slices, as cubit_bitslice_compare is the compare's: d_slices
 * as there (n_slices 0 ... 64 device pointers, each cubit_padded_words(n_rows) words, 16-byte
 * aligned), d_validity NULL = every row valid, read only below ceil(n_rows / 64) words; d_filter =
 * the qualifying rows as a bitvector of cubit_padded_words(n_rows) words (bits at or past n_rows are
 * ignored), NULL = every row below n_rows. type / base: the column's type (CUBIT_TYPE_INT32, _INT64,
 * _UINT64, _FLOAT, _DOUBLE, _VARCHAR; SUM refused as above) and the slices' base key; ops = CUBIT_AGG_SUM |
 * _MIN | _MAX. d_out as cubit_table_aggregate's. */
int cubit_bitslice_aggregate(cubit_ctx *ctx, const uint64_t *const *d_slices, uint32_t n_slices,
                             const uint64_t *d_validity, const uint64_t *d_filter, uint64_t n_rows,
                             int type, int64_t base, uint32_t ops, int64_t *d_out);

/* Selection by rank: the k-th smallest / largest value of col, or quantile_disc(col, q), over the
 * qualifying rows where col is not NULL (the reference's quantile ignores NULLs), ready on the
 * context's stream with no host round trip. d_out (device, 6 int64) =
 * {value, found, count_below, count_equal, count_valid, count_rows}: value in the form
 * cubit_table_column_statistics reports (FLOAT / DOUBLE bit patterns with NaN greatest and -0.0 = +0.0
 * reported as +0.0, UINT64 bits, a dictionary column's codes), as cubit_table_aggregate's min / max;
 * found = 0 (and value = count_below = count_equal = 0) when no non-NULL row qualifies or the rank is
 * at or past count_valid; count_below = the qualifying non-NULL rows strictly before the value in
 * the direction asked, count_equal = those equal to it; count_valid / count_rows as
 * cubit_table_aggregate's. An empty partition, or a filter that folds to FALSE, gives six zeros.
 *   mode: CUBIT_SELECT_RANK (k = the 0-based rank, ascending), CUBIT_SELECT_RANK_DESC (k = 0 is the
 * largest) or CUBIT_SELECT_QUANTILE: the rank is max(1, n - floor(n - n * q)) - 1 with n =
 * count_valid, computed on the device in double arithmetic — the reference's Interpolator<true>::Index
 * for a non-DECIMAL q (src/include/duckdb/core_functions/aggregate/quantile_sort_tree.hpp:166-188);
 * q outside [0, 1] or NaN is CUBIT_ERR_INVALID. k is ignored with QUANTILE, q otherwise.
 *   Two paths give the same six numbers, chosen as cubit_table_aggregate chooses (flags below; without
 * a force flag the path estimated to move fewer bytes). From the slices (a usable bit-sliced index
 * on col, cubit_table_use_sliced on, no update record of col visible to txn): a radix select over
 * the slices, most significant first, 4 slices per pass; pass 0 evaluates the filter program
 * (visibility and zonemap skip included), writes the candidates F AND valid to one scratch bitvector
 * and histograms the first chunk, each later pass narrows the candidates by the chosen bucket and
 * histograms the next chunk, and one workgroup after each pass walks the histogram on the device. About
 * (K [+ 1] + 1 + 2b - 4 + 2 * (passes - 1)) / 8 bytes per row of the evaluated zones. From the column:
 * scan into scratch, probe with validity (visible MVCC updates applied), then a radix select over
 * the probed values, 8 bits per pass. cubit_table_last_select tells which ran and its passes (either
 * pointer may be NULL). Partitions of 2^47 rows or more are refused on the slice path.
 *   Not offered: several ranks per call; quantile_cont and median (they interpolate between two
 * ranks, which a caller gets from two RANK calls); a DECIMAL-typed q; anything through the table
 * function (DuckDB v1.1.2 pushes neither an aggregate nor a LIMIT into seq_scan). */
#define CUBIT_SELECT_RANK 0      /* k = 0-based rank among the qualifying non-NULL rows, ascending */
#define CUBIT_SELECT_RANK_DESC 1 /* ... descending: k = 0 is the largest */
#define CUBIT_SELECT_QUANTILE 2  /* quantile_disc(col, q), 0 <= q <= 1 */
#define CUBIT_SELECT_DESC_ROWS 1u     /* cubit_table_top_n: ORDER BY col DESC */
#define CUBIT_SELECT_FROM_SLICES 16u  /* as CUBIT_AGG_FROM_SLICES */
#define CUBIT_SELECT_FROM_COLUMN 32u  /* as CUBIT_AGG_FROM_COLUMN */
#define CUBIT_SELECT_NO_ZONEMAP 64u   /* as CUBIT_AGG_NO_ZONEMAP */
int cubit_table_select(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                       int col, int mode, uint64_t k, double q, uint32_t flags, int64_t *d_out);
int cubit_table_last_select(cubit_table *t, int *from_slices, uint32_t *n_passes);
/* The slice path's kernels on a caller's slices: arguments as cubit_bitslice_aggregate's, mode / k / q
 * and d_out as cubit_table_select's. The candidate bitvector lives in context scratch. */
int cubit_bitslice_select(cubit_ctx *ctx, const uint64_t *const *d_slices, uint32_t n_slices,
                          const uint64_t *d_validity, const uint64_t *d_filter, uint64_t n_rows, int type,
                          int64_t base, int mode, uint64_t k, double q, int64_t *d_out);
/* Selection by rank per group: SELECT g, quantile_disc(col, q) ... GROUP BY g, the per-group k-th
 * value likewise. The groups and their numbering are exactly cubit_table_aggregate_groups' (one or two
 * group columns, each with an EQUALITY index over every distinct value; a NULL slot last; slots made
 * by update values included; g = i1 * n2 + i2; at most CUBIT_AGG_MAX_GROUPS), and the refusals are
 * cubit_table_aggregate_grouped's: CUBIT_ERR_UNSUPPORTED names the column, cap_groups below the group
 * count is CUBIT_ERR_CAPACITY, n_group_cols = 0 is CUBIT_ERR_INVALID (cubit_table_select is that call).
 *   For group g, d_out + 6 * g (device, cap_groups * 6 int64) holds the six slots of cubit_table_select
 * over the group's qualifying rows, with its value form, NULL handling and type rules (FLOAT / DOUBLE /
 * UINT64 / dictionary columns work: a select needs only the order). mode, k and q are
 * cubit_table_select's and the same for every group: with CUBIT_SELECT_RANK / _RANK_DESC a group with
 * count_valid <= k has found = 0 and its counts still written; with CUBIT_SELECT_QUANTILE each group's
 * rank comes from its own count_valid, computed on the device. A group without a qualifying row has six
 * zeros; so has every group of an empty partition or under a filter that folds to FALSE. The result
 * is ready on the context's stream with no host round trip.
 *   flags: CUBIT_SELECT_FROM_SLICES | _FROM_COLUMN | _NO_ZONEMAP (any other bit, or both force flags, is
 * CUBIT_ERR_INVALID). From the slices (usable as cubit_table_aggregate_grouped's slice path: a non-empty
 * bit-sliced index on col, cubit_table_use_sliced on, no update record of col or of a group column
 * visible to txn; FROM_SLICES without that is CUBIT_ERR_INVALID): the groups of a call are pairwise
 * disjoint, so one scratch candidate bitvector carries the radix selects of a whole batch of up to 8
 * groups. Pass 0 evaluates the filter program, forms each group's rows as F AND E1 AND E2 in registers,
 * writes the union of the groups' candidates and histograms the first chunk per group; each later
 * pass narrows the candidates by each group's own chosen bucket and histograms the next chunk; one
 * workgroup after each pass steps every group's state. A batch runs through all its passes before
 * the next starts. Per batch about (K [+ 1] + 1 + 2b - 4 + 2 * (passes - 1) + leaves * passes) / 8
 * bytes per row of the evaluated zones. A slot that exists only because of an update value has no
 * bitvector and no rows on this path. From the column: scan into scratch, probe col and each group
 * column with validity (visible MVCC updates applied), then one radix select for all groups over the
 * probed values, 4 bits per pass. cubit_table_last_select_grouped tells which ran, the group count, the
 * batches (0 on the column path) and the passes per batch (the column path: its 16 array passes); any
 * of its pointers may be NULL. cubit_table_last_select stays the ungrouped call's. */
int cubit_table_select_grouped(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn,
                               int col, const int *group_cols, uint32_t n_group_cols, int mode, uint64_t k, double q,
                               uint32_t flags, int64_t *d_out, uint32_t cap_groups);
int cubit_table_last_select_grouped(cubit_table *t, int *from_slices, uint32_t *n_groups, uint32_t *n_launches,
                                    uint32_t *n_passes);
/* The grouped slice path's kernels on a caller's slices: arguments as cubit_bitslice_select's, plus
 * n_groups (1 ... CUBIT_AGG_MAX_GROUPS) group bitvectors d_groups, each cubit_padded_words(n_rows) words,
 * 16-byte aligned. d_out + 6 * g = the six slots over the rows of group g. The group bitvectors must be
 * PAIRWISE DISJOINT: that is the caller's contract, and overlapping groups give unspecified numbers.
 * A row in no group belongs to no result. */
int cubit_bitslice_select_grouped(cubit_ctx *ctx, const uint64_t *const *d_slices, uint32_t n_slices,
                                  const uint64_t *d_validity, const uint64_t *d_filter,
                                  const uint64_t *const *d_groups, uint32_t n_groups, uint64_t n_rows, int type,
                                  int64_t base, int mode, uint64_t k, double q, int64_t *d_out);
/* ... WHERE <filter> ORDER BY col [DESC], rowid LIMIT k: the global row ids of the first k qualifying
 * non-NULL rows into d_rowids, in ascending row-id order — every row strictly before the threshold
 * value (the value of rank k - 1), then the lowest row ids among the rows equal to it until k.
 * *d_count = min(k, count_valid); d_out as cubit_table_select's for rank k - 1 in the direction asked.
 * NULL rows are never returned: when fewer than k non-NULL rows qualify, found = 0 and
 * count_rows - count_valid is what NULLS LAST would append. k = 0 writes no id, *d_count = 0 and six
 * zeros. capacity < k is CUBIT_ERR_CAPACITY; a VARCHAR or dictionary column is CUBIT_ERR_UNSUPPORTED.
 * flags: CUBIT_SELECT_DESC_ROWS | the path flags above. The call waits for its result: it reads the
 * six numbers back and then runs two ordered scans through the planner with the same txn (filter AND
 * col before the threshold; filter AND col = the threshold), so any column and either select path
 * works and visible MVCC updates are the planner's; scratch for count_below + count_equal ids is
 * allocated for the call. */
int cubit_table_top_n(cubit_table *t, const cubit_filter_node *nodes, uint32_t n_nodes, const cubit_txn *txn, int col,
                      uint64_t k, uint32_t flags, int64_t *d_rowids, uint64_t capacity, uint64_t *d_count,
                      int64_t *d_out);

#ifdef __cplusplus
}
#endif
#endif /* CUBIT_GPU_H */
