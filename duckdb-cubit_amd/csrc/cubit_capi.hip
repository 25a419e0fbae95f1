// C ABI of libcubitgpu.so (include/cubit_gpu.h) and the host-side planner that turns a
// DuckDB-style predicate tree (TableFilter mirror) into bitvector programs for the
// fused eval/decode kernel. The expressions, the emitter that writes a program and the walk of a
// filter tree are in cubit_program.hpp (HIP-free, run on the CPU by tests/program_core.cpp), the
// policy of the kept leaf combinations in cubit_derived.hpp (tests/derived_core.cpp); what touches
// a table or the device is here.
//
// Planner semantics (all exact; a leaf the index cannot answer exactly is built from the raw
// column — by the candidate check of its bin, or by K0 — never approximated):
//   range index, L(k) = {valid & v < k}:  v<c = L(c'), v<=c = L(c+1), v>c = NN∖L(c+1),
//     v>=c = NN∖L(c), v==c = L(c+1)∖L(c), v!=c = (NN∖L(c+1)) ∪ L(c); where L(c') is the
//     bitvector of the smallest key ≥ c when the index holds every distinct value. A
//     constant between keys k_lo < c < k_hi: v<c = L(k_lo) ∪ {r ∈ L(k_hi)∖L(k_lo) : v[r] < c}
//     (candidate check), v==c = {r ∈ L(k_hi)∖L(k_lo) : v[r] == c}.
//   equality index, E(k) = {v == k}: v==c = E(c), v!=c = NN∖E(c), ranges = ∪ E(k).
//   NULLs never satisfy a comparison (TemplatedFilterSelection HAS_NULL path,
//   column_segment.cpp:261-276) — NN is the column's validity bitvector.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/cubit_gpu.h"
#include "cubit_derived.hpp"
#include "cubit_internal.hpp"

using namespace cubit;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_CHECK(expr)                                                                                  \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) return fail(CUBIT_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                          __FILE__, __LINE__);                                           \
    } while (0)

}  // namespace

// ------------------------------------------------------------------ context

struct cubit_ctx {
    int device = 0;
    // n_cus: the compute units the launchers size their grids by — the device's (device_cus), or
    // fewer under cubit_ctx_set_compute_units, never more
    int n_cus = 256;
    int device_cus = 256;
    LaunchShape last_grid;  // cubit_ctx_last_grid: the last tile-walking launch's workgroups and tiles
    hipStream_t stream = nullptr;
    bool timing = false;
    // one (start, stop) event pair per timed filter-kernel launch since the last reset
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
    size_t n_timed = 0;
    // tile directory of the last decode ({start, length} per tile) + ordered-pass scratch
    uint64_t* dir = nullptr;
    uint64_t* dst_off = nullptr;
    uint64_t dir_tiles = 0;
    uint32_t last_tiles = 0;
    uint64_t last_tile_rows = 0;
    int64_t* tmp_ids = nullptr;
    uint64_t tmp_cap = 0;
    int64_t* partials = nullptr;
    int64_t* agg = nullptr;      // workspace of the aggregate kernels (kAggWorkspace int64)
    // the grouped aggregate's workspace (kGroupWorkspace int64) and the slot keys of its column path
    // (2 × CUBIT_AGG_MAX_GROUPS int64, staged in page-locked memory like the live-tile list),
    // allocated by the first grouped call (ensure_grouped)
    int64_t* gagg = nullptr;
    int64_t* gkeys_dev = nullptr;
    int64_t* gkeys_host = nullptr;
    hipEvent_t gkeys_ev = nullptr;
    bool gkeys_pending = false;
    int64_t* sel = nullptr;      // workspace of the select kernels (kSelectWorkspace int64; ensure_select)
    int64_t* gsel = nullptr;     // … of the grouped select's (kSelectGroupWorkspace int64; ensure_select_grouped)
    uint64_t* ticket = nullptr;  // claim ticket of the evaluate kernels (EvalArgs::ticket)
    uint64_t* flags = nullptr;   // look-back flag words of eval_decode_lookback (EvalArgs::flags)
    uint64_t epoch = 0;          // the last look-back launch's epoch (EvalArgs::epoch)
    uint32_t lookback_spins = 0; // EvalArgs::spin_limit (cubit_ctx_set_lookback_spins; 0 = default)
    int decode_kernel = CUBIT_DECODE_AUTO;  // cubit_ctx_set_decode_kernel
    int last_decode = 0;                    // kernel of the last decode (CUBIT_DECODE_PAIRS / _RUNS)
    bool last_from_list = false;            // the last decode read a row list, not the bitvector
    // zonemap skip: the live-tile list of a launch, staged in page-locked memory and copied to
    // the device on the stream; live_ev marks the copy done before the staging is rewritten
    uint32_t* live_host = nullptr;
    uint32_t* live_dev = nullptr;
    uint64_t live_cap = 0;
    hipEvent_t live_ev = nullptr;
    bool live_pending = false;
    // cubit_ctx_set_repeat: the next decode launch is issued `repeat` times back to back
    // between two stream events (rep_ev); rep_launches of them went into the last measurement
    uint32_t repeat = 0;
    uint32_t rep_launches = 0;
    hipEvent_t rep_ev[2] = {nullptr, nullptr};
    // copy streams handed back by cubit_copy_stream_destroy, each with its ordering event
    // (creating a HIP stream costs milliseconds; the table function's tasks take one per scan)
    std::vector<std::pair<hipStream_t, hipEvent_t>> copy_pool;
    std::unordered_map<hipStream_t, hipEvent_t> copy_live;
    // copy events (cubit_copy_event_record): handed out and returned through a pool
    std::vector<hipEvent_t> copy_ev_pool;
    std::unordered_set<hipEvent_t> copy_ev_live;
    std::recursive_mutex mu;     // CUBIT_LOCK
};

namespace {

// Every entry point that reads or changes a context's state (its stream, claim ticket, tile
// directory, timing events, tables) holds the context's mutex, so DuckDB pipeline threads
// may share one context; results named "last" belong to its most recent call.
#define CUBIT_LOCK(c) std::lock_guard<std::recursive_mutex> cubit_lock_((c)->mu)

int ensure_dir(cubit_ctx* ctx, uint64_t tiles) {
    if (tiles <= ctx->dir_tiles && ctx->dir) return CUBIT_OK;
    if (ctx->dir) HIP_CHECK(hipFree(ctx->dir));
    if (ctx->dst_off) HIP_CHECK(hipFree(ctx->dst_off));
    ctx->dir = ctx->dst_off = nullptr;
    const uint64_t want = std::max<uint64_t>(tiles, 1024);
    if (hipMalloc(&ctx->dir, 2 * want * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&ctx->dst_off, want * sizeof(uint64_t)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "tile directory allocation of %llu tiles failed", (unsigned long long)want);
    ctx->dir_tiles = want;
    return CUBIT_OK;
}

int ensure_tmp(cubit_ctx* ctx, uint64_t cap) {
    if (cap <= ctx->tmp_cap && ctx->tmp_ids) return CUBIT_OK;
    if (ctx->tmp_ids) HIP_CHECK(hipFree(ctx->tmp_ids));
    ctx->tmp_ids = nullptr;
    if (hipMalloc(&ctx->tmp_ids, std::max<uint64_t>(cap, 1) * sizeof(int64_t)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "ordered-pass scratch of %llu ids failed", (unsigned long long)cap);
    ctx->tmp_cap = cap;
    return CUBIT_OK;
}

int set_device(cubit_ctx* ctx) {
    HIP_CHECK(hipSetDevice(ctx->device));
    return CUBIT_OK;
}

// the select kernels' workspace, allocated by the first select on the context
int ensure_select(cubit_ctx* ctx) {
    if (ctx->sel) return CUBIT_OK;
    if (hipMalloc(&ctx->sel, kSelectWorkspace * sizeof(int64_t)) != hipSuccess) {
        ctx->sel = nullptr;
        return fail(CUBIT_ERR_OOM, "select workspace allocation failed");
    }
    return CUBIT_OK;
}

// the grouped select's workspace, allocated on the context when the first grouped select needs it
int ensure_select_grouped(cubit_ctx* ctx) {
    if (ctx->gsel) return CUBIT_OK;
    if (hipMalloc(&ctx->gsel, kSelectGroupWorkspace * sizeof(int64_t)) != hipSuccess) {
        ctx->gsel = nullptr;
        return fail(CUBIT_ERR_OOM, "grouped select workspace allocation failed");
    }
    return CUBIT_OK;
}

// Start/stop events for the next timed kernel (stamped by its dispatch through
// hipExtLaunchKernelGGL); both stay null when timing is off.
int timing_events(cubit_ctx* ctx, hipEvent_t& start, hipEvent_t& stop) {
    start = stop = nullptr;
    if (!ctx->timing) return CUBIT_OK;
    if (ctx->n_timed == ctx->evs.size()) {
        // timing-only events: no system-scope release when they are recorded, so a stamp does
        // not wait for an L2 writeback of the kernel's dirty lines (HIP documents this for
        // timing accuracy on AMD devices). Measured: the stamped mean stays 2-4 % above
        // rocprofv3's kernel trace (73.7 vs 71.1 µs at SF100 Q6), as with default events.
        // Results stay ordered by the stream; readers synchronise on it.
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));
        HIP_CHECK(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
        ctx->evs.emplace_back(e0, e1);
    }
    start = ctx->evs[ctx->n_timed].first;
    stop = ctx->evs[ctx->n_timed].second;
    ctx->n_timed++;
    return CUBIT_OK;
}

// Stage the live-tile list of a zonemap-skipping launch on the device (asynchronous on the
// context stream): zone z becomes tiles z·per_zone … z·per_zone + per_zone - 1 of the kernel.
int upload_live(cubit_ctx* ctx, const std::vector<uint32_t>& zones, uint32_t per_zone, const uint32_t** d_live,
                uint32_t* n_live) {
    const uint64_t n = (uint64_t)zones.size() * per_zone;
    if (ctx->live_pending) {  // the previous list's copy must be done before its staging is reused
        HIP_CHECK(hipEventSynchronize(ctx->live_ev));
        ctx->live_pending = false;
    }
    if (n > ctx->live_cap) {
        if (ctx->live_dev) HIP_CHECK(hipFree(ctx->live_dev));
        if (ctx->live_host) HIP_CHECK(hipHostFree(ctx->live_host));
        ctx->live_dev = nullptr;
        ctx->live_host = nullptr;
        ctx->live_cap = 0;
        const uint64_t cap = std::max<uint64_t>(n, 4096);
        if (hipMalloc(&ctx->live_dev, cap * 4) != hipSuccess || hipHostMalloc(&ctx->live_host, cap * 4) != hipSuccess)
            return fail(CUBIT_ERR_OOM, "live-tile list of %llu tiles failed", (unsigned long long)cap);
        ctx->live_cap = cap;
    }
    if (!ctx->live_ev) HIP_CHECK(hipEventCreateWithFlags(&ctx->live_ev, hipEventDisableTiming));
    uint64_t k = 0;
    for (uint32_t z : zones)
        for (uint32_t j = 0; j < per_zone; ++j) ctx->live_host[k++] = z * per_zone + j;
    HIP_CHECK(hipMemcpyAsync(ctx->live_dev, ctx->live_host, n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipEventRecord(ctx->live_ev, ctx->stream));
    ctx->live_pending = true;
    *d_live = ctx->live_dev;
    *n_live = (uint32_t)n;
    return CUBIT_OK;
}

// The EvalArgs of a fused kernel that walks tiles of tile_words words and arrives on the context's
// ticket: the tiles that hold rows, or — live non-empty (zonemap skip) — the live zones' tiles, staged
// by upload_live. The caller sets `count` when its launcher does not.
int tile_eval_args(cubit_ctx* ctx, const EvalProgram& prog, uint64_t n_rows, int64_t row_base, uint64_t tile_words,
                   const std::vector<uint32_t>& live, EvalArgs& a) {
    a = EvalArgs{};
    a.prog = prog;
    a.n_rows = n_rows;
    a.n_words = (n_rows + 63) / 64;
    a.row_base = row_base;
    a.ticket = ctx->ticket;
    a.num_tiles = (uint32_t)((a.n_words + tile_words - 1) / tile_words);
    if (!live.empty()) {
        uint32_t n_live = 0;
        if (int rc = upload_live(ctx, live, (uint32_t)(kZoneWords / tile_words), &a.live, &n_live)) return rc;
        a.num_tiles = n_live;
    }
    return CUBIT_OK;
}

enum class RunMode { kDecode, kCount };

// What a decode of one bitvector alone does with the bitvector's row list (cubit_row_list.hpp):
// write it beside the row ids (kRowListBuild), or read it in the bitvector's place (kRowListRead).
struct RowListUse {
    RowListStep step = kRowListNone;
    uint16_t* off = nullptr;
    uint32_t* lo_cnt = nullptr;
};

// Launch the evaluator over a compiled program (asynchronous on the context stream).
//   kDecode: row ids as per-tile ascending runs + tile directory (ordered = lay them out in
//            row order: the look-back decode writes them so, up to kLookbackMaxTiles tiles;
//            past that, one extra pass); kCount: count(*) and/or result words.
// live_zones (optional, non-empty, ascending): evaluate only these zones (zonemap skip); the
// other tiles hold no qualifying row. Not with result_words (the skipped words stay unwritten).
int run_eval(cubit_ctx* ctx, const EvalProgram& prog, uint64_t n_rows, int64_t row_base, int64_t* rowids,
             uint64_t capacity, uint64_t* d_count, uint64_t* result_words, RunMode mode, bool timed = false,
             bool ordered = false, bool check_capacity = false, const std::vector<uint32_t>* live_zones = nullptr,
             const uint64_t* tile_prefix = nullptr, const RowListUse* row_list = nullptr) {
    // the directory describes only the decode launched here: a count, a failed launch or a
    // folded-away filter leaves no tiles behind for cubit_ctx_last_tiles to hand out
    ctx->last_tiles = 0;
    ctx->last_from_list = false;
    // the claim ticket carries row sums in 48 bits (finish_ticket)
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    EvalArgs a{};
    a.prog = prog;
    a.n_rows = n_rows;
    a.n_words = (n_rows + 63) / 64;
    a.row_base = row_base;
    a.count = d_count;
    a.result_words = result_words;
    a.ticket = ctx->ticket;
    const uint64_t pw = padded_words(n_rows);
    if (live_zones && (live_zones->empty() || result_words)) live_zones = nullptr;
    hipEvent_t start = nullptr, stop = nullptr;
    if (timed)
        if (int rc = timing_events(ctx, start, stop)) return rc;
    if (mode == RunMode::kCount) {
        a.num_tiles = (uint32_t)(pw / count_tile_words(prog.n_leaves));
        if (live_zones) {
            uint32_t n_live = 0;
            if (int rc = upload_live(ctx, *live_zones, (uint32_t)(kZoneWords / count_tile_words(prog.n_leaves)),
                                     &a.live, &n_live))
                return rc;
            a.num_tiles = n_live;
        }
        HIP_CHECK(launch_eval_count(a, ctx->stream, start, stop));
        return CUBIT_OK;
    }
    // the tiles that hold rows (the padding past the last word needs no workgroup); the
    // directory is sized for every padded tile, as a live-tile list may name any of them
    const uint64_t tiles = (a.n_words + decode_tile_words() - 1) / decode_tile_words();
    if (int rc = ensure_dir(ctx, pw / decode_tile_words())) return rc;
    // per-tile offsets known up front (tile_prefix): the look-back kernel without its walk, at any
    // size, unless another kernel is forced; an ordered scan takes the look-back decode (runs in
    // tile order) unless a kernel is forced
    const bool prefixed = tile_prefix && rowids && (ctx->decode_kernel == 0 || ctx->decode_kernel == 3);
    const int kernel = prefixed || (ordered && rowids && ctx->decode_kernel == 0 && tiles <= kLookbackMaxTiles)
                           ? 3
                           : ctx->decode_kernel;
    const bool order_pass = ordered && rowids && !(kernel == 3 && (prefixed || tiles <= kLookbackMaxTiles));
    if (order_pass)
        if (int rc = ensure_tmp(ctx, capacity)) return rc;
    a.num_tiles = (uint32_t)tiles;
    a.flags = ctx->flags;
    a.epoch = ++ctx->epoch;
    a.spin_limit = ctx->lookback_spins;
    a.tile_prefix = prefixed ? tile_prefix : nullptr;
    a.rowids = order_pass ? ctx->tmp_ids : rowids;
    a.capacity = rowids ? capacity : 0;
    // a row list goes with the prefixed decode only: built as its side output, or read by a kernel of
    // its own that visits every tile (an empty one costs a directory entry), so no live-tile list
    const bool from_list = prefixed && prog.n_leaves == 1 && row_list && row_list->step == kRowListRead;
    if (prefixed && prog.n_leaves == 1 && row_list && row_list->step == kRowListBuild) {
        a.list_off = row_list->off;
        a.list_lo = row_list->lo_cnt;
    }
    RowListArgs la{};
    if (from_list) {
        la.prefix = tile_prefix;
        la.off = row_list->off;
        la.lo_cnt = row_list->lo_cnt;
        la.tiles = (uint32_t)tiles;
        la.row_base = row_base;
        la.rowids = a.rowids;
        la.capacity = a.capacity;
        la.count = d_count;
    }
    if (live_zones && !from_list) {
        static_assert(kZoneWords == 2048, "a zone is one decode tile");
        uint32_t n_live = 0;
        if (int rc = upload_live(ctx, *live_zones, 1, &a.live, &n_live)) return rc;
        a.num_tiles = n_live;
        // skipped tiles hold no rows: their directory entries are {0, 0}
        HIP_CHECK(hipMemsetAsync(ctx->dir, 0, 2 * tiles * sizeof(uint64_t), ctx->stream));
    }
    // persistent grid: two 512-thread workgroups per CU (VGPR-limited to 4 waves per SIMD).
    // Between one and two tiles per workgroup, every workgroup takes a whole pair instead
    // (grid = tiles / 2): the same critical path (one pair), a third fewer claims queued on
    // the ticket word at once (768 tiles: 384 instead of 512, ≈11 ns each).
    const uint64_t work = a.num_tiles;
    const uint64_t max_grid = (uint64_t)ctx->n_cus * 2;
    // (a grid of ceil(work / ceil(work / max_grid)) workgroups, every one the same number of tiles,
    // measured slower: SF100 / 4 18.5 -> 21.0 µs, fewer workgroups than the last round's leave HBM
    // unsaturated; profiles/r06k_balanced_grid_not_kept.txt)
    const unsigned grid = (unsigned)(work <= max_grid ? work : work <= 2 * max_grid ? (work + 1) / 2 : max_grid);
    auto launch = [&](hipEvent_t e0, hipEvent_t e1) {
        return from_list ? launch_decode_row_list(la, ctx->dir, ctx->stream, e0, e1)
                         : launch_eval_decode(a, ctx->dir, grid, ctx->stream, e0, e1, kernel, ctx->n_cus);
    };
    if (tiles == 0) {  // no row: the count is 0 and no kernel runs
        if (start) ctx->n_timed--;
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
        ctx->last_decode = 0;
        return CUBIT_OK;
    }
    if (ctx->repeat) {
        // steady-state kernel time: the same launch `repeat` times back to back, bracketed by two
        // stream events (a dispatch-stamped pair adds a marker and its gap to each sample). Every
        // repeat rewrites the same outputs from the same inputs; the look-back takes a new epoch.
        if (start) {
            ctx->n_timed--;
            start = stop = nullptr;
        }
        if (!ctx->rep_ev[0]) {
            HIP_CHECK(hipEventCreate(&ctx->rep_ev[0]));
            HIP_CHECK(hipEventCreate(&ctx->rep_ev[1]));
        }
        HIP_CHECK(hipEventRecord(ctx->rep_ev[0], ctx->stream));
        for (uint32_t i = 1; i < ctx->repeat; ++i) {
            HIP_CHECK(launch(nullptr, nullptr));
            a.epoch = ++ctx->epoch;
        }
    }
    HIP_CHECK(launch(start, stop));
    ctx->last_from_list = from_list;
    if (ctx->repeat) {
        HIP_CHECK(hipEventRecord(ctx->rep_ev[1], ctx->stream));
        ctx->rep_launches = ctx->repeat;
        ctx->repeat = 0;
    }
    ctx->last_decode = prefixed && prog.n_leaves == 1
                           ? CUBIT_DECODE_PREFIXED
                           : decode_kernel_for(prog.n_leaves, a.num_tiles, grid, kernel, a.live != nullptr, ctx->n_cus,
                                               prefixed);
    // the look-back kernel, its prefixed form and the row-list kernel launch one workgroup per tile
    const bool per_tile =
        from_list || ctx->last_decode == CUBIT_DECODE_LOOKBACK || ctx->last_decode == CUBIT_DECODE_PREFIXED;
    const uint32_t walked = from_list ? la.tiles : a.num_tiles;
    ctx->last_grid = LaunchShape{per_tile ? walked : grid, walked};
    ctx->last_tiles = (uint32_t)tiles;
    ctx->last_tile_rows = decode_tile_words() * 64;
    if (order_pass)
        HIP_CHECK(launch_order_runs(ctx->dir, (uint32_t)tiles, ctx->dst_off, ctx->tmp_ids, capacity, rowids,
                                    ctx->stream));
    if (check_capacity && rowids) {
        uint64_t n = 0;
        HIP_CHECK(hipMemcpyAsync(&n, d_count, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (n > capacity)
            return fail(CUBIT_ERR_CAPACITY, "%llu qualifying rows exceed the capacity of %llu row ids",
                        (unsigned long long)n, (unsigned long long)capacity);
    }
    return CUBIT_OK;
}

}  // namespace

extern "C" {

int cubit_abi_version(void) { return 1; }
int cubit_vector_size(void) { return (int)kVectorSize; }
int cubit_row_group_size(void) { return (int)kRowGroupSize; }
uint64_t cubit_padded_words(uint64_t n_rows) { return padded_words(n_rows); }
const char* cubit_last_error(void) { return g_last_error.c_str(); }

int cubit_device_count(int* n) {
    if (!n) return fail(CUBIT_ERR_INVALID, "null argument");
    HIP_CHECK(hipGetDeviceCount(n));
    return CUBIT_OK;
}

int cubit_ctx_create(int device, cubit_ctx** out) {
    if (!out) return fail(CUBIT_ERR_INVALID, "out is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(CUBIT_ERR_HIP, "no HIP device visible");
    if (device < 0 || device >= n) return fail(CUBIT_ERR_INVALID, "device %d out of range (%d devices)", device, n);
    HIP_CHECK(hipSetDevice(device));
    auto* ctx = new cubit_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->n_cus = ctx->device_cus = prop.multiProcessorCount;
    if (hipMalloc(&ctx->partials, 2 * kSumBlocks * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&ctx->agg, kAggWorkspace * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&ctx->ticket, kTicketWords * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(ctx->ticket, 0, kTicketWords * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&ctx->flags, kLookbackMaxTiles * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(ctx->flags, 0, kLookbackMaxTiles * sizeof(uint64_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        if (ctx->partials) (void)hipFree(ctx->partials);
        if (ctx->agg) (void)hipFree(ctx->agg);
        if (ctx->ticket) (void)hipFree(ctx->ticket);
        if (ctx->flags) (void)hipFree(ctx->flags);
        delete ctx;
        return fail(CUBIT_ERR_OOM, "context workspace allocation failed");
    }
    *out = ctx;
    return CUBIT_OK;
}

int cubit_ctx_destroy(cubit_ctx* ctx) {
    if (!ctx) return CUBIT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->dir) (void)hipFree(ctx->dir);
    if (ctx->dst_off) (void)hipFree(ctx->dst_off);
    if (ctx->tmp_ids) (void)hipFree(ctx->tmp_ids);
    if (ctx->partials) (void)hipFree(ctx->partials);
    if (ctx->agg) (void)hipFree(ctx->agg);
    if (ctx->gkeys_pending) (void)hipEventSynchronize(ctx->gkeys_ev);
    if (ctx->gagg) (void)hipFree(ctx->gagg);
    if (ctx->sel) (void)hipFree(ctx->sel);
    if (ctx->gsel) (void)hipFree(ctx->gsel);
    if (ctx->gkeys_dev) (void)hipFree(ctx->gkeys_dev);
    if (ctx->gkeys_host) (void)hipHostFree(ctx->gkeys_host);
    if (ctx->gkeys_ev) (void)hipEventDestroy(ctx->gkeys_ev);
    if (ctx->ticket) (void)hipFree(ctx->ticket);
    if (ctx->flags) (void)hipFree(ctx->flags);
    if (ctx->live_pending) (void)hipEventSynchronize(ctx->live_ev);
    if (ctx->live_dev) (void)hipFree(ctx->live_dev);
    if (ctx->live_host) (void)hipHostFree(ctx->live_host);
    if (ctx->live_ev) (void)hipEventDestroy(ctx->live_ev);
    for (hipEvent_t e : ctx->rep_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& se : ctx->copy_live) ctx->copy_pool.push_back(se);
    for (auto& se : ctx->copy_pool) {
        (void)hipStreamDestroy(se.first);
        (void)hipEventDestroy(se.second);
    }
    for (hipEvent_t e : ctx->copy_ev_live) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->copy_ev_pool) (void)hipEventDestroy(e);
    for (auto& e : ctx->evs) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    delete ctx;
    return CUBIT_OK;
}

int cubit_ctx_set_stream(cubit_ctx* ctx, void* stream) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    CUBIT_LOCK(ctx);
    hipStream_t next = static_cast<hipStream_t>(stream);
    if (next != ctx->stream) {
        // the claim ticket, tile directory, scratch ids and partials are re-armed / reused in
        // stream order: a launch still in flight on the old stream must finish before the
        // first launch on the new one
        if (int rc = set_device(ctx)) return rc;
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    ctx->stream = next;
    return CUBIT_OK;
}

int cubit_ctx_set_decode_kernel(cubit_ctx* ctx, int kernel) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "null context");
    if (kernel < CUBIT_DECODE_AUTO || kernel > CUBIT_DECODE_LOOKBACK) return fail(CUBIT_ERR_INVALID, "decode kernel %d", kernel);
    CUBIT_LOCK(ctx);
    ctx->decode_kernel = kernel;
    return CUBIT_OK;
}

int cubit_ctx_last_decode_from_list(cubit_ctx* ctx, int* from_list) {
    if (!ctx || !from_list) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    *from_list = ctx->last_from_list ? 1 : 0;
    return CUBIT_OK;
}

int cubit_ctx_set_lookback_spins(cubit_ctx* ctx, uint32_t spins) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "null context");
    CUBIT_LOCK(ctx);
    ctx->lookback_spins = spins;
    return CUBIT_OK;
}

int cubit_ctx_set_compute_units(cubit_ctx* ctx, int n) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "null context");
    CUBIT_LOCK(ctx);
    // lower only: a count above the device's could size a grid past what is co-resident
    if (n < 0 || n > ctx->device_cus)
        return fail(CUBIT_ERR_INVALID, "compute units %d (the device has %d)", n, ctx->device_cus);
    ctx->n_cus = n == 0 ? ctx->device_cus : n;
    return CUBIT_OK;
}

int cubit_ctx_compute_units(cubit_ctx* ctx, int* device, int* in_use) {
    if (!ctx || !device || !in_use) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    *device = ctx->device_cus;
    *in_use = ctx->n_cus;
    return CUBIT_OK;
}

int cubit_ctx_last_grid(cubit_ctx* ctx, uint32_t* workgroups, uint32_t* tiles) {
    if (!ctx || !workgroups || !tiles) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    *workgroups = ctx->last_grid.workgroups;
    *tiles = ctx->last_grid.tiles;
    return CUBIT_OK;
}

int cubit_ctx_last_decode_kernel(cubit_ctx* ctx, int* kernel) {
    if (!ctx || !kernel) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    *kernel = ctx->last_decode;
    return CUBIT_OK;
}

int cubit_ctx_enable_timing(cubit_ctx* ctx, int on) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    CUBIT_LOCK(ctx);
    ctx->timing = on != 0;
    return CUBIT_OK;
}

int cubit_last_kernel_ms(cubit_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (ctx->n_timed == 0) return fail(CUBIT_ERR_INVALID, "no timed kernel recorded (enable timing first)");
    const auto& e = ctx->evs[ctx->n_timed - 1];
    HIP_CHECK(hipEventSynchronize(e.second));
    HIP_CHECK(hipEventElapsedTime(ms, e.first, e.second));
    return CUBIT_OK;
}

int cubit_ctx_timing_reset(cubit_ctx* ctx) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    CUBIT_LOCK(ctx);
    ctx->n_timed = 0;
    return CUBIT_OK;
}

int cubit_ctx_kernel_times(cubit_ctx* ctx, float* ms, uint32_t cap, uint32_t* n) {
    if (!ctx || !n) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    const uint32_t m = (uint32_t)std::min<size_t>(cap, ctx->n_timed);
    for (uint32_t i = 0; i < m; ++i) {
        HIP_CHECK(hipEventSynchronize(ctx->evs[i].second));
        HIP_CHECK(hipEventElapsedTime(&ms[i], ctx->evs[i].first, ctx->evs[i].second));
    }
    *n = (uint32_t)ctx->n_timed;
    return CUBIT_OK;
}

int cubit_ctx_set_repeat(cubit_ctx* ctx, uint32_t reps) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    if (reps > 100000) return fail(CUBIT_ERR_INVALID, "%u repeats", reps);
    CUBIT_LOCK(ctx);
    ctx->repeat = reps;
    return CUBIT_OK;
}

int cubit_ctx_repeat_time(cubit_ctx* ctx, double* ms_per_launch, uint32_t* launches) {
    if (!ctx || !ms_per_launch) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (!ctx->rep_launches) return fail(CUBIT_ERR_INVALID, "no repeated decode launch recorded (cubit_ctx_set_repeat)");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipEventSynchronize(ctx->rep_ev[1]));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->rep_ev[0], ctx->rep_ev[1]));
    *ms_per_launch = (double)ms / ctx->rep_launches;
    if (launches) *launches = ctx->rep_launches;
    return CUBIT_OK;
}

int cubit_dev_alloc(cubit_ctx* ctx, uint64_t bytes, void** dptr) {
    if (!ctx || !dptr) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    if (hipMalloc(dptr, std::max<uint64_t>(bytes, 16)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "hipMalloc(%llu) failed", (unsigned long long)bytes);
    return CUBIT_OK;
}

int cubit_dev_free(cubit_ctx* ctx, void* dptr) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    if (dptr) HIP_CHECK(hipFree(dptr));
    return CUBIT_OK;
}

int cubit_host_alloc(cubit_ctx* ctx, uint64_t bytes, void** hptr) {
    if (!ctx || !hptr) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    // portable: the table function's pinned pool serves copies from every device's partitions
    if (hipHostMalloc(hptr, std::max<uint64_t>(bytes, 16), hipHostMallocPortable) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "hipHostMalloc(%llu) failed", (unsigned long long)bytes);
    return CUBIT_OK;
}

int cubit_host_free(cubit_ctx* ctx, void* hptr) {
    (void)ctx;  // page-locked memory is not tied to a context: NULL is accepted
    if (hptr) HIP_CHECK(hipHostFree(hptr));
    return CUBIT_OK;
}

int cubit_memcpy_h2d(cubit_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return CUBIT_OK;
}

int cubit_memcpy_d2h(cubit_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return CUBIT_OK;
}

int cubit_copy_stream_create(cubit_ctx* ctx, void** stream) {
    if (!ctx || !stream) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (int rc = set_device(ctx)) return rc;
    std::pair<hipStream_t, hipEvent_t> se{nullptr, nullptr};
    if (!ctx->copy_pool.empty()) {
        se = ctx->copy_pool.back();
        ctx->copy_pool.pop_back();
    } else {
        HIP_CHECK(hipStreamCreateWithFlags(&se.first, hipStreamNonBlocking));
        if (hipEventCreateWithFlags(&se.second, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(se.first);
            return fail(CUBIT_ERR_DEVICE, "copy stream: event creation failed");
        }
    }
    ctx->copy_live[se.first] = se.second;
    // the stream starts behind the context stream's enqueued work (the scan and its probes)
    HIP_CHECK(hipEventRecord(se.second, ctx->stream));
    HIP_CHECK(hipStreamWaitEvent(se.first, se.second, 0));
    *stream = se.first;
    return CUBIT_OK;
}

int cubit_copy_stream_destroy(cubit_ctx* ctx, void* stream) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    if (!stream) return CUBIT_OK;
    CUBIT_LOCK(ctx);
    auto it = ctx->copy_live.find(static_cast<hipStream_t>(stream));
    if (it == ctx->copy_live.end()) return fail(CUBIT_ERR_INVALID, "not a copy stream of this context");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipStreamSynchronize(it->first));  // its copies are done before another task reuses it
    ctx->copy_pool.push_back(*it);
    ctx->copy_live.erase(it);
    return CUBIT_OK;
}

int cubit_memcpy_d2h_stream(cubit_ctx* ctx, void* stream, void* dst, const void* src, uint64_t bytes) {
    if (!ctx || !stream) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return CUBIT_OK;
}

int cubit_memcpy_d2h_async(cubit_ctx* ctx, void* stream, void* dst, const void* src, uint64_t bytes) {
    if (!ctx || !stream) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    return CUBIT_OK;
}

int cubit_copy_stream_sync(cubit_ctx* ctx, void* stream) {
    if (!ctx || !stream) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return CUBIT_OK;
}

int cubit_copy_event_record(cubit_ctx* ctx, void* stream, void** event) {
    if (!ctx || !event) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (int rc = set_device(ctx)) return rc;
    hipEvent_t e = nullptr;
    if (!ctx->copy_ev_pool.empty()) {
        e = ctx->copy_ev_pool.back();
        ctx->copy_ev_pool.pop_back();
    } else {
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    ctx->copy_ev_live.insert(e);
    HIP_CHECK(hipEventRecord(e, stream ? static_cast<hipStream_t>(stream) : ctx->stream));
    *event = e;
    return CUBIT_OK;
}

int cubit_copy_stream_wait_event(cubit_ctx* ctx, void* stream, void* event) {
    if (!ctx || !stream || !event) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
    return CUBIT_OK;
}

int cubit_copy_event_sync(cubit_ctx* ctx, void* event) {
    if (!ctx || !event) return fail(CUBIT_ERR_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipEventSynchronize(static_cast<hipEvent_t>(event)));
    return CUBIT_OK;
}

int cubit_copy_event_destroy(cubit_ctx* ctx, void* event) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    if (!event) return CUBIT_OK;
    CUBIT_LOCK(ctx);
    auto it = ctx->copy_ev_live.find(static_cast<hipEvent_t>(event));
    if (it == ctx->copy_ev_live.end()) return fail(CUBIT_ERR_INVALID, "not a copy event of this context");
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipEventSynchronize(*it));  // its copies are done before the event is reused
    ctx->copy_ev_pool.push_back(*it);
    ctx->copy_ev_live.erase(it);
    return CUBIT_OK;
}

int cubit_memset_d(cubit_ctx* ctx, void* dst, int value, uint64_t bytes) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    HIP_CHECK(hipMemsetAsync(dst, value, bytes, ctx->stream));
    return CUBIT_OK;
}

int cubit_memcpy_d2d(cubit_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    if (!ctx || ((!dst || !src) && bytes)) return fail(CUBIT_ERR_INVALID, "null argument");
    if (!bytes) return CUBIT_OK;
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CUBIT_OK;
}

int cubit_ctx_check(cubit_ctx* ctx) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipGetLastError());
    return CUBIT_OK;
}

int cubit_ctx_last_tiles(cubit_ctx* ctx, const uint64_t** d_dir, uint32_t* n_tiles, uint64_t* rows_per_tile) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    CUBIT_LOCK(ctx);
    if (d_dir) *d_dir = ctx->dir;
    if (n_tiles) *n_tiles = ctx->last_tiles;
    if (rows_per_tile) *rows_per_tile = ctx->last_tile_rows;
    return CUBIT_OK;
}

int cubit_sync(cubit_ctx* ctx) {
    if (!ctx) return fail(CUBIT_ERR_INVALID, "ctx is null");
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return CUBIT_OK;
}

int cubit_build_bitvector(cubit_ctx* ctx, const void* d_col, int type, const uint64_t* d_validity, uint64_t n_rows,
                          int cmp, int64_t constant, uint64_t* d_words) {
    if (!ctx || !d_col || !d_words) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (cmp < 0 || cmp > 5) return fail(CUBIT_ERR_INVALID, "cmp %d", cmp);
    HIP_CHECK(launch_compare_bitvector(d_col, type, d_validity, n_rows, cmp, value_key(type, constant), d_words,
                                       ctx->stream));
    return CUBIT_OK;
}

int cubit_bitslice_build(cubit_ctx* ctx, const void* d_col, int type, const uint64_t* d_validity, uint64_t n_rows,
                         int64_t base, uint32_t n_slices, uint64_t* const* d_slices) {
    if (!ctx || !d_col || (n_slices && !d_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (n_slices > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u slices (0 … 64)", n_slices);
    SliceSet out{};
    for (uint32_t s = 0; s < n_slices; ++s) {
        if (!d_slices[s]) return fail(CUBIT_ERR_INVALID, "slice %u is null", s);
        out.s[s] = d_slices[s];
    }
    hipEvent_t e0, e1;
    if (int rc = timing_events(ctx, e0, e1)) return rc;
    HIP_CHECK(launch_bitslice_build(d_col, type, d_validity, n_rows, base, n_slices, out, ctx->stream, e0, e1));
    if (n_slices == 0 && e0) {  // nothing launched: the timed slot still reads as a (zero) launch
        HIP_CHECK(hipEventRecord(e0, ctx->stream));
        HIP_CHECK(hipEventRecord(e1, ctx->stream));
    }
    return CUBIT_OK;
}

int cubit_bitslice_compare(cubit_ctx* ctx, const uint64_t* const* d_slices, uint32_t n_slices,
                           const uint64_t* d_validity, uint64_t n_rows, uint64_t lo, uint64_t hi, int negate,
                           uint64_t* d_words) {
    if (!ctx || !d_words || (n_slices && !d_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_slices > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u slices (0 … 64)", n_slices);
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (!aligned(d_words) || !aligned(d_validity)) return fail(CUBIT_ERR_INVALID, "bitvectors must be 16-byte aligned");
    SliceSet sl{};
    for (uint32_t s = 0; s < n_slices; ++s) {
        if (!d_slices[s] || !aligned(d_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u is null or unaligned", s);
        sl.s[s] = const_cast<uint64_t*>(d_slices[s]);
    }
    hipEvent_t e0, e1;
    if (int rc = timing_events(ctx, e0, e1)) return rc;
    HIP_CHECK(launch_bitslice_compare(sl, n_slices, d_validity, n_rows, lo, hi, negate, d_words, ctx->stream, e0, e1));
    return CUBIT_OK;
}

int cubit_bitslice_aggregate(cubit_ctx* ctx, const uint64_t* const* d_slices, uint32_t n_slices,
                             const uint64_t* d_validity, const uint64_t* d_filter, uint64_t n_rows, int type,
                             int64_t base, uint32_t ops, int64_t* d_out) {
    if (!ctx || !d_out || (n_slices && !d_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_slices > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u slices (0 … 64)", n_slices);
    if (ops & ~(CUBIT_AGG_SUM | CUBIT_AGG_MIN | CUBIT_AGG_MAX)) return fail(CUBIT_ERR_INVALID, "ops %u", ops);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && type != CUBIT_TYPE_VARCHAR && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if ((ops & CUBIT_AGG_SUM) && (type_is_fp(type) || type == CUBIT_TYPE_VARCHAR))
        return fail(CUBIT_ERR_UNSUPPORTED, "SUM of a type %d column: its keys are not linear in the value", type);
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (!aligned(d_filter) || !aligned(d_validity)) return fail(CUBIT_ERR_INVALID, "bitvectors must be 16-byte aligned");
    SliceAggArgs g{};
    for (uint32_t s = 0; s < n_slices; ++s) {
        if (!d_slices[s] || !aligned(d_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u is null or unaligned", s);
        g.slices.s[s] = const_cast<uint64_t*>(d_slices[s]);
    }
    if (int rc = set_device(ctx)) return rc;
    if (n_rows == 0) {  // no rows: zero counts, nothing to launch
        HIP_CHECK(hipMemsetAsync(d_out, 0, 6 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    g.n_slices = n_slices;
    g.validity = d_validity;
    g.workspace = ctx->agg;
    EvalProgram prog{};
    if (d_filter) {  // a one-leaf program; NULL: the zero-leaf form, every row below n_rows
        prog.leaf[0] = d_filter;
        prog.n_leaves = 1;
    }
    EvalArgs a;
    if (int rc = tile_eval_args(ctx, prog, n_rows, 0, kAggTileWords, {}, a)) return rc;
    hipEvent_t e0, e1;
    if (int rc = timing_events(ctx, e0, e1)) return rc;
    HIP_CHECK(launch_eval_slice_aggregate(a, g, ops, type, base,
                                          ctx->n_cus, &ctx->last_grid, d_out, ctx->stream, e0, e1));
    return CUBIT_OK;
}

int cubit_bitslice_sum_product(cubit_ctx* ctx, const uint64_t* const* d_a_slices, uint32_t n_a,
                               const uint64_t* d_a_validity, int64_t base_a, const uint64_t* const* d_b_slices,
                               uint32_t n_b, const uint64_t* d_b_validity, int64_t base_b, const uint64_t* d_filter,
                               uint64_t n_rows, int64_t* d_out) {
    if (!ctx || !d_out || (n_a && !d_a_slices) || (n_b && !d_b_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_a > kMaxSlices || n_b > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u and %u slices (0 … 64)", n_a, n_b);
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (!aligned(d_filter) || !aligned(d_a_validity) || !aligned(d_b_validity))
        return fail(CUBIT_ERR_INVALID, "bitvectors must be 16-byte aligned");
    // the operand with fewer slices is the inner one (the sum is symmetric)
    const bool a_outer = n_a >= n_b;
    SliceProductArgs g{};
    for (uint32_t s = 0; s < n_a; ++s) {
        if (!d_a_slices[s] || !aligned(d_a_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u of a is null or unaligned", s);
        (a_outer ? g.outer : g.inner).s[s] = const_cast<uint64_t*>(d_a_slices[s]);
    }
    for (uint32_t s = 0; s < n_b; ++s) {
        if (!d_b_slices[s] || !aligned(d_b_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u of b is null or unaligned", s);
        (a_outer ? g.inner : g.outer).s[s] = const_cast<uint64_t*>(d_b_slices[s]);
    }
    if (int rc = set_device(ctx)) return rc;
    if (n_rows == 0) {  // no rows: a zero sum and zero counts, nothing to launch
        HIP_CHECK(hipMemsetAsync(d_out, 0, 4 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    g.n_outer = a_outer ? n_a : n_b;
    g.n_inner = a_outer ? n_b : n_a;
    g.valid_a = d_a_validity;
    g.valid_b = d_b_validity;
    g.workspace = ctx->agg;
    EvalProgram prog{};
    if (d_filter) {  // a one-leaf program; NULL: the zero-leaf form, every row below n_rows
        prog.leaf[0] = d_filter;
        prog.n_leaves = 1;
    }
    EvalArgs a;
    if (int rc = tile_eval_args(ctx, prog, n_rows, 0, kAggTileWords, {}, a)) return rc;
    hipEvent_t e0, e1;
    if (int rc = timing_events(ctx, e0, e1)) return rc;
    HIP_CHECK(launch_eval_slice_sum_product(a, g, a_outer ? base_a : base_b, a_outer ? base_b : base_a,
                                            ctx->n_cus, &ctx->last_grid, d_out,
                                            4, nullptr, ctx->stream, e0, e1));
    return CUBIT_OK;
}

int cubit_bitslice_select(cubit_ctx* ctx, const uint64_t* const* d_slices, uint32_t n_slices, const uint64_t* d_validity,
                          const uint64_t* d_filter, uint64_t n_rows, int type, int64_t base, int mode, uint64_t k, double q,
                          int64_t* d_out) {
    if (!ctx || !d_out || (n_slices && !d_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_slices > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u slices (0 … 64)", n_slices);
    if (mode != CUBIT_SELECT_RANK && mode != CUBIT_SELECT_RANK_DESC && mode != CUBIT_SELECT_QUANTILE)
        return fail(CUBIT_ERR_INVALID, "mode %d", mode);
    if (mode == CUBIT_SELECT_QUANTILE && !(q >= 0.0 && q <= 1.0)) return fail(CUBIT_ERR_INVALID, "quantile %g outside [0, 1]", q);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && type != CUBIT_TYPE_VARCHAR && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (!aligned(d_filter) || !aligned(d_validity)) return fail(CUBIT_ERR_INVALID, "bitvectors must be 16-byte aligned");
    SliceSelectArgs g{};
    for (uint32_t s = 0; s < n_slices; ++s) {
        if (!d_slices[s] || !aligned(d_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u is null or unaligned", s);
        g.slices.s[s] = const_cast<uint64_t*>(d_slices[s]);
    }
    if (int rc = set_device(ctx)) return rc;
    if (n_rows == 0) {  // no rows: zero counts, nothing to launch
        HIP_CHECK(hipMemsetAsync(d_out, 0, 6 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    if (int rc = ensure_select(ctx)) return rc;
    if (int rc = ensure_tmp(ctx, padded_words(n_rows))) return rc;  // the candidate bitvector
    g.n_slices = n_slices;
    g.validity = d_validity;
    g.cand = reinterpret_cast<uint64_t*>(ctx->tmp_ids);
    g.workspace = ctx->sel;
    EvalProgram prog{};
    if (d_filter) {  // a one-leaf program; NULL: the zero-leaf form, every row below n_rows
        prog.leaf[0] = d_filter;
        prog.n_leaves = 1;
    }
    EvalArgs a;
    if (int rc = tile_eval_args(ctx, prog, n_rows, 0, kAggTileWords, {}, a)) return rc;
    hipEvent_t e0, e1;
    if (int rc = timing_events(ctx, e0, e1)) return rc;
    HIP_CHECK(launch_slice_select(a, g, mode, k, q, type, base,
                                  ctx->n_cus, &ctx->last_grid, d_out, ctx->stream, nullptr, e0, e1));
    return CUBIT_OK;
}

int cubit_bitslice_select_grouped(cubit_ctx* ctx, const uint64_t* const* d_slices, uint32_t n_slices,
                                  const uint64_t* d_validity, const uint64_t* d_filter, const uint64_t* const* d_groups,
                                  uint32_t n_groups, uint64_t n_rows, int type, int64_t base, int mode, uint64_t k, double q,
                                  int64_t* d_out) {
    if (!ctx || !d_out || !d_groups || (n_slices && !d_slices)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_slices > kMaxSlices) return fail(CUBIT_ERR_INVALID, "%u slices (0 … 64)", n_slices);
    if (n_groups == 0 || n_groups > CUBIT_AGG_MAX_GROUPS)
        return fail(CUBIT_ERR_INVALID, "%u groups (1 … %d)", n_groups, CUBIT_AGG_MAX_GROUPS);
    if (mode != CUBIT_SELECT_RANK && mode != CUBIT_SELECT_RANK_DESC && mode != CUBIT_SELECT_QUANTILE)
        return fail(CUBIT_ERR_INVALID, "mode %d", mode);
    if (mode == CUBIT_SELECT_QUANTILE && !(q >= 0.0 && q <= 1.0)) return fail(CUBIT_ERR_INVALID, "quantile %g outside [0, 1]", q);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && type != CUBIT_TYPE_VARCHAR && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    if (!aligned(d_filter) || !aligned(d_validity)) return fail(CUBIT_ERR_INVALID, "bitvectors must be 16-byte aligned");
    SliceSelectArgs g{};
    for (uint32_t s = 0; s < n_slices; ++s) {
        if (!d_slices[s] || !aligned(d_slices[s])) return fail(CUBIT_ERR_INVALID, "slice %u is null or unaligned", s);
        g.slices.s[s] = const_cast<uint64_t*>(d_slices[s]);
    }
    for (uint32_t i = 0; i < n_groups; ++i)
        if (!d_groups[i] || !aligned(d_groups[i])) return fail(CUBIT_ERR_INVALID, "group %u is null or unaligned", i);
    if (int rc = set_device(ctx)) return rc;
    HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n_groups * 6 * sizeof(int64_t), ctx->stream));
    if (n_rows == 0) return CUBIT_OK;  // no rows: zero counts, nothing to launch
    if (int rc = ensure_select_grouped(ctx)) return rc;
    if (int rc = ensure_tmp(ctx, padded_words(n_rows))) return rc;  // the candidate bitvector
    g.n_slices = n_slices;
    g.validity = d_validity;
    g.cand = reinterpret_cast<uint64_t*>(ctx->tmp_ids);
    g.workspace = ctx->gsel;
    EvalProgram prog{};
    if (d_filter) {  // a one-leaf program; NULL: the zero-leaf form, every row below n_rows
        prog.leaf[0] = d_filter;
        prog.n_leaves = 1;
    }
    EvalArgs a;
    if (int rc = tile_eval_args(ctx, prog, n_rows, 0, kAggTileWords, {}, a)) return rc;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kGroupBatchSelect) {  // a batch through all its passes, then the next
        GroupAggArgs qa{};
        qa.n1 = std::min(kGroupBatchSelect, n_groups - g0);
        for (uint32_t j = 0; j < kGroupBatchSum; ++j) qa.group[j] = kNoGroup;
        for (uint32_t x = 0; x < qa.n1; ++x) {
            qa.e1[x] = d_groups[g0 + x];
            qa.group[x] = g0 + x;
        }
        hipEvent_t e0, e1;
        if (int rc = timing_events(ctx, e0, e1)) return rc;
        HIP_CHECK(launch_slice_select_grouped(a, g, qa, mode, k, q, type, base,
                                              ctx->n_cus, &ctx->last_grid, d_out, ctx->stream, nullptr, e0, e1));
    }
    return CUBIT_OK;
}

}  // extern "C"

extern "C" int cubit_bitvector_eval(cubit_ctx* ctx, const uint64_t* const* d_leaves, uint32_t n_leaves,
                                    uint32_t leaf_negate, const int32_t* prog, uint32_t n_prog, uint64_t n_rows,
                                    int64_t row_base, int64_t* d_rowids, uint64_t capacity, uint64_t* d_count,
                                    uint64_t* d_result_words, uint32_t flags) {
    if (!ctx || !d_leaves || !prog || !d_count) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n_rows == 0) {  // no rows: nothing qualifies, nothing to launch
        if (int rc = set_device(ctx)) return rc;
        ctx->last_tiles = 0;
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
        return CUBIT_OK;
    }
    const bool count_only = (flags & CUBIT_SCAN_COUNT_ONLY) != 0;
    if (!count_only && !d_rowids) return fail(CUBIT_ERR_INVALID, "d_rowids is null without COUNT_ONLY");
    // postfix → expression (parse_postfix validates arity), then the emitter re-linearises it
    const PostfixParse pp = parse_postfix(d_leaves, n_leaves, leaf_negate, prog, n_prog);
    switch (pp.error) {
    case PostfixParse::kNone: break;
    case PostfixParse::kLeafRange: return fail(CUBIT_ERR_INVALID, "leaf %d out of range", pp.value);
    case PostfixParse::kUnderflow: return fail(CUBIT_ERR_INVALID, "program underflow at %u", pp.at);
    case PostfixParse::kBadOpcode: return fail(CUBIT_ERR_INVALID, "bad opcode %d", pp.value);
    default: return fail(CUBIT_ERR_INVALID, "program leaves %zu values on the stack", pp.left);
    }
    Emitter em;
    em.emit_top(pp.expr);
    if (!em.ok || em.max_depth > kMaxDepth)
        return fail(CUBIT_ERR_UNSUPPORTED, "program needs %d leaves / depth %d (max %d / %d)", count_leaves(pp.expr),
                    em.max_depth, kMaxLeaves, kMaxDepth);
    return run_eval(ctx, em.prog, n_rows, row_base, count_only ? nullptr : d_rowids, capacity, d_count, d_result_words,
                    count_only ? RunMode::kCount : RunMode::kDecode, true, (flags & CUBIT_SCAN_ORDERED) != 0,
                    (flags & CUBIT_SCAN_CHECK_CAPACITY) != 0);
}

extern "C" int cubit_gather(cubit_ctx* ctx, const void* d_col, int type, const int64_t* d_rowids,
                            const uint64_t* d_count, uint64_t max_n, int64_t row_base, int64_t* d_out) {
    if (!ctx || !d_col || !d_rowids || !d_count || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && !type_is_keyed(type))
        return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    HIP_CHECK(launch_gather(d_col, type, d_rowids, d_count, max_n, row_base, d_out, ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_narrow_i32(cubit_ctx* ctx, const int64_t* d_in, const uint64_t* d_count, uint64_t max_n,
                                int64_t offset, int32_t* d_out) {
    if (!ctx || !d_in || !d_count || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    HIP_CHECK(launch_narrow_i32(d_in, d_count, max_n, offset, d_out, ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_narrow_checked(cubit_ctx* ctx, const int64_t* d_in, const uint64_t* d_count, uint64_t max_n,
                                    int64_t offset, int width, void* d_out, uint32_t* d_overflow) {
    if (!ctx || !d_in || !d_count || !d_out || !d_overflow) return fail(CUBIT_ERR_INVALID, "null argument");
    if (width < 1 || width > 4) return fail(CUBIT_ERR_INVALID, "width %d: 1, 2, 3 or 4 bytes", width);
    CUBIT_LOCK(ctx);
    HIP_CHECK(launch_narrow_unsigned(d_in, d_count, max_n, offset, width, d_out, d_overflow, ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_narrow_i32_checked(cubit_ctx* ctx, const int64_t* d_in, const uint64_t* d_count, uint64_t max_n,
                                        int64_t offset, int32_t* d_out, uint32_t* d_overflow) {
    if (!ctx || !d_in || !d_count || !d_out || !d_overflow) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    HIP_CHECK(launch_narrow_i32(d_in, d_count, max_n, offset, d_out, ctx->stream, d_overflow));
    return CUBIT_OK;
}

extern "C" int cubit_gather_sum_product(cubit_ctx* ctx, const int64_t* d_a, const int64_t* d_b,
                                        const int64_t* d_rowids, const uint64_t* d_count, uint64_t max_n,
                                        int64_t row_base, int64_t* d_out) {
    if (!ctx || !d_a || !d_b || !d_rowids || !d_count || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    HIP_CHECK(launch_gather_sum_product(d_a, d_b, d_rowids, d_count, max_n, row_base, ctx->partials, d_out,
                                        ctx->stream));
    return CUBIT_OK;
}

// ------------------------------------------------------------------ table partition

namespace {

struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// A VARCHAR column's dictionary: its distinct strings in DuckDB's string order
// (string_type.hpp:143-206: the bytes as unsigned — std::string_view's order — then the length,
// a prefix before its extensions), string `code` = bytes[offs[code], offs[code + 1]).
struct DictData {
    std::vector<char> bytes;
    std::vector<uint64_t> offs{0};
    uint64_t fingerprint = 0;  // FNV-1a over the entries and their lengths: an index file names its dictionary
    uint64_t size() const { return offs.size() - 1; }
    std::string_view at(uint64_t code) const {
        return std::string_view(bytes.data() + offs[code], offs[code + 1] - offs[code]);
    }
    // the first code whose string is >= s (size() when none), and whether it is s
    uint64_t lower_bound(std::string_view s, bool* present) const {
        uint64_t lo = 0, hi = size();
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (at(mid) < s) lo = mid + 1;
            else hi = mid;
        }
        *present = lo < size() && at(lo) == s;
        return lo;
    }
};

struct Column {
    int type = 0;
    std::shared_ptr<const DictData> dict;  // VARCHAR: the dictionary its codes index
    // FLOAT / DOUBLE: `data` holds the comparison keys (an INT32 / INT64 column to every compare
    // kernel, key_type) and `raw` the bit patterns as registered (probes, downloads), both owned and
    // kept in step by appends and merges; raw = data for every other type
    const void* raw = nullptr;
    std::unique_ptr<DevBuf> raw_buf;
    const void* data = nullptr;        // device
    const uint64_t* validity = nullptr;  // device, padded to the table's cap_words (null = no NULLs)
    uint64_t cap_rows = 0;  // rows the owned data buffer holds (0 = caller-owned device data)
    std::vector<std::unique_ptr<DevBuf>> owned;
    // a column registered as BITPACKING segments keeps them on the device (packed bytes + the
    // group table): constant comparisons on it unpack and compare in one pass
    // (bitpacked_compare_kernel) instead of reading the plain column. Dropped when the values
    // change (appends, merges).
    std::unique_ptr<DevBuf> bp_bytes, bp_groups;
    std::unique_ptr<DevBuf> bp_vgroup;  // per 2,048-row vector: the group holding its first row
    uint64_t bp_n_groups = 0;
    // every group FOR ≤ 32 bits / CONSTANT / CONSTANT_DELTA: the widest FOR group's bits (≥ 1);
    // else 0 (launch_bitpacked_compare)
    int bp_simple_width = 0;
    void drop_packed() {
        bp_bytes.reset();
        bp_groups.reset();
        bp_vgroup.reset();
        bp_n_groups = 0;
    }
};

// the type and values the compare kernels read for a column, and the values its probes read
int ktype(const Column& c) { return key_type(c.type); }
const void* raw_of(const Column& c) { return type_is_fp(c.type) ? c.raw : c.data; }

struct Index {
    int encoding = CUBIT_INDEX_RANGE;
    bool exact_all = false;  // keys = every distinct value
    int64_t vmin = 0, vmax = 0;
    bool empty = true;       // no valid rows
    std::vector<int64_t> keys;
    std::vector<uint64_t*> bvs;  // parallel to keys
    std::vector<std::unique_ptr<DevBuf>> owned;
    uint64_t bytes = 0;
};

struct Updates {
    std::unique_ptr<DevBuf> rows, values, versions;
    std::vector<int64_t> h_rows, h_values;
    std::vector<uint64_t> h_versions;
    // NULL-ness per record (the validity column's update chain, InitializeUpdateValidity,
    // update_segment.cpp:588-600): 1 = the record's value, 0 = SET NULL. Empty / null when every
    // record carries a value.
    std::vector<uint8_t> h_valids;
    std::unique_ptr<DevBuf> valids;
    bool any_null = false;
    const uint8_t* d_valids() const { return valids ? static_cast<const uint8_t*>(valids->p) : nullptr; }
    bool valid_at(uint64_t i) const { return h_valids.empty() || h_valids[i]; }
    std::vector<uint64_t> distinct_versions;  // sorted
    uint64_t n = 0;
    bool unique_rows = true;  // one record per row (the checkpoint fast path merges the list as is)
    // distinct updated values, sorted: the update statistics the planner widens the index
    // statistics with (DuckDB's zonemaps consult update statistics the same way,
    // standard_column_data.cpp:50-57)
    std::vector<int64_t> stat_values;
    // does any record pass TransactionVersionOperator::UseInsertedVersion for this
    // transaction (id < start_time || id == transaction_id)? If not, the transaction sees
    // the base values and no patch is needed.
    bool any_visible(const cubit_txn* txn) const {
        if (!txn || distinct_versions.empty()) return false;
        if (distinct_versions.front() < txn->start_time) return true;
        return std::binary_search(distinct_versions.begin(), distinct_versions.end(), txn->transaction_id);
    }
    // Patched leaves kept across scans. A leaf's content is fixed by its predicate on this
    // column (index leaf or K0 bitvector alike), and for a reader without updates of its own
    // the visible records are a version prefix, so (predicate, prefix) names the patched
    // copy. Dropped whenever the column, its indexes or the update list change.
    struct PatchKey {
        int pred, cmp;
        int64_t c, c2;
        bool operator<(const PatchKey& o) const {
            return std::tie(pred, cmp, c, c2) < std::tie(o.pred, o.cmp, o.c, o.c2);
        }
    };
    struct Patched {
        int64_t prefix = -1;
        std::unique_ptr<DevBuf> bv;
    };
    std::map<PatchKey, Patched> cache;
    // zones holding an update record of any version (bit per zone), for the zone classes of
    // patched leaves; computed on first use for dirty_nz zones
    std::vector<uint64_t> dirty;
    uint32_t dirty_nz = 0;
};

// A kept combination of one column's bitvectors (cubit_derived.hpp): the table-owned bitvector
// that holds it and the leaf later plans put in the group's place.
struct DerivedLeaf {
    std::unique_ptr<DevBuf> bv;
    uint64_t block_bytes = 0;  // as allocated (the table's pool takes blocks of its own size only)
    Leaf leaf;
    // a chain: what it replaced, and the selectivity estimate made from it the first time a plan
    // asks (conj_selectivity; < 0 = not yet). The estimate reads the columns' zone statistics,
    // which a plan that only reads the kept leaf never needs.
    ExprP replaced;
    double sel = -1.0;
};

}  // namespace

struct cubit_table {
    cubit_ctx* ctx = nullptr;
    uint64_t n_rows = 0;
    int64_t row_base = 0;
    uint64_t nwp = 0;  // padded words
    // words allocated per table-owned bitvector (index leaves, validity): ≥ nwp, zero past the
    // rows; appends grow the table in place until nwp would exceed it (cubit_table_append)
    uint64_t cap_words = 0;
    std::map<int, Column> cols;
    std::map<int, Index> idx;
    std::map<int, Index> bins;  // CUBIT_INDEX_BINS (secondary)
    // CUBIT_INDEX_SLICED (secondary): bvs = the slices of key - vmin, least significant first (as
    // many as the bit length of vmax - vmin), keys empty
    std::map<int, Index> sliced;
    // MVCC delta
    std::unique_ptr<DevBuf> del_rows, del_ids;
    uint64_t n_del = 0;
    // Committed-delete visibility bitvector, kept across scans (CUBIT keeps deletions as a
    // maintained bitvector rather than re-deriving them per query). For a transaction with no
    // deletes of its own, the deletes in effect are exactly those with id < start_time — a
    // prefix of the id-sorted list — so the bitvector is reused while that prefix length is
    // unchanged. vis_prefix = -1: not built.
    std::vector<uint64_t> del_ids_sorted;
    std::unique_ptr<DevBuf> vis_cache;
    int64_t vis_prefix = -1;
    // Insert versions: row ranges [begin, end) appended by one transaction with its insert
    // id (ChunkConstantInfo::insert_id / ChunkVectorInfo::inserted, chunk_info.cpp); rows
    // outside every range were inserted before any snapshot. Sorted by id: for a reader
    // without inserts of its own the visible ranges are an id prefix, which also keys the
    // cached visibility bitvector (vis_ins_prefix).
    struct InsRange {
        int64_t begin, end;
        uint64_t id;
    };
    std::vector<InsRange> ins;
    std::unique_ptr<DevBuf> hidden_dev;  // invisible ranges of the last visibility build
    std::vector<int64_t> hidden_host;
    int64_t vis_ins_prefix = -1;
    std::map<int, Updates> upd;
    // scratch bitvectors (reused across scans)
    std::vector<std::unique_ptr<DevBuf>> scratch;
    size_t scratch_used = 0;
    std::unique_ptr<DevBuf> ones;  // all valid rows
    uint32_t last_leaves = 0, last_passes = 0;
    uint32_t last_form = 0;  // eval_form of the last planned program (FORM_*), 0 with last_leaves
    // the last planned program, when it is one table-owned index bitvector as it stands (no
    // complement, no patch): its per-zone counts give the decode its offsets up front
    const uint64_t* single_leaf = nullptr;
    // CUBIT_HOST_TIMING: host time of cubit_table_scan split into planning, tile offsets and
    // launch (ns, summed), printed when the table is destroyed (diagnostic)
    uint64_t host_ns[3] = {0, 0, 0};
    uint64_t host_scans = 0;
    uint32_t last_decoded = 0;  // sum_product: values of b decoded from its index (0 = gathered)
    uint64_t* dummy_count = nullptr;
    std::unique_ptr<DevBuf> dummy;
    // Zonemaps (RowGroup::CheckZonemap / CheckZonemapSegments, row_group.cpp:361-371, 407-445,
    // over bitvector zones of kZoneRows rows): per table-owned bitvector (index leaf, bin,
    // validity) a bit per zone for "no row set" (z) and "every row set" (o). Computed on the
    // first scan that reads the bitvector; dropped (drop_zones) whenever a table-owned
    // bitvector is written, grown or freed, so an entry always describes the current bits.
    struct ZoneMap {
        std::vector<uint64_t> z, o;
        bool informative = false;  // some zone is all-zero or all-one
        std::vector<uint32_t> cnt;  // set rows per zone
        // exclusive prefix of cnt on the device (nz + 1 entries), built the first time a scan of
        // this bitvector alone decodes (EvalArgs::tile_prefix); dropped with the zone map
        std::shared_ptr<DevBuf> prefix;
        std::vector<uint64_t> prefix_host;
        // decodes of this bitvector alone so far, and its row list (cubit_row_list.hpp) once the
        // second of them wrote it: off[prefix_host.back()] and lo_cnt[cnt.size()]. Dropped with the
        // zone map, or alone when the budget needs its bytes (drop_row_lists); row_lists accounts it.
        uint64_t solo_decodes = 0;
        std::shared_ptr<DevBuf> list_off, list_lo;
    };
    std::unordered_map<const uint64_t*, ZoneMap> zones;
    std::unique_ptr<DevBuf> zone_dev;  // class bytes of the bitvectors being summarised
    uint64_t zone_dev_bytes = 0;
    // per-zone statistics of raw columns (min / max of the valid rows, any / every row valid),
    // for leaves built from the column values (K0, candidate check), and the zone maps derived
    // from them per predicate; dropped with the bitvector zone maps
    struct ColZones {
        std::vector<int64_t> mn, mx;
        std::vector<uint8_t> fl;  // bit 0 = some row valid, bit 1 = every row valid
    };
    std::map<int, ColZones> col_zones;
    std::map<std::tuple<int, int, int, int64_t, int64_t>, ZoneMap> pred_zones;
    uint32_t last_live = 0, last_zones = 0;  // zones the last scan evaluated / the partition has
    bool use_packed = false;  // cubit_table_use_packed_filter (off by default: slower than K0)
    uint32_t last_packed = 0;  // leaves the last plan built straight from packed segments
    bool use_sliced = true;  // cubit_table_use_sliced
    uint32_t last_sliced = 0;  // leaves the last plan built from a bit-sliced index
    bool use_narrowing = true;  // cubit_table_use_narrowing
    uint32_t last_narrowed = 0;  // K0 leaves the last plan built only at the rows a mask kept
    std::vector<int32_t> last_narrow_cols;  // columns of the last plan's K0 leaves, in build order
    bool last_sum_packed = false;  // the last sum_product read a from its BITPACKING segments
    bool last_sum_slices = false;  // the last cubit_table_sum_product read both operands' slices …
    uint32_t last_sum_launches = 0;  // … in this many launches of the slice kernel
    bool last_agg_slices = false;  // the last cubit_table_aggregate read the column's slices
    bool last_sel_slices = false;  // the last cubit_table_select read the column's slices
    uint32_t last_sel_passes = 0;  // its passes over the slices or the probed values
    // the last cubit_table_aggregate_grouped: its path, group count and fused-kernel launches
    bool last_grouped_slices = false;
    uint32_t last_grouped_groups = 0, last_grouped_launches = 0;
    // the last cubit_table_select_grouped: its path, group count, batches and passes per batch
    bool last_gsel_slices = false;
    uint32_t last_gsel_groups = 0, last_gsel_launches = 0, last_gsel_passes = 0;
    // Derived leaves: combinations of one column's table-owned bitvectors that scans keep asking
    // for (a RANGE interval's L(hi) AND NOT L(lo), a union of EQUALITY / BINS leaves), each kept
    // as one bitvector once it has been planned often enough (derive_leaves). Dropped with the
    // zone maps (drop_zones): an entry always holds the combination of the current bits.
    DerivedCache<DerivedLeaf> derived;
    std::unordered_map<const uint64_t*, DerivedLeaf*> derived_bvs;  // the entries by their bitvectors
    bool derived_budget_set = false;  // cubit_table_set_derived_budget (else: the default share)
    // Row lists (cubit_row_list.hpp) of the bitvectors in `zones`, by bitvector: their bytes count
    // against the derived budget beside the kept bitvectors, and they go first.
    RowListBook<const uint64_t*> row_lists;
    bool use_row_lists = true;  // cubit_table_use_row_lists
    uint64_t list_scans = 0;    // decodes answered from a list
    // The free blocks of dropped derived bitvectors (cap_words words each), handed to the next
    // admission instead of a device allocation; bounded by the derived budget.
    BlockPool<void*> bv_pool;
    ~cubit_table() {
        bv_pool.clear([](void* p) { (void)hipFree(p); });
    }
};

namespace {

// A derived bitvector leaves the cache: its block waits in the table's pool when that has room
// (work queued on it is ahead of the next owner's in stream order); else the DevBuf frees it.
void pool_derived_bv(cubit_table* t, DerivedLeaf& d) {
    if (d.bv && d.bv->p && t->bv_pool.give(d.bv->p, d.block_bytes)) d.bv->p = nullptr;
}

// The pool follows the table's block size and the derived budget: free blocks of another size, or
// beyond the budget, go back to the device (a budget of 0 keeps none).
void size_bv_pool(cubit_table* t) {
    t->bv_pool.reset(std::max<uint64_t>(t->cap_words, 1) * 8, t->derived.budget(), [](void* p) { (void)hipFree(p); });
}

// A table-owned bitvector is about to be written, grown or freed: every zone map goes (they
// are recomputed on the next scan that needs them).
void drop_zones(cubit_table* t) {
    t->zones.clear();  // the row lists with them
    t->row_lists.clear();
    t->col_zones.clear();
    t->pred_zones.clear();
    // the derived leaves combine bits that are about to change: they and their use counters go,
    // their blocks wait in the pool for the next admission
    t->derived.clear([t](DerivedLeaf& d) { pool_derived_bv(t, d); });
    t->derived_bvs.clear();
}

// Every row list goes, the zone maps they hang on stay.
void drop_row_lists(cubit_table* t) {
    if (!t->row_lists.size()) return;
    for (auto& kv : t->zones) {
        kv.second.list_off.reset();
        kv.second.list_lo.reset();
    }
    t->row_lists.clear();
}

// Row lists beyond what the budget leaves beside the kept bitvectors go, the oldest first.
void shed_row_lists(cubit_table* t) {
    t->row_lists.shed(t->derived.budget(), t->derived.bytes(), [t](const uint64_t* bv) {
        auto it = t->zones.find(bv);
        if (it == t->zones.end()) return;
        it->second.list_off.reset();
        it->second.list_lo.reset();
    });
}

// A derived leaf leaves the cache: its zone map goes with it (the map is keyed by pointer, and
// the address may be handed out again). The budget is short, so every row list went first.
void forget_derived(cubit_table* t, DerivedLeaf& d) {
    drop_row_lists(t);
    const uint64_t* bv = static_cast<const uint64_t*>(d.bv->p);
    t->zones.erase(bv);
    t->derived_bvs.erase(bv);
    pool_derived_bv(t, d);
}

// The column's values or indexes changed: its patched leaves are stale.
void drop_patches(cubit_table* t, int col) {
    drop_zones(t);
    auto it = t->upd.find(col);
    if (it != t->upd.end()) it->second.cache.clear();
}

// a table-owned bitvector of cap_words words, all zero (the kernels that fill it write nwp
// words; the rest must stay zero for appends that grow into it). A caller whose next kernel on
// the stream writes the first `written` words says so, and only the rest is cleared.
int alloc_table_bv(cubit_table* t, DevBuf& b, uint64_t written = 0) {
    const uint64_t words = std::max<uint64_t>(t->cap_words, 1);
    if (hipMalloc(&b.p, words * 8) != hipSuccess) return CUBIT_ERR_OOM;
    written = std::min(written, words);
    if (written < words &&
        hipMemsetAsync(static_cast<uint64_t*>(b.p) + written, 0, (words - written) * 8, t->ctx->stream) != hipSuccess)
        return CUBIT_ERR_HIP;
    return CUBIT_OK;
}

// The same for a derived bitvector (a kept group or chain), from the table's pool when it holds a
// block: hipMalloc of a 75 MB block measured 185-200 µs and blocks the device, inside the scan that
// admits. A pooled block held another derived bitvector: words past its nwp are zero,
// as alloc_table_bv left them, and the tail is cleared here all the same.
int alloc_derived_bv(cubit_table* t, DevBuf& b, uint64_t written) {
    size_bv_pool(t);
    if (!t->bv_pool.take(&b.p)) {
        const bool first = t->bv_pool.device_allocs() == 0;
        if (int rc = alloc_table_bv(t, b, written)) return rc;
        t->bv_pool.allocated();
        // The table's first admission also takes the blocks of the next few (a repeated WHERE clause
        // over three columns keeps two or three groups and then their chain), as far as the budget
        // goes: those admissions, and every one after a write, then find a block waiting. One that
        // cannot be had is simply not pooled.
        const uint64_t bytes = t->bv_pool.block_bytes();
        for (uint64_t i = 1; first && i < kDerivedSlabBlocks && (i + 1) * bytes <= t->derived.budget(); ++i) {
            void* p = nullptr;
            if (hipMalloc(&p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                break;
            }
            t->bv_pool.allocated();
            if (!t->bv_pool.give(p, bytes)) {
                (void)hipFree(p);
                break;
            }
        }
        return CUBIT_OK;
    }
    const uint64_t words = std::max<uint64_t>(t->cap_words, 1);
    written = std::min(written, words);
    if (written < words &&
        hipMemsetAsync(static_cast<uint64_t*>(b.p) + written, 0, (words - written) * 8, t->ctx->stream) != hipSuccess)
        return CUBIT_ERR_HIP;
    return CUBIT_OK;
}

// Everything derived from the row count (scratch / ones / visibility / patched leaves, all
// nwp words): dropped when the table grows or its base changes.
void drop_derived(cubit_table* t) {
    drop_zones(t);
    t->scratch.clear();
    t->scratch_used = 0;
    t->ones.reset();
    t->vis_cache.reset();
    t->vis_prefix = -1;
    t->vis_ins_prefix = -1;
    for (auto& kv : t->upd) kv.second.cache.clear();
}

int scratch_bv(cubit_table* t, uint64_t** out) {
    if (t->scratch_used < t->scratch.size()) {
        *out = static_cast<uint64_t*>(t->scratch[t->scratch_used++]->p);
        return CUBIT_OK;
    }
    auto b = std::make_unique<DevBuf>();
    if (hipMalloc(&b->p, t->nwp * sizeof(uint64_t)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "scratch bitvector allocation failed");
    *out = static_cast<uint64_t*>(b->p);
    t->scratch.push_back(std::move(b));
    t->scratch_used++;
    return CUBIT_OK;
}

int ones_bv(cubit_table* t, const uint64_t** out) {
    if (!t->ones) {
        t->ones = std::make_unique<DevBuf>();
        if (hipMalloc(&t->ones->p, t->nwp * sizeof(uint64_t)) != hipSuccess)
            return fail(CUBIT_ERR_OOM, "ones bitvector allocation failed");
        HIP_CHECK(launch_fill_valid(static_cast<uint64_t*>(t->ones->p), t->n_rows, t->ctx->stream));
    }
    *out = static_cast<const uint64_t*>(t->ones->p);
    return CUBIT_OK;
}

// padded device copy of a validity mask (the NN bitvector: kernels read whole tiles), bits
// past n_rows cleared
int copy_validity(cubit_table* t, Column& c, const uint64_t* validity, int on_device) {
    hipStream_t s = t->ctx->stream;
    auto b = std::make_unique<DevBuf>();
    if (hipMalloc(&b->p, t->cap_words * 8) != hipSuccess) return fail(CUBIT_ERR_OOM, "validity allocation failed");
    HIP_CHECK(hipMemsetAsync(b->p, 0, t->cap_words * 8, s));
    const uint64_t nw = (t->n_rows + 63) / 64;
    HIP_CHECK(hipMemcpyAsync(b->p, validity, nw * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (t->n_rows & 63) {
        uint64_t last = 0;
        HIP_CHECK(hipMemcpyAsync(&last, static_cast<uint64_t*>(b->p) + nw - 1, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        last &= (1ull << (t->n_rows & 63)) - 1;
        HIP_CHECK(hipMemcpyAsync(static_cast<uint64_t*>(b->p) + nw - 1, &last, 8, hipMemcpyHostToDevice, s));
    }
    c.validity = static_cast<const uint64_t*>(b->p);
    c.owned.push_back(std::move(b));
    return CUBIT_OK;
}

int value_stats(cubit_table* t, const void* data, int type, const uint64_t* validity, uint64_t n,
                std::vector<int64_t>& distinct, bool want_distinct, int64_t& vmin, int64_t& vmax, bool& any,
                uint64_t* n_valid = nullptr);

// Store a column under `col`; what depended on the old one goes: its patched leaves and the zone
// maps (drop_patches), its indexes.
int install_column(cubit_table* t, int col, Column&& c) {
    t->cols[col] = std::move(c);
    drop_patches(t, col);
    t->idx.erase(col);
    t->bins.erase(col);
    t->sliced.erase(col);
    return CUBIT_OK;
}

// A column of a narrower or unsigned type code: its values (host or device) widened on the
// device into an owned INT32 / INT64 column (UINT64 columns are held as their bits, keyed).
int widen_column(cubit_table* t, Column& c, int type, const void* data, const uint64_t* validity, int on_device) {
    const TypeInfo& ti = *type_info(type);
    const uint64_t ssz = ti.size, esz = ti.col_type == CUBIT_TYPE_INT32 ? 4 : 8;
    c.type = ti.col_type;
    if (t->n_rows == 0) return CUBIT_OK;
    hipStream_t s = t->ctx->stream;
    DevBuf staged;
    const void* src = data;
    if (!on_device) {
        if (hipMalloc(&staged.p, t->n_rows * ssz) != hipSuccess) return fail(CUBIT_ERR_OOM, "column staging failed");
        HIP_CHECK(hipMemcpyAsync(staged.p, data, t->n_rows * ssz, hipMemcpyHostToDevice, s));
        src = staged.p;
    }
    auto b = std::make_unique<DevBuf>();
    if (hipMalloc(&b->p, std::max<uint64_t>(t->n_rows * esz, 16)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "column allocation failed");
    HIP_CHECK(launch_widen(src, type, t->n_rows, b->p, s));
    c.data = b->p;
    c.cap_rows = t->n_rows;
    c.owned.push_back(std::move(b));
    if (validity) {
        if (int rc = copy_validity(t, c, validity, on_device)) return rc;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return CUBIT_OK;
}

// A FLOAT / DOUBLE column: the patterns copied into an owned buffer (from host or device memory) and
// their keys computed beside them into `data`.
int fp_column(cubit_table* t, Column& c, int type, const void* data, const uint64_t* validity, int on_device) {
    const uint64_t esz = type_is32(type) ? 4 : 8;
    hipStream_t s = t->ctx->stream;
    c.type = type;
    c.raw_buf = std::make_unique<DevBuf>();
    auto keys = std::make_unique<DevBuf>();
    if (hipMalloc(&c.raw_buf->p, std::max<uint64_t>(t->n_rows * esz, 16)) != hipSuccess ||
        hipMalloc(&keys->p, std::max<uint64_t>(t->n_rows * esz, 16)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "column allocation failed");
    if (t->n_rows)
        HIP_CHECK(hipMemcpyAsync(c.raw_buf->p, data, t->n_rows * esz, on_device ? hipMemcpyDeviceToDevice
                                                                                : hipMemcpyHostToDevice, s));
    HIP_CHECK(launch_fp_keys(c.raw_buf->p, type, t->n_rows, keys->p, s));
    c.raw = c.raw_buf->p;
    c.data = keys->p;
    c.cap_rows = t->n_rows;
    c.owned.push_back(std::move(keys));
    if (validity) {
        if (int rc = copy_validity(t, c, validity, on_device)) return rc;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return CUBIT_OK;
}

int copy_column(cubit_table* t, Column& c, int type, const void* data, const uint64_t* validity, int on_device) {
    if (type_is_fp(type)) return fp_column(t, c, type, data, validity, on_device);
    if (type != CUBIT_TYPE_INT32 && type != CUBIT_TYPE_INT64 && type != CUBIT_TYPE_VARCHAR && !type_is_keyed(type))
        return widen_column(t, c, type, data, validity, on_device);
    const uint64_t esz = type_is32(type) ? 4 : 8;  // FLOAT / DOUBLE: the bit patterns as they are
    if (t->n_rows == 0) {  // empty partition: nothing to copy
        c.type = type;
        c.data = on_device ? data : nullptr;
        return CUBIT_OK;
    }
    hipStream_t s = t->ctx->stream;
    if (on_device) {
        c.data = data;
    } else {
        auto b = std::make_unique<DevBuf>();
        if (hipMalloc(&b->p, std::max<uint64_t>(t->n_rows * esz, 16)) != hipSuccess)
            return fail(CUBIT_ERR_OOM, "column allocation failed");
        HIP_CHECK(hipMemcpyAsync(b->p, data, t->n_rows * esz, hipMemcpyHostToDevice, s));
        c.data = b->p;
        c.cap_rows = t->n_rows;
        c.owned.push_back(std::move(b));
    }
    if (validity) {
        if (int rc = copy_validity(t, c, validity, on_device)) return rc;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    c.type = type;
    return CUBIT_OK;
}

std::vector<int64_t> distinct_sorted(const int64_t* v, uint64_t n);

// an exact index over a span ≥ 2^32 keeps at most this many keys (one bitvector each)
constexpr size_t kMaxWideDistinct = 1 << 16;

// Index-build statistics on the device: min / max / any valid, and (want_distinct) the
// distinct valid values through a presence bitmap of vmax - vmin + 1 bits when the span is
// below 2^32, else by sorting the valid values on the host.
int value_stats(cubit_table* t, const void* data, int type, const uint64_t* validity, uint64_t n,
                std::vector<int64_t>& distinct, bool want_distinct, int64_t& vmin, int64_t& vmax, bool& any,
                uint64_t* n_valid) {
    Column c;
    c.type = type;
    c.data = data;
    c.validity = validity;
    DevBuf stats;
    if (hipMalloc(&stats.p, 3 * sizeof(int64_t)) != hipSuccess) return fail(CUBIT_ERR_OOM, "stats allocation failed");
    int64_t h[3] = {INT64_MAX, INT64_MIN, 0};
    HIP_CHECK(hipMemcpyAsync(stats.p, h, sizeof(h), hipMemcpyHostToDevice, t->ctx->stream));
    HIP_CHECK(launch_column_minmax(c.data, c.type, c.validity, n, static_cast<int64_t*>(stats.p), t->ctx->stream));
    HIP_CHECK(hipMemcpyAsync(h, stats.p, sizeof(h), hipMemcpyDeviceToHost, t->ctx->stream));
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    any = h[2] > 0;
    if (n_valid) *n_valid = (uint64_t)h[2];
    vmin = h[0];
    vmax = h[1];
    if (!want_distinct) return CUBIT_OK;
    distinct.clear();
    if (!any) return CUBIT_OK;
    const uint64_t span = (uint64_t)vmax - (uint64_t)vmin;  // no signed overflow
    if (span >= (1ull << 32)) {
        // a wide span (TIMESTAMP microseconds, BIGINT ids) over few distinct values: sort the
        // valid values on the host instead (only INT64 and DOUBLE columns get here: a DOUBLE's
        // patterns become their keys first)
        std::vector<int64_t> hv(n);
        std::vector<uint64_t> hvalid(validity ? (n + 63) / 64 : 0);
        HIP_CHECK(hipMemcpyAsync(hv.data(), data, n * 8, hipMemcpyDeviceToHost, t->ctx->stream));
        if (validity)
            HIP_CHECK(hipMemcpyAsync(hvalid.data(), validity, hvalid.size() * 8, hipMemcpyDeviceToHost,
                                     t->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
        if (validity) {
            uint64_t k = 0;
            for (uint64_t i = 0; i < n; ++i)
                if ((hvalid[i >> 6] >> (i & 63)) & 1) hv[k++] = hv[i];
            hv.resize(k);
        }
        if (type == CUBIT_TYPE_UINT64)  // (a DOUBLE column's `data` already holds keys)
            for (int64_t& v : hv) v = value_key(type, v);
        distinct = distinct_sorted(hv.data(), hv.size());
        if (distinct.size() > kMaxWideDistinct)
            return fail(CUBIT_ERR_UNSUPPORTED, "%zu distinct values over a span of 2^32 or more; give keys",
                        distinct.size());
        return CUBIT_OK;
    }
    const uint64_t range = span + 1;
    const uint64_t nw = (range + 63) / 64;
    DevBuf bits;
    if (hipMalloc(&bits.p, nw * 8) != hipSuccess) return fail(CUBIT_ERR_OOM, "presence bitmap allocation failed");
    HIP_CHECK(hipMemsetAsync(bits.p, 0, nw * 8, t->ctx->stream));
    HIP_CHECK(launch_presence(c.data, c.type, c.validity, n, vmin, range, static_cast<uint64_t*>(bits.p),
                              t->ctx->stream));
    std::vector<uint64_t> hb(nw);
    HIP_CHECK(hipMemcpyAsync(hb.data(), bits.p, nw * 8, hipMemcpyDeviceToHost, t->ctx->stream));
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    for (uint64_t w = 0; w < nw; ++w)
        for (uint64_t x = hb[w]; x; x &= x - 1) distinct.push_back(vmin + (int64_t)(w * 64 + __builtin_ctzll(x)));
    return CUBIT_OK;
}

int column_stats(cubit_table* t, const Column& c, std::vector<int64_t>& distinct, bool want_distinct,
                 int64_t& vmin, int64_t& vmax, bool& any, uint64_t* n_valid = nullptr) {
    return value_stats(t, c.data, ktype(c), c.validity, t->n_rows, distinct, want_distinct, vmin, vmax, any, n_valid);
}

}  // namespace

extern "C" int cubit_table_create(cubit_ctx* ctx, uint64_t n_rows, int64_t row_base, cubit_table** out) {
    if (!ctx || !out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    // n_rows = 0 is an empty partition (an empty table, or a rank with no rows): every scan
    // of it returns no rows without a launch
    if (n_rows >= (1ull << 47)) return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_rows);
    if (int rc = set_device(ctx)) return rc;
    auto* t = new cubit_table();
    t->ctx = ctx;
    t->n_rows = n_rows;
    t->row_base = row_base;
    t->nwp = padded_words(n_rows);
    t->cap_words = t->nwp;
    t->dummy = std::make_unique<DevBuf>();
    if (hipMalloc(&t->dummy->p, 64) != hipSuccess) {
        delete t;
        return fail(CUBIT_ERR_OOM, "allocation failed");
    }
    t->dummy_count = static_cast<uint64_t*>(t->dummy->p);
    *out = t;
    return CUBIT_OK;
}

bool host_timing() {
    static const bool on = std::getenv("CUBIT_HOST_TIMING") != nullptr;
    return on;
}
// CUBIT_SYNC_TIMING: cubit_table_sync_column prints its phases (host time, the stream synchronised
// at each boundary) on stderr (diagnostic; scripts/sync_timing.py)
bool sync_timing() {
    static const bool on = std::getenv("CUBIT_SYNC_TIMING") != nullptr;
    return on;
}
uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

extern "C" int cubit_table_destroy(cubit_table* t) {
    if (!t) return CUBIT_OK;
    CUBIT_LOCK(t->ctx);
    if (host_timing() && t->host_scans)
        std::fprintf(stderr, "cubit host timing: %llu scans; per scan plan %.2f us, tile offsets %.2f us, launch %.2f us\n",
                     (unsigned long long)t->host_scans, t->host_ns[0] * 1e-3 / t->host_scans,
                     t->host_ns[1] * 1e-3 / t->host_scans, t->host_ns[2] * 1e-3 / t->host_scans);
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    delete t;
    return CUBIT_OK;
}

extern "C" int cubit_table_add_column(cubit_table* t, int col, int type, const void* data, const uint64_t* validity,
                                      int on_device) {
    if (!t || !data) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (!type_info(type)) return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (type == CUBIT_TYPE_VARCHAR)
        return fail(CUBIT_ERR_INVALID, "a VARCHAR column is registered with its dictionary (cubit_table_add_dict_column)");
    if (col < 0) return fail(CUBIT_ERR_INVALID, "column %d", col);
    if (int rc = set_device(t->ctx)) return rc;
    Column c;
    if (int rc = copy_column(t, c, type, data, validity, on_device)) return rc;
    return install_column(t, col, std::move(c));
}

// ------------------------------------------------------------------ VARCHAR dictionaries

struct cubit_dict {
    std::shared_ptr<const DictData> d;
};

extern "C" int cubit_dict_create(const char* bytes, const uint64_t* offsets, uint64_t n, cubit_dict** out) {
    if (!out || (n && (!offsets || (!bytes && offsets[n] > offsets[0])))) return fail(CUBIT_ERR_INVALID, "null argument");
    std::vector<std::string_view> v;
    v.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(CUBIT_ERR_INVALID, "offsets descend at string %llu", (unsigned long long)i);
        v.emplace_back(bytes + offsets[i], offsets[i + 1] - offsets[i]);
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() > (uint64_t)INT32_MAX) return fail(CUBIT_ERR_UNSUPPORTED, "%zu distinct strings exceed 2^31 - 1", v.size());
    auto d = std::make_shared<DictData>();
    uint64_t total = 0;
    for (auto sv : v) total += sv.size();
    d->bytes.reserve(total);
    d->offs.reserve(v.size() + 1);
    for (auto sv : v) {
        d->bytes.insert(d->bytes.end(), sv.begin(), sv.end());
        d->offs.push_back(d->bytes.size());
    }
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t b) { h = (h ^ b) * 1099511628211ull; };
    for (auto sv : v) {
        mix(sv.size());
        for (char c : sv) mix((unsigned char)c);
    }
    d->fingerprint = h;
    *out = new cubit_dict{std::move(d)};
    return CUBIT_OK;
}

extern "C" int cubit_dict_destroy(cubit_dict* d) {
    delete d;
    return CUBIT_OK;
}

extern "C" int cubit_dict_size(const cubit_dict* d, uint64_t* n) {
    if (!d || !n) return fail(CUBIT_ERR_INVALID, "null argument");
    *n = d->d->size();
    return CUBIT_OK;
}

extern "C" int cubit_dict_entry(const cubit_dict* d, uint64_t code, const char** data, uint64_t* size) {
    if (!d || !data || !size) return fail(CUBIT_ERR_INVALID, "null argument");
    if (code >= d->d->size()) return fail(CUBIT_ERR_INVALID, "code %llu past the dictionary's %llu strings",
                                          (unsigned long long)code, (unsigned long long)d->d->size());
    const std::string_view sv = d->d->at(code);
    *data = sv.data();
    *size = sv.size();
    return CUBIT_OK;
}

extern "C" int cubit_dict_encode(const cubit_dict* d, const char* bytes, const uint64_t* offsets, uint64_t n,
                                 const uint64_t* validity, int32_t* codes) {
    if (!d || (n && (!offsets || !codes))) return fail(CUBIT_ERR_INVALID, "null argument");
    for (uint64_t i = 0; i < n; ++i) {
        if (validity && !((validity[i >> 6] >> (i & 63)) & 1ull)) {
            codes[i] = 0;
            continue;
        }
        if (offsets[i + 1] < offsets[i]) return fail(CUBIT_ERR_INVALID, "offsets descend at string %llu", (unsigned long long)i);
        bool present = false;
        const uint64_t c = d->d->lower_bound(std::string_view(bytes + offsets[i], offsets[i + 1] - offsets[i]), &present);
        if (!present) return fail(CUBIT_ERR_UNSUPPORTED, "string %llu is not in the dictionary", (unsigned long long)i);
        codes[i] = (int32_t)c;
    }
    return CUBIT_OK;
}

// cubit_dict_encode on the device: the dictionary's entries are copied to the context's device
// for the call, one lane per string searches them (dict_encode_kernel).
extern "C" int cubit_dict_encode_device(cubit_ctx* ctx, const cubit_dict* d, const char* d_bytes,
                                        const uint64_t* d_offsets, uint64_t n, const uint64_t* d_validity,
                                        int32_t* d_codes) {
    if (!ctx || !d || (n && (!d_offsets || !d_codes))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(ctx);
    if (n == 0) return CUBIT_OK;
    if (int rc = set_device(ctx)) return rc;
    const DictData& dd = *d->d;
    hipStream_t s = ctx->stream;
    DevBuf db, doffs, miss;
    if (hipMalloc(&db.p, std::max<uint64_t>(dd.bytes.size(), 16)) != hipSuccess ||
        hipMalloc(&doffs.p, dd.offs.size() * 8) != hipSuccess || hipMalloc(&miss.p, 8) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "dictionary upload failed");
    if (!dd.bytes.empty()) HIP_CHECK(hipMemcpyAsync(db.p, dd.bytes.data(), dd.bytes.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(doffs.p, dd.offs.data(), dd.offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(miss.p, 0, 8, s));
    HIP_CHECK(launch_dict_encode(reinterpret_cast<const uint8_t*>(d_bytes), d_offsets, n, d_validity,
                                 static_cast<const uint8_t*>(db.p), static_cast<const uint64_t*>(doffs.p), dd.size(),
                                 d_codes, static_cast<unsigned long long*>(miss.p), s));
    unsigned long long missing = 0;
    HIP_CHECK(hipMemcpyAsync(&missing, miss.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (missing)
        return fail(CUBIT_ERR_UNSUPPORTED, "%llu strings are not in the dictionary (their codes are -1)", missing);
    return CUBIT_OK;
}

extern "C" int cubit_dict_lookup(const cubit_dict* d, const char* data, uint64_t size, uint64_t* lower_bound,
                                 int* present) {
    if (!d || !lower_bound || (size && !data)) return fail(CUBIT_ERR_INVALID, "null argument");
    bool p = false;
    *lower_bound = d->d->lower_bound(std::string_view(data ? data : "", size), &p);
    if (present) *present = p ? 1 : 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_add_dict_column(cubit_table* t, int col, cubit_dict* d, const int32_t* codes,
                                           const uint64_t* validity, int on_device) {
    if (!t || !d || (!codes && t->n_rows)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (col < 0) return fail(CUBIT_ERR_INVALID, "column %d", col);
    if (int rc = set_device(t->ctx)) return rc;
    Column c;
    if (int rc = copy_column(t, c, CUBIT_TYPE_VARCHAR, codes, validity, on_device)) return rc;
    c.dict = d->d;
    if (t->n_rows) {  // every valid code names a dictionary string
        std::vector<int64_t> unused;
        int64_t vmin = 0, vmax = 0;
        bool any = false;
        if (int rc = value_stats(t, c.data, CUBIT_TYPE_VARCHAR, c.validity, t->n_rows, unused, false, vmin, vmax, any))
            return rc;
        if (any && (vmin < 0 || (uint64_t)vmax >= c.dict->size()))
            return fail(CUBIT_ERR_INVALID, "code %lld outside the dictionary's %llu strings",
                        (long long)(vmin < 0 ? vmin : vmax), (unsigned long long)c.dict->size());
    }
    return install_column(t, col, std::move(c));
}

namespace {
// codes handed to a VARCHAR column (updates, appends): each valid one must name a dictionary string
int check_codes(const Column& c, const int64_t* v, const uint8_t* valid, uint64_t n) {
    if (c.type != CUBIT_TYPE_VARCHAR) return CUBIT_OK;
    for (uint64_t i = 0; i < n; ++i)
        if ((!valid || valid[i]) && (v[i] < 0 || (uint64_t)v[i] >= c.dict->size()))
            return fail(CUBIT_ERR_INVALID, "code %lld outside the dictionary's %llu strings", (long long)v[i],
                        (unsigned long long)c.dict->size());
    return CUBIT_OK;
}
}  // namespace

// ------------------------------------------------------------------ columns given as DuckDB segments
// The three entry points below share one path: a plan of what the segments ask of the device
// (SegmentPlan, cubit_segments.hpp: walked and bounds-checked on the host), one build that uploads
// it and launches a stage for each part the plan has, and install_column. A call refused at any
// point leaves the table as it was.

namespace {

// The plan of a column's segments: segment i has codec seg_codecs[i], or `codec` for all when
// seg_codecs is null. With seg_codecs every segment adds its runs to the one run list: a CONSTANT
// segment one run of its value, an RLE segment its runs, the others a placeholder run that their
// stage writes over. Ends with the segments' rows checked against the partition's.
int plan_segments(const cubit_table* t, const TypeInfo& ti, const uint8_t* bytes, uint64_t n_bytes,
                  const uint64_t* seg_offsets, const uint64_t* seg_rows, const int32_t* seg_codecs, int codec,
                  const int64_t* seg_constants, uint32_t n_segments, SegmentPlan& p) {
    const uint64_t bytes_padded = (n_bytes + 15) / 16 * 16;
    char err[192];
    for (uint32_t sg = 0; sg < n_segments; ++sg) {
        const uint64_t rows = seg_rows[sg], row = p.rows;
        if (seg_codecs) codec = seg_codecs[sg];
        if (codec != CUBIT_CODEC_CONSTANT && (!bytes || seg_offsets[sg] > n_bytes))
            return fail(CUBIT_ERR_INVALID, "segment %u: bad offset", sg);
        int64_t run = 0;  // the placeholder
        switch (codec) {
        case CUBIT_CODEC_CONSTANT:
            if (!seg_constants) return fail(CUBIT_ERR_INVALID, "segment %u: CONSTANT without a value", sg);
            run = seg_constants[sg];
            p.rows += rows;
            break;
        case CUBIT_CODEC_RLE:
            if (int rc = walk_rle_segment(bytes, n_bytes, seg_offsets[sg], rows, ti, sg, p, err, sizeof(err)))
                return fail(rc, "%s", err);
            continue;  // its own runs
        case CUBIT_CODEC_BITPACKING:
            if (int rc = walk_bp_segment(bytes, n_bytes, seg_offsets[sg], rows, ti, bytes_padded, sg, p, err, sizeof(err)))
                return fail(rc, "%s", err);
            break;
        case CUBIT_CODEC_UNCOMPRESSED:
            if (seg_offsets[sg] % ti.size || rows * ti.size > n_bytes - seg_offsets[sg])
                return fail(CUBIT_ERR_INVALID, "segment %u: %llu values past the bytes", sg, (unsigned long long)rows);
            p.plain.push_back({seg_offsets[sg], rows, row});
            p.rows += rows;
            break;
        default:
            return fail(CUBIT_ERR_UNSUPPORTED, "segment %u: codec %d", sg, codec);
        }
        if (seg_codecs) {
            p.vals.push_back(run);
            p.ends.push_back(row + rows);
        }
    }
    if (p.rows != t->n_rows)
        return fail(CUBIT_ERR_INVALID, "segments hold %llu rows, partition has %llu", (unsigned long long)p.rows,
                    (unsigned long long)t->n_rows);
    return CUBIT_OK;
}

// The column of a plan, built in stream order, each stage only when the plan has something for it:
// rle_expand_kernel writes the runs, bitunpack_kernel (K5) unpacks the BITPACKING groups over their
// rows, the UNCOMPRESSED spans are copied (INT32, INT64, UINT64: the values as held) or widened over
// theirs. With timing on, the start event goes to the first kernel and the stop event to the last,
// or behind the last span. `type` is the segments' T, `bytes` the caller's segment bytes (read only
// by the groups and spans), `what` names the entry point in an allocation failure.
// keep_packed: the column keeps the bytes, the group records and the group of each 2,048-row
// vector's first row (SumArgs::a_vgroup) for the packed filter and the packed fused sum.
int build_segment_column(cubit_table* t, int type, const TypeInfo& ti, const SegmentPlan& p, const uint8_t* bytes,
                         uint64_t n_bytes, const uint64_t* validity, bool keep_packed, const char* what, Column& c) {
    if (int rc = set_device(t->ctx)) return rc;
    hipStream_t s = t->ctx->stream;
    const bool wide = ti.col_type != CUBIT_TYPE_INT32;
    const uint64_t esz = wide ? 8 : 4;
    const uint64_t bytes_padded = (n_bytes + 15) / 16 * 16;
    const bool has_runs = !p.ends.empty(), has_groups = !p.groups.empty(), has_plain = !p.plain.empty();
    std::vector<int32_t> narrow;
    if (!wide) narrow.assign(p.vals.begin(), p.vals.end());
    const uint64_t n_tiles = (t->n_rows + 2047) / 2048;
    std::vector<uint32_t> vgroup;
    if (keep_packed) {
        vgroup.assign(std::max<uint64_t>(n_tiles, 1), 0);
        for (uint64_t v = 0, g = 0; v < n_tiles; ++v) {
            while (g + 1 < p.groups.size() && p.groups[g].row_start + p.groups[g].count <= v * 2048) ++g;
            vgroup[v] = (uint32_t)g;
        }
    }
    DevBuf d_vals, d_ends, d_tiles;
    auto out = std::make_unique<DevBuf>(), d_bytes = std::make_unique<DevBuf>(), d_groups = std::make_unique<DevBuf>(),
         d_vgroup = std::make_unique<DevBuf>();
    // bytes + 16: the kernels stage packed words with 16-byte-aligned loads that may run past the end
    if (hipMalloc(&out->p, std::max<uint64_t>(t->n_rows * esz, 16)) != hipSuccess ||
        (has_runs && (hipMalloc(&d_vals.p, std::max<uint64_t>(p.vals.size() * esz, 16)) != hipSuccess ||
                      hipMalloc(&d_ends.p, std::max<uint64_t>(p.ends.size() * 8, 16)) != hipSuccess ||
                      hipMalloc(&d_tiles.p, (n_tiles + 1) * 8) != hipSuccess)) ||
        ((has_groups || has_plain) && hipMalloc(&d_bytes->p, bytes_padded + p.moved.size() + 16) != hipSuccess) ||
        (has_groups && hipMalloc(&d_groups->p, p.groups.size() * sizeof(BpGroup)) != hipSuccess) ||
        (keep_packed && hipMalloc(&d_vgroup->p, vgroup.size() * 4) != hipSuccess))
        return fail(CUBIT_ERR_OOM, "%s column allocation failed", what);
    if (has_runs) {
        HIP_CHECK(hipMemcpyAsync(d_vals.p, wide ? (const void*)p.vals.data() : (const void*)narrow.data(),
                                 p.vals.size() * esz, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_ends.p, p.ends.data(), p.ends.size() * 8, hipMemcpyHostToDevice, s));
    }
    if (has_groups || has_plain) {
        HIP_CHECK(hipMemcpyAsync(d_bytes->p, bytes, n_bytes, hipMemcpyHostToDevice, s));
        if (!p.moved.empty())
            HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(d_bytes->p) + bytes_padded, p.moved.data(), p.moved.size(),
                                     hipMemcpyHostToDevice, s));
    }
    if (has_groups)
        HIP_CHECK(hipMemcpyAsync(d_groups->p, p.groups.data(), p.groups.size() * sizeof(BpGroup), hipMemcpyHostToDevice, s));
    if (keep_packed) HIP_CHECK(hipMemcpyAsync(d_vgroup->p, vgroup.data(), vgroup.size() * 4, hipMemcpyHostToDevice, s));
    hipEvent_t e0, e1;
    if (int rc = timing_events(t->ctx, e0, e1)) return rc;
    if (has_runs)
        HIP_CHECK(launch_rle_expand(d_vals.p, static_cast<const uint64_t*>(d_ends.p), p.ends.size(), t->n_rows, wide ? 1 : 0,
                                    static_cast<uint64_t*>(d_tiles.p), out->p, s, e0, has_groups || has_plain ? nullptr : e1));
    if (has_groups)
        HIP_CHECK(launch_bitunpack(static_cast<const uint8_t*>(d_bytes->p), static_cast<const BpGroup*>(d_groups->p),
                                   p.groups.size(), ti.col_type, out->p, s, has_runs ? nullptr : e0, has_plain ? nullptr : e1));
    for (const SegmentPlan::Span& pl : p.plain) {
        const uint8_t* src = static_cast<const uint8_t*>(d_bytes->p) + pl.off;
        uint8_t* dst = static_cast<uint8_t*>(out->p) + pl.row * esz;
        if (ti.size == esz)
            HIP_CHECK(hipMemcpyAsync(dst, src, pl.rows * esz, hipMemcpyDeviceToDevice, s));
        else
            HIP_CHECK(launch_widen(src, type, pl.rows, dst, s));
    }
    if (e1 && has_plain) HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipStreamSynchronize(s));
    c.type = ti.col_type;
    c.data = out->p;
    c.cap_rows = t->n_rows;
    c.owned.push_back(std::move(out));
    if (keep_packed) {
        c.bp_bytes = std::move(d_bytes);
        c.bp_groups = std::move(d_groups);
        c.bp_vgroup = std::move(d_vgroup);
        c.bp_n_groups = p.groups.size();
        c.bp_simple_width = 0;
        if (std::all_of(p.groups.begin(), p.groups.end(), [](const BpGroup& g) {
                return g.mode == 2 || g.mode == 3 || (g.mode == 5 && g.width <= 32);
            })) {
            int wmax = 1;
            for (const BpGroup& g : p.groups)
                if (g.mode == 5) wmax = std::max<int>(wmax, g.width);
            c.bp_simple_width = wmax;
        }
    }
    if (validity) {
        if (int rc = copy_validity(t, c, validity, 0)) return rc;
        HIP_CHECK(hipStreamSynchronize(s));
    }
    return CUBIT_OK;
}

}  // namespace

// DuckDB BITPACKING segments → device column: bitunpack_kernel alone, and the column keeps the
// packed form.
extern "C" int cubit_table_add_bitpacked_column(cubit_table* t, int col, int type, const uint8_t* bytes,
                                                uint64_t n_bytes, const uint64_t* seg_offsets,
                                                const uint64_t* seg_rows, uint32_t n_segments,
                                                const uint64_t* validity) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    const TypeInfo* ti = segment_type(type);
    if (!ti) return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (col < 0) return fail(CUBIT_ERR_INVALID, "column %d", col);
    Column c;
    if (t->n_rows == 0 && n_segments == 0) {  // empty partition, no segments
        c.type = ti->col_type;
        return install_column(t, col, std::move(c));
    }
    if (!bytes || !seg_offsets || !seg_rows || n_segments == 0) return fail(CUBIT_ERR_INVALID, "null argument");
    SegmentPlan p;
    if (int rc = plan_segments(t, *ti, bytes, n_bytes, seg_offsets, seg_rows, nullptr, CUBIT_CODEC_BITPACKING, nullptr,
                               n_segments, p))
        return rc;
    if (int rc = build_segment_column(t, type, *ti, p, bytes, n_bytes, validity, true, "bitpacked", c)) return rc;
    return install_column(t, col, std::move(c));
}

// DuckDB RLE segments → device column: only the runs cross to the device, rle_expand_kernel writes
// the column.
extern "C" int cubit_table_add_rle_column(cubit_table* t, int col, int type, const uint8_t* bytes, uint64_t n_bytes,
                                          const uint64_t* seg_offsets, const uint64_t* seg_rows, uint32_t n_segments,
                                          const uint64_t* validity) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    const TypeInfo* ti = segment_type(type);
    if (!ti) return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (col < 0) return fail(CUBIT_ERR_INVALID, "column %d", col);
    if (n_segments && (!bytes || !seg_offsets || !seg_rows)) return fail(CUBIT_ERR_INVALID, "null argument");
    SegmentPlan p;
    Column c;
    if (int rc = plan_segments(t, *ti, bytes, n_bytes, seg_offsets, seg_rows, nullptr, CUBIT_CODEC_RLE, nullptr,
                               n_segments, p))
        return rc;
    if (int rc = build_segment_column(t, type, *ti, p, bytes, n_bytes, validity, false, "RLE", c)) return rc;
    return install_column(t, col, std::move(c));
}

// A column given as DuckDB segments of mixed codecs, one per row group as DuckDB's checkpoint chose
// (UNCOMPRESSED, CONSTANT, RLE, BITPACKING); bytes may be null when every segment is CONSTANT. The
// packed form is not kept, even when every segment is BITPACKING.
extern "C" int cubit_table_add_segment_column(cubit_table* t, int col, int type, const uint8_t* bytes, uint64_t n_bytes,
                                              const uint64_t* seg_offsets, const uint64_t* seg_rows,
                                              const int32_t* seg_codecs, const int64_t* seg_constants,
                                              uint32_t n_segments, const uint64_t* validity) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    const TypeInfo* ti = segment_type(type);
    if (!ti) return fail(CUBIT_ERR_UNSUPPORTED, "type %d", type);
    if (col < 0) return fail(CUBIT_ERR_INVALID, "column %d", col);
    if (n_segments && (!seg_offsets || !seg_rows || !seg_codecs)) return fail(CUBIT_ERR_INVALID, "null argument");
    SegmentPlan p;
    Column c;
    if (int rc = plan_segments(t, *ti, bytes, n_bytes, seg_offsets, seg_rows, seg_codecs, 0, seg_constants, n_segments, p))
        return rc;
    if (int rc = build_segment_column(t, type, *ti, p, bytes, n_bytes, validity, false, "segment", c)) return rc;
    return install_column(t, col, std::move(c));
}

namespace {

// The bitvectors of an index whose keys are chosen (ix: encoding, keys ascending and distinct, the
// column's statistics): K0 over the column, one pass per kMultiKeys bitvectors. Installs the index.
int build_index_bitvectors(cubit_table* t, int col, const Column& c, Index&& ix) {
    const int encoding = ix.encoding;
    const size_t n_bv = encoding == CUBIT_INDEX_BINS ? ix.keys.size() - 1 : ix.keys.size();
    // one pass of the column per kMultiKeys bitvectors
    const int cmp = encoding == CUBIT_INDEX_BINS ? kCmpBetween : encoding == CUBIT_INDEX_RANGE ? CUBIT_CMP_LT : CUBIT_CMP_EQ;
    for (size_t k0 = 0; k0 < n_bv; k0 += kMultiKeys) {
        MultiKeyArgs mk{};
        for (size_t k = k0; k < std::min(n_bv, k0 + kMultiKeys); ++k) {
            auto b = std::make_unique<DevBuf>();
            if (int rc = alloc_table_bv(t, *b))
                return fail(rc, "index bitvector allocation failed after %zu of %zu", ix.bvs.size(), n_bv);
            mk.c[mk.m] = ix.keys[k];
            mk.c2[mk.m] = encoding == CUBIT_INDEX_BINS ? ix.keys[k + 1] : 0;
            mk.out[mk.m] = static_cast<uint64_t*>(b->p);
            ++mk.m;
            ix.bvs.push_back(static_cast<uint64_t*>(b->p));
            ix.owned.push_back(std::move(b));
            ix.bytes += t->cap_words * 8;
        }
        HIP_CHECK(launch_compare_bitvectors(c.data, ktype(c), c.validity, t->n_rows, cmp, mk, t->ctx->stream));
    }
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    drop_patches(t, col);
    if (encoding == CUBIT_INDEX_BINS) t->bins[col] = std::move(ix);
    else t->idx[col] = std::move(ix);
    return CUBIT_OK;
}

// ---- bit-sliced index (CUBIT_INDEX_SLICED): bvs = the slices of key - vmin

SliceSet slice_set(const Index& ix) {
    SliceSet s{};
    for (size_t k = 0; k < ix.bvs.size() && k < kMaxSlices; ++k) s.s[k] = ix.bvs[k];
    return s;
}

// all-zero high slices until the index holds n of them (rows already sliced have 0 there)
int sliced_grow(cubit_table* t, Index& ix, uint32_t n) {
    while (ix.bvs.size() < n) {
        auto b = std::make_unique<DevBuf>();
        if (int rc = alloc_table_bv(t, *b)) return fail(rc, "slice allocation failed after %zu of %u", ix.bvs.size(), n);
        ix.bvs.push_back(static_cast<uint64_t*>(b->p));
        ix.owned.push_back(std::move(b));
    }
    ix.bytes = ix.owned.size() * t->cap_words * 8;
    return CUBIT_OK;
}

// The slices of a column as it stands (n_rows rows), base = its smallest valid key: one build.
// `into` keeps its bitvectors where their count allows (a rebuild after maintenance).
int build_sliced(cubit_table* t, const Column& c, uint64_t n_rows, Index& into) {
    Index& ix = into;
    ix.encoding = CUBIT_INDEX_SLICED;
    ix.exact_all = false;
    ix.keys.clear();
    bool any = false;
    if (n_rows) {
        std::vector<int64_t> distinct;
        if (int rc = value_stats(t, c.data, ktype(c), c.validity, n_rows, distinct, false, ix.vmin, ix.vmax, any)) return rc;
    }
    ix.empty = !any;
    const uint32_t bits = any ? sliced_bits(ix.vmin, ix.vmax) : 0;
    if (ix.bvs.size() > bits) {  // a narrower span: the high slices go
        ix.bvs.resize(bits);
        ix.owned.resize(bits);
    }
    if (int rc = sliced_grow(t, ix, bits)) return rc;
    if (bits) {
        hipEvent_t e0, e1;
        if (int rc = timing_events(t->ctx, e0, e1)) return rc;
        HIP_CHECK(launch_bitslice_build(c.data, ktype(c), c.validity, n_rows, ix.vmin, bits, slice_set(ix), t->ctx->stream,
                                        e0, e1));
    }
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    return CUBIT_OK;
}

// Take the slices instead of K0's pass over the column when they move fewer bytes: the compare
// reads b slices and the validity and writes one bitvector, (b + 2)/8 bytes per row, where K0 reads
// the column's element. From traffic alone (b < 30 on a 4-byte column, b < 62 on an 8-byte one), and
// the measurement agrees: both kernels stream at the same rate, 12 and 24 slices take 0.40 of K0's
// time at 612 M rows and 64 slices of an 8-byte column tie with it (DESIGN.md §3,
// scripts/sliced_timing.py).
bool sliced_moves_fewer_bytes(uint32_t bits, uint64_t elem_bytes) { return bits + 2 < 8 * elem_bytes; }
// (its counterpart for cubit_table_aggregate, aggregate_from_slices, is in cubit_program.hpp, where
// the CPU test of the path rule reaches it)

// CUBIT_QUANTILE_PLAIN_ADDS: the histogram passes without the wave-level pre-aggregation
// (diagnostic; scripts/quantile_timing.py times both forms)
bool quantile_wave_agg() {
    static const bool on = std::getenv("CUBIT_QUANTILE_PLAIN_ADDS") == nullptr;
    return on;
}

// Equi-depth edges of a column with m > 0 valid rows whose keys span [vmin, vmax]:
// q[j - 1] = k[(j·m) / n_bins] for j = 1 … n_bins - 1, k the valid rows' keys in ascending order.
// A radix select for all n_bins - 1 ranks at once over u = key - vmin, most significant bits first
// (launch_quantile_hist): after each pass the host walks the counters (≤ 128 KiB) once, finds each
// rank's bucket and its rank inside the bucket, and hands the distinct buckets to the next pass as
// its active prefixes. Passes: 1 + ⌈(bits - 12) / d⌉, d = ⌊log2(16,384 / active prefixes)⌋ ≥ 4.
// With timing on, each pass is a timed launch.
int quantile_keys(cubit_table* t, const Column& c, uint32_t n_bins, int64_t vmin, int64_t vmax, uint64_t m,
                  std::vector<int64_t>& q) {
    cubit_ctx* ctx = t->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t span = (uint64_t)vmax - (uint64_t)vmin;  // no signed overflow
    const uint32_t bits = span ? 64 - (uint32_t)__builtin_clzll(span) : 0;
    const size_t nt = n_bins - 1;
    std::vector<uint64_t> prefix(nt, 0), rank(nt), active, next, h(kQuantileCounters);
    for (size_t j = 0; j < nt; ++j) rank[j] = (uint64_t)(j + 1) * m / n_bins;  // m < 2^47, j < 2^10
    DevBuf d_counts, d_pre;
    if (hipMalloc(&d_counts.p, kQuantileCounters * 8) != hipSuccess ||
        hipMalloc(&d_pre.p, (kQuantileMaxActive + 1) * 8) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "quantile counters allocation failed");
    uint32_t consumed = 0;
    do {
        const bool first = consumed == 0;
        QuantileHistArgs a{};
        a.vmin = vmin;
        a.bits = bits;
        a.consumed = consumed;
        a.n_active = first ? 0 : (uint32_t)active.size();
        a.d = first ? std::min(bits, kQuantileD0) : quantile_pass_bits(a.n_active, bits - consumed);
        a.prefixes = static_cast<const uint64_t*>(d_pre.p);
        a.counts = static_cast<uint64_t*>(d_counts.p);
        const size_t per = (size_t)1 << a.d, blocks = first ? 1 : active.size();
        if (!first) HIP_CHECK(hipMemcpyAsync(d_pre.p, active.data(), active.size() * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_counts.p, 0, blocks * per * 8, s));
        hipEvent_t e0, e1;
        if (int rc = timing_events(ctx, e0, e1)) return rc;
        HIP_CHECK(launch_quantile_hist(c.data, ktype(c), c.validity, t->n_rows, a, ctx->n_cus, s, e0, e1,
                                       quantile_wave_agg()));
        HIP_CHECK(hipMemcpyAsync(h.data(), d_counts.p, blocks * per * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (first) {  // every valid row falls into one pass-0 counter
            uint64_t total = 0;
            for (size_t b = 0; b < per; ++b) total += h[b];
            if (total != m)
                return fail(CUBIT_ERR_DEVICE, "quantile pass 0 counted %llu rows, the column has %llu valid",
                            (unsigned long long)total, (unsigned long long)m);
        }
        // ranks ascend, so the targets under one prefix are consecutive and their buckets ascend
        next.clear();
        size_t j = 0;
        for (size_t i = 0; i < blocks; ++i) {
            const uint64_t* cnt = h.data() + i * per;
            uint64_t below = 0;  // rows of this prefix in the buckets before b
            size_t b = 0;
            for (; j < nt && (first || prefix[j] == active[i]); ++j) {
                while (b < per && below + cnt[b] <= rank[j]) below += cnt[b++];
                if (b == per)
                    return fail(CUBIT_ERR_DEVICE, "quantile pass at bit %u: a rank lies past the counted rows", consumed);
                prefix[j] = (prefix[j] << a.d) | b;
                rank[j] -= below;  // now its rank among the rows of bucket b
                if (next.empty() || next.back() != prefix[j]) next.push_back(prefix[j]);
            }
        }
        if (j != nt) return fail(CUBIT_ERR_DEVICE, "quantile pass at bit %u: a prefix went missing", consumed);
        active.swap(next);
        consumed += a.d;
    } while (consumed < bits);
    q.resize(nt);
    for (size_t j = 0; j < nt; ++j) q[j] = (int64_t)((uint64_t)vmin + prefix[j]);
    return CUBIT_OK;
}

}  // namespace

extern "C" int cubit_table_build_index(cubit_table* t, int col, int encoding, const int64_t* values, uint32_t n) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    auto it = t->cols.find(col);
    if (it == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (encoding != CUBIT_INDEX_RANGE && encoding != CUBIT_INDEX_EQUALITY && encoding != CUBIT_INDEX_BINS &&
        encoding != CUBIT_INDEX_SLICED)
        return fail(CUBIT_ERR_INVALID, "encoding %d", encoding);
    if (encoding == CUBIT_INDEX_BINS && (n < 2 || !values)) return fail(CUBIT_ERR_INVALID, "bins need >= 2 edges");
    if (encoding == CUBIT_INDEX_SLICED && n) return fail(CUBIT_ERR_INVALID, "a bit-sliced index takes no keys");
    if (n && !values) return fail(CUBIT_ERR_INVALID, "values is null");
    if (int rc = set_device(t->ctx)) return rc;
    const Column& c = it->second;
    if (encoding == CUBIT_INDEX_SLICED) {  // an empty partition or no valid row: an empty index, no slices
        Index ix;
        if (int rc = build_sliced(t, c, t->n_rows, ix)) return rc;
        drop_patches(t, col);
        t->sliced[col] = std::move(ix);
        return CUBIT_OK;
    }
    // a FLOAT / DOUBLE column's keys are given as bit patterns and held as their comparison keys
    // (-0.0 and +0.0, or two NaNs, become one key)
    std::vector<int64_t> keyed;
    if (n && type_is_keyed(c.type)) {
        keyed.resize(n);
        for (uint32_t k = 0; k < n; ++k) keyed[k] = value_key(c.type, values[k]);
        values = keyed.data();
    }
    // a VARCHAR column's keys are given as addresses of cubit_strings and held as the code bound
    // each names (the first code whose string is >= the key: exact for every key of RANGE and BINS,
    // and an EQUALITY key absent from the dictionary becomes a bitvector of its neighbour's code)
    if (n && c.type == CUBIT_TYPE_VARCHAR) {
        keyed.resize(n);
        for (uint32_t k = 0; k < n; ++k) {
            const cubit_string* str = reinterpret_cast<const cubit_string*>((intptr_t)values[k]);
            if (!str || (str->size && !str->data)) return fail(CUBIT_ERR_INVALID, "VARCHAR key %u is not a cubit_string", k);
            bool present = false;
            keyed[k] = (int64_t)c.dict->lower_bound(std::string_view(str->data ? str->data : "", str->size), &present);
        }
        values = keyed.data();
    }
    Index ix;
    ix.encoding = encoding;
    if (t->n_rows == 0) {  // empty partition: an empty index (scans of it launch nothing)
        ix.empty = true;
        ix.exact_all = n == 0;  // every distinct value of no rows; appends keep it exact
        if (n) ix.keys.assign(values, values + n);
        if (n && !std::is_sorted(ix.keys.begin(), ix.keys.end()))
            return fail(CUBIT_ERR_INVALID, "index keys must be sorted ascending");
        ix.keys.erase(std::unique(ix.keys.begin(), ix.keys.end()), ix.keys.end());
        if (encoding == CUBIT_INDEX_BINS && ix.keys.size() < 2) return fail(CUBIT_ERR_INVALID, "bins need >= 2 edges");
        drop_patches(t, col);
        if (encoding == CUBIT_INDEX_BINS) t->bins[col] = std::move(ix);
        else t->idx[col] = std::move(ix);
        return CUBIT_OK;
    }
    std::vector<int64_t> distinct;
    bool any = false;
    if (int rc = column_stats(t, c, distinct, n == 0, ix.vmin, ix.vmax, any)) return rc;
    ix.empty = !any;
    if (n == 0) {
        ix.exact_all = true;
        ix.keys = distinct;
        // range encoding: L(min) is empty, keep keys above the minimum
        if (encoding == CUBIT_INDEX_RANGE && !ix.keys.empty()) ix.keys.erase(ix.keys.begin());
    } else {
        ix.keys.assign(values, values + n);
        if (!std::is_sorted(ix.keys.begin(), ix.keys.end()))
            return fail(CUBIT_ERR_INVALID, "index keys must be sorted ascending");
        ix.keys.erase(std::unique(ix.keys.begin(), ix.keys.end()), ix.keys.end());
        if (encoding == CUBIT_INDEX_BINS && ix.keys.size() < 2) return fail(CUBIT_ERR_INVALID, "bins need >= 2 edges");
    }
    return build_index_bitvectors(t, col, c, std::move(ix));
}

extern "C" int cubit_table_build_index_quantiles(cubit_table* t, int col, int encoding, uint32_t n_bins, int64_t* keys,
                                                 uint32_t cap, uint32_t* n_keys) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    auto it = t->cols.find(col);
    if (it == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (encoding != CUBIT_INDEX_RANGE && encoding != CUBIT_INDEX_BINS)
        return fail(CUBIT_ERR_INVALID, "quantile edges serve a RANGE or BINS index, not encoding %d", encoding);
    if (n_bins < 2 || n_bins > kQuantileMaxActive + 1) return fail(CUBIT_ERR_INVALID, "%u bins (2 … 1,024)", n_bins);
    if (cap && !keys) return fail(CUBIT_ERR_INVALID, "keys is null");
    if (int rc = set_device(t->ctx)) return rc;
    const Column& c = it->second;
    Index ix;
    ix.encoding = encoding;
    std::vector<int64_t> distinct, q;
    bool any = false;
    uint64_t m = 0;
    if (t->n_rows) {
        if (int rc = column_stats(t, c, distinct, false, ix.vmin, ix.vmax, any, &m)) return rc;
        if (any)
            if (int rc = quantile_keys(t, c, n_bins, ix.vmin, ix.vmax, m, q)) return rc;
    }
    ix.empty = !any;
    if (encoding == CUBIT_INDEX_RANGE) {
        // L(min) is empty: the edges above the minimum. One distinct value or no valid row: no
        // bitvector, and that is every distinct value, as the n = 0 form of cubit_table_build_index
        for (int64_t k : q)
            if (k > ix.vmin && (ix.keys.empty() || k != ix.keys.back())) ix.keys.push_back(k);
        ix.exact_all = !any || ix.vmin == ix.vmax;
    } else {
        if (!any) return fail(CUBIT_ERR_INVALID, "bins need a valid row");
        // the edge above the maximum, as a key the column's type can carry back: none past INT64_MAX,
        // and a FLOAT / DOUBLE's next pattern is taken through its key (past +inf: the NaN key; the
        // NaN key stays, as INT64_MAX does)
        const int64_t top = ix.vmax == INT64_MAX ? ix.vmax : value_key(c.type, cubit_fp_value(c.type, ix.vmax + 1));
        ix.keys.push_back(ix.vmin);
        for (int64_t k : q)
            if (k != ix.keys.back()) ix.keys.push_back(k);
        if (top != ix.keys.back()) ix.keys.push_back(top);
        if (ix.keys.size() < 2) return fail(CUBIT_ERR_INVALID, "bins need >= 2 edges: the column holds one value that nothing follows");
    }
    const std::vector<int64_t> chosen = ix.keys;
    if (int rc = build_index_bitvectors(t, col, c, std::move(ix))) return rc;
    if (n_keys) *n_keys = (uint32_t)chosen.size();
    for (size_t k = 0; k < chosen.size() && k < cap; ++k) keys[k] = cubit_fp_value(c.type, chosen[k]);
    return CUBIT_OK;
}

extern "C" int cubit_table_index_info(cubit_table* t, int col, uint32_t* n_bitvectors, uint64_t* bytes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    uint32_t nb = 0;
    uint64_t by = 0;
    for (auto* m : {&t->idx, &t->bins, &t->sliced}) {
        auto it = m->find(col);
        if (it != m->end()) {
            nb += (uint32_t)it->second.bvs.size();
            by += it->second.bytes;
        }
    }
    if (n_bitvectors) *n_bitvectors = nb;
    if (bytes) *bytes = by;
    return CUBIT_OK;
}

// ------------------------------------------------------------------ index persistence

namespace {

constexpr char kIndexMagic[8] = {'C', 'U', 'B', 'I', 'T', 'I', 'X', '1'};

struct IndexFileHeader {
    char magic[8];
    uint32_t version;
    uint32_t encoding;
    uint64_t n_rows;
    uint64_t nwp;
    uint32_t exact_all;
    uint32_t empty;
    int64_t vmin;
    int64_t vmax;
    uint64_t n_keys;
    uint64_t n_bv;
};
static_assert(sizeof(IndexFileHeader) == 72, "stable on-disk header");
// version 2 appends what the keys and leaves are relative to: the column's type (keys of FLOAT /
// DOUBLE are comparison keys, of VARCHAR / HUGEINT codes) and, for a dictionary column, its
// dictionary's fingerprint — codes of another dictionary would name other strings. A version-1
// file (no tail) loads onto a column that is not a dictionary column.
struct IndexFileTail {
    int32_t col_type;
    uint32_t reserved;
    uint64_t dict_fingerprint;
};
static_assert(sizeof(IndexFileTail) == 16, "stable on-disk tail");

}  // namespace

extern "C" int cubit_table_save_index(cubit_table* t, int col, int encoding, const char* path) {
    if (!t || !path) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    const Index* ix = nullptr;
    if (encoding == CUBIT_INDEX_BINS) {
        auto it = t->bins.find(col);
        if (it != t->bins.end()) ix = &it->second;
    } else if (encoding == CUBIT_INDEX_SLICED) {
        auto it = t->sliced.find(col);
        if (it != t->sliced.end()) ix = &it->second;
    } else {
        auto it = t->idx.find(col);
        if (it != t->idx.end() && it->second.encoding == encoding) ix = &it->second;
    }
    if (!ix) return fail(CUBIT_ERR_INVALID, "column %d has no index of encoding %d", col, encoding);
    if (int rc = set_device(t->ctx)) return rc;
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(CUBIT_ERR_INVALID, "cannot open %s for writing", path);
    IndexFileHeader h{};
    std::memcpy(h.magic, kIndexMagic, 8);
    h.version = 2;
    const Column& sc = t->cols.at(col);
    const IndexFileTail tail{sc.type, 0u, sc.dict ? sc.dict->fingerprint : 0ull};
    h.encoding = (uint32_t)ix->encoding;
    h.n_rows = t->n_rows;
    h.nwp = t->nwp;
    h.exact_all = ix->exact_all ? 1u : 0u;
    h.empty = ix->empty ? 1u : 0u;
    h.vmin = ix->vmin;
    h.vmax = ix->vmax;
    h.n_keys = ix->keys.size();
    h.n_bv = ix->bvs.size();
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1 && std::fwrite(&tail, sizeof(tail), 1, f) == 1 &&
              (h.n_keys == 0 || std::fwrite(ix->keys.data(), 8, h.n_keys, f) == h.n_keys);
    std::vector<uint64_t> host(ok ? t->nwp : 0);
    for (size_t k = 0; ok && k < ix->bvs.size(); ++k) {
        if (hipMemcpyAsync(host.data(), ix->bvs[k], t->nwp * 8, hipMemcpyDeviceToHost, t->ctx->stream) != hipSuccess ||
            hipStreamSynchronize(t->ctx->stream) != hipSuccess) {
            std::fclose(f);
            return fail(CUBIT_ERR_HIP, "index download failed");
        }
        ok = std::fwrite(host.data(), 8, t->nwp, f) == t->nwp;
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? CUBIT_OK : fail(CUBIT_ERR_INVALID, "short write to %s", path);
}

extern "C" int cubit_table_load_index(cubit_table* t, int col, const char* path) {
    if (!t || !path) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (!t->cols.count(col)) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (int rc = set_device(t->ctx)) return rc;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(CUBIT_ERR_INVALID, "cannot open %s", path);
    auto bad = [&](const char* why) {
        std::fclose(f);
        return fail(CUBIT_ERR_INVALID, "%s: %s", path, why);
    };
    IndexFileHeader h{};
    if (std::fread(&h, sizeof(h), 1, f) != 1 || std::memcmp(h.magic, kIndexMagic, 8) != 0 ||
        (h.version != 1 && h.version != 2))
        return bad("not a cubit index file");
    const Column& lc = t->cols.at(col);
    if (h.version == 2) {
        IndexFileTail tail{};
        if (std::fread(&tail, sizeof(tail), 1, f) != 1) return bad("truncated header");
        if (tail.col_type != lc.type) return bad("index was built on a column of another type");
        if (tail.dict_fingerprint != (lc.dict ? lc.dict->fingerprint : 0ull))
            return bad("index was built against another dictionary");
    } else if (lc.dict) {
        return bad("a version-1 index file does not name its dictionary");
    } else if (lc.type != CUBIT_TYPE_INT32 && lc.type != CUBIT_TYPE_INT64) {
        // version 1 predates the typed columns: its keys are raw values, where a UBIGINT, FLOAT or
        // DOUBLE index is keyed by comparison keys
        return bad("a version-1 index file holds raw-value keys, this column's type needs comparison keys");
    }
    if (h.n_rows != t->n_rows || h.nwp != t->nwp) return bad("index was built for a partition of another size");
    if (h.encoding > CUBIT_INDEX_SLICED) return bad("unknown encoding");
    // a bit-sliced index holds no keys and one slice per bit of vmax - vmin (none without a valid row)
    const uint64_t want_bv = h.encoding == CUBIT_INDEX_SLICED ? (h.empty ? 0 : sliced_bits(h.vmin, h.vmax))
                             : h.encoding == CUBIT_INDEX_BINS ? (h.n_keys ? h.n_keys - 1 : 0)
                                                              : h.n_keys;
    if (h.n_bv != want_bv || h.n_keys > (1ull << 32) || (h.encoding == CUBIT_INDEX_SLICED && h.n_keys))
        return bad("inconsistent header");
    Index ix;
    ix.encoding = (int)h.encoding;
    ix.exact_all = h.exact_all != 0;
    ix.empty = h.empty != 0;
    ix.vmin = h.vmin;
    ix.vmax = h.vmax;
    ix.keys.resize(h.n_keys);
    if (h.n_keys && std::fread(ix.keys.data(), 8, h.n_keys, f) != h.n_keys) return bad("truncated keys");
    if (!std::is_sorted(ix.keys.begin(), ix.keys.end())) return bad("keys not sorted");
    std::vector<uint64_t> host(t->nwp);
    for (uint64_t k = 0; k < h.n_bv; ++k) {
        if (std::fread(host.data(), 8, t->nwp, f) != t->nwp) return bad("truncated bitvectors");
        auto b = std::make_unique<DevBuf>();
        if (alloc_table_bv(t, *b)) {
            std::fclose(f);
            return fail(CUBIT_ERR_OOM, "index bitvector allocation failed");
        }
        // on the context stream, behind alloc_table_bv's memset; host is refilled by the next read
        if (hipMemcpyAsync(b->p, host.data(), t->nwp * 8, hipMemcpyHostToDevice, t->ctx->stream) != hipSuccess ||
            hipStreamSynchronize(t->ctx->stream) != hipSuccess) {
            std::fclose(f);
            return fail(CUBIT_ERR_HIP, "index upload failed");
        }
        ix.bvs.push_back(static_cast<uint64_t*>(b->p));
        ix.owned.push_back(std::move(b));
        ix.bytes += t->cap_words * 8;
    }
    std::fclose(f);
    drop_patches(t, col);
    if (ix.encoding == CUBIT_INDEX_BINS) t->bins[col] = std::move(ix);
    else if (ix.encoding == CUBIT_INDEX_SLICED) t->sliced[col] = std::move(ix);
    else t->idx[col] = std::move(ix);
    return CUBIT_OK;
}

extern "C" int cubit_table_set_deletes(cubit_table* t, const int64_t* rows, const uint64_t* ids, uint64_t n) {
    if (!t || (n && (!rows || !ids))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (int rc = set_device(t->ctx)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || (uint64_t)rows[i] >= t->n_rows) return fail(CUBIT_ERR_INVALID, "delete row out of range");
    t->del_rows = std::make_unique<DevBuf>();
    t->del_ids = std::make_unique<DevBuf>();
    if (hipMalloc(&t->del_rows->p, std::max<uint64_t>(n, 1) * 8) != hipSuccess ||
        hipMalloc(&t->del_ids->p, std::max<uint64_t>(n, 1) * 8) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "delete list allocation failed");
    if (n) {
        HIP_CHECK(hipMemcpyAsync(t->del_rows->p, rows, n * 8, hipMemcpyHostToDevice, t->ctx->stream));
        HIP_CHECK(hipMemcpyAsync(t->del_ids->p, ids, n * 8, hipMemcpyHostToDevice, t->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(t->ctx->stream));  // rows / ids are the caller's
    }
    t->n_del = n;
    t->del_ids_sorted.assign(ids, ids + n);
    std::sort(t->del_ids_sorted.begin(), t->del_ids_sorted.end());
    t->vis_prefix = -1;
    return CUBIT_OK;
}

extern "C" int cubit_table_set_inserts(cubit_table* t, const int64_t* row_begin, const int64_t* row_end,
                                       const uint64_t* ids, uint64_t n) {
    if (!t || (n && (!row_begin || !row_end || !ids))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    std::vector<cubit_table::InsRange> r(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (row_begin[i] < 0 || row_begin[i] >= row_end[i] || (uint64_t)row_end[i] > t->n_rows)
            return fail(CUBIT_ERR_INVALID, "insert range %llu out of range", (unsigned long long)i);
        r[i] = {row_begin[i], row_end[i], ids[i]};
    }
    std::sort(r.begin(), r.end(), [](const auto& a, const auto& b) { return a.begin < b.begin; });
    for (uint64_t i = 1; i < n; ++i)
        if (r[i].begin < r[i - 1].end) return fail(CUBIT_ERR_INVALID, "insert ranges overlap");
    std::stable_sort(r.begin(), r.end(), [](const auto& a, const auto& b) { return a.id < b.id; });
    t->ins = std::move(r);
    t->vis_prefix = -1;
    t->vis_ins_prefix = -1;
    return CUBIT_OK;
}

namespace {

// The distinct values of v, ascending. Update lists hold millions of records over few
// distinct values: a presence bitmap over [min, max] when that span is small, else sort.
std::vector<int64_t> distinct_sorted(const int64_t* v, uint64_t n) {
    std::vector<int64_t> out;
    if (n == 0) return out;
    const auto mm = std::minmax_element(v, v + n);
    const uint64_t span = (uint64_t)*mm.second - (uint64_t)*mm.first;
    if (span < (1ull << 26)) {
        std::vector<uint64_t> bits(span / 64 + 1, 0);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t d = (uint64_t)v[i] - (uint64_t)*mm.first;
            bits[d >> 6] |= 1ull << (d & 63);
        }
        for (uint64_t w = 0; w < bits.size(); ++w)
            for (uint64_t x = bits[w]; x; x &= x - 1)
                out.push_back((int64_t)((uint64_t)*mm.first + w * 64 + (uint64_t)__builtin_ctzll(x)));
        return out;
    }
    out.assign(v, v + n);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

// store an update list (rows, values, versions, and NULL-ness when valids is not null) for col:
// records grouped by row, each row's records kept in chronological order (UpdateInfo chains,
// update_info.hpp)
int store_updates(cubit_table* t, int col, const int64_t* rows, const int64_t* values, const uint64_t* versions,
                  uint64_t n, const uint8_t* valids = nullptr) {
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    if (!std::is_sorted(rows, rows + n))  // grouping keeps each row's records in list order
        std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return rows[x] < rows[y]; });
    Updates u;
    u.n = n;
    const int type = t->cols.at(col).type;
    for (uint64_t i = 0; valids && i < n; ++i) u.any_null |= valids[i] == 0;
    u.h_rows.reserve(n);
    u.h_values.reserve(n);
    u.h_versions.reserve(n);
    for (uint64_t i : order) {
        if (!u.h_rows.empty() && u.h_rows.back() == rows[i]) u.unique_rows = false;
        u.h_rows.push_back(rows[i]);
        // a FLOAT value is its 32-bit pattern, zero-extended (as the probe hands it back)
        u.h_values.push_back(type == CUBIT_TYPE_FLOAT ? (int64_t)(uint32_t)values[i] : values[i]);
        u.h_versions.push_back(versions[i]);
        if (u.any_null) u.h_valids.push_back(valids[i] ? 1 : 0);
    }
    {
        const auto dv = distinct_sorted(reinterpret_cast<const int64_t*>(u.h_versions.data()), n);
        // versions are unsigned: distinct_sorted ordered them as signed, restore unsigned order
        u.distinct_versions.assign(dv.begin(), dv.end());
        std::sort(u.distinct_versions.begin(), u.distinct_versions.end());
    }
    {  // the statistics cover the records that carry a value (FLOAT / DOUBLE: their keys)
        std::vector<int64_t> vv;
        vv.reserve(n);
        for (uint64_t i = 0; i < n; ++i)
            if (u.valid_at(i)) vv.push_back(value_key(type, u.h_values[i]));
        u.stat_values = distinct_sorted(vv.data(), vv.size());
    }
    hipStream_t s = t->ctx->stream;
    u.rows = std::make_unique<DevBuf>();
    u.values = std::make_unique<DevBuf>();
    u.versions = std::make_unique<DevBuf>();
    if (hipMalloc(&u.rows->p, std::max<uint64_t>(n, 1) * 8) != hipSuccess ||
        hipMalloc(&u.values->p, std::max<uint64_t>(n, 1) * 8) != hipSuccess ||
        hipMalloc(&u.versions->p, std::max<uint64_t>(n, 1) * 8) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "update list allocation failed");
    if (n) {
        HIP_CHECK(hipMemcpyAsync(u.rows->p, u.h_rows.data(), n * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(u.values->p, u.h_values.data(), n * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(u.versions->p, u.h_versions.data(), n * 8, hipMemcpyHostToDevice, s));
    }
    if (u.any_null) {
        u.valids = std::make_unique<DevBuf>();
        if (hipMalloc(&u.valids->p, n) != hipSuccess) return fail(CUBIT_ERR_OOM, "update list allocation failed");
        HIP_CHECK(hipMemcpyAsync(u.valids->p, u.h_valids.data(), n, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));  // uploaded on return, and a failed copy is reported here
    t->upd[col] = std::move(u);
    return CUBIT_OK;
}

}  // namespace

extern "C" int cubit_table_set_updates(cubit_table* t, int col, const int64_t* rows, const int64_t* values,
                                       const uint64_t* versions, uint64_t n) {
    if (!t || (n && (!rows || !values || !versions))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (!t->cols.count(col)) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (int rc = set_device(t->ctx)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || (uint64_t)rows[i] >= t->n_rows) return fail(CUBIT_ERR_INVALID, "update row out of range");
    if (int rc = check_codes(t->cols.at(col), values, nullptr, n)) return rc;
    return store_updates(t, col, rows, values, versions, n);
}

namespace {

// A validity bitvector for a column registered without one (every row valid): a SET NULL
// record, visible or merged, needs the NN leaf to patch or flip (the planner folds IS NOT NULL on
// a column without validity to TRUE).
int ensure_validity(cubit_table* t, Column& c) {
    if (c.validity) return CUBIT_OK;
    auto b = std::make_unique<DevBuf>();
    if (int rc = alloc_table_bv(t, *b)) return fail(rc, "validity allocation failed");
    if (t->n_rows) HIP_CHECK(launch_fill_valid(static_cast<uint64_t*>(b->p), t->n_rows, t->ctx->stream));
    c.validity = static_cast<const uint64_t*>(b->p);
    c.owned.push_back(std::move(b));
    drop_zones(t);
    return CUBIT_OK;
}

}  // namespace

extern "C" int cubit_table_set_updates_nullable(cubit_table* t, int col, const int64_t* rows, const int64_t* values,
                                                const uint8_t* valid, const uint64_t* versions, uint64_t n) {
    if (!t || (n && (!rows || !values || !versions))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (int rc = set_device(t->ctx)) return rc;
    bool any_null = false;
    for (uint64_t i = 0; i < n; ++i) {
        if (rows[i] < 0 || (uint64_t)rows[i] >= t->n_rows) return fail(CUBIT_ERR_INVALID, "update row out of range");
        any_null |= valid && !valid[i];
    }
    if (int rc = check_codes(cit->second, values, valid, n)) return rc;
    if (any_null)
        if (int rc = ensure_validity(t, cit->second)) return rc;
    return store_updates(t, col, rows, values, versions, n, any_null ? valid : nullptr);
}

// ------------------------------------------------------------------ index maintenance

namespace {

// Every table-owned bitvector (index leaves, bins, validity) grown to `words` words: copy the
// nwp words in use, zero the rest. Index leaf pointers change, so everything derived from them
// (patched leaves, scratch) is dropped by the caller.
int grow_bitvectors(cubit_table* t, uint64_t words) {
    drop_zones(t);
    t->bv_pool.clear([](void* p) { (void)hipFree(p); });  // blocks of the old size
    hipStream_t s = t->ctx->stream;
    auto regrow = [&](void*& p) -> int {
        void* np = nullptr;
        if (hipMalloc(&np, words * 8) != hipSuccess) return fail(CUBIT_ERR_OOM, "bitvector growth failed");
        HIP_CHECK(hipMemsetAsync(np, 0, words * 8, s));
        if (p && t->nwp) HIP_CHECK(hipMemcpyAsync(np, p, t->nwp * 8, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (p) (void)hipFree(p);
        p = np;
        return CUBIT_OK;
    };
    for (auto* m : {&t->idx, &t->bins, &t->sliced}) {
        for (auto& kv : *m) {
            Index& ix = kv.second;
            for (size_t k = 0; k < ix.owned.size(); ++k) {
                if (int rc = regrow(ix.owned[k]->p)) return rc;
                ix.bvs[k] = static_cast<uint64_t*>(ix.owned[k]->p);
            }
            ix.bytes = ix.owned.size() * words * 8;
        }
    }
    for (auto& kv : t->cols) {
        Column& c = kv.second;
        if (!c.validity) continue;
        for (auto& b : c.owned) {
            if (b->p != (const void*)c.validity) continue;
            if (int rc = regrow(b->p)) return rc;
            c.validity = static_cast<const uint64_t*>(b->p);
            break;
        }
    }
    t->cap_words = words;
    return CUBIT_OK;
}

// an owned data buffer of at least `rows` rows holding the column's first n_rows values
int own_column(cubit_table* t, Column& c, uint64_t rows) {
    if (c.cap_rows >= rows && c.cap_rows) return CUBIT_OK;
    const uint64_t esz = type_is32(c.type) ? 4 : 8;
    auto b = std::make_unique<DevBuf>();
    if (hipMalloc(&b->p, std::max<uint64_t>(rows * esz, 16)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "column allocation failed");
    if (c.data && t->n_rows)
        HIP_CHECK(hipMemcpyAsync(b->p, c.data, t->n_rows * esz, hipMemcpyDeviceToDevice, t->ctx->stream));
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    // release the old owned data buffer (not the validity buffer)
    for (auto it = c.owned.begin(); it != c.owned.end(); ++it)
        if ((*it)->p == c.data) {
            c.owned.erase(it);
            break;
        }
    c.data = b->p;
    c.cap_rows = rows;
    c.owned.push_back(std::move(b));
    if (type_is_fp(c.type)) {  // the patterns grow beside the keys
        auto r = std::make_unique<DevBuf>();
        if (hipMalloc(&r->p, std::max<uint64_t>(rows * esz, 16)) != hipSuccess)
            return fail(CUBIT_ERR_OOM, "column allocation failed");
        if (t->n_rows)
            HIP_CHECK(hipMemcpyAsync(r->p, c.raw, t->n_rows * esz, hipMemcpyDeviceToDevice, t->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
        c.raw_buf = std::move(r);
        c.raw = c.raw_buf->p;
    }
    return CUBIT_OK;
}

// The keys an exact_all index must hold after the column gained the values `added` (sorted,
// distinct, all valid): RANGE keeps every distinct value but the minimum, EQUALITY every
// distinct value. Missing keys get full-column bitvectors (the column already holds its new
// values); more than kMaxNewKeys missing keys turn the index into an edges index instead
// (exact for its keys, the candidate check for other constants).
constexpr size_t kMaxNewKeys = 64;
int maintain_exact_keys(cubit_table* t, int col, Index& ix, const std::vector<int64_t>& added, int64_t old_min,
                        bool was_empty) {
    if (!ix.exact_all || ix.encoding == CUBIT_INDEX_BINS || added.empty()) return CUBIT_OK;
    std::vector<int64_t> want;  // keys the index must hold
    if (ix.encoding == CUBIT_INDEX_RANGE) {
        // old distinct values ⊆ keys ∪ {old_min}; the new minimum needs no key
        if (!was_empty && old_min > ix.vmin) want.push_back(old_min);
        for (int64_t v : added)
            if (v > ix.vmin) want.push_back(v);
    } else {
        want = added;
    }
    std::vector<int64_t> missing;
    for (int64_t v : want)
        if (!std::binary_search(ix.keys.begin(), ix.keys.end(), v)) missing.push_back(v);
    std::sort(missing.begin(), missing.end());
    missing.erase(std::unique(missing.begin(), missing.end()), missing.end());
    if (missing.empty()) return CUBIT_OK;
    if (missing.size() > kMaxNewKeys) {
        ix.exact_all = false;
        return CUBIT_OK;
    }
    const Column& c = t->cols.at(col);
    const int cmp = ix.encoding == CUBIT_INDEX_RANGE ? CUBIT_CMP_LT : CUBIT_CMP_EQ;
    std::vector<std::pair<int64_t, std::unique_ptr<DevBuf>>> fresh;
    for (size_t k0 = 0; k0 < missing.size(); k0 += kMultiKeys) {
        MultiKeyArgs mk{};
        for (size_t k = k0; k < std::min(missing.size(), k0 + kMultiKeys); ++k) {
            auto b = std::make_unique<DevBuf>();
            if (int rc = alloc_table_bv(t, *b)) return fail(rc, "index bitvector allocation failed");
            mk.c[mk.m] = missing[k];
            mk.out[mk.m] = static_cast<uint64_t*>(b->p);
            ++mk.m;
            fresh.emplace_back(missing[k], std::move(b));
        }
        HIP_CHECK(launch_compare_bitvectors(c.data, ktype(c), c.validity, t->n_rows, cmp, mk, t->ctx->stream));
    }
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    // merge into the sorted key list (keys, bvs and owned stay parallel)
    std::vector<int64_t> keys;
    std::vector<uint64_t*> bvs;
    std::vector<std::unique_ptr<DevBuf>> owned;
    size_t i = 0, j = 0;
    std::vector<std::unique_ptr<DevBuf>> old_owned = std::move(ix.owned);
    while (i < ix.keys.size() || j < fresh.size()) {
        if (j == fresh.size() || (i < ix.keys.size() && ix.keys[i] < fresh[j].first)) {
            keys.push_back(ix.keys[i]);
            bvs.push_back(ix.bvs[i]);
            owned.push_back(std::move(old_owned[i]));
            ++i;
        } else {
            keys.push_back(fresh[j].first);
            bvs.push_back(static_cast<uint64_t*>(fresh[j].second->p));
            owned.push_back(std::move(fresh[j].second));
            ++j;
        }
    }
    ix.keys = std::move(keys);
    ix.bvs = std::move(bvs);
    ix.owned = std::move(owned);
    ix.bytes = ix.owned.size() * t->cap_words * 8;
    return CUBIT_OK;
}

// bitvectors an index of this encoding holds for its keys
size_t index_bv_count(const Index& ix) {
    return ix.encoding == CUBIT_INDEX_BINS ? (ix.keys.size() >= 2 ? ix.keys.size() - 1 : 0) : ix.keys.size();
}

}  // namespace

// Append rows to the partition (RowGroupCollection::Append + every BoundIndex::Append,
// bound_index.hpp:67-70): the new rows get local ids n_rows … n_rows + n_new - 1. Values are
// host arrays, one per registered column (cols[i] names the column of data[i]); validity[i]
// (LSB-first words for the appended rows, bit 0 = first appended row) may be null = all valid.
// Every index of every column is maintained incrementally: the index-build compare kernel runs
// over the appended slice only and its words are spliced into each bitvector at bit n_rows;
// statistics widen, and an index over every distinct value gains keys for new values.
// insert_id ≠ 0 records the rows as an insert range of that transaction (ChunkVectorInfo
// inserted ids): readers with start_time ≤ insert_id (other than the inserting transaction)
// do not see them. Storage grows in place, geometrically, when the padding is exhausted.
extern "C" int cubit_table_append(cubit_table* t, uint64_t n_new, const int* cols, const void* const* data,
                                  const uint64_t* const* validity, uint32_t n_cols, uint64_t insert_id) {
    if (!t || (n_cols && (!cols || !data))) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_new == 0) return CUBIT_OK;
    const uint64_t n_old = t->n_rows, n_total = n_old + n_new;
    if (n_total >= (1ull << 47) || n_total < n_old)
        return fail(CUBIT_ERR_INVALID, "%llu rows exceed 2^47", (unsigned long long)n_total);
    if (n_cols != t->cols.size())
        return fail(CUBIT_ERR_INVALID, "append gives %u columns, the table has %zu", n_cols, t->cols.size());
    std::map<int, uint32_t> at;
    for (uint32_t i = 0; i < n_cols; ++i) {
        if (!t->cols.count(cols[i])) return fail(CUBIT_ERR_INVALID, "column %d not registered", cols[i]);
        if (!data[i]) return fail(CUBIT_ERR_INVALID, "column %d: null data", cols[i]);
        if (!at.emplace(cols[i], i).second) return fail(CUBIT_ERR_INVALID, "column %d given twice", cols[i]);
        const Column& c = t->cols.at(cols[i]);
        if (c.type == CUBIT_TYPE_VARCHAR) {  // the appended codes name dictionary strings (NULL rows: any)
            const int32_t* codes = static_cast<const int32_t*>(data[i]);
            const uint64_t* vw = validity ? validity[i] : nullptr;
            for (uint64_t r = 0; r < n_new; ++r)
                if ((!vw || ((vw[r >> 6] >> (r & 63)) & 1ull)) && (codes[r] < 0 || (uint64_t)codes[r] >= c.dict->size()))
                    return fail(CUBIT_ERR_INVALID, "column %d: appended code %d outside the dictionary", cols[i], codes[r]);
        }
    }
    if (int rc = set_device(t->ctx)) return rc;
    hipStream_t s = t->ctx->stream;
    HIP_CHECK(hipStreamSynchronize(s));
    drop_zones(t);  // every bitvector gains the appended rows
    // 1. capacity: bitvectors and columns grow together (×1.25 at least)
    const uint64_t need_words = padded_words(n_total);
    if (need_words > t->cap_words) {
        const uint64_t words = std::max(need_words, padded_words(n_old + n_old / 4));
        if (int rc = grow_bitvectors(t, words)) return rc;
    }
    for (auto& kv : t->cols)
        if (int rc = own_column(t, kv.second, std::max(n_total, kv.second.cap_rows >= n_total ? kv.second.cap_rows
                                                                                          : t->cap_words * 64)))
            return rc;
    // 2. per column: values, validity, then every index on it
    const uint64_t slice_words = padded_words(n_new);
    DevBuf tmp_col, tmp_valid, tmp_bits;
    const uint32_t n_tmp_bv = (uint32_t)kMultiKeys;
    if (hipMalloc(&tmp_col.p, n_new * 8 + 16) != hipSuccess || hipMalloc(&tmp_valid.p, slice_words * 8) != hipSuccess ||
        hipMalloc(&tmp_bits.p, slice_words * 8 * n_tmp_bv) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "append staging allocation failed");
    for (auto& kv : t->cols) {
        const int col = kv.first;
        Column& c = kv.second;
        c.drop_packed();  // the segments do not hold the appended rows
        const uint32_t i = at[col];
        const uint64_t esz = type_is32(c.type) ? 4 : 8;
        HIP_CHECK(hipMemcpyAsync(tmp_col.p, data[i], n_new * esz, hipMemcpyHostToDevice, s));
        if (type_is_fp(c.type)) {  // the patterns appended as given, the slice keyed in place for the rest
            HIP_CHECK(hipMemcpyAsync(static_cast<char*>(const_cast<void*>(c.raw)) + n_old * esz, tmp_col.p,
                                     n_new * esz, hipMemcpyDeviceToDevice, s));
            HIP_CHECK(launch_fp_keys(tmp_col.p, c.type, n_new, tmp_col.p, s));
        }
        HIP_CHECK(hipMemcpyAsync(static_cast<char*>(const_cast<void*>(c.data)) + n_old * esz, tmp_col.p, n_new * esz,
                                 hipMemcpyDeviceToDevice, s));
        const uint64_t* slice_valid = nullptr;
        if (validity && validity[i]) {
            HIP_CHECK(hipMemsetAsync(tmp_valid.p, 0, slice_words * 8, s));
            HIP_CHECK(hipMemcpyAsync(tmp_valid.p, validity[i], (n_new + 63) / 64 * 8, hipMemcpyHostToDevice, s));
            if (n_new & 63) {  // bits past the appended rows are not rows
                uint64_t last = validity[i][(n_new - 1) / 64] & ((1ull << (n_new & 63)) - 1);
                HIP_CHECK(hipMemcpyAsync(static_cast<uint64_t*>(tmp_valid.p) + (n_new - 1) / 64, &last, 8,
                                         hipMemcpyHostToDevice, s));
                HIP_CHECK(hipStreamSynchronize(s));
            }
            slice_valid = static_cast<const uint64_t*>(tmp_valid.p);
            if (!c.validity) {  // first NULLs of the column: the old rows are all valid
                auto b = std::make_unique<DevBuf>();
                if (int rc = alloc_table_bv(t, *b)) return fail(rc, "validity allocation failed");
                if (n_old) HIP_CHECK(launch_fill_valid(static_cast<uint64_t*>(b->p), n_old, s));
                c.validity = static_cast<const uint64_t*>(b->p);
                c.owned.push_back(std::move(b));
            }
            HIP_CHECK(launch_splice_bits(const_cast<uint64_t*>(c.validity), slice_valid, n_old, n_new, s));
        } else if (c.validity) {  // a column with NULLs gets all-valid rows
            HIP_CHECK(launch_fill_valid(static_cast<uint64_t*>(tmp_valid.p), n_new, s));
            HIP_CHECK(launch_splice_bits(const_cast<uint64_t*>(c.validity), static_cast<const uint64_t*>(tmp_valid.p),
                                         n_old, n_new, s));
        }
        Index* ixs[2] = {t->idx.count(col) ? &t->idx[col] : nullptr, t->bins.count(col) ? &t->bins[col] : nullptr};
        Index* sx = t->sliced.count(col) ? &t->sliced[col] : nullptr;
        if (!ixs[0] && !ixs[1] && !sx) continue;
        // statistics of the appended slice (+ its distinct values for an every-distinct-value index)
        bool want_distinct = ixs[0] && ixs[0]->exact_all;
        std::vector<int64_t> added;
        int64_t smin = 0, smax = 0;
        bool sany = false;
        int rc = value_stats(t, tmp_col.p, ktype(c), slice_valid, n_new, added, want_distinct, smin, smax, sany);
        if (rc == CUBIT_ERR_UNSUPPORTED && want_distinct) {  // too wide a span for a presence bitmap
            ixs[0]->exact_all = false;
            want_distinct = false;
            rc = value_stats(t, tmp_col.p, ktype(c), slice_valid, n_new, added, false, smin, smax, sany);
        }
        if (rc) return rc;
        for (Index* ix : ixs) {
            if (!ix) continue;
            const int enc = ix->encoding;
            const size_t n_bv = index_bv_count(*ix);
            while (ix->owned.size() < n_bv) {  // an index built on an empty partition has no bitvectors yet
                auto b = std::make_unique<DevBuf>();
                if (int rc2 = alloc_table_bv(t, *b)) return fail(rc2, "index bitvector allocation failed");
                ix->owned.push_back(std::move(b));
            }
            ix->bvs.resize(n_bv);
            for (size_t k = 0; k < n_bv; ++k) ix->bvs[k] = static_cast<uint64_t*>(ix->owned[k]->p);
            ix->bytes = ix->owned.size() * t->cap_words * 8;
            const int cmp = enc == CUBIT_INDEX_BINS ? kCmpBetween : enc == CUBIT_INDEX_RANGE ? CUBIT_CMP_LT : CUBIT_CMP_EQ;
            for (size_t k0 = 0; k0 < n_bv; k0 += kMultiKeys) {
                MultiKeyArgs mk{};
                for (size_t k = k0; k < std::min(n_bv, k0 + kMultiKeys); ++k) {
                    mk.c[mk.m] = ix->keys[k];
                    mk.c2[mk.m] = enc == CUBIT_INDEX_BINS ? ix->keys[k + 1] : 0;
                    mk.out[mk.m] = static_cast<uint64_t*>(tmp_bits.p) + (uint64_t)mk.m * slice_words;
                    ++mk.m;
                }
                HIP_CHECK(launch_compare_bitvectors(tmp_col.p, ktype(c), slice_valid, n_new, cmp, mk, s));
                for (uint32_t m = 0; m < mk.m; ++m)
                    HIP_CHECK(launch_splice_bits(ix->bvs[k0 + m], mk.out[m], n_old, n_new, s));
            }
            if (sany) {
                const bool was_empty = ix->empty;
                const int64_t old_min = ix->vmin;
                ix->vmin = was_empty ? smin : std::min(ix->vmin, smin);
                ix->vmax = was_empty ? smax : std::max(ix->vmax, smax);
                ix->empty = false;
                // the new keys' bitvectors span the whole column: counted with the new rows
                t->n_rows = n_total;
                t->nwp = need_words;
                rc = maintain_exact_keys(t, col, *ix, added, old_min, was_empty);
                t->n_rows = n_old;
                t->nwp = padded_words(n_old);
                if (rc) return rc;
            }
        }
        // the bit-sliced index (NULL appended rows are 0 in every slice, as the padding they replace)
        if (sx && sany) {
            if (sx->empty || smin < sx->vmin) {
                // the first valid rows, or a key below the base: every offset changes, so the slices
                // are rebuilt in one build from the whole column, which holds the appended rows already
                if (int rc2 = build_sliced(t, c, n_total, *sx)) return rc2;
            } else {
                // a key above the top first adds all-zero high slices (the old rows have 0 there); then
                // the appended rows are sliced alone and every slice spliced at bit n_old
                const int64_t top = std::max(sx->vmax, smax);
                const uint32_t bits = sliced_bits(sx->vmin, top);
                DevBuf tmp_sl;
                if (bits && hipMalloc(&tmp_sl.p, slice_words * 8 * bits) != hipSuccess)
                    return fail(CUBIT_ERR_OOM, "append staging allocation failed");
                if (int rc2 = sliced_grow(t, *sx, bits)) return rc2;
                sx->vmax = top;
                SliceSet fresh{};
                for (uint32_t k = 0; k < bits; ++k) fresh.s[k] = static_cast<uint64_t*>(tmp_sl.p) + (uint64_t)k * slice_words;
                HIP_CHECK(launch_bitslice_build(tmp_col.p, ktype(c), slice_valid, n_new, sx->vmin, bits, fresh, s));
                for (uint32_t k = 0; k < bits; ++k) HIP_CHECK(launch_splice_bits(sx->bvs[k], fresh.s[k], n_old, n_new, s));
                HIP_CHECK(hipStreamSynchronize(s));  // tmp_sl goes out of scope
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));  // tmp_col / tmp_valid reused by the next column
    }
    HIP_CHECK(hipStreamSynchronize(s));
    t->n_rows = n_total;
    t->nwp = need_words;
    if (insert_id) {
        t->ins.push_back({(int64_t)n_old, (int64_t)n_total, insert_id});
        std::stable_sort(t->ins.begin(), t->ins.end(), [](const auto& a, const auto& b) { return a.id < b.id; });
    }
    drop_derived(t);
    return CUBIT_OK;
}

namespace {

// The second half of a merge, shared by cubit_table_merge_updates and cubit_table_sync_column:
// the m records (device lists, rows ascending, one record per row; valid_p null = every record
// carries its value, a NULL record holds value 0) written into the base values, the validity and
// every index bitvector of the column (merge_words_kernel). `added` = the records' distinct valid
// values as keys, ascending (the statistics and exact keys they add); any_null = some record is
// NULL (the column then needs a validity bitvector).
int apply_records(cubit_table* t, int col, Column& c, const int64_t* rows_p, const int64_t* vals_p,
                  const uint8_t* valid_p, uint64_t m, const std::vector<int64_t>& added, bool any_null) {
    hipStream_t s = t->ctx->stream;
    HIP_CHECK(hipStreamSynchronize(s));
    drop_zones(t);  // the merge rewrites index words in place
    if (int rc = own_column(t, c, std::max<uint64_t>(t->n_rows, c.cap_rows))) return rc;
    if (any_null)
        if (int rc = ensure_validity(t, c)) return rc;
    c.drop_packed();  // merged values are not in the segments
    Index* ixs[2] = {t->idx.count(col) ? &t->idx[col] : nullptr, t->bins.count(col) ? &t->bins[col] : nullptr};
    MergeIndex mi[2] = {};
    DevBuf d_keys[2], d_bvs[2];
    for (int x = 0; x < 2; ++x) {
        Index* ix = ixs[x];
        if (!ix || index_bv_count(*ix) == 0 || ix->bvs.size() != index_bv_count(*ix)) continue;
        if (hipMalloc(&d_keys[x].p, ix->keys.size() * 8) != hipSuccess ||
            hipMalloc(&d_bvs[x].p, ix->bvs.size() * sizeof(uint64_t*)) != hipSuccess)
            return fail(CUBIT_ERR_OOM, "merge index descriptor allocation failed");
        HIP_CHECK(hipMemcpyAsync(d_keys[x].p, ix->keys.data(), ix->keys.size() * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_bvs[x].p, ix->bvs.data(), ix->bvs.size() * sizeof(uint64_t*), hipMemcpyHostToDevice, s));
        mi[x].keys = static_cast<const int64_t*>(d_keys[x].p);
        mi[x].bvs = static_cast<uint64_t* const*>(d_bvs[x].p);
        mi[x].n_keys = (uint32_t)ix->keys.size();
        mi[x].encoding = ix->encoding == CUBIT_INDEX_RANGE ? 0 : ix->encoding == CUBIT_INDEX_EQUALITY ? 1 : 2;
    }
    // every 64-row word holding merged rows, rewritten by one wave (rows ascend, each once)
    // FLOAT / DOUBLE: the merge compares and writes keys (the key column is what the indexes were built
    // from); the patterns are scattered into the pattern column beside it
    DevBuf d_keys_of;
    const int64_t* merge_vals = vals_p;
    if (type_is_fp(c.type)) {
        if (hipMalloc(&d_keys_of.p, m * 8) != hipSuccess) return fail(CUBIT_ERR_OOM, "merge key allocation failed");
        HIP_CHECK(launch_value_keys(vals_p, m, c.type, static_cast<int64_t*>(d_keys_of.p), s));
        merge_vals = static_cast<const int64_t*>(d_keys_of.p);
    }
    HIP_CHECK(launch_merge_words(rows_p, merge_vals, valid_p, m, t->n_rows, const_cast<void*>(c.data), ktype(c),
                                 const_cast<uint64_t*>(c.validity), mi[0], mi[1], s));
    if (type_is_fp(c.type))
        HIP_CHECK(launch_scatter_raw(rows_p, vals_p, valid_p, m, c.type, const_cast<void*>(c.raw), s));
    HIP_CHECK(hipStreamSynchronize(s));
    // statistics and exact keys for the merged values (a merged NULL leaves the index bounds:
    // they only have to contain the valid values)
    for (Index* ix : ixs) {
        if (!ix || added.empty()) continue;
        const bool was_empty = ix->empty;
        const int64_t old_min = ix->vmin;
        ix->vmin = was_empty ? added.front() : std::min(ix->vmin, added.front());
        ix->vmax = was_empty ? added.back() : std::max(ix->vmax, added.back());
        ix->empty = false;
        if (int rc = maintain_exact_keys(t, col, *ix, added, old_min, was_empty)) return rc;
    }
    // the bit-sliced index, from the column as the merge left it: the words holding a merged row are
    // sliced again (a merged NULL clears its row in every slice, NULL → value sets it); a value above
    // the top first adds all-zero high slices; one below the base (or the first valid rows) moves
    // every offset, so the slices are rebuilt in one build
    auto sit = t->sliced.find(col);
    if (sit != t->sliced.end()) {
        Index& sx = sit->second;
        if (!added.empty() && (sx.empty || added.front() < sx.vmin)) {
            if (int rc = build_sliced(t, c, t->n_rows, sx)) return rc;
        } else if (!sx.empty) {
            if (!added.empty() && added.back() > sx.vmax) {
                if (int rc = sliced_grow(t, sx, sliced_bits(sx.vmin, added.back()))) return rc;
                sx.vmax = added.back();
            }
            HIP_CHECK(launch_bitslice_reslice(rows_p, m, c.data, ktype(c), c.validity, t->n_rows, sx.vmin,
                                              (uint32_t)sx.bvs.size(), slice_set(sx), s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
    }
    return CUBIT_OK;
}

}  // namespace

// Merge committed updates of one column into its base values and indexes (the checkpoint of
// update chains; CUBIT folds its update bitvectors into the index the same way). Every record
// with version < horizon — visible to every snapshot the caller still serves (start_time ≥
// horizon, as DuckDB's lowest active start bounds what a checkpoint may fold) — leaves the
// update list: each row takes its newest such value (records of a row are chronological; the
// merged records are the row's prefix below horizon) and its NULL-ness, and every index bitvector
// of the column whose membership can change is rewritten for each 64-row word holding a merged
// row (merge_words_kernel). Records
// at or past horizon stay in the list. *n_merged (optional) = rows whose base changed.
extern "C" int cubit_table_merge_updates(cubit_table* t, int col, uint64_t horizon, uint64_t* n_merged) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (n_merged) *n_merged = 0;
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    auto uit = t->upd.find(col);
    if (uit == t->upd.end() || uit->second.n == 0) return CUBIT_OK;
    if (int rc = set_device(t->ctx)) return rc;
    hipStream_t s = t->ctx->stream;
    Column& c = cit->second;
    const Updates& u = uit->second;
    // The merged records: each row's newest record below horizon. When every record is below it
    // and each row has one record (a checkpoint after the writers committed: the common case),
    // that is the update list itself, already on the device, and nothing is left.
    const bool all = u.unique_rows && u.distinct_versions.back() < horizon;
    std::vector<int64_t> m_rows, m_vals, k_rows, k_vals;
    std::vector<uint8_t> m_valid, k_valid;
    std::vector<uint64_t> k_vers;
    bool m_null = all && u.any_null;
    uint64_t m = all ? u.n : 0;
    if (!all) {
        for (uint64_t i = 0; i < u.n;) {
            uint64_t j = i;
            while (j < u.n && u.h_rows[j] == u.h_rows[i]) ++j;
            uint64_t p = i;  // merged prefix [i, p)
            while (p < j && u.h_versions[p] < horizon) ++p;
            if (p > i) {
                const int64_t v = u.h_values[p - 1];
                const bool ok = u.valid_at(p - 1);  // the newest merged record decides value and NULL-ness
                m_rows.push_back(u.h_rows[i]);
                m_vals.push_back(ok ? v : 0);
                m_valid.push_back(ok ? 1 : 0);
                m_null |= !ok;
            }
            for (uint64_t q = p; q < j; ++q) {
                k_rows.push_back(u.h_rows[q]);
                k_vals.push_back(u.h_values[q]);
                k_vers.push_back(u.h_versions[q]);
                k_valid.push_back(u.valid_at(q) ? 1 : 0);
            }
            i = j;
        }
        m = m_rows.size();
    }
    if (m == 0) return CUBIT_OK;
    // the merged values' distinct valid values: the statistics and exact keys they add
    std::vector<int64_t> added;
    if (all) {
        added = u.stat_values;  // the records' distinct valid values, computed when they were set
    } else {
        std::vector<int64_t> valid_vals;
        for (uint64_t i = 0; i < m; ++i)
            if (m_valid[i]) valid_vals.push_back(value_key(c.type, m_vals[i]));
        added = distinct_sorted(valid_vals.data(), valid_vals.size());
    }
    if (c.type == CUBIT_TYPE_INT32 && !added.empty() && (added.front() < INT32_MIN || added.back() > INT32_MAX))
        return fail(CUBIT_ERR_INVALID, "merged value %lld does not fit an INT32 column",
                    (long long)(added.front() < INT32_MIN ? added.front() : added.back()));
    DevBuf d_rows, d_vals, d_valid;
    const int64_t* rows_p;
    const int64_t* vals_p;
    const uint8_t* valid_p;
    if (all) {
        rows_p = static_cast<const int64_t*>(u.rows->p);
        vals_p = static_cast<const int64_t*>(u.values->p);
        valid_p = u.any_null ? u.d_valids() : nullptr;  // a NULL record holds value 0 (store_updates)
    } else {
        if (hipMalloc(&d_rows.p, m * 8) != hipSuccess || hipMalloc(&d_vals.p, m * 8) != hipSuccess ||
            (m_null && hipMalloc(&d_valid.p, m) != hipSuccess))
            return fail(CUBIT_ERR_OOM, "merge list allocation failed");
        HIP_CHECK(hipMemcpyAsync(d_rows.p, m_rows.data(), m * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_vals.p, m_vals.data(), m * 8, hipMemcpyHostToDevice, s));
        if (m_null) HIP_CHECK(hipMemcpyAsync(d_valid.p, m_valid.data(), m, hipMemcpyHostToDevice, s));
        rows_p = static_cast<const int64_t*>(d_rows.p);
        vals_p = static_cast<const int64_t*>(d_vals.p);
        valid_p = m_null ? static_cast<const uint8_t*>(d_valid.p) : nullptr;
    }
    if (int rc = apply_records(t, col, c, rows_p, vals_p, valid_p, m, added, m_null)) return rc;
    // the records left (each row's suffix at or past horizon), still grouped and chronological
    if (k_rows.empty()) {
        t->upd.erase(col);
    } else if (int rc = store_updates(t, col, k_rows.data(), k_vals.data(), k_vers.data(), k_rows.size(),
                                      k_valid.data())) {
        return rc;
    }
    drop_derived(t);
    if (n_merged) *n_merged = m;
    return CUBIT_OK;
}

// Bring one column to new contents given whole (what a host engine holds after committed UPDATEs:
// the values, with no list of the rows that changed). The changed rows are found on the device —
// column_diff_kernel over the old and the new column and validity, one "changed" bitvector and its
// count — decoded into ascending row ids by the ordered decode, their new values gathered
// (sync_gather_kernel), and the records go through the merge's second half (apply_records). More
// than max_changed changed rows: nothing is touched and *applied = 0 (the caller rebuilds).
// Device memory beside the table while the call runs: the staged column and validity for host
// input (n_rows × element size + nwp × 8 bytes; none with on_device), the changed bitvector
// (nwp × 8) and 17 bytes per changed row (row id, value, valid flag; 25 for FLOAT / DOUBLE).
extern "C" int cubit_table_sync_column(cubit_table* t, int col, const void* values, const uint64_t* validity,
                                       int on_device, uint64_t max_changed, uint64_t* n_changed, int* applied) {
    if (!t || !n_changed || !applied) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    auto uit = t->upd.find(col);
    if (uit != t->upd.end() && uit->second.n)
        return fail(CUBIT_ERR_INVALID, "column %d has %llu update records outstanding (merge or clear them first)", col,
                    (unsigned long long)uit->second.n);
    const uint64_t n = t->n_rows;
    if (n == 0) {
        *n_changed = 0;
        *applied = 1;
        return CUBIT_OK;
    }
    if (!values) return fail(CUBIT_ERR_INVALID, "null values");
    if (int rc = set_device(t->ctx)) return rc;
    hipStream_t s = t->ctx->stream;
    Column& c = cit->second;
    const uint64_t esz = type_is32(c.type) ? 4 : 8, n_words = (n + 63) / 64, nwp = padded_words(n);
    // 1. the new contents on the device: read in place, or staged
    DevBuf st_col, st_valid, d_changed, d_cnt;
    const void* new_col = values;
    const uint64_t* new_valid = validity;
    if (hipMalloc(&d_changed.p, nwp * 8) != hipSuccess || hipMalloc(&d_cnt.p, 16) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "sync bitvector allocation failed");
    const bool tm = sync_timing();
    uint64_t ns[5] = {tm ? now_ns() : 0, 0, 0, 0, 0};
    if (!on_device) {
        if (hipMalloc(&st_col.p, std::max<uint64_t>(n * esz, 16)) != hipSuccess ||
            (validity && hipMalloc(&st_valid.p, n_words * 8) != hipSuccess))
            return fail(CUBIT_ERR_OOM, "sync staging allocation of %llu bytes failed",
                        (unsigned long long)(n * esz + (validity ? n_words * 8 : 0)));
        HIP_CHECK(hipMemcpyAsync(st_col.p, values, n * esz, hipMemcpyHostToDevice, s));
        if (validity) HIP_CHECK(hipMemcpyAsync(st_valid.p, validity, n_words * 8, hipMemcpyHostToDevice, s));
        new_col = st_col.p;
        new_valid = validity ? static_cast<const uint64_t*>(st_valid.p) : nullptr;
    }
    if (tm) {
        HIP_CHECK(hipStreamSynchronize(s));  // the staging copies
        ns[1] = now_ns();
    }
    // 2. the diff: one pass, the changed bitvector and its count (a timed launch with timing on)
    HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 16, s));
    hipEvent_t e0, e1;
    if (int rc = timing_events(t->ctx, e0, e1)) return rc;
    HIP_CHECK(launch_column_diff(raw_of(c), c.validity, new_col, new_valid, c.type, n, static_cast<uint64_t*>(d_changed.p),
                                 static_cast<uint64_t*>(d_cnt.p), s, e0, e1));
    uint64_t m = 0;
    HIP_CHECK(hipMemcpyAsync(&m, d_cnt.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (tm) {
        ns[2] = now_ns();
        std::fprintf(stderr, "cubit sync timing: %llu rows, %llu changed: staging + H2D %.2f ms, diff %.2f ms\n",
                     (unsigned long long)n, (unsigned long long)m, (ns[1] - ns[0]) * 1e-6, (ns[2] - ns[1]) * 1e-6);
    }
    *n_changed = m;
    if (m > max_changed) {
        *applied = 0;
        return CUBIT_OK;
    }
    *applied = 1;
    if (m == 0) return CUBIT_OK;  // nothing written: zone maps and patched leaves stand
    // 3. the changed rows as records: ascending local ids (the ordered decode of the one leaf),
    //    then their new values and NULL-ness
    DevBuf d_rows, d_vals, d_valid;
    if (hipMalloc(&d_rows.p, m * 8) != hipSuccess || hipMalloc(&d_vals.p, m * 8) != hipSuccess ||
        hipMalloc(&d_valid.p, m) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "sync record list allocation failed");
    EvalProgram prog{};
    prog.leaf[0] = static_cast<const uint64_t*>(d_changed.p);
    prog.n_leaves = 1;
    uint64_t* d_decoded = static_cast<uint64_t*>(d_cnt.p) + 1;
    if (int rc = run_eval(t->ctx, prog, n, 0, static_cast<int64_t*>(d_rows.p), m, d_decoded, nullptr, RunMode::kDecode,
                          false, true))
        return rc;
    HIP_CHECK(launch_sync_gather(new_col, new_valid, c.type, static_cast<const int64_t*>(d_rows.p), m,
                                 static_cast<int64_t*>(d_vals.p), static_cast<uint8_t*>(d_valid.p), s));
    std::unique_ptr<int64_t[]> h_vals(new int64_t[m]);  // not zeroed: the copy fills it
    std::vector<uint8_t> h_valid;
    if (new_valid) h_valid.resize(m);
    uint64_t decoded = 0;
    HIP_CHECK(hipMemcpyAsync(&decoded, d_decoded, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_vals.get(), d_vals.p, m * 8, hipMemcpyDeviceToHost, s));
    if (new_valid) HIP_CHECK(hipMemcpyAsync(h_valid.data(), d_valid.p, m, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (decoded != m)
        return fail(CUBIT_ERR_HIP, "sync decoded %llu changed rows, the diff counted %llu", (unsigned long long)decoded,
                    (unsigned long long)m);
    if (int rc = check_codes(c, h_vals.get(), new_valid ? h_valid.data() : nullptr, m)) return rc;
    // the records' distinct valid values as keys (compacted in place): the statistics and exact
    // keys they add
    uint64_t n_valid = m;
    if (new_valid || type_is_keyed(c.type)) {
        n_valid = 0;
        for (uint64_t i = 0; i < m; ++i)
            if (!new_valid || h_valid[i]) h_vals[n_valid++] = value_key(c.type, h_vals[i]);
    }
    const bool any_null = n_valid < m;
    const std::vector<int64_t> added = distinct_sorted(h_vals.get(), n_valid);
    if (tm) ns[3] = now_ns();
    // 4. the merge's second half
    if (int rc = apply_records(t, col, c, static_cast<const int64_t*>(d_rows.p), static_cast<const int64_t*>(d_vals.p),
                               new_valid ? static_cast<const uint8_t*>(d_valid.p) : nullptr, m, added, any_null))
        return rc;
    drop_derived(t);
    if (tm) {
        ns[4] = now_ns();
        std::fprintf(stderr, "cubit sync timing: decode + gather + records to host %.2f ms, merge %.2f ms\n",
                     (ns[3] - ns[2]) * 1e-6, (ns[4] - ns[3]) * 1e-6);
    }
    return CUBIT_OK;
}

// ------------------------------------------------------------------ planner

namespace {

// An index as the planner may use it: its keys and bitvectors with statistics widened by the
// column's update records (any version: wider bounds are always safe). Folding a constant
// against the base statistics alone would drop rows whose visible updated value lies outside
// them, and "every distinct value" exactness holds only while every updated value is a key.
struct IndexView {
    int encoding;
    bool exact_all, empty;
    int64_t vmin, vmax;
    const std::vector<int64_t>& keys;
    const std::vector<uint64_t*>& bvs;
};

IndexView view_of(const cubit_table* t, int col, const Index& ix) {
    IndexView v{ix.encoding, ix.exact_all, ix.empty, ix.vmin, ix.vmax, ix.keys, ix.bvs};
    auto uit = t->upd.find(col);
    if (uit == t->upd.end() || uit->second.stat_values.empty()) return v;
    const std::vector<int64_t>& uv = uit->second.stat_values;
    v.vmin = ix.empty ? uv.front() : std::min(ix.vmin, uv.front());
    v.vmax = ix.empty ? uv.back() : std::max(ix.vmax, uv.back());
    v.empty = false;
    if (v.exact_all) {
        auto is_key = [&](int64_t x) { return std::binary_search(ix.keys.begin(), ix.keys.end(), x); };
        if (ix.encoding == CUBIT_INDEX_RANGE) {
            // values ⊆ keys ∪ {vmin}: the base minimum and every updated value
            if (!ix.empty && ix.vmin != v.vmin && !is_key(ix.vmin)) v.exact_all = false;
            for (int64_t x : uv)
                if (x != v.vmin && !is_key(x)) {
                    v.exact_all = false;
                    break;
                }
        } else {
            for (int64_t x : uv)
                if (!is_key(x)) {
                    v.exact_all = false;
                    break;
                }
        }
    }
    return v;
}

// A K0 leaf whose bitvector is not built yet: {valid rows: v cmp c} of column col into bv.
// cmp = kCmpBetween: the interval c <= v < c2 (a Leaf of pred 2).
struct PendingK0 {
    uint64_t* bv;
    int col, cmp;
    int64_t c;
    int64_t c2 = 0;
};

// the column's bit-sliced index when a whole-column comparison should be answered from it
const Index* sliced_for_k0(const cubit_table* t, int col) {
    if (!t->use_sliced) return nullptr;
    auto it = t->sliced.find(col);
    if (it == t->sliced.end() || it->second.empty) return nullptr;
    const Column& cl = t->cols.at(col);
    return sliced_moves_fewer_bytes((uint32_t)it->second.bvs.size(), type_is32(cl.type) ? 4 : 8) ? &it->second : nullptr;
}

// Build a K0 leaf over the whole column (from the column's slices where they move fewer bytes, or
// from the BITPACKING segments when enabled).
int compute_k0(cubit_table* t, const PendingK0& k) {
    const Column& cl = t->cols.at(k.col);
    hipError_t e;
    if (const Index* sx = sliced_for_k0(t, k.col)) {
        // bit for bit the leaf K0 builds: the valid rows whose base key passes. An interval that
        // misses or covers the slices' range is built all the same (all zero / the valid rows), so
        // the leaf keeps its predicate for the patches of visible updates.
        const uint32_t bits = (uint32_t)sx->bvs.size();
        const SlicedInterval si = sliced_interval(k.cmp, k.c, k.c2, sx->vmin, bits);
        const uint64_t max = bits >= 64 ? ~0ull : (1ull << bits) - 1;
        const bool iv = si.kind == SlicedInterval::kInterval;
        hipEvent_t e0, e1;
        if (int rc = timing_events(t->ctx, e0, e1)) return rc;
        e = launch_bitslice_compare(slice_set(*sx), bits, cl.validity, t->n_rows, iv ? si.lo : 0, iv ? si.hi : max,
                                    iv ? si.negate : si.kind == SlicedInterval::kFalse, k.bv, t->ctx->stream, e0, e1);
        t->last_sliced++;
        if (e != hipSuccess) return fail(CUBIT_ERR_HIP, "bit-slice compare kernel: %s", hipGetErrorString(e));
        return CUBIT_OK;
    }
    // (UBIGINT segments: the packed compare orders values as signed; such columns compare unpacked)
    if (cl.bp_n_groups && t->use_packed && cl.type != CUBIT_TYPE_UINT64 && k.cmp != kCmpBetween) {
        // straight from the BITPACKING segments: w/8 bytes per row instead of sizeof(T)
        e = hipMemsetAsync(k.bv, 0, t->nwp * 8, t->ctx->stream);
        if (e == hipSuccess)
            e = launch_bitpacked_compare(static_cast<const uint8_t*>(cl.bp_bytes->p),
                                         static_cast<const BpGroup*>(cl.bp_groups->p), cl.bp_n_groups, cl.type,
                                         cl.validity, k.cmp, k.c, 0, k.bv, t->ctx->stream, cl.bp_simple_width);
        t->last_packed++;
    } else {
        e = launch_compare_bitvector(cl.data, ktype(cl), cl.validity, t->n_rows, k.cmp, k.c, k.bv, t->ctx->stream, k.c2);
    }
    if (e != hipSuccess) return fail(CUBIT_ERR_HIP, "compare kernel: %s", hipGetErrorString(e));
    return CUBIT_OK;
}

// A filter node against the table: its kind, its column registered, its comparison.
int check_node(const cubit_table* t, const cubit_filter_node& f) {
    const NodeCheck c = check_filter_node(f);
    if (c == NodeCheck::kBadKind) return fail(CUBIT_ERR_INVALID, "filter node kind %d", f.kind);
    if (f.kind != CUBIT_FILTER_OR && f.kind != CUBIT_FILTER_AND && !t->cols.count(f.column))
        return fail(CUBIT_ERR_INVALID, "filter references unregistered column %d", f.column);
    if (c == NodeCheck::kBadCmp) return fail(CUBIT_ERR_INVALID, "comparison %d", f.cmp);
    return CUBIT_OK;
}

// An inclusive range as the half-open bounds lo <= v < hi that interval_from_bins and eq_interval
// take, either side open: no bound where the range reaches the end of INT64.
struct HalfOpen {
    int64_t lo, hi;
    bool has_lo, has_hi;
    explicit HalfOpen(const CmpRange& r)
        : lo(r.lo), hi(r.hi == INT64_MAX ? r.hi : r.hi + 1), has_lo(r.lo != INT64_MIN), has_hi(r.hi != INT64_MAX) {}
};

struct Planner {
    cubit_table* t;
    const cubit_filter_node* nodes;
    uint32_t n_nodes;
    int rc = CUBIT_OK;

    ExprP nn(int col) {
        const Column& c = t->cols.at(col);
        if (!c.validity) return mk_true();
        Leaf l;
        l.bv = c.validity;
        l.column = col;
        l.pred = 1;
        l.zsrc = kZoneBits;
        return mk_leaf(l);
    }

    // K0 fallback: the comparison from the raw column into a scratch bitvector. The launch is
    // deferred (pending) until the plan is complete: inside a conjunction it may be narrowed to
    // the rows the other filters keep (narrow_k0), as the reference's filter loop does.
    std::vector<PendingK0> pending;
    // cmp = kCmpBetween: the interval c <= v < c2 as one leaf of pred 2 (plan_and, sliced columns).
    // A column with a bit-sliced index folds a comparison that no key of the slices' range passes,
    // or every one does, into FALSE / the valid rows without a launch — only when it also folds
    // against the range widened by the column's update records (the rule view_of applies to the
    // other encodings); inside the widened range the leaf is built and keeps its predicate.
    ExprP raw_compare(int col, int cmp, int64_t c, int64_t c2 = 0) {
        if (const Index* sx = sliced_for_k0(t, col)) {
            const SlicedInterval si = sliced_interval(cmp, c, c2, sx->vmin, (uint32_t)sx->bvs.size());
            if (si.kind != SlicedInterval::kInterval) {
                int64_t wmin = sx->vmin, wmax = sx->vmax;
                auto uit = t->upd.find(col);
                if (uit != t->upd.end() && !uit->second.stat_values.empty()) {
                    wmin = std::min(wmin, uit->second.stat_values.front());
                    wmax = std::max(wmax, uit->second.stat_values.back());
                }
                if (sliced_interval(cmp, c, c2, wmin, sliced_bits(wmin, wmax)).kind == si.kind)
                    return si.kind == SlicedInterval::kFalse ? mk_false() : nn(col);
            }
        }
        uint64_t* bv = nullptr;
        if ((rc = scratch_bv(t, &bv))) return nullptr;
        pending.push_back({bv, col, cmp, c, c2});
        Leaf l;
        l.bv = bv;
        l.column = col;
        if (cmp == kCmpBetween) {
            l.pred = 2;
            l.constant2 = c2;
        } else {
            l.cmp = cmp;
        }
        l.constant = c;
        l.zsrc = kZoneStats;
        return mk_leaf(l);
    }

    // lo <= v <= hi (folded constant filters, not empty) on a column whose only index is bit-sliced:
    // one leaf, so `a <= x AND x < b` is one pass over the slices, not two
    ExprP sliced_range(int col, const CmpRange& r) {
        const bool has_lo = r.lo != INT64_MIN, has_hi = r.hi != INT64_MAX;
        if (!has_lo && !has_hi) return nn(col);
        if (!has_hi) return raw_compare(col, CUBIT_CMP_GE, r.lo);
        if (!has_lo) return raw_compare(col, CUBIT_CMP_LE, r.hi);
        if (r.lo == r.hi) return raw_compare(col, CUBIT_CMP_EQ, r.lo);
        return raw_compare(col, kCmpBetween, r.lo, r.hi + 1);
    }
    bool sliced_only(int col) const { return t->sliced.count(col) && !t->idx.count(col) && !t->bins.count(col); }

    // {v < c} from a range index; nullptr when the index cannot answer exactly
    ExprP range_lt(int col, const IndexView& ix, int64_t c) {
        if (ix.empty || c <= ix.vmin) return mk_false();
        if (c > ix.vmax) return nn(col);
        auto it = std::lower_bound(ix.keys.begin(), ix.keys.end(), c);
        if (it != ix.keys.end() && (*it == c || ix.exact_all)) {
            Leaf l;
            l.bv = ix.bvs[it - ix.keys.begin()];
            l.column = col;
            l.cmp = CUBIT_CMP_LT;
            l.constant = *it;
            l.zsrc = kZoneBits;
            return mk_leaf(l);
        }
        return nullptr;
    }

    // {v < c} (cmp LT) or {v == c} (cmp EQ) for a constant that is not a key of the range
    // index: the constant lies in one bin [k_lo, k_hi) between neighbouring keys, and only that
    // bin's rows are checked on the raw column (launch_candidate_check). This is the binned
    // bitmap index's candidate check: reads L(k_lo), L(k_hi) and the column at the bin's rows
    // instead of K0's whole column. nullptr when the bin is estimated (uniform values over
    // [vmin, vmax]) to hold more than a quarter of the rows, where K0's sequential read of the
    // column is cheaper; rc is set on a launch or allocation failure.
    ExprP candidate(int col, const IndexView& ix, int cmp, int64_t c) {
        auto hi_it = std::upper_bound(ix.keys.begin(), ix.keys.end(), c);  // first key > c
        const bool has_lo = hi_it != ix.keys.begin(), has_hi = hi_it != ix.keys.end();
        const double lo_v = has_lo ? (double)*(hi_it - 1) : (double)ix.vmin;
        const double hi_v = has_hi ? (double)*hi_it : (double)ix.vmax + 1.0;
        const double span = (double)ix.vmax - (double)ix.vmin + 1.0;
        if ((std::min(hi_v, (double)ix.vmax + 1.0) - std::max(lo_v, (double)ix.vmin)) > 0.25 * span) return nullptr;
        const Column& cl = t->cols.at(col);
        uint64_t* bv = nullptr;
        if ((rc = scratch_bv(t, &bv))) return nullptr;
        const uint64_t* lo_bv = has_lo ? ix.bvs[hi_it - 1 - ix.keys.begin()] : nullptr;
        const uint64_t* hi_bv = has_hi ? ix.bvs[hi_it - ix.keys.begin()] : nullptr;
        hipError_t e = launch_candidate_check(cl.data, ktype(cl), cl.validity, lo_bv, hi_bv, t->n_rows, cmp, c, bv,
                                              t->ctx->stream);
        if (e != hipSuccess) {
            rc = fail(CUBIT_ERR_HIP, "candidate check kernel: %s", hipGetErrorString(e));
            return nullptr;
        }
        Leaf l;
        l.bv = bv;
        l.column = col;
        l.cmp = cmp;
        l.constant = c;
        l.zsrc = kZoneStats;
        return mk_leaf(l);
    }

    // lo <= v < hi (either side open) on a column whose equality index holds every distinct
    // value (exact_all): the union of the keys' bitvectors inside, or the valid rows minus the
    // union of those outside — the fewer leaves; nullptr when both exceed 16.
    ExprP eq_interval(int col, const IndexView& ix, int64_t lo, int64_t hi, bool has_lo, bool has_hi) {
        const size_t b = has_lo ? (size_t)(std::lower_bound(ix.keys.begin(), ix.keys.end(), lo) - ix.keys.begin()) : 0;
        const size_t e = has_hi ? (size_t)(std::lower_bound(ix.keys.begin(), ix.keys.end(), hi) - ix.keys.begin())
                                : ix.keys.size();
        auto leaf = [&](size_t k) {
            Leaf l;
            l.bv = ix.bvs[k];
            l.column = col;
            l.cmp = CUBIT_CMP_EQ;
            l.constant = ix.keys[k];
            l.zsrc = kZoneBits;
            return mk_leaf(l);
        };
        const size_t inside = e > b ? e - b : 0, outside = ix.keys.size() - inside;
        if (inside <= 16 && inside <= outside + 1) {
            ExprP acc = mk_false();
            for (size_t k = b; k < e; ++k) acc = mk_bin(Expr::OR, acc, leaf(k));
            return acc;
        }
        if (outside > 16) return nullptr;
        ExprP out = mk_false();
        for (size_t k = 0; k < ix.keys.size(); ++k)
            if (k < b || k >= e) out = mk_bin(Expr::OR, out, leaf(k));
        return mk_bin(Expr::ANDNOT, nn(col), out);
    }

    // the column's equality index when it holds every distinct value (an interval over it is a
    // union of its bitvectors), else null
    const Index* exact_equality(int col) const {
        auto it = t->idx.find(col);
        return it != t->idx.end() && it->second.encoding == CUBIT_INDEX_EQUALITY && it->second.exact_all &&
                       !it->second.empty
                   ? &it->second
                   : nullptr;
    }

    ExprP eq_leaf(int col, const IndexView& ix, int64_t c, bool& exact) {
        exact = true;
        auto it = std::lower_bound(ix.keys.begin(), ix.keys.end(), c);
        if (it != ix.keys.end() && *it == c) {
            Leaf l;
            l.bv = ix.bvs[it - ix.keys.begin()];
            l.column = col;
            l.cmp = CUBIT_CMP_EQ;
            l.constant = c;
            l.zsrc = kZoneBits;
            return mk_leaf(l);
        }
        if (ix.exact_all || ix.empty || c < ix.vmin || c > ix.vmax) return mk_false();
        exact = false;
        return nullptr;
    }

    ExprP constant(int col, int cmp, int64_t c) {
        auto ixit = t->idx.find(col);
        if (ixit != t->idx.end()) {
            const IndexView ix = view_of(t, col, ixit->second);
            const bool top = c == INT64_MAX;
            if (ix.encoding == CUBIT_INDEX_RANGE) {
                // {v < k}: an index leaf when k is a key, else the candidate check of k's bin
                auto lt = [&](int64_t k) -> ExprP {
                    ExprP e = range_lt(col, ix, k);
                    return e ? e : candidate(col, ix, CUBIT_CMP_LT, k);
                };
                ExprP r;
                switch (cmp) {
                case CUBIT_CMP_LT: r = lt(c); break;
                case CUBIT_CMP_LE: r = top ? nn(col) : lt(c + 1); break;
                case CUBIT_CMP_GT: {
                    ExprP e = top ? nn(col) : lt(c + 1);
                    r = e ? mk_bin(Expr::ANDNOT, nn(col), e) : nullptr;
                    break;
                }
                case CUBIT_CMP_GE: {
                    ExprP e = lt(c);
                    r = e ? mk_bin(Expr::ANDNOT, nn(col), e) : nullptr;
                    break;
                }
                case CUBIT_CMP_EQ:
                case CUBIT_CMP_NE: {
                    ExprP lt_c = range_lt(col, ix, c);
                    ExprP lt_c1 = top ? nn(col) : range_lt(col, ix, c + 1);
                    if (lt_c && lt_c1) {
                        r = cmp == CUBIT_CMP_EQ ? mk_bin(Expr::ANDNOT, lt_c1, lt_c)
                                                : mk_bin(Expr::OR, mk_bin(Expr::ANDNOT, nn(col), lt_c1), lt_c);
                    } else if (ExprP eq = candidate(col, ix, CUBIT_CMP_EQ, c)) {
                        r = cmp == CUBIT_CMP_EQ ? eq : mk_bin(Expr::ANDNOT, nn(col), eq);
                    }
                    break;
                }
                default: break;
                }
                if (rc) return nullptr;
                if (r) return r;
            } else {
                bool exact = true;
                if (cmp == CUBIT_CMP_EQ) {
                    ExprP e = eq_leaf(col, ix, c, exact);
                    if (exact) return e;
                } else if (cmp == CUBIT_CMP_NE) {
                    ExprP e = eq_leaf(col, ix, c, exact);
                    if (exact) return mk_bin(Expr::ANDNOT, nn(col), e);
                } else if (ix.exact_all) {
                    // the equality bitvectors in range, or the valid rows outside the others
                    // (whichever reads fewer); wide ranges both ways go to K0
                    const CmpRange r = cmp_range(cmp, c, 0);
                    if (r.empty()) return mk_false();
                    if (cmp == CUBIT_CMP_LE && top) return nn(col);
                    const HalfOpen h(r);
                    if (ExprP e = eq_interval(col, ix, h.lo, h.hi, h.has_lo, h.has_hi)) return e;
                }
            }
        }
        return raw_compare(col, cmp, c);
    }

    // Cheapest exact plan of lo <= v < hi (half-open, from folded constant filters) out of
    // the column's binned index, or nullptr when the bins cannot answer it in fewer leaves than
    // the range index would (2, or 1 for a one-sided bound).
    ExprP interval_from_bins(int col, int64_t lo, int64_t hi, bool has_lo, bool has_hi) {
        auto bit = t->bins.find(col);
        if (bit == t->bins.end()) return nullptr;
        const IndexView b = view_of(t, col, bit->second);
        if (b.empty) return mk_false();
        const std::vector<int64_t>& e = b.keys;
        const size_t nb = e.size() - 1;
        size_t first, last;  // bins [first, last)
        if (!has_lo || lo <= b.vmin) {
            if (e.front() > b.vmin) return nullptr;  // rows below the first edge are in no bin
            first = 0;
        } else {
            auto it = std::lower_bound(e.begin(), e.end(), lo);
            if (it == e.end() || *it != lo) return nullptr;
            first = (size_t)(it - e.begin());
        }
        if (!has_hi || hi > b.vmax) {
            if (e.back() <= b.vmax) return nullptr;  // rows at or above the last edge
            last = nb;
        } else {
            auto it = std::lower_bound(e.begin(), e.end(), hi);
            if (it == e.end() || *it != hi) return nullptr;
            last = (size_t)(it - e.begin());
        }
        if (last <= first) return mk_false();
        const size_t range_cost = (has_lo && lo > b.vmin ? 1 : 0) + (has_hi && hi <= b.vmax ? 1 : 0);
        if (last - first >= std::max<size_t>(range_cost, 1) && t->idx.count(col)) return nullptr;
        if (last - first > 16) return nullptr;
        ExprP acc = mk_false();
        for (size_t k = first; k < last; ++k) {
            Leaf l;
            l.bv = b.bvs[k];
            l.column = col;
            l.pred = 2;
            l.constant = e[k];
            l.constant2 = e[k + 1];
            l.zsrc = kZoneBits;
            acc = mk_bin(Expr::OR, acc, mk_leaf(l));
        }
        return acc;
    }

    // AND node: constant comparisons on one column fold into an interval first (DuckDB
    // pushes "a <= x AND x < b" as one ConjunctionAndFilter on x, table_filter.cpp:20-40).
    ExprP plan_and(uint32_t i) {
        const cubit_filter_node& f = nodes[i];
        struct Bounds { CmpRange r; std::vector<uint32_t> members; };
        std::map<int, Bounds> by_col;
        std::vector<uint32_t> kids;
        uint32_t j = i + 1;
        for (int k = 0; k < f.n_children; ++k) {
            kids.push_back(j);
            const cubit_filter_node& c = nodes[j];
            if (c.kind == CUBIT_FILTER_CONSTANT && c.n_children == 0 && c.cmp != CUBIT_CMP_NE && c.cmp >= 0 &&
                c.cmp <= 5 &&
                (t->bins.count(c.column) || exact_equality(c.column) ||
                 (sliced_only(c.column) && sliced_for_k0(t, c.column)))) {
                Bounds& bd = by_col[c.column];
                bd.r = bd.r.intersect(cmp_range(c.cmp, c.constant, 0));
                bd.members.push_back(j);
            }
            j = (uint32_t)filter_subtree_end(nodes, n_nodes, j);
        }
        std::vector<char> done(n_nodes, 0);
        ExprP acc = mk_true();
        for (auto& [col, bd] : by_col) {
            ExprP e;
            const HalfOpen h(bd.r);
            if (bd.r.empty()) e = mk_false();
            else if (t->bins.count(col)) e = interval_from_bins(col, h.lo, h.hi, h.has_lo, h.has_hi);
            else if (bd.members.size() > 1 && sliced_only(col)) e = sliced_range(col, bd.r);
            if (!e && !rc && bd.members.size() > 1) {
                // two or more bounds on an every-value equality index: one union for the interval
                if (const Index* eq = exact_equality(col)) {
                    const IndexView v = view_of(t, col, *eq);  // exact only while every updated value is a key
                    if (v.exact_all && !v.empty) e = eq_interval(col, v, h.lo, h.hi, h.has_lo, h.has_hi);
                }
            }
            if (rc) return nullptr;
            if (!e) continue;
            for (uint32_t m : bd.members) done[m] = 1;
            acc = mk_bin(Expr::AND, acc, e);
        }
        for (uint32_t k : kids) {
            if (done[k]) continue;
            ExprP c = plan(k);
            if (!c) return nullptr;
            acc = mk_bin(Expr::AND, acc, c);
        }
        return acc;
    }

    ExprP plan(uint32_t i) {
        if (rc) return nullptr;
        const cubit_filter_node& f = nodes[i];
        if ((rc = check_node(t, f))) return nullptr;
        switch (f.kind) {
        case CUBIT_FILTER_AND:
            return plan_and(i);
        case CUBIT_FILTER_OR: {
            ExprP acc = mk_false();
            uint32_t j = i + 1;
            for (int k = 0; k < f.n_children; ++k) {
                ExprP c = plan(j);
                if (!c) return nullptr;
                acc = mk_bin(Expr::OR, acc, c);
                j = (uint32_t)filter_subtree_end(nodes, n_nodes, j);
            }
            return acc;
        }
        case CUBIT_FILTER_IS_NOT_NULL: return nn(f.column);
        case CUBIT_FILTER_IS_NULL: return mk_not(nn(f.column));
        default: return constant(f.column, f.cmp, f.constant);
        }
    }
};

// Materialise a subexpression into a scratch bitvector (bits-only pass).
int materialize(cubit_table* t, const ExprP& e, uint64_t** out) {
    Emitter em;
    em.emit_top(e);
    if (!em.ok || em.max_depth > kMaxDepth) return fail(CUBIT_ERR_UNSUPPORTED, "subexpression too deep");
    if (int rc = scratch_bv(t, out)) return rc;
    t->last_passes++;
    return run_eval(t->ctx, em.prog, t->n_rows, 0, nullptr, 0, t->dummy_count, *out, RunMode::kCount);
}

int fit(cubit_table* t, ExprP& e);
double literal_selectivity(cubit_table* t, const Leaf& l, bool neg, int* rc);
double conj_selectivity(cubit_table* t, const Emitter::Lits& lits, int* rc);

// estimated fraction of rows a subtree keeps, from its literals' estimates
double expr_selectivity(cubit_table* t, const ExprP& e, int* rc) {
    switch (e->kind) {
    case Expr::LEAF: return literal_selectivity(t, e->leaf, e->neg, rc);
    case Expr::AND: return expr_selectivity(t, e->a, rc) * expr_selectivity(t, e->b, rc);
    case Expr::OR: return std::min(1.0, expr_selectivity(t, e->a, rc) + expr_selectivity(t, e->b, rc));
    case Expr::ANDNOT: return expr_selectivity(t, e->a, rc) * (1.0 - expr_selectivity(t, e->b, rc));
    case Expr::CONST_TRUE: return 1.0;
    default: return 0.0;
    }
}

// Selection narrowing of K0 leaves (RowGroup::TemplatedScan's filter loop, row_group.cpp:537-550:
// each filter column after the first is read only at the rows the earlier ones kept). When the
// planned expression is a conjunction of literals holding non-negated K0 leaves, the other
// literals are materialised into a mask; with none, the most selective K0 comparison is built in
// full and is the mask. Each remaining K0 leaf, most selective first, is then built by
// masked_compare_kernel — its column read only at the mask's rows, the result already the AND
// with the mask, and the next leaf's mask — and the conjunction becomes that one leaf. The order
// and the decision come from selectivity estimates of every literal over the columns' per-zone
// min / max (literal_selectivity; the statistics the zonemaps use, computed once per table
// version), the reference's AdaptiveFilter ordering its filters by observed cost
// (adaptive_filter.cpp:21-88) made up front: when the mask is estimated to keep more than one
// row in 32, the K0 leaves are built in full (gathering most lines costs more than reading the
// column in order). The other conjuncts need not be literals: a union of equality bitvectors (an
// interval on an every-value equality index) or any subtree joins the mask, its selectivity
// estimated from its literals (OR: their sum, AND: their product). No count is read back:
// planning never waits for the device. allow = false
// (visible MVCC updates, whose patches need whole leaves) builds every leaf in full. Every
// pending leaf is built on return; t->last_narrow_cols lists the K0 columns in build order.
int narrow_k0(cubit_table* t, ExprP& e, std::vector<PendingK0>& pending, bool allow) {
    t->last_narrow_cols.clear();
    auto compute_rest = [&]() -> int {
        for (const PendingK0& k : pending) {
            if (int rc = compute_k0(t, k)) return rc;
            t->last_narrow_cols.push_back(k.col);
        }
        pending.clear();
        return CUBIT_OK;
    };
    auto take = [&](const uint64_t* bv, PendingK0* out) {
        for (size_t i = 0; i < pending.size(); ++i)
            if (pending[i].bv == bv) {
                if (out) *out = pending[i];
                pending.erase(pending.begin() + (long)i);
                return true;
            }
        return false;
    };
    auto is_pending = [&](const uint64_t* bv) {
        return std::any_of(pending.begin(), pending.end(), [&](const PendingK0& k) { return k.bv == bv; });
    };
    if (pending.empty()) return CUBIT_OK;
    if (!allow || t->n_rows == 0 || e->kind == Expr::LEAF) return compute_rest();
    std::vector<ExprP> parts;
    conj_parts(e, parts);
    Emitter::Lits lits;  // the literal conjuncts
    std::vector<ExprP> others;  // the other conjuncts (unions, subtrees)
    for (const ExprP& p : parts) {
        if (p->kind == Expr::LEAF) lits.push_back({p->leaf, p->neg});
        else others.push_back(p);
    }
    std::vector<const uint64_t*> narrow_bvs;
    Emitter::Lits rest;
    for (const auto& lit : lits) {
        // (an interval leaf, pred 2, is built in full: the masked compare takes one comparison)
        if (!lit.second && lit.first.pred != 2 && is_pending(lit.first.bv) &&
            std::find(narrow_bvs.begin(), narrow_bvs.end(), lit.first.bv) == narrow_bvs.end())
            narrow_bvs.push_back(lit.first.bv);
        else
            rest.push_back(lit);
    }
    std::vector<const uint64_t*> other_bvs;
    for (const ExprP& p : others) leaves_of(p, other_bvs);
    for (const auto& lit : rest)  // a narrowed leaf must not also be read whole
        if (std::find(narrow_bvs.begin(), narrow_bvs.end(), lit.first.bv) != narrow_bvs.end()) return compute_rest();
    for (const uint64_t* bv : other_bvs)
        if (std::find(narrow_bvs.begin(), narrow_bvs.end(), bv) != narrow_bvs.end()) return compute_rest();
    if (narrow_bvs.empty()) return compute_rest();
    // selectivity estimates: the mask of the other conjuncts (independent columns: the
    // product; literals on one column as one interval), each K0 comparison
    int rc = CUBIT_OK;
    double rest_sel = conj_selectivity(t, rest, &rc);
    for (const ExprP& p : others) rest_sel *= expr_selectivity(t, p, &rc);
    if (rc) return rc;
    std::vector<std::pair<double, PendingK0>> narrow;
    for (const uint64_t* bv : narrow_bvs) {
        Leaf l;
        for (const auto& lit : lits)
            if (lit.first.bv == bv) l = lit.first;
        const double s = literal_selectivity(t, l, false, &rc);
        if (rc) return rc;
        PendingK0 k;
        take(bv, &k);
        narrow.push_back({s, k});
    }
    // most selective first (ties: column order, so the plan does not depend on the text order)
    std::sort(narrow.begin(), narrow.end(), [](const auto& x, const auto& y) {
        return x.first != y.first ? x.first < y.first
                                  : (x.second.col != y.second.col ? x.second.col < y.second.col : x.second.c < y.second.c);
    });
    std::vector<const uint64_t*> rest_bvs = other_bvs;  // K0 leaves inside the other conjuncts: in full
    for (const auto& lit : rest) rest_bvs.push_back(lit.first.bv);
    for (const uint64_t* bv : rest_bvs) {
        PendingK0 k;
        if (take(bv, &k)) {
            if (int rc2 = compute_k0(t, k)) return rc2;
            t->last_narrow_cols.push_back(k.col);
        }
    }
    const bool has_rest = !rest.empty() || !others.empty();
    const double mask_sel = has_rest ? rest_sel : narrow.front().first;
    uint64_t* mask = nullptr;
    cubit_ctx* ctx = t->ctx;
    if (has_rest) {
        ExprP r = mk_true();
        for (const auto& lit : rest) r = mk_bin(Expr::AND, r, mk_leaf(lit.first, lit.second));
        for (const ExprP& p : others) r = mk_bin(Expr::AND, r, p);
        if (mask_sel * 32 > 1.0) {
            for (const auto& kv : narrow) pending.push_back(kv.second);
            return compute_rest();
        }
        if (int rc2 = fit(t, r)) return rc2;  // a mask of more leaves than one pass: split
        if (int rc2 = materialize(t, r, &mask)) return rc2;
    } else {
        const PendingK0 first = narrow.front().second;
        narrow.erase(narrow.begin());
        if (int rc2 = compute_k0(t, first)) return rc2;
        t->last_narrow_cols.push_back(first.col);
        mask = first.bv;
        if (mask_sel * 32 > 1.0) {  // too dense a mask: every other K0 leaf in full
            Leaf ml;
            ml.bv = mask;
            ExprP acc = mk_leaf(ml);
            for (const auto& kv : narrow) {
                if (int rc2 = compute_k0(t, kv.second)) return rc2;
                t->last_narrow_cols.push_back(kv.second.col);
                Leaf l;
                l.bv = kv.second.bv;
                acc = mk_bin(Expr::AND, acc, mk_leaf(l));
            }
            e = acc;
            return compute_rest();
        }
    }
    for (const auto& kv : narrow) {
        const PendingK0& k = kv.second;
        const Column& cl = t->cols.at(k.col);
        HIP_CHECK(launch_masked_compare(cl.data, ktype(cl), cl.validity, mask, t->n_rows, k.cmp, k.c, k.bv, ctx->stream));
        mask = k.bv;
        t->last_narrowed++;
        t->last_narrow_cols.push_back(k.col);
    }
    Leaf ml;
    ml.bv = mask;
    e = mk_leaf(ml);
    return compute_rest();
}

// Reduce an expression until it fits one kernel pass (<= kMaxLeaves leaves, depth <= 4):
// descend into a child that does not fit; when both children fit but not together,
// materialise the larger one into a scratch bitvector (one bits-only pass).
int fit(cubit_table* t, ExprP& e) {
    for (int guard = 0; guard < 256; ++guard) {
        if (fits(e)) return CUBIT_OK;
        ExprP* cur = &e;
        for (;;) {
            if ((*cur)->kind == Expr::LEAF) return fail(CUBIT_ERR_UNSUPPORTED, "cannot split program");
            ExprP& a = (*cur)->a;
            ExprP& b = (*cur)->b;
            if (!fits(a)) {
                cur = &a;
                continue;
            }
            if (!fits(b)) {
                cur = &b;
                continue;
            }
            ExprP* m = count_leaves(a) >= count_leaves(b) ? &a : &b;
            if ((*m)->kind == Expr::LEAF) m = (m == &a) ? &b : &a;
            uint64_t* bv = nullptr;
            if (int rc = materialize(t, *m, &bv)) return rc;
            Leaf l;
            l.bv = bv;
            *m = mk_leaf(l);
            break;
        }
    }
    return fail(CUBIT_ERR_UNSUPPORTED, "program too large");
}

// Copy-on-write patch of every leaf on an updated column: rows whose update is visible to
// the transaction get the bit their visible value implies (UpdatesForTransaction,
// update_info.hpp:44-55). Done on the device: copy the leaf, clear the updated rows, then
// set the rows whose visible value passes the leaf predicate.
__global__ void patch_leaf_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ values,
                                  const uint8_t* __restrict__ valids, const uint64_t* __restrict__ versions, uint64_t n,
                                  uint64_t start_time, uint64_t tid, int pred, int cmp, int64_t c, int64_t c2,
                                  int type, uint64_t* __restrict__ bv) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t ver = versions[i];
        if (!(ver < start_time || ver == tid)) continue;
        const int64_t r = rows[i];
        // only the newest visible update of a row decides (records are chronological and
        // grouped by row by the host)
        bool newest = true;
        for (uint64_t j = i + 1; j < n && rows[j] == r; ++j) {
            const uint64_t vj = versions[j];
            if (vj < start_time || vj == tid) {
                newest = false;
                break;
            }
        }
        if (!newest) continue;
        const int64_t v = value_key(type, values[i]);  // the leaf's constants are keys (FLOAT / DOUBLE)
        // a SET NULL record: the row leaves the validity leaf and fails every comparison
        // (UpdateMergeValidity, update_segment.cpp:94-99; NULL never passes a filter)
        const bool ok = !valids || valids[i];
        bool p;
        if (pred == 1) p = ok;
        else if (!ok) p = false;
        else if (pred == 2) p = v >= c && v < c2;
        else if (cmp == 0) p = v == c;
        else if (cmp == 1) p = v != c;
        else if (cmp == 2) p = v < c;
        else if (cmp == 3) p = v <= c;
        else if (cmp == 4) p = v > c;
        else p = v >= c;
        unsigned long long* w = reinterpret_cast<unsigned long long*>(&bv[r >> 6]);
        const uint64_t bit = 1ull << (r & 63);
        if (p) atomicOr(w, bit);
        else atomicAnd(w, ~bit);
    }
}

int patch_updates(cubit_table* t, ExprP& e, const cubit_txn* txn, std::map<const uint64_t*, uint64_t*>& patched) {
    if (e->kind == Expr::LEAF) {
        auto uit = t->upd.find(e->leaf.column);
        if (uit == t->upd.end() || !uit->second.any_visible(txn)) return CUBIT_OK;
        auto pit = patched.find(e->leaf.bv);
        uint64_t* copy = nullptr;
        Updates& u = uit->second;
        const auto& dv = u.distinct_versions;
        const bool own = txn->transaction_id >= txn->start_time &&
                         std::binary_search(dv.begin(), dv.end(), txn->transaction_id);
        const int64_t prefix = std::lower_bound(dv.begin(), dv.end(), txn->start_time) - dv.begin();
        const Updates::PatchKey key{e->leaf.pred, e->leaf.cmp, e->leaf.constant, e->leaf.constant2};
        Updates::Patched* slot = own ? nullptr : &u.cache[key];
        if (pit != patched.end()) {
            copy = pit->second;
        } else if (slot && slot->bv && slot->prefix == prefix) {
            copy = static_cast<uint64_t*>(slot->bv->p);  // patched by an earlier scan of this snapshot set
            patched[e->leaf.bv] = copy;
        } else {
            if (slot) {
                if (!slot->bv) {
                    auto b = std::make_unique<DevBuf>();
                    if (hipMalloc(&b->p, t->nwp * 8) != hipSuccess)
                        return fail(CUBIT_ERR_OOM, "patched leaf allocation failed");
                    slot->bv = std::move(b);
                }
                copy = static_cast<uint64_t*>(slot->bv->p);
                slot->prefix = prefix;
            } else if (int rc = scratch_bv(t, &copy)) {
                return rc;
            }
            HIP_CHECK(hipMemcpyAsync(copy, e->leaf.bv, t->nwp * 8, hipMemcpyDeviceToDevice, t->ctx->stream));
            const unsigned grid = (unsigned)std::min<uint64_t>((u.n + 255) / 256, 4096);
            hipLaunchKernelGGL(patch_leaf_kernel, dim3(std::max(grid, 1u)), dim3(256), 0, t->ctx->stream,
                               static_cast<const int64_t*>(u.rows->p), static_cast<const int64_t*>(u.values->p),
                               u.d_valids(), static_cast<const uint64_t*>(u.versions->p), u.n, txn->start_time,
                               txn->transaction_id, e->leaf.pred, e->leaf.cmp, e->leaf.constant, e->leaf.constant2,
                               t->cols.at(e->leaf.column).type, copy);
            HIP_CHECK(hipGetLastError());
            patched[e->leaf.bv] = copy;
        }
        Leaf l = e->leaf;
        l.bv = copy;
        // the copy differs from the base only in zones holding an update record of the column
        if (!l.zbv) l.zbv = e->leaf.bv;
        l.zdirty = e->leaf.column;
        e = mk_leaf(l, e->neg);
        return CUBIT_OK;
    }
    if (e->kind == Expr::CONST_TRUE || e->kind == Expr::CONST_FALSE) return CUBIT_OK;
    if (int rc = patch_updates(t, e->a, txn, patched)) return rc;
    return patch_updates(t, e->b, txn, patched);
}

// ---- zonemaps: the reference skips a row group (RowGroup::CheckZonemap, row_group.cpp:361-371)
// or a run of vectors (CheckZonemapSegments, row_group.cpp:407-445) when a filter's
// CheckStatistics (constant_filter.cpp:11-32) proves it false on the segment's min/max. Here the
// statistics are the bitvectors themselves: per zone, "no row set" / "every row set". The
// expression's zone classes follow three-valued logic, and zones it proves empty are skipped.

using ZoneMap = cubit_table::ZoneMap;

// zones that hold at least one row of the partition
uint32_t real_zones(const cubit_table* t) { return (uint32_t)((t->n_rows + kZoneRows - 1) / kZoneRows); }

// the table-owned bitvectors (kZoneBits) and the columns (kZoneStats) an expression's leaves
// take their zone classes from
void collect_zone_sources(const ExprP& e, std::vector<const uint64_t*>& bvs, std::vector<int>& cols) {
    if (e->kind == Expr::LEAF) {
        const uint64_t* key = e->leaf.zbv ? e->leaf.zbv : e->leaf.bv;
        if (e->leaf.zsrc == kZoneBits && std::find(bvs.begin(), bvs.end(), key) == bvs.end()) bvs.push_back(key);
        if (e->leaf.zsrc == kZoneStats && std::find(cols.begin(), cols.end(), e->leaf.column) == cols.end())
            cols.push_back(e->leaf.column);
        return;
    }
    if (e->a) collect_zone_sources(e->a, bvs, cols);
    if (e->b) collect_zone_sources(e->b, bvs, cols);
}

// device scratch for zone summaries
uint8_t* zone_scratch(cubit_table* t, uint64_t bytes) {
    if (bytes > t->zone_dev_bytes) {
        t->zone_dev = std::make_unique<DevBuf>();
        t->zone_dev_bytes = 0;
        if (hipMalloc(&t->zone_dev->p, bytes) != hipSuccess) return nullptr;
        t->zone_dev_bytes = bytes;
    }
    return static_cast<uint8_t*>(t->zone_dev->p);
}

// Zone maps for the table-owned bitvectors `bvs` and zone statistics for the columns `cols`
// that have none yet: one classification launch per bitvector (zone_class_kernel reads it
// once), one statistics launch per column, one copy back.
int ensure_zones(cubit_table* t, const std::vector<const uint64_t*>& bvs, const std::vector<int>& cols) {
    std::vector<const uint64_t*> todo;
    for (const uint64_t* b : bvs)
        if (!t->zones.count(b)) todo.push_back(b);
    std::vector<int> todo_c;
    for (int c : cols)
        if (!t->col_zones.count(c)) todo_c.push_back(c);
    if (todo.empty() && todo_c.empty()) return CUBIT_OK;
    const uint32_t nz = real_zones(t);
    // min, max (int64) + flags per zone, each column's block 8-byte aligned
    const uint64_t per_col = ((uint64_t)nz * 17 + 7) / 8 * 8;
    // class bytes of the bitvectors, then their per-zone counts (4-byte aligned), then the
    // columns' statistics (8-byte aligned)
    const uint64_t cnt_base = ((uint64_t)todo.size() * nz + 3) / 4 * 4;
    const uint64_t cbase = (cnt_base + (uint64_t)todo.size() * nz * 4 + 7) / 8 * 8;
    const uint64_t bytes = cbase + (uint64_t)todo_c.size() * per_col + 16;
    uint8_t* dev = zone_scratch(t, bytes);
    if (!dev) return fail(CUBIT_ERR_OOM, "zone classes allocation failed");
    hipStream_t s = t->ctx->stream;
    for (size_t i = 0; i < todo.size(); ++i)
        HIP_CHECK(launch_zone_classes(todo[i], t->n_rows, 0, nz, dev + i * nz, s,
                                      reinterpret_cast<uint32_t*>(dev + cnt_base) + i * nz));
    for (size_t i = 0; i < todo_c.size(); ++i) {
        const Column& c = t->cols.at(todo_c[i]);
        uint8_t* p = dev + cbase + i * per_col;
        HIP_CHECK(launch_column_zone_stats(c.data, ktype(c), c.validity, t->n_rows, nz, reinterpret_cast<int64_t*>(p),
                                           reinterpret_cast<int64_t*>(p + 8ull * nz), p + 16ull * nz, s));
    }
    std::vector<uint8_t> host(cbase + todo_c.size() * per_col);
    HIP_CHECK(hipMemcpyAsync(host.data(), dev, host.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t nw = (nz + 63) / 64;
    for (size_t i = 0; i < todo.size(); ++i) {
        ZoneMap m;
        m.z.assign(nw, 0);
        m.o.assign(nw, 0);
        for (uint32_t z = 0; z < nz; ++z) {
            const uint8_t c = host[i * nz + z];
            if (c & 1) m.z[z >> 6] |= 1ull << (z & 63);
            if (c & 2) m.o[z >> 6] |= 1ull << (z & 63);
            m.informative |= c != 0;
        }
        m.cnt.resize(nz);
        std::memcpy(m.cnt.data(), host.data() + cnt_base + 4ull * i * nz, 4ull * nz);
        t->zones.emplace(todo[i], std::move(m));
    }
    for (size_t i = 0; i < todo_c.size(); ++i) {
        const uint8_t* p = host.data() + cbase + i * per_col;
        cubit_table::ColZones cz;
        cz.mn.resize(nz);
        cz.mx.resize(nz);
        std::memcpy(cz.mn.data(), p, 8ull * nz);
        std::memcpy(cz.mx.data(), p + 8ull * nz, 8ull * nz);
        cz.fl.assign(p + 16ull * nz, p + 17ull * nz);
        t->col_zones.emplace(todo_c[i], std::move(cz));
    }
    return CUBIT_OK;
}

// Zone map of the leaf {valid rows with v cmp c} of column col from the column's zone statistics:
// ConstantFilter::CheckStatistics → NumericStats::CheckZonemap (constant_filter.cpp:11-32,
// numeric_stats.cpp:157-228) — FILTER_ALWAYS_FALSE = every valid value fails (or no row is
// valid), FILTER_ALWAYS_TRUE = every value passes and every row is valid.
const ZoneMap& stats_zone_map(cubit_table* t, const Leaf& l) {
    const auto key = std::make_tuple(l.column, l.pred, l.cmp, l.constant, l.constant2);
    auto it = t->pred_zones.find(key);
    if (it != t->pred_zones.end()) return it->second;
    const cubit_table::ColZones& cz = t->col_zones.at(l.column);
    const uint32_t nz = (uint32_t)cz.fl.size();
    ZoneMap m;
    m.z.assign((nz + 63) / 64, 0);
    m.o.assign((nz + 63) / 64, 0);
    const int64_t c = l.constant;
    for (uint32_t z = 0; z < nz; ++z) {
        const int64_t lo = cz.mn[z], hi = cz.mx[z];
        bool none, all;
        if (!(cz.fl[z] & 1)) {
            none = true;
            all = false;
        } else if (l.pred == 2) {  // c <= v < constant2
            none = hi < c || lo >= l.constant2;
            all = lo >= c && hi < l.constant2 && (cz.fl[z] & 2);
        } else {
            switch (l.cmp) {
            case CUBIT_CMP_EQ: none = c < lo || c > hi; all = lo == c && hi == c; break;
            case CUBIT_CMP_NE: none = lo == c && hi == c; all = c < lo || c > hi; break;
            case CUBIT_CMP_LT: none = lo >= c; all = hi < c; break;
            case CUBIT_CMP_LE: none = lo > c; all = hi <= c; break;
            case CUBIT_CMP_GT: none = hi <= c; all = lo > c; break;
            default: none = hi < c; all = lo >= c; break;  // GE
            }
            all = all && (cz.fl[z] & 2);
        }
        if (none) m.z[z >> 6] |= 1ull << (z & 63);
        if (all) m.o[z >> 6] |= 1ull << (z & 63);
        m.informative |= none || all;
    }
    return t->pred_zones.emplace(key, std::move(m)).first->second;
}

// Estimated fraction of the partition's rows whose value of column col lies in [lo, hi) (valid
// rows only), from the column's per-zone min / max (values uniform between them in each zone):
// the planner's cost model for narrowing. Exactness never depends on it.
double interval_selectivity(cubit_table* t, int col, double lo_c, double hi_c, int* rc) {
    if (!t->cols.count(col) || t->n_rows == 0) return 1.0;
    if ((*rc = ensure_zones(t, {}, {col}))) return 1.0;
    const cubit_table::ColZones& cz = t->col_zones.at(col);
    const uint32_t nz = (uint32_t)cz.fl.size();
    // FLOAT / DOUBLE: zone bounds and the interval are keys; values are taken uniform in value
    // (not key) space, so every bound is mapped back to the value it names (NaN, the greatest
    // value, and ±inf as ±inf; a zone with an infinite span counts as an outlier below)
    const int type = t->cols.at(col).type;
    const bool fp = type_is_fp(type);
    auto value_of = [type](double k) -> double {
        if (std::isinf(k)) return k;
        const int64_t key = k >= 9.2e18 ? INT64_MAX : k <= -9.2e18 ? INT64_MIN + 1 : (int64_t)k;
        const int64_t bits = cubit_fp_value(type, key);
        double v;
        if (type == CUBIT_TYPE_FLOAT) {
            float f;
            const uint32_t u = (uint32_t)bits;
            std::memcpy(&f, &u, 4);
            v = f;
        } else {
            std::memcpy(&v, &bits, 8);
        }
        return std::isnan(v) ? std::numeric_limits<double>::infinity() : v;
    };
    if (fp) {
        lo_c = value_of(lo_c);
        hi_c = value_of(hi_c);
    }
    auto zone_bounds = [&](uint32_t z, double& lo, double& hi) {
        if (fp) {
            lo = value_of((double)cz.mn[z]);
            hi = value_of((double)cz.mx[z]);
            if (hi == lo) hi = std::nextafter(hi, std::numeric_limits<double>::infinity());
        } else {
            lo = (double)cz.mn[z];
            hi = (double)cz.mx[z] + 1.0;
        }
    };
    // a zone whose value span is far wider than the typical zone's holds a few outliers (one
    // extreme value stretches the uniform assumption over the whole type range): it counts at
    // the other zones' mean fraction instead
    std::vector<double> spans;
    for (uint32_t z = 0; z < nz; ++z) {
        if (!(cz.fl[z] & 1)) continue;
        double lo, hi;
        zone_bounds(z, lo, hi);
        if (std::isfinite(hi - lo)) spans.push_back(hi - lo);
    }
    double median_span = 0.0;
    if (!spans.empty()) {
        std::nth_element(spans.begin(), spans.begin() + spans.size() / 2, spans.end());
        median_span = spans[spans.size() / 2];
    }
    double kept = 0.0, normal_rows = 0.0, outlier_rows = 0.0;
    for (uint32_t z = 0; z < nz; ++z) {
        const double rows = (double)std::min<uint64_t>(kZoneRows, t->n_rows - (uint64_t)z * kZoneRows);
        if (!(cz.fl[z] & 1)) continue;  // no valid row passes a comparison
        double lo, hi;
        zone_bounds(z, lo, hi);
        const double span = hi - lo;
        if (!std::isfinite(span) || ((median_span > 1.0 || (fp && median_span > 0.0)) && span > 8.0 * median_span)) {
            outlier_rows += rows;
            continue;
        }
        const double f = std::max(0.0, std::min(hi, hi_c) - std::max(lo, lo_c)) / span;
        kept += f * rows;  // NULL rows of a mixed zone counted as valid: an over-estimate
        normal_rows += rows;
    }
    if (outlier_rows > 0.0) kept += outlier_rows * (normal_rows > 0.0 ? kept / normal_rows : 0.5);
    return std::min(1.0, kept / (double)t->n_rows);
}

// Estimated fraction of rows a conjunction of literals keeps: the literals of one column fold
// into one interval (a range index answers `a <= v < b` as L(b) AND NOT L(a): two literals of
// one predicate, not independent ones), the columns multiply (independence), literals that
// fold into no interval (NOT (v = c), NOT of a bin) multiply as 1 - their own fraction, and
// leaves not derived from a column value (visibility, materialised subtrees) keep every row.
double conj_selectivity(cubit_table* t, const Emitter::Lits& lits, int* rc) {
    const double inf = std::numeric_limits<double>::infinity();
    std::map<int, std::pair<double, double>> iv;
    double sel = 1.0;
    for (const auto& lit : lits) {
        const Leaf& l = lit.first;
        const bool neg = lit.second;
        if (l.sel >= 0.0) {  // a derived leaf that is no interval: the estimate of what it replaced
            sel *= neg ? 1.0 - l.sel : l.sel;
            continue;
        }
        if (l.pred == 3 && l.column < 0) {  // a kept chain: the estimate of what it replaced, made once
            auto it = t->derived_bvs.find(l.bv);
            if (it == t->derived_bvs.end()) continue;
            DerivedLeaf& d = *it->second;
            if (d.sel < 0.0) {
                std::vector<ExprP> parts;
                conj_parts(d.replaced, parts);
                Emitter::Lits c;
                double s = 1.0;
                for (const ExprP& p : parts) {
                    if (p->kind == Expr::LEAF) c.push_back({p->leaf, p->neg});
                    else s *= expr_selectivity(t, p, rc);
                }
                s *= conj_selectivity(t, c, rc);
                if (*rc) return 1.0;
                d.sel = std::min(1.0, std::max(0.0, s));
            }
            sel *= neg ? 1.0 - d.sel : d.sel;
            continue;
        }
        if (l.column < 0 || l.pred == 1) continue;
        auto& r = iv.emplace(l.column, std::make_pair(-inf, inf)).first->second;
        const double c = (double)l.constant;
        double lo = -inf, hi = inf;  // the literal as [lo, hi), when it is one interval
        bool interval = true;
        if (l.pred == 2) {
            lo = c;
            hi = (double)l.constant2;
            interval = !neg;
        } else {
            switch (l.cmp) {
            case CUBIT_CMP_EQ: lo = c; hi = c + 1; interval = !neg; break;
            case CUBIT_CMP_NE: lo = c; hi = c + 1; interval = neg; break;  // NOT (v != c) = (v = c)
            case CUBIT_CMP_LT: (neg ? lo : hi) = c; break;
            case CUBIT_CMP_LE: (neg ? lo : hi) = c + 1; break;
            case CUBIT_CMP_GT: (neg ? hi : lo) = c + 1; break;
            default: (neg ? hi : lo) = c; break;  // GE
            }
        }
        if (interval) {
            r.first = std::max(r.first, lo);
            r.second = std::min(r.second, hi);
        } else {
            sel *= 1.0 - interval_selectivity(t, l.column, lo, hi, rc);
            if (*rc) return 1.0;
        }
    }
    for (const auto& kv : iv) {
        if (kv.second.first == -inf && kv.second.second == inf) continue;
        sel *= interval_selectivity(t, kv.first, kv.second.first, kv.second.second, rc);
        if (*rc) return 1.0;
    }
    return sel;
}

double literal_selectivity(cubit_table* t, const Leaf& l, bool neg, int* rc) {
    Emitter::Lits one{{l, neg}};
    return conj_selectivity(t, one, rc);
}

struct ZoneSet {
    std::vector<uint64_t> z, o;  // zones where the expression is false / true on every row
};

// zones holding an update record of column col (any version), a bit per zone
const std::vector<uint64_t>& dirty_zones(cubit_table* t, int col) {
    static const std::vector<uint64_t> none;
    auto it = t->upd.find(col);
    if (it == t->upd.end()) return none;
    Updates& u = it->second;
    const uint32_t nz = real_zones(t);
    if (u.dirty_nz != nz) {
        u.dirty.assign((nz + 63) / 64, 0);
        for (int64_t r : u.h_rows) {
            const uint64_t z = (uint64_t)r / kZoneRows;
            if (z < nz) u.dirty[z >> 6] |= 1ull << (z & 63);
        }
        u.dirty_nz = nz;
    }
    return u.dirty;
}

// three-valued evaluation of an expression over zone classes; leaves without zone classes are
// mixed everywhere
void zone_eval(cubit_table* t, const ExprP& e, size_t nw, ZoneSet& r) {
    switch (e->kind) {
    case Expr::LEAF: {
        const ZoneMap* m = nullptr;
        if (e->leaf.zsrc == kZoneBits) {
            auto it = t->zones.find(e->leaf.zbv ? e->leaf.zbv : e->leaf.bv);
            if (it != t->zones.end()) m = &it->second;
        } else if (e->leaf.zsrc == kZoneStats) {
            m = &stats_zone_map(t, e->leaf);
        }
        if (m) {
            r.z = m->z;
            r.o = m->o;
        } else {
            r.z.assign(nw, 0);
            r.o.assign(nw, 0);
        }
        if (m && e->leaf.zdirty >= 0) {  // patched: zones with an update record are mixed
            const std::vector<uint64_t>& d = dirty_zones(t, e->leaf.zdirty);
            for (size_t w = 0; w < nw && w < d.size(); ++w) {
                r.z[w] &= ~d[w];
                r.o[w] &= ~d[w];
            }
        }
        if (e->neg) std::swap(r.z, r.o);
        return;
    }
    case Expr::CONST_TRUE:
        r.z.assign(nw, 0);
        r.o.assign(nw, ~0ull);
        return;
    case Expr::CONST_FALSE:
        r.z.assign(nw, ~0ull);
        r.o.assign(nw, 0);
        return;
    default: break;
    }
    ZoneSet b;
    zone_eval(t, e->a, nw, r);
    zone_eval(t, e->b, nw, b);
    for (size_t w = 0; w < nw; ++w) {
        const uint64_t az = r.z[w], ao = r.o[w];
        switch (e->kind) {
        case Expr::AND: r.z[w] = az | b.z[w]; r.o[w] = ao & b.o[w]; break;
        case Expr::OR: r.z[w] = az & b.z[w]; r.o[w] = ao | b.o[w]; break;
        default: r.z[w] = az | b.o[w]; r.o[w] = ao & b.z[w]; break;  // ANDNOT
        }
    }
}

// does any leaf carry a zone class other than "mixed"?
bool zone_informative(cubit_table* t, const ExprP& e) {
    if (e->kind == Expr::LEAF) {
        if (e->leaf.zsrc == kZoneBits) {
            auto it = t->zones.find(e->leaf.zbv ? e->leaf.zbv : e->leaf.bv);
            return it != t->zones.end() && it->second.informative;
        }
        if (e->leaf.zsrc == kZoneStats) return stats_zone_map(t, e->leaf).informative;
        return false;
    }
    return (e->a && zone_informative(t, e->a)) || (e->b && zone_informative(t, e->b));
}

// The zonemap skip of a planned expression. live = the zones a kernel must evaluate, when at
// least one zone in 32 provably holds no qualifying row (below that the list and the cleared
// directory cost about what the skipped reads save); left empty otherwise = every zone.
// *none = no zone can hold a qualifying row.
int zone_plan(cubit_table* t, const ExprP& e, std::vector<uint32_t>& live, bool* none) {
    live.clear();
    *none = false;
    std::vector<const uint64_t*> bvs;
    std::vector<int> cols;
    collect_zone_sources(e, bvs, cols);
    if (bvs.empty() && cols.empty()) return CUBIT_OK;
    if (int rc = ensure_zones(t, bvs, cols)) return rc;
    if (!zone_informative(t, e)) return CUBIT_OK;  // every zone of every leaf mixed: nothing to skip
    const uint32_t nz = real_zones(t);
    ZoneSet r;
    zone_eval(t, e, (nz + 63) / 64, r);
    uint32_t dead = 0;
    for (uint32_t z = 0; z < nz; ++z) dead += (uint32_t)((r.z[z >> 6] >> (z & 63)) & 1);
    if (dead == nz) {
        *none = true;
        return CUBIT_OK;
    }
    if (dead == 0 || (uint64_t)dead * 32 < nz) return CUBIT_OK;
    live.reserve(nz - dead);
    for (uint32_t z = 0; z < nz; ++z)
        if (!((r.z[z >> 6] >> (z & 63)) & 1)) live.push_back(z);
    return CUBIT_OK;
}

// [lo, hi) of the values a comparison keeps (NE: the interval it removes); false for NE.
bool cmp_interval(int cmp, int64_t c, double* lo, double* hi) {
    const double inf = std::numeric_limits<double>::infinity(), x = (double)c;
    *lo = -inf;
    *hi = inf;
    switch (cmp) {
    case CUBIT_CMP_EQ: *lo = x; *hi = x + 1; return true;
    case CUBIT_CMP_NE: *lo = x; *hi = x + 1; return false;
    case CUBIT_CMP_LT: *hi = x; return true;
    case CUBIT_CMP_LE: *hi = x + 1; return true;
    case CUBIT_CMP_GT: *lo = x + 1; return true;
    default: *lo = x; return true;  // GE
    }
}

// Filter nodes with the constants on FLOAT / DOUBLE columns replaced by their comparison keys
// (cubit_fp_key): the planner, the zone statistics, the index keys and every kernel compare keys,
// so DuckDB's floating-point operators (NaN greatest and equal to NaN, -0.0 == +0.0) become integer
// comparisons. Nodes on other columns are used as given (no copy when there are none).
struct KeyedNodes {
    std::vector<cubit_filter_node> buf;
    const cubit_filter_node* p;
    int rc = CUBIT_OK;
    KeyedNodes(const cubit_table* t, const cubit_filter_node* nodes, uint32_t n) : p(nodes) {
        for (uint32_t k = 0; k < n; ++k) {
            if (nodes[k].kind != CUBIT_FILTER_CONSTANT) continue;
            auto it = t->cols.find(nodes[k].column);
            if (it == t->cols.end() || (!type_is_keyed(it->second.type) && it->second.type != CUBIT_TYPE_VARCHAR)) continue;
            if (buf.empty()) {
                buf.assign(nodes, nodes + n);
                p = buf.data();
            }
            if (it->second.type != CUBIT_TYPE_VARCHAR) {
                buf[k].constant = value_key(it->second.type, nodes[k].constant);
                continue;
            }
            // a string constant → a comparison of codes with the same rows: lb = the first code whose
            // string is >= s; s absent: = matches nothing (code -1), != every valid row, <= is < lb,
            // > is >= lb
            const cubit_string* str = reinterpret_cast<const cubit_string*>((intptr_t)nodes[k].constant);
            if (!str || (str->size && !str->data)) {
                rc = fail(CUBIT_ERR_INVALID, "filter node %u: a VARCHAR constant must be a cubit_string", k);
                return;
            }
            bool present = false;
            const int64_t lb =
                (int64_t)it->second.dict->lower_bound(std::string_view(str->data ? str->data : "", str->size), &present);
            int cmp = nodes[k].cmp;
            int64_t c = lb;
            if (!present) {
                if (cmp == CUBIT_CMP_EQ || cmp == CUBIT_CMP_NE) c = -1;
                else if (cmp == CUBIT_CMP_LE) cmp = CUBIT_CMP_LT;
                else if (cmp == CUBIT_CMP_GT) cmp = CUBIT_CMP_GE;
            }
            buf[k].cmp = cmp;
            buf[k].constant = c;
        }
    }
};

// Estimated fraction of the partition's rows a filter tree (prefix nodes from i; i ends past the
// subtree) keeps, on the planner's cost model (interval_selectivity: per-zone min / max, values
// uniform within a zone, columns independent). An AND folds its constant children on one column
// into one interval (a pushed TableFilterSet's `a <= v AND v < b`); an OR keeps 1 - Π(1 - s);
// IS NULL counts the zones that hold a NULL. MVCC deletes only lower the true fraction.
double tree_selectivity(cubit_table* t, const cubit_filter_node* nodes, uint32_t& i, int* rc) {
    const cubit_filter_node& f = nodes[i++];
    double lo, hi;
    switch (f.kind) {
    case CUBIT_FILTER_AND: {
        std::map<int, std::pair<double, double>> iv;
        double sel = 1.0;
        for (int k = 0; k < f.n_children && !*rc; ++k) {
            const cubit_filter_node& c = nodes[i];
            if (c.kind == CUBIT_FILTER_CONSTANT && c.cmp != CUBIT_CMP_NE) {
                cmp_interval(c.cmp, c.constant, &lo, &hi);
                const double inf = std::numeric_limits<double>::infinity();
                auto& r = iv.emplace(c.column, std::make_pair(-inf, inf)).first->second;
                r.first = std::max(r.first, lo);
                r.second = std::min(r.second, hi);
                ++i;
            } else {
                sel *= tree_selectivity(t, nodes, i, rc);
            }
        }
        for (const auto& kv : iv) {
            if (*rc) break;
            sel *= kv.second.second <= kv.second.first ? 0.0
                                                       : interval_selectivity(t, kv.first, kv.second.first, kv.second.second, rc);
        }
        return sel;
    }
    case CUBIT_FILTER_OR: {
        double none = 1.0;
        for (int k = 0; k < f.n_children && !*rc; ++k) none *= 1.0 - tree_selectivity(t, nodes, i, rc);
        return 1.0 - none;
    }
    case CUBIT_FILTER_CONSTANT: {
        const bool in = cmp_interval(f.cmp, f.constant, &lo, &hi);
        const double s = interval_selectivity(t, f.column, lo, hi, rc);
        return in ? s : 1.0 - s;
    }
    case CUBIT_FILTER_IS_NULL: {
        if (!t->cols.at(f.column).validity || t->n_rows == 0) return 0.0;
        if ((*rc = ensure_zones(t, {}, {f.column}))) return 1.0;
        const auto& fl = t->col_zones.at(f.column).fl;
        double rows = 0.0;
        for (uint32_t z = 0; z < (uint32_t)fl.size(); ++z)
            if (!(fl[z] & 2)) rows += (double)std::min<uint64_t>(kZoneRows, t->n_rows - (uint64_t)z * kZoneRows);
        return std::min(1.0, rows / (double)t->n_rows);
    }
    default:  // IS NOT NULL
        return 1.0;
    }
}

}  // namespace

extern "C" int cubit_table_estimate_rows(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                         uint64_t* rows) {
    if (!t || !rows || (n_nodes && !nodes)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *rows = t->n_rows;
    if (n_nodes == 0 || t->n_rows == 0) return CUBIT_OK;
    if (filter_subtree_end(nodes, n_nodes, 0) != (int)n_nodes) return fail(CUBIT_ERR_INVALID, "malformed filter tree");
    for (uint32_t k = 0; k < n_nodes; ++k)
        if (int rc = check_node(t, nodes[k])) return rc;
    if (int rc = set_device(t->ctx)) return rc;
    int rc = CUBIT_OK;
    uint32_t i = 0;
    const KeyedNodes keyed(t, nodes, n_nodes);
    if (keyed.rc) return keyed.rc;
    const double s = std::min(1.0, std::max(0.0, tree_selectivity(t, keyed.p, i, &rc)));
    if (rc) return rc;
    *rows = std::min<uint64_t>(t->n_rows, (uint64_t)std::ceil(s * (double)t->n_rows));
    return CUBIT_OK;
}

namespace {

// ---- derived leaves (policy: cubit_derived.hpp). A pass over the planned expression, before the
// MVCC patches, the zonemap skip and the split into passes: in every AND chain and every OR chain
// the literals on table-owned bitvectors of one column form a group (the interval of a RANGE index,
// L(hi) AND NOT L(lo), with or without the validity leaf; the union of EQUALITY or BINS leaves).
// A group planned often enough is evaluated once by the bits-only pass into a table-owned
// bitvector, and this and later plans read that one leaf in its place. In every AND chain (those
// under an OR included) the derivable literals of all columns together, with the unions of one
// column's leaves, form a chain: a repeated WHERE clause. A kept chain is looked up first and one
// leaf replaces all its literals; otherwise the column groups take theirs, the chain's request is
// counted, and it is bought by cost (derived_chain_admit) from what the plan reads in its place.
// Literals that are not derivable (K0, candidate-check, sliced and scratch leaves, a column whose
// update records the transaction sees; the visibility leaf is added later) stay outside and are
// ANDed with the kept leaf.

// bytes the derived leaves of a table may hold unless cubit_table_set_derived_budget said
// otherwise: a quarter of its own index bitvectors
uint64_t default_derived_budget(const cubit_table* t) {
    uint64_t n = 0;
    for (const auto* m : {&t->idx, &t->bins, &t->sliced})
        for (const auto& kv : *m) n += kv.second.bvs.size();
    return n * std::max<uint64_t>(t->cap_words, 1) * 8 / 4;
}

// a literal that may join a group: a table-owned index or validity bitvector as it stands (not a
// derived leaf: its address can be handed out again), on a column whose leaves this transaction
// does not see patched
bool derivable(const cubit_table* t, const ExprP& p, const cubit_txn* txn) {
    if (p->kind != Expr::LEAF) return false;
    const Leaf& l = p->leaf;
    if (l.zsrc != kZoneBits || l.zbv || l.zdirty >= 0 || l.column < 0 || t->derived_bvs.count(l.bv)) return false;
    auto u = t->upd.find(l.column);
    return u == t->upd.end() || !u->second.any_visible(txn);
}

// Evaluate e (the combination `key` names, as the plan reads it now) with the bits-only pass into
// a table-owned bitvector, keep it under `key` and hand out the leaf l on it. *out stays null
// when there is no memory to keep it: the plan reads its literals.
int keep_derived(cubit_table* t, const DerivedKey& key, uint64_t bytes, const ExprP& e, Leaf l, ExprP* out) {
    const bool is_chain = derived_is_chain(key);
    auto b = std::make_unique<DevBuf>();
    if (alloc_derived_bv(t, *b, padded_words(t->n_rows)) != CUBIT_OK) {  // the pass below writes those words
        (void)hipGetLastError();
        return CUBIT_OK;
    }
    Emitter em;
    em.emit_top(e);
    uint64_t* words = static_cast<uint64_t*>(b->p);
    t->last_passes++;
    if (int rc = run_eval(t->ctx, em.prog, t->n_rows, 0, nullptr, 0, t->dummy_count, words, RunMode::kCount)) return rc;
    l.bv = words;
    DerivedLeaf d;
    d.bv = std::move(b);
    d.block_bytes = std::max<uint64_t>(t->cap_words, 1) * 8;
    d.leaf = l;
    if (is_chain) d.replaced = e;
    t->derived_bvs[words] = t->derived.insert(key, bytes, std::move(d));
    shed_row_lists(t);  // the bitvectors grew: lists keep only the room they leave
    *out = mk_leaf(l);
    return CUBIT_OK;
}

// The group g (literals of column col combined by op) as one leaf when it is kept or admitted
// now, else *out = null and the plan keeps its literals.
int derive_group(cubit_table* t, int op, int col, const std::vector<ExprP>& g, ExprP* out) {
    *out = nullptr;
    std::vector<DerivedLit> lits;
    for (const ExprP& p : g) lits.push_back({reinterpret_cast<uintptr_t>(p->leaf.bv), p->neg});
    DerivedKey key;
    if (!derived_key(col, op, std::move(lits), &key)) return CUBIT_OK;
    if (DerivedLeaf* d = t->derived.find(key)) {
        *out = mk_leaf(d->leaf);
        return CUBIT_OK;
    }
    ExprP e = g[0];
    for (size_t i = 1; i < g.size(); ++i) e = mk_bin(op == kDerivedAnd ? Expr::AND : Expr::OR, e, g[i]);
    if (!fits(e)) return CUBIT_OK;
    const uint64_t bytes = std::max<uint64_t>(t->cap_words, 1) * 8;
    if (!t->derived.request(key, bytes)) return CUBIT_OK;
    Leaf l;
    l.column = col;
    l.zsrc = kZoneBits;
    l.pred = 3;
    if (op == kDerivedAnd) {
        // L(hi) AND NOT L(lo) of a range index (its rows are valid ones: the validity leaf adds
        // nothing): the interval lo <= v < hi
        const Leaf *lo = nullptr, *hi = nullptr;
        bool interval = true;
        for (const ExprP& p : g) {
            const Leaf& x = p->leaf;
            if (x.pred == 1 && !p->neg) continue;
            const Leaf*& slot = p->neg ? lo : hi;
            if (x.pred != 0 || x.cmp != CUBIT_CMP_LT || (slot && slot->bv != x.bv)) interval = false;
            slot = &x;
        }
        if (interval && lo && hi && lo->constant < hi->constant) {
            l.pred = 2;
            l.constant = lo->constant;
            l.constant2 = hi->constant;
        }
    }
    if (l.pred == 3) {
        int rc = CUBIT_OK;
        Emitter::Lits c;
        l.sel = op == kDerivedAnd && Emitter::conj_leaves(e, c) ? conj_selectivity(t, c, &rc) : expr_selectivity(t, e, &rc);
        if (rc) return rc;
    }
    return keep_derived(t, key, bytes, e, l, out);
}

// The chain `key` (the AND of g: what the plan reads in its place now, kept column groups and
// unions included) as one leaf when it is admitted now, else *out = null. The leaf has no column:
// it takes its zone classes from its own bits, and the conjunction's selectivity estimate from
// its entry (made from what it replaced when a plan first asks: conj_selectivity).
int derive_chain(cubit_table* t, const DerivedKey& key, const std::vector<ExprP>& g, ExprP* out) {
    *out = nullptr;
    ExprP e = g[0];
    for (size_t i = 1; i < g.size(); ++i) e = mk_bin(Expr::AND, e, g[i]);
    if (!fits(e)) return CUBIT_OK;
    std::vector<const uint64_t*> bvs;
    leaves_of(e, bvs);
    std::sort(bvs.begin(), bvs.end());
    const uint64_t k = std::unique(bvs.begin(), bvs.end()) - bvs.begin();
    const uint64_t bytes = std::max<uint64_t>(t->cap_words, 1) * 8;
    // priced by what this admission would pay: a block waiting in the pool (one of another size is no
    // such block: it goes now, as alloc_derived_bv would send it), or a device allocation
    size_bv_pool(t);
    if (!t->derived.request(key, bytes, k, t->bv_pool.free_blocks() > 0)) return CUBIT_OK;
    Leaf l;
    l.zsrc = kZoneBits;
    l.pred = 3;
    return keep_derived(t, key, bytes, e, l, out);
}

// the key of an OR group that is the union of one column's derivable leaves and nothing else (an
// IN-list on an EQUALITY index, a range over BINS): it may join a chain
bool union_key(const cubit_table* t, const ExprP& p, const cubit_txn* txn, DerivedKey* key) {
    if (p->kind != Expr::OR) return false;
    std::vector<ExprP> parts;
    Emitter::or_parts(p, parts);
    std::vector<DerivedLit> lits;
    for (const ExprP& q : parts) {
        if (!derivable(t, q, txn) || q->leaf.column != parts[0]->leaf.column) return false;
        lits.push_back({reinterpret_cast<uintptr_t>(q->leaf.bv), q->neg});
    }
    return derived_key(parts[0]->leaf.column, kDerivedOr, std::move(lits), key);
}

int derive_leaves(cubit_table* t, ExprP& e, const cubit_txn* txn) {
    if (e->kind == Expr::LEAF || e->kind == Expr::CONST_TRUE || e->kind == Expr::CONST_FALSE) return CUBIT_OK;
    const bool conj = e->kind == Expr::AND || (e->kind == Expr::ANDNOT && e->b->kind == Expr::LEAF);
    if (!conj && e->kind != Expr::OR) {  // a AND NOT (subtree): each side on its own
        if (int rc = derive_leaves(t, e->a, txn)) return rc;
        return derive_leaves(t, e->b, txn);
    }
    std::vector<ExprP> parts;
    if (conj) conj_parts(e, parts);
    else Emitter::or_parts(e, parts);
    bool changed = false;
    std::map<int, std::vector<size_t>> by_col;
    // the chain of an AND chain: its derivable literals and its unions of one column's leaves
    std::vector<size_t> chain_at;
    std::vector<ChainLit> chain_lits;
    std::vector<DerivedKey> chain_unions;
    for (size_t i = 0; i < parts.size(); ++i) {
        if (parts[i]->kind == Expr::LEAF) {
            if (!derivable(t, parts[i], txn)) continue;
            const Leaf& l = parts[i]->leaf;
            by_col[l.column].push_back(i);
            if (conj) {
                chain_at.push_back(i);
                chain_lits.push_back({l.column, {reinterpret_cast<uintptr_t>(l.bv), parts[i]->neg}});
            }
            continue;
        }
        DerivedKey u;
        if (conj && union_key(t, parts[i], txn, &u)) {
            chain_at.push_back(i);
            chain_unions.push_back(std::move(u));
        }
    }
    // the whole chain kept: one leaf in the place of all its literals
    DerivedKey chain;
    bool chain_wanted = conj && derived_chain_key(chain_lits, std::move(chain_unions), &chain);
    if (chain_wanted) {
        if (DerivedLeaf* d = t->derived.find(chain)) {
            for (size_t i : chain_at) parts[i] = nullptr;
            parts[chain_at[0]] = mk_leaf(d->leaf);
            by_col.clear();
            chain_wanted = false;
            changed = true;
        }
    }
    for (size_t i = 0; i < parts.size(); ++i) {
        if (!parts[i] || parts[i]->kind == Expr::LEAF) continue;
        ExprP q = parts[i];
        if (int rc = derive_leaves(t, q, txn)) return rc;
        changed |= q != parts[i];
        parts[i] = q;
    }
    for (const auto& [col, at] : by_col) {
        if (at.size() < 2) continue;
        std::vector<ExprP> g;
        for (size_t i : at) g.push_back(parts[i]);
        ExprP d;
        if (int rc = derive_group(t, conj ? kDerivedAnd : kDerivedOr, col, g, &d)) return rc;
        if (!d) continue;
        for (size_t i : at) parts[i] = nullptr;
        parts[at[0]] = d;
        changed = true;
    }
    // no entry: the chain's request counts, with what the plan reads in its place after the column
    // groups took theirs
    if (chain_wanted) {
        std::vector<ExprP> g;
        for (size_t i : chain_at)
            if (parts[i]) g.push_back(parts[i]);
        ExprP d;
        if (int rc = derive_chain(t, chain, g, &d)) return rc;
        if (d) {
            for (size_t i : chain_at) parts[i] = nullptr;
            parts[chain_at[0]] = d;
            changed = true;
        }
    }
    if (!changed) return CUBIT_OK;  // the expression as the planner built it
    ExprP acc = conj ? mk_true() : mk_false();
    for (const ExprP& p : parts)
        if (p) acc = mk_bin(conj ? Expr::AND : Expr::OR, acc, p);
    e = acc;
    return CUBIT_OK;
}

// Plan a pushed filter tree for a transaction into one program (front half of every scan):
// planner → MVCC update patches → visibility leaf → constant folding → split until it fits
// one pass → emit. *empty = the filter is FALSE (no kernel needed). live (optional) receives the
// zonemap skip's live zones (empty = evaluate every zone); a filter false on every zone is
// *empty too.
int plan_program(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes, const cubit_txn* txn,
                 Emitter& em, bool* empty, std::vector<uint32_t>* live = nullptr) {
    *empty = false;
    if (live) live->clear();
    cubit_ctx* ctx = t->ctx;
    t->single_leaf = nullptr;
    t->scratch_used = 0;
    t->last_passes = 0;
    t->last_packed = 0;
    t->last_sliced = 0;
    t->last_narrowed = 0;
    t->last_narrow_cols.clear();
    ExprP e;
    std::vector<PendingK0> pending;  // K0 leaves not built yet (narrow_k0)
    if (n_nodes == 0) {
        e = mk_true();
    } else {
        const KeyedNodes keyed(t, nodes, n_nodes);
        if (keyed.rc) return keyed.rc;
        if (filter_subtree_end(keyed.p, n_nodes, 0) != (int)n_nodes)
            return fail(CUBIT_ERR_INVALID, "malformed filter tree");
        Planner p{t, keyed.p, n_nodes};
        e = p.plan(0);
        if (!e) return p.rc ? p.rc : fail(CUBIT_ERR_INVALID, "planning failed");
        pending = std::move(p.pending);
    }
    // kept leaf combinations take their groups' places; evictions owed happen first and none
    // until the plan is complete (its program holds the pointers)
    auto forget = [t](DerivedLeaf& d) { forget_derived(t, d); };
    if (!t->derived_budget_set) t->derived.set_budget(default_derived_budget(t), forget);
    t->derived.begin_plan(forget);
    struct EndPlan {
        cubit_table* t;
        ~EndPlan() { t->derived.end_plan(); }
    } end_plan{t};
    if (int rc = derive_leaves(t, e, txn)) return rc;
    // a transaction that sees updates patches whole leaves: build the K0 leaves in full first
    bool visible_updates = false;
    if (txn)
        for (auto& kv : t->upd) visible_updates |= kv.second.any_visible(txn);
    if (visible_updates) {
        for (const PendingK0& k : pending) {
            if (int rc = compute_k0(t, k)) return rc;
            t->last_narrow_cols.push_back(k.col);
        }
        pending.clear();
    }
    if (txn) {
        std::map<const uint64_t*, uint64_t*> patched;
        // bound the patched-leaf caches between scans (never during one: a slot freed
        // mid-plan could be reallocated to another leaf of the same plan)
        for (auto& kv : t->upd)
            if (kv.second.cache.size() >= 16) kv.second.cache.clear();
        if (!t->upd.empty()) {
            if (int rc = patch_updates(t, e, txn, patched)) return rc;
        }
        // visibility leaf: insert ranges the reader may not see, then deletes in effect
        // (ChunkVectorInfo::TemplatedGetSelVector, chunk_info.cpp:123-161)
        const auto& ids = t->del_ids_sorted;
        const int64_t prefix = std::lower_bound(ids.begin(), ids.end(), txn->start_time) - ids.begin();
        const bool own_del = t->n_del && std::binary_search(ids.begin(), ids.end(), txn->transaction_id) &&
                             txn->transaction_id >= txn->start_time;
        const int64_t ins_prefix =
            std::lower_bound(t->ins.begin(), t->ins.end(), txn->start_time,
                             [](const cubit_table::InsRange& a, uint64_t v) { return a.id < v; }) -
            t->ins.begin();
        bool own_ins = false, any_hidden = false;
        for (int64_t i = ins_prefix; i < (int64_t)t->ins.size(); ++i) {
            own_ins |= t->ins[i].id == txn->transaction_id;
            any_hidden |= t->ins[i].id != txn->transaction_id;
        }
        if (prefix > 0 || own_del || any_hidden) {
            const bool own = own_del || own_ins;
            uint64_t* vis = nullptr;
            if (!own) {
                if (!t->vis_cache) {
                    auto b = std::make_unique<DevBuf>();
                    if (hipMalloc(&b->p, t->nwp * sizeof(uint64_t)) != hipSuccess)
                        return fail(CUBIT_ERR_OOM, "visibility bitvector allocation failed");
                    t->vis_cache = std::move(b);
                }
                vis = static_cast<uint64_t*>(t->vis_cache->p);
            } else if (int rc = scratch_bv(t, &vis)) {
                return rc;
            }
            if (own || prefix != t->vis_prefix || ins_prefix != t->vis_ins_prefix) {
                // hidden insert ranges: ids at or past start_time, except the reader's own
                t->hidden_host.clear();
                for (int64_t i = ins_prefix; i < (int64_t)t->ins.size(); ++i)
                    if (t->ins[i].id != txn->transaction_id) {
                        t->hidden_host.push_back(t->ins[i].begin);
                        t->hidden_host.push_back(t->ins[i].end);
                    }
                const uint32_t n_hidden = (uint32_t)(t->hidden_host.size() / 2);
                if (n_hidden) {
                    t->hidden_dev = std::make_unique<DevBuf>();
                    if (hipMalloc(&t->hidden_dev->p, t->hidden_host.size() * 8) != hipSuccess)
                        return fail(CUBIT_ERR_OOM, "insert range allocation failed");
                    HIP_CHECK(hipMemcpyAsync(t->hidden_dev->p, t->hidden_host.data(), t->hidden_host.size() * 8,
                                             hipMemcpyHostToDevice, ctx->stream));
                }
                HIP_CHECK(launch_visibility(t->n_del ? static_cast<const int64_t*>(t->del_rows->p) : nullptr,
                                            t->n_del ? static_cast<const uint64_t*>(t->del_ids->p) : nullptr,
                                            t->n_del, t->n_rows, txn->start_time, txn->transaction_id, vis,
                                            ctx->stream,
                                            n_hidden ? static_cast<const int64_t*>(t->hidden_dev->p) : nullptr,
                                            n_hidden));
                if (n_hidden) HIP_CHECK(hipStreamSynchronize(ctx->stream));  // hidden_host / hidden_dev reuse
                if (!own) {  // a reader with its own versions builds into scratch: the cache stays
                    t->vis_prefix = prefix;
                    t->vis_ins_prefix = ins_prefix;
                }
            }
            Leaf l;
            l.bv = vis;
            e = mk_bin(Expr::AND, e, mk_leaf(l));
        }
    }
    if (e->kind == Expr::CONST_FALSE) {
        *empty = true;
        t->last_leaves = t->last_form = 0;
        return CUBIT_OK;
    }
    if (e->kind == Expr::CONST_TRUE) {
        const uint64_t* ones = nullptr;
        if (int rc = ones_bv(t, &ones)) return rc;
        Leaf l;
        l.bv = ones;
        e = mk_leaf(l);
    }
    if (live) {
        bool none = false;
        if (int rc = zone_plan(t, e, *live, &none)) return rc;
        if (none) {
            *empty = true;
            t->last_leaves = t->last_form = 0;
            return CUBIT_OK;
        }
    }
    // the K0 leaves last: narrowed to the rows the rest of a conjunction keeps, or in full
    if (int rc = narrow_k0(t, e, pending, t->use_narrowing)) return rc;
    if (int rc = fit(t, e)) return rc;
    em.emit_top(e);
    if (!em.ok) return fail(CUBIT_ERR_UNSUPPORTED, "program does not fit one pass");
    t->last_leaves = em.prog.n_leaves;
    t->last_form = eval_form(em.prog);
    t->last_passes++;
    t->single_leaf = e->kind == Expr::LEAF && !e->neg && e->leaf.zsrc == kZoneBits && !e->leaf.zbv &&
                             e->leaf.zdirty < 0 && em.prog.n_leaves == 1 && em.prog.negate == 0
                         ? e->leaf.bv
                         : nullptr;
    return CUBIT_OK;
}

// The device prefix of the per-zone counts of a table-owned bitvector whose zone map is built
// (null when it is not): the offsets of a decode of that bitvector alone.
const uint64_t* tile_prefix_of(cubit_table* t, const uint64_t* bv, int* rc) {
    *rc = CUBIT_OK;
    auto it = t->zones.find(bv);
    if (it == t->zones.end() || it->second.cnt.empty()) return nullptr;
    ZoneMap& m = it->second;
    if (!m.prefix) {
        m.prefix_host.assign(m.cnt.size() + 1, 0);
        for (size_t z = 0; z < m.cnt.size(); ++z) m.prefix_host[z + 1] = m.prefix_host[z] + m.cnt[z];
        auto b = std::make_shared<DevBuf>();
        if (hipMalloc(&b->p, m.prefix_host.size() * sizeof(uint64_t)) != hipSuccess) {
            *rc = fail(CUBIT_ERR_OOM, "tile prefix allocation failed");
            return nullptr;
        }
        if (hipMemcpyAsync(b->p, m.prefix_host.data(), m.prefix_host.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                           t->ctx->stream) != hipSuccess) {
            *rc = fail(CUBIT_ERR_HIP, "tile prefix upload failed");
            return nullptr;
        }
        m.prefix = std::move(b);
    }
    return static_cast<const uint64_t*>(m.prefix->p);
}

// What this decode of `bv` alone (its prefix is built) does with the bitvector's row list
// (row_list_step): nothing the first time; the second time, when the byte rule holds and the budget
// has room nobody uses, the list's buffers are made here and the decode fills them; later decodes
// read them. A list that cannot be allocated is not built: the decode reads the bitvector.
int plan_row_list(cubit_table* t, const uint64_t* bv, RowListUse* use) {
    auto it = t->zones.find(bv);
    if (it == t->zones.end() || it->second.prefix_host.empty()) return CUBIT_OK;
    cubit_table::ZoneMap& m = it->second;
    const uint64_t tiles = m.cnt.size(), q = m.prefix_host.back(), bytes = row_list_bytes(q, tiles);
    const bool on = t->use_row_lists;
    const RowListStep step =
        row_list_step(m.solo_decodes++, on && m.list_off, on && row_list_wanted(q, tiles, t->nwp * 8), bytes,
                      t->row_lists.room(t->derived.budget(), t->derived.bytes()));
    if (step == kRowListBuild) {
        auto off = std::make_shared<DevBuf>(), lo = std::make_shared<DevBuf>();
        if (hipMalloc(&off->p, std::max<uint64_t>(2 * q, 16)) != hipSuccess ||
            hipMalloc(&lo->p, std::max<uint64_t>(4 * tiles, 16)) != hipSuccess) {
            (void)hipGetLastError();
            return CUBIT_OK;
        }
        // a tile the zone maps let the decode skip holds no row
        HIP_CHECK(hipMemsetAsync(lo->p, 0, std::max<uint64_t>(4 * tiles, 16), t->ctx->stream));
        m.list_off = std::move(off);
        m.list_lo = std::move(lo);
        t->row_lists.add(bv, bytes);
    }
    if (step != kRowListNone) {
        use->step = step;
        use->off = static_cast<uint16_t*>(m.list_off->p);
        use->lo_cnt = static_cast<uint32_t*>(m.list_lo->p);
    }
    return CUBIT_OK;
}

// The list a failed building scan left half written goes.
void drop_row_list(cubit_table* t, const uint64_t* bv) {
    auto it = t->zones.find(bv);
    if (it != t->zones.end()) {
        it->second.list_off.reset();
        it->second.list_lo.reset();
    }
    t->row_lists.drop(bv);
}

// The values `col` can take among the rows the filter keeps, when its constant filters in the
// top-level AND pin it to a short list that the column's exact range index can decode:
// v0 < v1 < … with leaves L(v_j). Returns false when it cannot (the kernel then gathers b).
bool decodable_values(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes, int col,
                      std::vector<int64_t>& vals, std::vector<const uint64_t*>& leaves) {
    auto ixit = t->idx.find(col);
    if (ixit == t->idx.end() || n_nodes == 0) return false;
    const IndexView ix = view_of(t, col, ixit->second);
    if (ix.encoding != CUBIT_INDEX_RANGE || !ix.exact_all || ix.empty) return false;
    CmpRange r;  // the column's values, narrowed by every bound
    r.lo = ix.vmin;
    r.hi = ix.vmax;
    bool bounded = false;
    // constants on col reachable through AND nodes only
    std::vector<uint32_t> stack{0};
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        const cubit_filter_node& f = nodes[i];
        if (f.kind == CUBIT_FILTER_AND) {
            uint32_t j = i + 1;
            for (int k = 0; k < f.n_children; ++k) {
                stack.push_back(j);
                j = (uint32_t)filter_subtree_end(nodes, n_nodes, j);
            }
        } else if (f.kind == CUBIT_FILTER_CONSTANT && f.column == col) {
            if (f.cmp == CUBIT_CMP_NE || check_filter_node(f) != NodeCheck::kOk) continue;
            r = r.intersect(cmp_range(f.cmp, f.constant, 0));  // < INT64_MIN, > INT64_MAX: empty, refused below
            bounded = true;
        }
    }
    if (!bounded || r.empty()) return false;
    vals.clear();
    leaves.clear();
    if (r.contains(ix.vmin)) vals.push_back(ix.vmin);
    for (size_t k = 0; k < ix.keys.size(); ++k) {
        if (!r.contains(ix.keys[k])) continue;
        if (!vals.empty()) leaves.push_back(ix.bvs[k]);  // L(v_j) for j >= 1
        vals.push_back(ix.keys[k]);
        if (vals.size() > (size_t)kMaxDecode + 1) return false;
    }
    return !vals.empty();
}

}  // namespace

extern "C" int cubit_table_scan(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                const cubit_txn* txn, int64_t* d_rowids, uint64_t capacity, uint64_t* d_count,
                                uint32_t flags) {
    if (!t || !d_count) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    const bool count_only = (flags & CUBIT_SCAN_COUNT_ONLY) != 0;
    if (!count_only && !d_rowids) return fail(CUBIT_ERR_INVALID, "d_rowids is null without COUNT_ONLY");
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    if (int rc = set_device(t->ctx)) return rc;
    t->ctx->last_tiles = 0;  // until this scan's decode is launched (a planning error leaves none)
    t->ctx->last_from_list = false;
    if (t->n_rows == 0) {  // empty partition
        t->last_leaves = t->last_passes = t->last_form = 0;
        t->last_live = t->last_zones = 0;
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), t->ctx->stream));
        return CUBIT_OK;
    }
    Emitter em;
    bool empty = false;
    std::vector<uint32_t> live;
    const bool zonemap = (flags & CUBIT_SCAN_NO_ZONEMAP) == 0;
    t->last_zones = real_zones(t);
    t->last_live = 0;
    const uint64_t h0 = host_timing() ? now_ns() : 0;
    if (int rc = plan_program(t, nodes, n_nodes, txn, em, &empty, zonemap ? &live : nullptr)) return rc;
    const uint64_t h1 = host_timing() ? now_ns() : 0;
    if (empty) {  // the filter folded to FALSE (or the zonemaps rule out every zone): no launch, no tiles
        t->ctx->last_tiles = 0;
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), t->ctx->stream));
        return CUBIT_OK;
    }
    t->last_live = live.empty() ? t->last_zones : (uint32_t)live.size();
    const uint64_t* prefix = nullptr;
    if (!count_only && t->single_leaf) {
        int rc = CUBIT_OK;
        prefix = tile_prefix_of(t, t->single_leaf, &rc);
        if (rc) return rc;
    }
    // the decode that takes the prefix (no PAIRS or RUNS kernel forced) may write or read a row list
    RowListUse row_list;
    const int forced = t->ctx->decode_kernel;
    if (prefix && (forced == CUBIT_DECODE_AUTO || forced == CUBIT_DECODE_LOOKBACK))
        if (int rc = plan_row_list(t, t->single_leaf, &row_list)) return rc;
    const uint64_t h2 = host_timing() ? now_ns() : 0;
    const int rc = run_eval(t->ctx, em.prog, t->n_rows, t->row_base, count_only ? nullptr : d_rowids, capacity, d_count,
                            nullptr, count_only ? RunMode::kCount : RunMode::kDecode, true,
                            (flags & CUBIT_SCAN_ORDERED) != 0, (flags & CUBIT_SCAN_CHECK_CAPACITY) != 0,
                            live.empty() ? nullptr : &live, prefix, &row_list);
    if (row_list.step == kRowListBuild && !t->ctx->last_tiles) drop_row_list(t, t->single_leaf);  // no launch
    if (t->ctx->last_from_list) t->list_scans++;
    if (host_timing()) {
        const uint64_t h3 = now_ns();
        t->host_ns[0] += h1 - h0;
        t->host_ns[1] += h2 - h1;
        t->host_ns[2] += h3 - h2;
        t->host_scans++;
    }
    return rc;
}

// cubit_table_scan and its tile directory under one hold of the context lock: the directory is
// copied on the context's stream before any other thread's scan can reuse the context's buffer
// (cubit_ctx_last_tiles read after a separate cubit_table_scan may describe another thread's
// scan when several DuckDB pipeline tasks share the context).
extern "C" int cubit_table_scan_tiles(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                      const cubit_txn* txn, int64_t* d_rowids, uint64_t capacity, uint64_t* d_count,
                                      uint32_t flags, uint64_t* d_dir, uint32_t dir_cap, uint32_t* n_tiles,
                                      uint64_t* rows_per_tile) {
    if (!t || !n_tiles) return fail(CUBIT_ERR_INVALID, "null argument");
    if (flags & CUBIT_SCAN_COUNT_ONLY) return fail(CUBIT_ERR_INVALID, "a count-only scan has no tile directory");
    CUBIT_LOCK(t->ctx);
    if (int rc = cubit_table_scan(t, nodes, n_nodes, txn, d_rowids, capacity, d_count, flags)) return rc;
    cubit_ctx* ctx = t->ctx;
    *n_tiles = ctx->last_tiles;
    if (rows_per_tile) *rows_per_tile = ctx->last_tile_rows;
    if (ctx->last_tiles > dir_cap)
        return fail(CUBIT_ERR_CAPACITY, "tile directory of %u tiles, room for %u", ctx->last_tiles, dir_cap);
    if (ctx->last_tiles) {
        if (!d_dir) return fail(CUBIT_ERR_INVALID, "d_dir is null");
        HIP_CHECK(hipMemcpyAsync(d_dir, ctx->dir, 2ull * ctx->last_tiles * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                                 ctx->stream));
    }
    return CUBIT_OK;
}

namespace {
int probe_impl(cubit_table* t, int col, const cubit_txn* txn, const int64_t* d_rowids, const uint64_t* d_count,
               uint64_t max_n, int64_t* d_out, uint64_t* d_valid);

// What cubit_table_aggregate, cubit_table_aggregate_grouped and cubit_table_select share: one plan of
// a query over a value column, answered from the column's bit slices (a fused evaluate + reduce) or
// by the plan's decode into scratch, the probe and a reduction of the probed values. Each entry
// point keeps its argument checks, its output shape, its path rule, its launches and its last_* flags.
struct SlicePlan {
    const Column* c = nullptr;   // the value column
    const Index* sx = nullptr;   // its bit-sliced index; null: the slices cannot answer (not usable)
    bool force_slices = false, force_column = false;
    Emitter em;                  // the filter's program
    std::vector<uint32_t> live;  // the live zones (empty: every zone)
    uint64_t est_rows = 0;       // the estimated qualifying rows: n_rows unless the path rule is asked
    uint64_t live_rows = 0;      // the rows of the live zones
    bool no_rows = false;        // an empty partition, or the filter folded to FALSE: nothing to launch
    uint32_t bits() const { return sx ? (uint32_t)sx->bvs.size() : 0; }
    uint64_t elem_bytes() const { return type_is32(c->type) ? 4 : 8; }
};
static_assert(kZoneWords == kAggTileWords, "a zone is one tile of the slice kernels");

// the two path flags; both together are refused
int forced_path(bool from_slices, bool from_column, SlicePlan& p) {
    p.force_slices = from_slices;
    p.force_column = from_column;
    if (from_slices && from_column) return fail(CUBIT_ERR_INVALID, "both paths forced");
    return CUBIT_OK;
}

// Binds the value column and, when the slices can answer, its sliced index: the index exists, the
// table uses sliced indexes, and no update record of a column the slice path reads (`ruling`: the value
// column, and the group columns of a grouped query) is visible to txn. FROM_SLICES without that is
// refused.
int bind_slices(cubit_table* t, const cubit_txn* txn, int col, const Column& c, const int* ruling, uint32_t n_ruling,
                SlicePlan& p) {
    if (int rc = set_device(t->ctx)) return rc;
    t->ctx->last_tiles = 0;  // no row ids reach the caller, so no tile directory
    p.c = &c;
    bool visible_updates = false;
    for (uint32_t i = 0; i < n_ruling; ++i) {
        auto uit = t->upd.find(ruling[i]);
        visible_updates |= txn && uit != t->upd.end() && uit->second.any_visible(txn);
    }
    auto sit = t->sliced.find(col);
    if (sit != t->sliced.end() && !sit->second.empty && t->use_sliced && !visible_updates) p.sx = &sit->second;
    if (p.force_slices && !p.sx)
        return fail(CUBIT_ERR_INVALID, "column %d has no usable bit-sliced index%s", col,
                    visible_updates ? " (an update record of a column the query reads is visible to the transaction)" : "");
    return CUBIT_OK;
}

// The plan itself: an empty partition resets the last_* counters; else the estimate (only when the
// path rule will be asked), the program with its live zones, and the zone counters. p.no_rows: the
// caller writes its zeros and returns.
int plan_slice_query(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes, const cubit_txn* txn, bool zonemap,
                     SlicePlan& p) {
    if (t->n_rows == 0) {
        t->last_leaves = t->last_passes = t->last_form = 0;
        t->last_live = t->last_zones = 0;
        t->last_sliced = 0;
        p.no_rows = true;
        return CUBIT_OK;
    }
    p.est_rows = t->n_rows;
    if (p.sx && !p.force_slices && !p.force_column)
        if (int rc = cubit_table_estimate_rows(t, nodes, n_nodes, &p.est_rows)) return rc;
    t->last_zones = real_zones(t);
    t->last_live = 0;
    if (int rc = plan_program(t, nodes, n_nodes, txn, p.em, &p.no_rows, zonemap ? &p.live : nullptr)) return rc;
    if (p.no_rows) return CUBIT_OK;  // folded to FALSE (or the zonemaps rule out every zone)
    t->last_live = p.live.empty() ? t->last_zones : (uint32_t)p.live.size();
    p.live_rows = std::min<uint64_t>(t->n_rows, (uint64_t)t->last_live * kZoneRows);
    return CUBIT_OK;
}

// The column path up to the reduction: the plan's decode into context scratch laid out as the ids,
// then the values of each of n_probed columns, then their validity words. The caller probes column k
// into values_of(k) / valid_of(k) and launches its reduction over `count` of `cap` rows.
struct ColumnScratch {
    int64_t* ids;
    uint64_t* count;
    uint64_t cap, vwords;
    uint32_t n_probed;
    int64_t* values_of(uint32_t k) const { return ids + (1 + k) * cap; }
    uint64_t* valid_of(uint32_t k) const { return reinterpret_cast<uint64_t*>(ids + (1 + n_probed) * cap + k * vwords); }
};
int decode_to_scratch(cubit_table* t, const SlicePlan& p, uint32_t n_probed, ColumnScratch& s) {
    cubit_ctx* ctx = t->ctx;
    s.cap = t->n_rows;
    s.vwords = (s.cap + 63) / 64;
    s.n_probed = n_probed;
    if (int rc = ensure_tmp(ctx, (1 + n_probed) * s.cap + n_probed * s.vwords)) return rc;
    s.ids = ctx->tmp_ids;
    s.count = agg_count_slot(ctx->agg);
    // (unordered: the decode must not take tmp_ids for an ordering pass)
    if (int rc = run_eval(ctx, p.em.prog, t->n_rows, t->row_base, s.ids, s.cap, s.count, nullptr, RunMode::kDecode, true,
                          false, false, p.live.empty() ? nullptr : &p.live, nullptr))
        return rc;
    ctx->last_tiles = 0;  // the directory described ids in scratch, not a caller's buffer
    return CUBIT_OK;
}
}  // namespace

extern "C" int cubit_table_sum_product(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                       const cubit_txn* txn, int col_a, int col_b, int64_t* d_out,
                                       uint64_t* d_count, uint32_t flags) {
    if (!t || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    auto ait = t->cols.find(col_a), bit = t->cols.find(col_b);
    if (ait == t->cols.end() || bit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column not registered");
    if (ait->second.type != CUBIT_TYPE_INT64 || bit->second.type != CUBIT_TYPE_INT64)
        return fail(CUBIT_ERR_UNSUPPORTED, "sum_product needs INT64 (DECIMAL storage) columns");
    // the slice path needs both operands' slices usable (bind_slices: no update record of either
    // visible); it writes no row ids, so no tile directory (the fallback's scan resets it below)
    SlicePlan pa, pb;
    if (int rc = forced_path(flags & CUBIT_SUM_FROM_SLICES, flags & CUBIT_SUM_FROM_COLUMN, pa)) return rc;
    pb.force_slices = pa.force_slices;
    pb.force_column = pa.force_column;
    const int ruling[2] = {col_a, col_b};
    if (int rc = bind_slices(t, txn, col_a, ait->second, ruling, 2, pa)) return rc;
    if (int rc = bind_slices(t, txn, col_b, bit->second, ruling, 2, pb)) return rc;
    const bool usable = pa.sx && pb.sx;
    t->last_sum_slices = false;
    t->last_sum_launches = 0;
    cubit_ctx* ctx = t->ctx;
    uint64_t* count = d_count ? d_count : t->dummy_count;
    if (t->n_rows == 0) {  // empty partition: sum 0 over 0 rows
        HIP_CHECK(hipMemsetAsync(d_out, 0, 2 * sizeof(int64_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint64_t), ctx->stream));
        return CUBIT_OK;
    }
    auto visible_updates = [&](int col) {
        auto u = t->upd.find(col);
        return txn && u != t->upd.end() && u->second.any_visible(txn);
    };
    if (visible_updates(col_a) || visible_updates(col_b)) {
        // MVCC fallback: row ids, then the probe (which applies the visible updates, NULL-ness
        // included), then a plain sum over the two value arrays. A nullable column probes with
        // its validity, which leaves 0 at NULL rows: those rows add nothing, as SUM skips NULLs.
        const bool nullable = ait->second.validity || bit->second.validity;
        const uint64_t cap = t->n_rows;
        const uint64_t vwords = nullable ? (cap + 63) / 64 : 0;
        if (int rc = ensure_tmp(ctx, 3 * cap + vwords)) return rc;
        int64_t* ids = ctx->tmp_ids + 0;
        int64_t* xa = ctx->tmp_ids + cap;
        int64_t* xb = ctx->tmp_ids + 2 * cap;
        uint64_t* vw = nullable ? reinterpret_cast<uint64_t*>(ctx->tmp_ids + 3 * cap) : nullptr;
        // the scan's own decode must not use tmp_ids (ordered flag off)
        if (int rc = cubit_table_scan(t, nodes, n_nodes, txn, ids, cap, count, 0)) return rc;
        if (int rc = probe_impl(t, col_a, txn, ids, count, cap, xa, vw)) return rc;
        if (int rc = probe_impl(t, col_b, txn, ids, count, cap, xb, vw)) return rc;
        HIP_CHECK(launch_sum_product_arrays(xa, xb, count, cap, ctx->partials, d_out, ctx->stream));
        ctx->last_tiles = 0;  // the directory described ids in scratch, not a caller's buffer
        return CUBIT_OK;
    }
    uint64_t est_rows = t->n_rows;  // estimated only when the path rule will be asked
    if (usable && !pa.force_slices && !pa.force_column)
        if (int rc = cubit_table_estimate_rows(t, nodes, n_nodes, &est_rows)) return rc;
    Emitter em;
    bool empty = false;
    std::vector<uint32_t> live;
    t->last_zones = real_zones(t);
    t->last_live = 0;
    if (int rc = plan_program(t, nodes, n_nodes, txn, em, &empty, (flags & CUBIT_SUM_NO_ZONEMAP) ? nullptr : &live))
        return rc;
    if (empty) {
        HIP_CHECK(hipMemsetAsync(d_out, 0, 2 * sizeof(int64_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint64_t), ctx->stream));
        return CUBIT_OK;
    }
    t->last_live = live.empty() ? t->last_zones : (uint32_t)live.size();
    std::vector<int64_t> vals;
    std::vector<const uint64_t*> dl;
    const bool decode_b = !(flags & CUBIT_SUM_GATHER_B) && decodable_values(t, nodes, n_nodes, col_b, vals, dl);
    if (usable) {
        // sum_product_from_slices (cubit_program.hpp) chooses between the slices of both operands and
        // the fused gather below
        const uint32_t n_a = pa.bits(), n_b = pb.bits();
        const uint64_t live_rows = std::min<uint64_t>(t->n_rows, (uint64_t)t->last_live * kZoneRows);
        if (sum_product_from_slices(pa.force_slices, pa.force_column, true, n_a, n_b, em.prog.n_leaves,
                                    ait->second.validity != nullptr, bit->second.validity != nullptr, live_rows, t->n_rows,
                                    est_rows, decode_b ? (int)dl.size() : -1)) {
            const bool a_outer = n_a >= n_b;
            const SlicePlan &po = a_outer ? pa : pb, &pi = a_outer ? pb : pa;
            SliceProductArgs g{};
            g.outer = slice_set(*po.sx);
            g.inner = slice_set(*pi.sx);
            g.n_outer = po.bits();
            g.n_inner = pi.bits();
            g.valid_a = ait->second.validity;
            g.valid_b = bit->second.validity;
            g.workspace = ctx->agg;
            EvalArgs a;
            if (int rc = tile_eval_args(ctx, em.prog, t->n_rows, t->row_base, kAggTileWords, live, a)) return rc;
            hipEvent_t e0, e1;
            if (int rc = timing_events(ctx, e0, e1)) return rc;
            HIP_CHECK(launch_eval_slice_sum_product(a, g, po.sx->vmin, pi.sx->vmin,
                                                    ctx->n_cus, &ctx->last_grid, d_out, 2,
                                                    count, ctx->stream, e0, e1));
            t->last_sum_slices = true;
            t->last_sum_launches = 1;
            t->last_sliced += 2;
            t->last_sum_packed = false;
            t->last_decoded = 0;
            return CUBIT_OK;
        }
    }
    SumArgs sa{};
    sa.a = static_cast<const int64_t*>(ait->second.data);
    sa.a_valid = ait->second.validity;
    t->last_sum_packed = false;
    if (!(flags & CUBIT_SUM_PLAIN_A) && ait->second.bp_n_groups) {
        sa.a_bytes = static_cast<const uint8_t*>(ait->second.bp_bytes->p);
        sa.a_groups = static_cast<const BpGroup*>(ait->second.bp_groups->p);
        sa.a_vgroup = static_cast<const uint32_t*>(ait->second.bp_vgroup->p);
        sa.a_plain = sa.a;
        sa.a_n_groups = ait->second.bp_n_groups;
        t->last_sum_packed = true;
    }
    sa.partials = ctx->partials;
    if (decode_b) {
        sa.b = nullptr;
        sa.v0 = vals[0];
        sa.n_decode = (uint32_t)dl.size();
        for (size_t j = 0; j < dl.size(); ++j) {
            sa.dleaf[j] = dl[j];
            sa.delta[j] = (int64_t)((uint64_t)vals[j + 1] - (uint64_t)vals[j]);  // modular: no signed overflow
        }
        t->last_decoded = (uint32_t)dl.size() + 1;
    } else {
        sa.b = static_cast<const int64_t*>(bit->second.data);
        sa.b_valid = bit->second.validity;
        t->last_decoded = 0;
    }
    EvalArgs a{};
    a.prog = em.prog;
    a.n_rows = t->n_rows;
    a.n_words = (t->n_rows + 63) / 64;
    a.row_base = t->row_base;
    a.count = count;
    a.ticket = ctx->ticket;
    a.num_tiles = (uint32_t)(padded_words(t->n_rows) / decode_tile_words());
    if (!live.empty()) {  // zonemap skip: a zone is one tile of the fused kernel
        uint32_t n_live = 0;
        if (int rc = upload_live(ctx, live, 1, &a.live, &n_live)) return rc;
        a.num_tiles = n_live;
    }
    const unsigned grid = std::min<unsigned>(a.num_tiles, sum_product_grid((unsigned)ctx->n_cus));
    HIP_CHECK(launch_eval_sum_product(a, sa, std::max(grid, 1u), d_out, ctx->stream));
    ctx->last_grid = LaunchShape{std::max(grid, 1u), a.num_tiles};
    return CUBIT_OK;
}

// SELECT sum(col), min(col), max(col), count(col), count(*) WHERE <filter>: one plan, then either the
// fused evaluate + aggregate over the column's slices, or the plan's decode into scratch, the probe
// (which applies the visible updates, NULL-ness included) and a reduction of the probed values —
// the structure of cubit_table_sum_product's MVCC fallback. aggregate_from_slices
// (cubit_program.hpp) chooses; both give the same six numbers.
extern "C" int cubit_table_aggregate(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                     const cubit_txn* txn, int col, uint32_t ops, int64_t* d_out) {
    if (!t || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    constexpr uint32_t kOps = CUBIT_AGG_SUM | CUBIT_AGG_MIN | CUBIT_AGG_MAX;
    if (ops & ~(kOps | CUBIT_AGG_FROM_SLICES | CUBIT_AGG_FROM_COLUMN | CUBIT_AGG_NO_ZONEMAP))
        return fail(CUBIT_ERR_INVALID, "ops %u", ops);
    SlicePlan p;
    if (int rc = forced_path(ops & CUBIT_AGG_FROM_SLICES, ops & CUBIT_AGG_FROM_COLUMN, p)) return rc;
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    const Column& c = cit->second;
    if ((ops & CUBIT_AGG_SUM) && (type_is_fp(c.type) || c.type == CUBIT_TYPE_VARCHAR || c.dict))
        return fail(CUBIT_ERR_UNSUPPORTED, "SUM of column %d (type %d): its keys are not linear in the value", col,
                    c.type);
    if (int rc = bind_slices(t, txn, col, c, &col, 1, p)) return rc;
    cubit_ctx* ctx = t->ctx;
    t->last_agg_slices = false;
    if (int rc = plan_slice_query(t, nodes, n_nodes, txn, !(ops & CUBIT_AGG_NO_ZONEMAP), p)) return rc;
    if (p.no_rows) {  // zero counts
        HIP_CHECK(hipMemsetAsync(d_out, 0, 6 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    if (aggregate_from_slices(p.force_slices, p.force_column, p.sx != nullptr, p.bits(), p.em.prog.n_leaves,
                              c.validity != nullptr, p.live_rows, t->n_rows, p.est_rows, p.elem_bytes())) {
        SliceAggArgs g{};
        g.slices = slice_set(*p.sx);
        g.n_slices = p.bits();
        g.validity = c.validity;
        g.workspace = ctx->agg;
        EvalArgs a;
        if (int rc = tile_eval_args(ctx, p.em.prog, t->n_rows, t->row_base, kAggTileWords, p.live, a)) return rc;
        hipEvent_t e0, e1;
        if (int rc = timing_events(ctx, e0, e1)) return rc;
        HIP_CHECK(launch_eval_slice_aggregate(a, g, ops & kOps, c.type, p.sx->vmin,
                                              ctx->n_cus, &ctx->last_grid, d_out, ctx->stream, e0, e1));
        t->last_agg_slices = true;
        t->last_sliced++;
        return CUBIT_OK;
    }
    ColumnScratch s;
    if (int rc = decode_to_scratch(t, p, 1, s)) return rc;
    if (int rc = probe_impl(t, col, txn, s.ids, s.count, s.cap, s.values_of(0), s.valid_of(0))) return rc;
    HIP_CHECK(launch_aggregate_arrays(s.values_of(0), s.valid_of(0), s.count, s.cap, ops & kOps, c.type, ctx->agg, d_out,
                                      ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_table_last_sum_product(cubit_table* t, int* from_slices, uint32_t* n_launches) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (from_slices) *from_slices = t->last_sum_slices ? 1 : 0;
    if (n_launches) *n_launches = t->last_sum_launches;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_aggregate(cubit_table* t, int* from_slices) {
    if (!t || !from_slices) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *from_slices = t->last_agg_slices ? 1 : 0;
    return CUBIT_OK;
}

// SELECT the k-th value / quantile_disc of col WHERE <filter>: cubit_table_aggregate's two paths with
// a radix select in the reduction's place. select_from_slices (cubit_program.hpp) chooses.
extern "C" int cubit_table_select(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes, const cubit_txn* txn,
                                  int col, int mode, uint64_t k, double q, uint32_t flags, int64_t* d_out) {
    if (!t || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    if (mode != CUBIT_SELECT_RANK && mode != CUBIT_SELECT_RANK_DESC && mode != CUBIT_SELECT_QUANTILE)
        return fail(CUBIT_ERR_INVALID, "mode %d", mode);
    if (mode == CUBIT_SELECT_QUANTILE && !(q >= 0.0 && q <= 1.0)) return fail(CUBIT_ERR_INVALID, "quantile %g outside [0, 1]", q);
    if (flags & ~(CUBIT_SELECT_FROM_SLICES | CUBIT_SELECT_FROM_COLUMN | CUBIT_SELECT_NO_ZONEMAP))
        return fail(CUBIT_ERR_INVALID, "flags %u", flags);
    SlicePlan p;
    if (int rc = forced_path(flags & CUBIT_SELECT_FROM_SLICES, flags & CUBIT_SELECT_FROM_COLUMN, p)) return rc;
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    const Column& c = cit->second;
    if (int rc = bind_slices(t, txn, col, c, &col, 1, p)) return rc;
    cubit_ctx* ctx = t->ctx;
    t->last_sel_slices = false;
    t->last_sel_passes = 0;
    if (int rc = plan_slice_query(t, nodes, n_nodes, txn, !(flags & CUBIT_SELECT_NO_ZONEMAP), p)) return rc;
    if (p.no_rows) {  // zero counts, found = 0
        HIP_CHECK(hipMemsetAsync(d_out, 0, 6 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    if (int rc = ensure_select(ctx)) return rc;
    if (select_from_slices(p.force_slices, p.force_column, p.sx != nullptr, p.bits(), p.em.prog.n_leaves,
                           c.validity != nullptr, p.live_rows, t->n_rows, p.est_rows, p.elem_bytes())) {
        if (int rc = ensure_tmp(ctx, padded_words(t->n_rows))) return rc;  // the candidate bitvector
        SliceSelectArgs g{};
        g.slices = slice_set(*p.sx);
        g.n_slices = p.bits();
        g.validity = c.validity;
        g.cand = reinterpret_cast<uint64_t*>(ctx->tmp_ids);
        g.workspace = ctx->sel;
        EvalArgs a;
        if (int rc = tile_eval_args(ctx, p.em.prog, t->n_rows, t->row_base, kAggTileWords, p.live, a)) return rc;
        hipEvent_t e0, e1;
        if (int rc = timing_events(ctx, e0, e1)) return rc;
        HIP_CHECK(launch_slice_select(a, g, mode, k, q, c.type, p.sx->vmin,
                                      ctx->n_cus, &ctx->last_grid, d_out, ctx->stream,
                                      &t->last_sel_passes, e0, e1));
        t->last_sel_slices = true;
        t->last_sliced++;
        return CUBIT_OK;
    }
    ColumnScratch s;
    if (int rc = decode_to_scratch(t, p, 1, s)) return rc;
    if (int rc = probe_impl(t, col, txn, s.ids, s.count, s.cap, s.values_of(0), s.valid_of(0))) return rc;
    HIP_CHECK(launch_select_arrays(s.values_of(0), s.valid_of(0), s.count, s.cap, mode, k, q, c.type, ctx->sel, d_out,
                                   ctx->stream, &t->last_sel_passes));
    return CUBIT_OK;
}

extern "C" int cubit_table_last_select(cubit_table* t, int* from_slices, uint32_t* n_passes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (from_slices) *from_slices = t->last_sel_slices ? 1 : 0;
    if (n_passes) *n_passes = t->last_sel_passes;
    return CUBIT_OK;
}

// ORDER BY col [DESC], rowid LIMIT k: the select for rank k - 1, its six numbers read back once, then
// two ordered scans through the planner with the same txn — the rows strictly before the threshold
// value and the rows equal to it — merged on the device, the ties cut at the lowest row ids.
extern "C" int cubit_table_top_n(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes, const cubit_txn* txn,
                                 int col, uint64_t k, uint32_t flags, int64_t* d_rowids, uint64_t capacity,
                                 uint64_t* d_count, int64_t* d_out) {
    if (!t || !d_count || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    constexpr uint32_t kPath = CUBIT_SELECT_FROM_SLICES | CUBIT_SELECT_FROM_COLUMN | CUBIT_SELECT_NO_ZONEMAP;
    if (flags & ~(kPath | CUBIT_SELECT_DESC_ROWS)) return fail(CUBIT_ERR_INVALID, "flags %u", flags);
    if (k && !d_rowids) return fail(CUBIT_ERR_INVALID, "d_rowids is null");
    if (capacity < k)
        return fail(CUBIT_ERR_CAPACITY, "capacity %llu below k = %llu", (unsigned long long)capacity, (unsigned long long)k);
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (cit->second.type == CUBIT_TYPE_VARCHAR || cit->second.dict)
        return fail(CUBIT_ERR_UNSUPPORTED, "top-N of dictionary column %d: the threshold is a code, not a filter constant", col);
    if (int rc = set_device(t->ctx)) return rc;
    cubit_ctx* ctx = t->ctx;
    if (k == 0) {  // nothing to write
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(d_out, 0, 6 * sizeof(int64_t), ctx->stream));
        return CUBIT_OK;
    }
    const bool desc = (flags & CUBIT_SELECT_DESC_ROWS) != 0;
    if (int rc = cubit_table_select(t, nodes, n_nodes, txn, col, desc ? CUBIT_SELECT_RANK_DESC : CUBIT_SELECT_RANK, k - 1, 0.0,
                                    flags & kPath, d_out))
        return rc;
    int64_t r[6];
    HIP_CHECK(hipMemcpyAsync(r, d_out, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const uint32_t scan_flags = CUBIT_SCAN_ORDERED | ((flags & CUBIT_SELECT_NO_ZONEMAP) ? CUBIT_SCAN_NO_ZONEMAP : 0u);
    // AND(the caller's tree, one more leaf on col)
    std::vector<cubit_filter_node> tree(n_nodes + 2);
    tree[0] = cubit_filter_node{CUBIT_FILTER_AND, 0, -1, n_nodes ? 2 : 1, 0};
    std::copy(nodes, nodes + n_nodes, tree.begin() + 1);
    cubit_filter_node& leaf = tree[n_nodes + 1];
    if (!r[1]) {  // fewer than k non-NULL rows qualify: every one of them
        if (r[4] == 0) {
            HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
            return CUBIT_OK;
        }
        leaf = cubit_filter_node{CUBIT_FILTER_IS_NOT_NULL, 0, col, 0, 0};
        return cubit_table_scan(t, tree.data(), n_nodes + 2, txn, d_rowids, capacity, d_count, scan_flags);
    }
    const uint64_t n_before = (uint64_t)r[2], n_equal = (uint64_t)r[3], n_ties = k - n_before;
    int64_t* buf = nullptr;  // the two scans' ids, then their counts
    if (hipMalloc(&buf, (n_before + n_equal + 2) * sizeof(int64_t)) != hipSuccess)
        return fail(CUBIT_ERR_OOM, "top-N scratch of %llu ids failed", (unsigned long long)(n_before + n_equal));
    struct Free {
        int64_t* p;
        ~Free() { (void)hipFree(p); }
    } free_buf{buf};
    int64_t* before = buf;
    int64_t* equal = buf + n_before;
    uint64_t* counts = reinterpret_cast<uint64_t*>(buf + n_before + n_equal);
    if (n_before) {
        leaf = cubit_filter_node{CUBIT_FILTER_CONSTANT, desc ? CUBIT_CMP_GT : CUBIT_CMP_LT, col, 0, r[0]};
        if (int rc = cubit_table_scan(t, tree.data(), n_nodes + 2, txn, before, n_before, counts, scan_flags)) return rc;
    }
    leaf = cubit_filter_node{CUBIT_FILTER_CONSTANT, CUBIT_CMP_EQ, col, 0, r[0]};
    if (int rc = cubit_table_scan(t, tree.data(), n_nodes + 2, txn, equal, n_equal, counts + 1, scan_flags)) return rc;
    uint64_t got[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(got, counts, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if ((n_before && got[0] != n_before) || got[1] != n_equal)  // the scans see what the select saw
        return fail(CUBIT_ERR_DEVICE, "top-N scans found %llu + %llu rows, the select %llu + %llu",
                    (unsigned long long)got[0], (unsigned long long)got[1], (unsigned long long)n_before,
                    (unsigned long long)n_equal);
    HIP_CHECK(launch_merge_ids(before, n_before, equal, n_ties, d_rowids, d_count, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // buf is freed on return
    return CUBIT_OK;
}

namespace {

// A group column of cubit_table_aggregate_grouped and its slots (group_slots, cubit_program.hpp)
struct GroupCol {
    int col = -1;
    const Column* c = nullptr;
    const Index* ix = nullptr;
    const Updates* upd = nullptr;
    GroupSlots slots;
};
// a group leaf: the bitvector, whether it is a validity to complement (the NULL slot), its slot
struct GroupLeaf {
    const uint64_t* bv;
    bool neg;
    uint32_t slot;
};

int group_columns(cubit_table* t, const int* group_cols, uint32_t n_group_cols, GroupCol (&gc)[CUBIT_AGG_MAX_GROUP_COLS],
                  uint32_t* n1, uint32_t* n2) {
    if (n_group_cols == 0) return fail(CUBIT_ERR_INVALID, "no group column");
    if (n_group_cols > CUBIT_AGG_MAX_GROUP_COLS)
        return fail(CUBIT_ERR_UNSUPPORTED, "%u group columns (at most %d)", n_group_cols, CUBIT_AGG_MAX_GROUP_COLS);
    for (uint32_t k = 0; k < n_group_cols; ++k) {
        GroupCol& g = gc[k];
        g.col = group_cols[k];
        auto cit = t->cols.find(g.col);
        if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "group column %d not registered", g.col);
        g.c = &cit->second;
        auto iit = t->idx.find(g.col);
        if (iit == t->idx.end() || iit->second.encoding != CUBIT_INDEX_EQUALITY || !iit->second.exact_all)
            return fail(CUBIT_ERR_UNSUPPORTED, "group column %d has no EQUALITY index over every distinct value", g.col);
        g.ix = &iit->second;
        auto uit = t->upd.find(g.col);
        g.upd = uit == t->upd.end() ? nullptr : &uit->second;
        static const std::vector<int64_t> none;
        g.slots = group_slots(g.ix->keys, g.upd ? g.upd->stat_values : none,
                              g.c->validity != nullptr || (g.upd && g.upd->any_null));
    }
    *n1 = gc[0].slots.size();
    *n2 = n_group_cols > 1 ? gc[1].slots.size() : 1u;
    if (group_count(*n1, *n2) < 0)
        return fail(CUBIT_ERR_UNSUPPORTED, "%u x %u groups (at most %d)", *n1, *n2, CUBIT_AGG_MAX_GROUPS);
    return CUBIT_OK;
}

// the grouped aggregate's workspace and key staging, on first use
int ensure_grouped(cubit_ctx* ctx) {
    if (ctx->gagg) return CUBIT_OK;
    constexpr size_t kKeyBytes = (size_t)CUBIT_AGG_MAX_GROUP_COLS * CUBIT_AGG_MAX_GROUPS * sizeof(int64_t);
    if (hipMalloc(&ctx->gkeys_dev, kKeyBytes) != hipSuccess || hipHostMalloc(&ctx->gkeys_host, kKeyBytes) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->gkeys_ev, hipEventDisableTiming) != hipSuccess ||
        hipMalloc(&ctx->gagg, kGroupWorkspace * sizeof(int64_t)) != hipSuccess) {
        if (ctx->gkeys_dev) (void)hipFree(ctx->gkeys_dev);
        if (ctx->gkeys_host) (void)hipHostFree(ctx->gkeys_host);
        if (ctx->gkeys_ev) (void)hipEventDestroy(ctx->gkeys_ev);
        ctx->gkeys_dev = ctx->gkeys_host = nullptr;
        ctx->gkeys_ev = nullptr;
        ctx->gagg = nullptr;
        return fail(CUBIT_ERR_OOM, "grouped aggregate workspace allocation failed");
    }
    return CUBIT_OK;
}

// The column path's group side: each group column probed into the scratch's columns first, first + 1
// (visible updates applied), and its slot keys staged to the device.
int probe_group_columns(cubit_table* t, const cubit_txn* txn, const GroupCol (&gc)[CUBIT_AGG_MAX_GROUP_COLS],
                        uint32_t n_group_cols, uint32_t n2, const ColumnScratch& cs, uint32_t first, GroupColArgs& ga) {
    cubit_ctx* ctx = t->ctx;
    ga.n_cols = n_group_cols;
    ga.n2 = n2;
    if (ctx->gkeys_pending) {  // the previous keys' copy must be done before the staging is reused
        HIP_CHECK(hipEventSynchronize(ctx->gkeys_ev));
        ctx->gkeys_pending = false;
    }
    for (uint32_t k = 0; k < n_group_cols; ++k) {
        if (int rc = probe_impl(t, gc[k].col, txn, cs.ids, cs.count, cs.cap, cs.values_of(first + k), cs.valid_of(first + k)))
            return rc;
        const GroupSlots& s = gc[k].slots;
        std::copy(s.keys.begin(), s.keys.end(), ctx->gkeys_host + (size_t)k * CUBIT_AGG_MAX_GROUPS);
        ga.v[k] = cs.values_of(first + k);
        ga.valid[k] = cs.valid_of(first + k);
        ga.keys[k] = ctx->gkeys_dev + (size_t)k * CUBIT_AGG_MAX_GROUPS;
        ga.n_keys[k] = (uint32_t)s.keys.size();
        ga.null_slot[k] = s.has_null ? (int32_t)s.keys.size() : -1;
        ga.type[k] = gc[k].c->type;
    }
    HIP_CHECK(hipMemcpyAsync(ctx->gkeys_dev, ctx->gkeys_host,
                             (size_t)CUBIT_AGG_MAX_GROUP_COLS * CUBIT_AGG_MAX_GROUPS * sizeof(int64_t),
                             hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipEventRecord(ctx->gkeys_ev, ctx->stream));
    ctx->gkeys_pending = true;
    return CUBIT_OK;
}

// The launch arguments of one rectangle of groups (GroupBatch) over the leaves of the two lists
void fill_group_batch(const GroupBatch& b, const std::vector<GroupLeaf>& la, const std::vector<GroupLeaf>& lb, bool two,
                      bool swapped, uint32_t n2, GroupAggArgs& q) {
    q.n1 = b.na;
    q.n2 = b.nb;
    for (uint32_t j = 0; j < kGroupBatchSum; ++j) q.group[j] = kNoGroup;
    for (uint32_t x = 0; x < b.na; ++x) {
        q.e1[x] = la[b.a0 + x].bv;
        q.neg1 |= la[b.a0 + x].neg ? 1u << x : 0u;
    }
    for (uint32_t y = 0; y < b.nb; ++y) {
        q.e2[y] = lb[b.b0 + y].bv;
        q.neg2 |= lb[b.b0 + y].neg ? 1u << y : 0u;
    }
    for (uint32_t x = 0; x < b.na; ++x) {
        if (!two) {
            q.group[x] = la[b.a0 + x].slot;
            continue;
        }
        for (uint32_t y = 0; y < b.nb; ++y) {
            const uint32_t sa = la[b.a0 + x].slot, sb = lb[b.b0 + y].slot;
            q.group[2 * x + y] = swapped ? group_index(sb, sa, n2) : group_index(sa, sb, n2);
        }
    }
}

// the slots that have a bitvector: a key's index leaf, and the NULL slot of a nullable column
void group_leaves(const GroupCol (&gc)[CUBIT_AGG_MAX_GROUP_COLS], uint32_t n_group_cols,
                  std::vector<GroupLeaf> (&leaves)[CUBIT_AGG_MAX_GROUP_COLS]) {
    for (uint32_t k = 0; k < n_group_cols; ++k) {
        const GroupSlots& s = gc[k].slots;
        for (uint32_t i = 0; i < s.keys.size(); ++i)
            if (s.leaf[i] >= 0) leaves[k].push_back({gc[k].ix->bvs[(size_t)s.leaf[i]], false, i});
        if (s.has_null && gc[k].c->validity) leaves[k].push_back({gc[k].c->validity, true, (uint32_t)s.keys.size()});
    }
}

}  // namespace

extern "C" int cubit_table_aggregate_groups(cubit_table* t, const int* group_cols, uint32_t n_group_cols, int64_t* keys,
                                            uint8_t* key_is_null, uint32_t cap, uint32_t* n_groups) {
    if (!t || !group_cols || !n_groups) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    GroupCol gc[CUBIT_AGG_MAX_GROUP_COLS];
    uint32_t n1 = 0, n2 = 1;
    if (int rc = group_columns(t, group_cols, n_group_cols, gc, &n1, &n2)) return rc;
    *n_groups = n1 * n2;
    for (uint32_t g = 0; g < std::min(cap, n1 * n2); ++g) {
        uint32_t i[2];
        group_tuple(g, n2, &i[0], &i[1]);
        for (uint32_t k = 0; k < n_group_cols; ++k) {
            const bool null = i[k] >= gc[k].slots.keys.size();
            if (keys) keys[(size_t)g * n_group_cols + k] = null ? 0 : agg_key_value(gc[k].c->type, gc[k].slots.keys[i[k]]);
            if (key_is_null) key_is_null[(size_t)g * n_group_cols + k] = null ? 1 : 0;
        }
    }
    return CUBIT_OK;
}

// cubit_table_aggregate per group of one or two EQUALITY-indexed columns: one plan, then either the
// fused evaluate + aggregate over the value column's slices, a batch of groups per launch, or the
// plan's decode into scratch, the probes of the value column and the group columns (which apply the
// visible updates) and a reduction per group. grouped_from_slices (cubit_program.hpp) chooses.
extern "C" int cubit_table_aggregate_grouped(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                             const cubit_txn* txn, int col, const int* group_cols,
                                             uint32_t n_group_cols, uint32_t ops, int64_t* d_out, uint32_t cap_groups) {
    if (!t || !d_out || !group_cols) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    constexpr uint32_t kOps = CUBIT_AGG_SUM | CUBIT_AGG_MIN | CUBIT_AGG_MAX;
    if (ops & ~(kOps | CUBIT_AGG_FROM_SLICES | CUBIT_AGG_FROM_COLUMN | CUBIT_AGG_NO_ZONEMAP))
        return fail(CUBIT_ERR_INVALID, "ops %u", ops);
    SlicePlan p;
    if (int rc = forced_path(ops & CUBIT_AGG_FROM_SLICES, ops & CUBIT_AGG_FROM_COLUMN, p)) return rc;
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    const Column& c = cit->second;
    if ((ops & CUBIT_AGG_SUM) && (type_is_fp(c.type) || c.type == CUBIT_TYPE_VARCHAR || c.dict))
        return fail(CUBIT_ERR_UNSUPPORTED, "SUM of column %d (type %d): its keys are not linear in the value", col,
                    c.type);
    GroupCol gc[CUBIT_AGG_MAX_GROUP_COLS];
    uint32_t n1 = 0, n2 = 1;
    if (int rc = group_columns(t, group_cols, n_group_cols, gc, &n1, &n2)) return rc;
    const uint32_t n_groups = n1 * n2;
    if (cap_groups < n_groups) return fail(CUBIT_ERR_CAPACITY, "%u groups, room for %u", n_groups, cap_groups);
    // an update record of the value column or of a group column rules the slices out
    int ruling[1 + CUBIT_AGG_MAX_GROUP_COLS] = {col};
    for (uint32_t k = 0; k < n_group_cols; ++k) ruling[1 + k] = gc[k].col;
    if (int rc = bind_slices(t, txn, col, c, ruling, 1 + n_group_cols, p)) return rc;
    cubit_ctx* ctx = t->ctx;
    t->last_grouped_slices = false;
    t->last_grouped_groups = n_groups;
    t->last_grouped_launches = 0;
    if (n_groups == 0) return CUBIT_OK;
    // every group starts as six zeros: the kernels write the groups that reach them
    HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n_groups * 6 * sizeof(int64_t), ctx->stream));
    if (int rc = plan_slice_query(t, nodes, n_nodes, txn, !(ops & CUBIT_AGG_NO_ZONEMAP), p)) return rc;
    if (p.no_rows) return CUBIT_OK;
    if (int rc = ensure_grouped(ctx)) return rc;

    std::vector<GroupLeaf> leaves[CUBIT_AGG_MAX_GROUP_COLS];
    group_leaves(gc, n_group_cols, leaves);
    const bool two = n_group_cols > 1;
    const bool minmax = (ops & (CUBIT_AGG_MIN | CUBIT_AGG_MAX)) != 0;
    const uint32_t row_bits = p.bits() + p.em.prog.n_leaves + (c.validity ? 1u : 0u);
    bool swapped = false;
    const std::vector<GroupBatch> batches =
        split_group_batches((uint32_t)leaves[0].size(), two ? (uint32_t)leaves[1].size() : 0u, two,
                            minmax ? kGroupBatchMinMax : kGroupBatchSum, row_bits, &swapped);
    uint64_t elem_bytes[1 + CUBIT_AGG_MAX_GROUP_COLS] = {p.elem_bytes(), 0, 0};
    for (uint32_t k = 0; k < n_group_cols; ++k) elem_bytes[1 + k] = type_is32(gc[k].c->type) ? 4 : 8;
    if (grouped_from_slices(p.force_slices, p.force_column, p.sx != nullptr,
                            batches.empty() ? row_bits : group_batches_bits(batches, row_bits), p.em.prog.n_leaves,
                            p.live_rows, t->n_rows, p.est_rows, elem_bytes, 1 + n_group_cols)) {
        SliceAggArgs g{};
        g.slices = slice_set(*p.sx);
        g.n_slices = p.bits();
        g.validity = c.validity;
        EvalArgs a;  // (the kernel counts each group's rows in its partials and takes no ticket)
        if (int rc = tile_eval_args(ctx, p.em.prog, t->n_rows, t->row_base, kAggTileWords, p.live, a)) return rc;
        const std::vector<GroupLeaf>& la = leaves[swapped ? 1 : 0];
        const std::vector<GroupLeaf>& lb = leaves[swapped ? 0 : 1];
        for (const GroupBatch& b : batches) {
            GroupAggArgs q{};
            q.partials = ctx->gagg;
            fill_group_batch(b, la, lb, two, swapped, n2, q);
            hipEvent_t e0, e1;
            if (int rc = timing_events(ctx, e0, e1)) return rc;
            HIP_CHECK(launch_eval_slice_aggregate_grouped(a, g, q, ops & kOps, c.type, p.sx->vmin,
                                                          ctx->n_cus, &ctx->last_grid, d_out,
                                                          ctx->stream, e0, e1));
            t->last_grouped_launches++;
        }
        t->last_grouped_slices = true;
        t->last_sliced++;
        return CUBIT_OK;
    }
    // the column path: the value column and the group columns are probed
    ColumnScratch cs;
    if (int rc = decode_to_scratch(t, p, 1 + n_group_cols, cs)) return rc;
    if (int rc = probe_impl(t, col, txn, cs.ids, cs.count, cs.cap, cs.values_of(0), cs.valid_of(0))) return rc;
    GroupColArgs ga{};
    if (int rc = probe_group_columns(t, txn, gc, n_group_cols, n2, cs, 1, ga)) return rc;
    HIP_CHECK(launch_aggregate_arrays_grouped(cs.values_of(0), cs.valid_of(0), ga, n_groups, cs.count, cs.cap, ops & kOps,
                                              c.type, ctx->gagg, d_out, ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_table_last_grouped(cubit_table* t, int* from_slices, uint32_t* n_groups, uint32_t* n_launches) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (from_slices) *from_slices = t->last_grouped_slices ? 1 : 0;
    if (n_groups) *n_groups = t->last_grouped_groups;
    if (n_launches) *n_launches = t->last_grouped_launches;
    return CUBIT_OK;
}

// cubit_table_select per group: cubit_table_aggregate_grouped's structure with a radix select in the
// reduction's place. From the slices a batch of groups runs through all its passes over the one
// scratch candidate bitvector before the next batch starts; from the column every group's select
// runs at once over the probed values. select_grouped_from_slices (cubit_program.hpp) chooses.
extern "C" int cubit_table_select_grouped(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                          const cubit_txn* txn, int col, const int* group_cols, uint32_t n_group_cols,
                                          int mode, uint64_t k, double q, uint32_t flags, int64_t* d_out,
                                          uint32_t cap_groups) {
    if (!t || !d_out || !group_cols) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    if (mode != CUBIT_SELECT_RANK && mode != CUBIT_SELECT_RANK_DESC && mode != CUBIT_SELECT_QUANTILE)
        return fail(CUBIT_ERR_INVALID, "mode %d", mode);
    if (mode == CUBIT_SELECT_QUANTILE && !(q >= 0.0 && q <= 1.0)) return fail(CUBIT_ERR_INVALID, "quantile %g outside [0, 1]", q);
    if (flags & ~(CUBIT_SELECT_FROM_SLICES | CUBIT_SELECT_FROM_COLUMN | CUBIT_SELECT_NO_ZONEMAP))
        return fail(CUBIT_ERR_INVALID, "flags %u", flags);
    SlicePlan p;
    if (int rc = forced_path(flags & CUBIT_SELECT_FROM_SLICES, flags & CUBIT_SELECT_FROM_COLUMN, p)) return rc;
    auto cit = t->cols.find(col);
    if (cit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    const Column& c = cit->second;
    GroupCol gc[CUBIT_AGG_MAX_GROUP_COLS];
    uint32_t n1 = 0, n2 = 1;
    if (int rc = group_columns(t, group_cols, n_group_cols, gc, &n1, &n2)) return rc;
    const uint32_t n_groups = n1 * n2;
    if (cap_groups < n_groups) return fail(CUBIT_ERR_CAPACITY, "%u groups, room for %u", n_groups, cap_groups);
    // an update record of the value column or of a group column rules the slices out
    int ruling[1 + CUBIT_AGG_MAX_GROUP_COLS] = {col};
    for (uint32_t i = 0; i < n_group_cols; ++i) ruling[1 + i] = gc[i].col;
    if (int rc = bind_slices(t, txn, col, c, ruling, 1 + n_group_cols, p)) return rc;
    cubit_ctx* ctx = t->ctx;
    t->last_gsel_slices = false;
    t->last_gsel_groups = n_groups;
    t->last_gsel_launches = t->last_gsel_passes = 0;
    if (n_groups == 0) return CUBIT_OK;
    // every group starts as six zeros: the kernels write the groups that reach them
    HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n_groups * 6 * sizeof(int64_t), ctx->stream));
    if (int rc = plan_slice_query(t, nodes, n_nodes, txn, !(flags & CUBIT_SELECT_NO_ZONEMAP), p)) return rc;
    if (p.no_rows) return CUBIT_OK;
    if (int rc = ensure_select_grouped(ctx)) return rc;

    std::vector<GroupLeaf> leaves[CUBIT_AGG_MAX_GROUP_COLS];
    group_leaves(gc, n_group_cols, leaves);
    const bool two = n_group_cols > 1;
    bool swapped = false;
    // (row_bits decides only which column takes the side of 2: a launch's passes all read its leaves)
    const std::vector<GroupBatch> batches =
        split_group_batches((uint32_t)leaves[0].size(), two ? (uint32_t)leaves[1].size() : 0u, two, kGroupBatchSelect,
                            p.bits() + p.em.prog.n_leaves + (c.validity ? 1u : 0u), &swapped);
    uint64_t elem_bytes[1 + CUBIT_AGG_MAX_GROUP_COLS] = {p.elem_bytes(), 0, 0};
    for (uint32_t i = 0; i < n_group_cols; ++i) elem_bytes[1 + i] = type_is32(gc[i].c->type) ? 4 : 8;
    if (select_grouped_from_slices(p.force_slices, p.force_column, p.sx != nullptr,
                                   select_grouped_slice_bits(batches, p.bits(), p.em.prog.n_leaves, c.validity != nullptr),
                                   p.em.prog.n_leaves, p.live_rows, t->n_rows, p.est_rows, elem_bytes, 1 + n_group_cols)) {
        if (int rc = ensure_tmp(ctx, padded_words(t->n_rows))) return rc;  // the candidate bitvector
        SliceSelectArgs g{};
        g.slices = slice_set(*p.sx);
        g.n_slices = p.bits();
        g.validity = c.validity;
        g.cand = reinterpret_cast<uint64_t*>(ctx->tmp_ids);
        g.workspace = ctx->gsel;
        EvalArgs a;  // (the kernels count each group's rows in their partials and take no ticket)
        if (int rc = tile_eval_args(ctx, p.em.prog, t->n_rows, t->row_base, kAggTileWords, p.live, a)) return rc;
        const std::vector<GroupLeaf>& la = leaves[swapped ? 1 : 0];
        const std::vector<GroupLeaf>& lb = leaves[swapped ? 0 : 1];
        for (const GroupBatch& b : batches) {  // a batch through all its passes, then the next
            GroupAggArgs qa{};
            fill_group_batch(b, la, lb, two, swapped, n2, qa);
            hipEvent_t e0, e1;
            if (int rc = timing_events(ctx, e0, e1)) return rc;
            HIP_CHECK(launch_slice_select_grouped(a, g, qa, mode, k, q, c.type, p.sx->vmin,
                                                  ctx->n_cus, &ctx->last_grid, d_out, ctx->stream,
                                                  &t->last_gsel_passes, e0, e1));
            t->last_gsel_launches++;
        }
        if (batches.empty()) t->last_gsel_passes = select_passes(p.bits(), kSelectChunk);
        t->last_gsel_slices = true;
        t->last_sliced++;
        return CUBIT_OK;
    }
    // the column path: the value column and the group columns are probed
    if (int rc = ensure_grouped(ctx)) return rc;  // (the slot keys' staging)
    ColumnScratch cs;
    if (int rc = decode_to_scratch(t, p, 1 + n_group_cols, cs)) return rc;
    if (int rc = probe_impl(t, col, txn, cs.ids, cs.count, cs.cap, cs.values_of(0), cs.valid_of(0))) return rc;
    GroupColArgs ga{};
    if (int rc = probe_group_columns(t, txn, gc, n_group_cols, n2, cs, 1, ga)) return rc;
    HIP_CHECK(launch_select_arrays_grouped(cs.values_of(0), cs.valid_of(0), ga, n_groups, cs.count, cs.cap, mode, k, q, c.type,
                                           ctx->gsel, d_out, ctx->stream, &t->last_gsel_passes));
    return CUBIT_OK;
}

extern "C" int cubit_table_last_select_grouped(cubit_table* t, int* from_slices, uint32_t* n_groups, uint32_t* n_launches,
                                               uint32_t* n_passes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (from_slices) *from_slices = t->last_gsel_slices ? 1 : 0;
    if (n_groups) *n_groups = t->last_gsel_groups;
    if (n_launches) *n_launches = t->last_gsel_launches;
    if (n_passes) *n_passes = t->last_gsel_passes;
    return CUBIT_OK;
}

// cubit_table_sum_product per group: cubit_table_aggregate_grouped's structure with two value columns.
// sum_product_grouped_from_slices (cubit_program.hpp) chooses between the fused kernel over both
// operands' slices and scan + probe (a, b, the group columns) + the grouped reduction.
extern "C" int cubit_table_sum_product_grouped(cubit_table* t, const cubit_filter_node* nodes, uint32_t n_nodes,
                                               const cubit_txn* txn, int col_a, int col_b, const int* group_cols,
                                               uint32_t n_group_cols, uint32_t flags, int64_t* d_out, uint32_t cap_groups) {
    if (!t || !d_out || !group_cols) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    if (n_nodes && !nodes) return fail(CUBIT_ERR_INVALID, "nodes is null");
    if (flags & ~(CUBIT_SUM_FROM_SLICES | CUBIT_SUM_FROM_COLUMN | CUBIT_SUM_NO_ZONEMAP))
        return fail(CUBIT_ERR_INVALID, "flags %u", flags);
    SlicePlan p, pb;
    if (int rc = forced_path(flags & CUBIT_SUM_FROM_SLICES, flags & CUBIT_SUM_FROM_COLUMN, p)) return rc;
    pb.force_slices = p.force_slices;
    pb.force_column = p.force_column;
    auto ait = t->cols.find(col_a), bit = t->cols.find(col_b);
    if (ait == t->cols.end() || bit == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column not registered");
    const Column &ca = ait->second, &cb = bit->second;
    if (ca.type != CUBIT_TYPE_INT64 || cb.type != CUBIT_TYPE_INT64)
        return fail(CUBIT_ERR_UNSUPPORTED, "sum_product needs INT64 (DECIMAL storage) columns");
    GroupCol gc[CUBIT_AGG_MAX_GROUP_COLS];
    uint32_t n1 = 0, n2 = 1;
    if (int rc = group_columns(t, group_cols, n_group_cols, gc, &n1, &n2)) return rc;
    const uint32_t n_groups = n1 * n2;
    if (cap_groups < n_groups) return fail(CUBIT_ERR_CAPACITY, "%u groups, room for %u", n_groups, cap_groups);
    // an update record of either operand or of a group column rules the slices out
    int ruling[2 + CUBIT_AGG_MAX_GROUP_COLS] = {col_a, col_b};
    for (uint32_t k = 0; k < n_group_cols; ++k) ruling[2 + k] = gc[k].col;
    if (int rc = bind_slices(t, txn, col_a, ca, ruling, 2 + n_group_cols, p)) return rc;
    if (int rc = bind_slices(t, txn, col_b, cb, ruling, 2 + n_group_cols, pb)) return rc;
    const Index* sxa = p.sx;
    if (!pb.sx) p.sx = nullptr;  // usable: both operands' slices
    const bool usable = p.sx != nullptr;
    cubit_ctx* ctx = t->ctx;
    t->last_sum_slices = false;
    t->last_sum_launches = 0;
    if (n_groups == 0) return CUBIT_OK;
    // every group starts as four zeros: the kernels write the groups that reach them
    HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n_groups * 4 * sizeof(int64_t), ctx->stream));
    if (int rc = plan_slice_query(t, nodes, n_nodes, txn, !(flags & CUBIT_SUM_NO_ZONEMAP), p)) return rc;
    if (p.no_rows) return CUBIT_OK;
    if (int rc = ensure_grouped(ctx)) return rc;

    std::vector<GroupLeaf> leaves[CUBIT_AGG_MAX_GROUP_COLS];
    group_leaves(gc, n_group_cols, leaves);
    const bool two = n_group_cols > 1;
    const uint32_t n_a = usable ? (uint32_t)sxa->bvs.size() : 0, n_b = usable ? pb.bits() : 0;
    const uint32_t row_bits = product_slice_bits(n_a, n_b, p.em.prog.n_leaves, ca.validity != nullptr, cb.validity != nullptr);
    bool swapped = false;
    const std::vector<GroupBatch> batches = split_group_batches(
        (uint32_t)leaves[0].size(), two ? (uint32_t)leaves[1].size() : 0u, two, kProductGroupBatch, row_bits, &swapped);
    uint64_t elem_bytes[2 + CUBIT_AGG_MAX_GROUP_COLS] = {8, 8, 0, 0};
    for (uint32_t k = 0; k < n_group_cols; ++k) elem_bytes[2 + k] = type_is32(gc[k].c->type) ? 4 : 8;
    if (sum_product_grouped_from_slices(p.force_slices, p.force_column, usable, n_a, n_b,
                                        batches.empty() ? row_bits : group_batches_bits(batches, row_bits),
                                        p.em.prog.n_leaves, p.live_rows, t->n_rows, p.est_rows, elem_bytes,
                                        2 + n_group_cols)) {
        const bool a_outer = n_a >= n_b;
        const Index &so = a_outer ? *sxa : *pb.sx, &si = a_outer ? *pb.sx : *sxa;
        SliceProductArgs g{};
        g.outer = slice_set(so);
        g.inner = slice_set(si);
        g.n_outer = (uint32_t)so.bvs.size();
        g.n_inner = (uint32_t)si.bvs.size();
        g.valid_a = ca.validity;
        g.valid_b = cb.validity;
        EvalArgs a;  // (the kernel counts each group's rows in its partials and takes no ticket)
        if (int rc = tile_eval_args(ctx, p.em.prog, t->n_rows, t->row_base, kAggTileWords, p.live, a)) return rc;
        const std::vector<GroupLeaf>& la = leaves[swapped ? 1 : 0];
        const std::vector<GroupLeaf>& lb = leaves[swapped ? 0 : 1];
        for (const GroupBatch& b : batches) {
            GroupAggArgs q{};
            q.partials = ctx->gagg;
            fill_group_batch(b, la, lb, two, swapped, n2, q);
            hipEvent_t e0, e1;
            if (int rc = timing_events(ctx, e0, e1)) return rc;
            HIP_CHECK(launch_eval_slice_sum_product_grouped(a, g, q, so.vmin, si.vmin,
                                                            ctx->n_cus, &ctx->last_grid, d_out, ctx->stream, e0, e1));
            t->last_sum_launches++;
        }
        t->last_sum_slices = true;
        t->last_sliced += 2;
        return CUBIT_OK;
    }
    // the column path: both operands and the group columns are probed
    ColumnScratch cs;
    if (int rc = decode_to_scratch(t, p, 2 + n_group_cols, cs)) return rc;
    if (int rc = probe_impl(t, col_a, txn, cs.ids, cs.count, cs.cap, cs.values_of(0), cs.valid_of(0))) return rc;
    if (int rc = probe_impl(t, col_b, txn, cs.ids, cs.count, cs.cap, cs.values_of(1), cs.valid_of(1))) return rc;
    GroupColArgs ga{};
    if (int rc = probe_group_columns(t, txn, gc, n_group_cols, n2, cs, 2, ga)) return rc;
    HIP_CHECK(launch_sum_product_arrays_grouped(cs.values_of(0), cs.valid_of(0), cs.values_of(1), cs.valid_of(1), ga, n_groups,
                                                cs.count, cs.cap, ctx->gagg, d_out, ctx->stream));
    return CUBIT_OK;
}

extern "C" int cubit_table_last_plan(cubit_table* t, uint32_t* n_leaves, uint32_t* n_passes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (n_leaves) *n_leaves = t->last_leaves;
    if (n_passes) *n_passes = t->last_passes;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_form(cubit_table* t, uint32_t* form) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (form) *form = t->last_form;
    return CUBIT_OK;
}

extern "C" int cubit_table_set_derived_budget(cubit_table* t, uint64_t bytes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (int rc = set_device(t->ctx)) return rc;
    t->derived_budget_set = true;
    t->derived.set_budget(bytes, [t](DerivedLeaf& d) { forget_derived(t, d); });
    size_bv_pool(t);
    shed_row_lists(t);
    return CUBIT_OK;
}

extern "C" int cubit_table_derived_pool_stats(cubit_table* t, uint32_t* free_blocks, uint64_t* device_allocs) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (free_blocks) *free_blocks = (uint32_t)t->bv_pool.free_blocks();
    if (device_allocs) *device_allocs = t->bv_pool.device_allocs();
    return CUBIT_OK;
}

extern "C" int cubit_table_use_row_lists(cubit_table* t, int on) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->use_row_lists = on != 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_row_list_stats(cubit_table* t, uint32_t* lists, uint64_t* bytes, uint64_t* scans_from_lists) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (lists) *lists = (uint32_t)t->row_lists.size();
    if (bytes) *bytes = t->row_lists.bytes();
    if (scans_from_lists) *scans_from_lists = t->list_scans;
    return CUBIT_OK;
}

extern "C" int cubit_table_set_derived_chain_cost(cubit_table* t, uint64_t fixed_bytes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->derived.set_chain_cost(fixed_bytes);
    return CUBIT_OK;
}

extern "C" int cubit_table_set_derived_chain_cost_pooled(cubit_table* t, uint64_t fixed_bytes) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->derived.set_chain_cost_pooled(fixed_bytes);
    return CUBIT_OK;
}

extern "C" int cubit_table_derived_chain_stats(cubit_table* t, uint32_t* chains, uint64_t* hits) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (chains) *chains = (uint32_t)t->derived.chain_size();
    if (hits) *hits = t->derived.chain_hits();
    return CUBIT_OK;
}

extern "C" int cubit_table_derived_stats(cubit_table* t, uint32_t* leaves, uint64_t* bytes, uint64_t* hits) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (leaves) *leaves = (uint32_t)t->derived.size();
    if (bytes) *bytes = t->derived.bytes();
    if (hits) *hits = t->derived.hits();
    return CUBIT_OK;
}

// Column statistics (DataTable::GetStatistics, behind seq_scan's `statistics` callback
// TableScanStatistics, table_scan.cpp:108-117): min / max of the valid values and whether the
// column has NULL / non-NULL rows, from the per-zone statistics the zonemaps use (computed once,
// cached until the column changes). As DuckDB's column statistics absorb every update
// (UpdateSegment merges its values into the segment statistics), the bounds widen by the
// column's update records of any version, and an updated row counts as a non-NULL one.
extern "C" int cubit_table_column_statistics(cubit_table* t, int col, int64_t* vmin, int64_t* vmax,
                                             int* has_null, int* has_no_null) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (!t->cols.count(col)) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (int rc = set_device(t->ctx)) return rc;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    bool any_null = false, any_valid = false;
    if (t->n_rows) {
        if (int rc = ensure_zones(t, {}, {col})) return rc;
        const cubit_table::ColZones& cz = t->col_zones.at(col);
        for (size_t z = 0; z < cz.fl.size(); ++z) {
            if (cz.fl[z] & 1) {
                any_valid = true;
                lo = std::min(lo, cz.mn[z]);
                hi = std::max(hi, cz.mx[z]);
            }
            if (!(cz.fl[z] & 2)) any_null = true;
        }
    }
    auto uit = t->upd.find(col);
    if (uit != t->upd.end() && !uit->second.stat_values.empty()) {
        any_valid = true;
        lo = std::min(lo, uit->second.stat_values.front());
        hi = std::max(hi, uit->second.stat_values.back());
    }
    // a SET NULL record makes the column nullable (UpdateValidityStatistics,
    // update_segment.cpp:907-918: an update vector with an invalid row sets has_null)
    if (uit != t->upd.end() && uit->second.any_null) any_null = true;
    // FLOAT / DOUBLE: the bounds are keys; handed out as the bit patterns of those values
    const int type = t->cols.at(col).type;
    if (vmin) *vmin = any_valid ? cubit_fp_value(type, lo) : 0;
    if (vmax) *vmax = any_valid ? cubit_fp_value(type, hi) : 0;
    if (has_null) *has_null = any_null ? 1 : 0;
    if (has_no_null) *has_no_null = any_valid ? 1 : 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_use_packed_filter(cubit_table* t, int on) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->use_packed = on != 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_use_narrowing(cubit_table* t, int on) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->use_narrowing = on != 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_column_changed(cubit_table* t, int col) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (!t->cols.count(col)) return fail(CUBIT_ERR_INVALID, "column %d is not registered", col);
    // statistics and zone classes derived from the values, and leaves patched from them
    drop_patches(t, col);
    return CUBIT_OK;
}

extern "C" int cubit_table_last_k0_order(cubit_table* t, int32_t* cols, uint32_t cap, uint32_t* n) {
    if (!t || !n || (cap && !cols)) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *n = (uint32_t)t->last_narrow_cols.size();
    for (uint32_t i = 0; i < *n && i < cap; ++i) cols[i] = t->last_narrow_cols[i];
    return CUBIT_OK;
}

extern "C" int cubit_table_last_narrowed(cubit_table* t, uint32_t* n_leaves) {
    if (!t || !n_leaves) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *n_leaves = t->last_narrowed;
    return CUBIT_OK;
}

extern "C" int cubit_table_use_sliced(cubit_table* t, int on) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    t->use_sliced = on != 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_sliced(cubit_table* t, uint32_t* n_leaves) {
    if (!t || !n_leaves) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *n_leaves = t->last_sliced;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_packed(cubit_table* t, uint32_t* n_leaves) {
    if (!t || !n_leaves) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *n_leaves = t->last_packed;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_zones(cubit_table* t, uint32_t* evaluated, uint32_t* zones) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    CUBIT_LOCK(t->ctx);
    if (evaluated) *evaluated = t->last_live;
    if (zones) *zones = t->last_zones;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_sum_packed(cubit_table* t, int* packed) {
    if (!t || !packed) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *packed = t->last_sum_packed ? 1 : 0;
    return CUBIT_OK;
}

extern "C" int cubit_table_last_sum_decode(cubit_table* t, uint32_t* n_values) {
    if (!t || !n_values) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    *n_values = t->last_decoded;
    return CUBIT_OK;
}

namespace {

// visible value of updated rows for a probe: patch gathered values in place — and their
// NULL-ness when out_valid is given (FetchRowValidity, update_segment.cpp:357-370: the newest
// visible record of the validity chain sets the row's bit)
__global__ void patch_probe_kernel(const int64_t* __restrict__ rowids, const uint64_t* __restrict__ d_count,
                                   uint64_t max_n, int64_t row_base, const int64_t* __restrict__ urows,
                                   const int64_t* __restrict__ uvalues, const uint8_t* __restrict__ uvalids,
                                   const uint64_t* __restrict__ uversions, uint64_t nu, uint64_t start_time,
                                   uint64_t tid, int64_t* __restrict__ out, uint64_t* __restrict__ out_valid) {
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = rowids[i] - row_base;
        // binary search the first record of row r (records grouped by row, ascending)
        uint64_t lo = 0, hi = nu;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (urows[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        int vis = -1;  // newest visible record of the row
        for (uint64_t j = lo; j < nu && urows[j] == r; ++j) {
            const uint64_t v = uversions[j];
            if (v < start_time || v == tid) vis = (int)(j - lo);
        }
        if (vis < 0) continue;
        const uint64_t j = lo + (uint64_t)vis;
        const bool ok = !uvalids || uvalids[j];
        out[i] = ok ? uvalues[j] : 0;
        if (out_valid) {
            unsigned long long* w = reinterpret_cast<unsigned long long*>(&out_valid[i >> 6]);
            if (ok) atomicOr(w, 1ull << (i & 63));
            else atomicAnd(w, ~(1ull << (i & 63)));
        }
    }
}

}  // namespace

namespace {

// K3 for cubit_table_probe (d_valid null: values only, a NULL row's slot as stored) and
// cubit_table_probe_validity (values, 0 at NULL rows, and the validity words), then the visible
// update records on top
int probe_impl(cubit_table* t, int col, const cubit_txn* txn, const int64_t* d_rowids, const uint64_t* d_count,
               uint64_t max_n, int64_t* d_out, uint64_t* d_valid) {
    auto it = t->cols.find(col);
    if (it == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    if (int rc = set_device(t->ctx)) return rc;
    const Column& c = it->second;
    if (d_valid)
        HIP_CHECK(launch_gather_valid(raw_of(c), c.type, c.validity, d_rowids, d_count, max_n, t->row_base, d_out, d_valid,
                                      t->ctx->stream));
    else
        HIP_CHECK(launch_gather(raw_of(c), c.type, d_rowids, d_count, max_n, t->row_base, d_out, t->ctx->stream));
    auto uit = t->upd.find(col);
    if (txn && uit != t->upd.end() && uit->second.any_visible(txn)) {
        const Updates& u = uit->second;
        const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((max_n + 255) / 256, 4096));
        hipLaunchKernelGGL(patch_probe_kernel, dim3(grid), dim3(256), 0, t->ctx->stream, d_rowids, d_count, max_n,
                           t->row_base, static_cast<const int64_t*>(u.rows->p),
                           static_cast<const int64_t*>(u.values->p), u.d_valids(),
                           static_cast<const uint64_t*>(u.versions->p), u.n, txn->start_time, txn->transaction_id,
                           d_out, d_valid);
        HIP_CHECK(hipGetLastError());
    }
    return CUBIT_OK;
}

}  // namespace

extern "C" int cubit_table_probe(cubit_table* t, int col, const cubit_txn* txn, const int64_t* d_rowids,
                                 const uint64_t* d_count, uint64_t max_n, int64_t* d_out) {
    if (!t || !d_rowids || !d_count || !d_out) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    return probe_impl(t, col, txn, d_rowids, d_count, max_n, d_out, nullptr);
}

extern "C" int cubit_table_probe_validity(cubit_table* t, int col, const cubit_txn* txn, const int64_t* d_rowids,
                                          const uint64_t* d_count, uint64_t max_n, int64_t* d_out,
                                          uint64_t* d_validity) {
    if (!t || !d_rowids || !d_count || !d_out || !d_validity) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    return probe_impl(t, col, txn, d_rowids, d_count, max_n, d_out, d_validity);
}

extern "C" int cubit_table_info(cubit_table* t, uint64_t* n_rows, int64_t* row_base, cubit_ctx** ctx) {
    if (!t) return fail(CUBIT_ERR_INVALID, "null table");
    if (n_rows) *n_rows = t->n_rows;
    if (row_base) *row_base = t->row_base;
    if (ctx) *ctx = t->ctx;
    return CUBIT_OK;
}

extern "C" int cubit_table_column_data(cubit_table* t, int col, const void** data, int* type) {
    if (!t || !data) return fail(CUBIT_ERR_INVALID, "null argument");
    CUBIT_LOCK(t->ctx);
    auto it = t->cols.find(col);
    if (it == t->cols.end()) return fail(CUBIT_ERR_INVALID, "column %d not registered", col);
    *data = raw_of(it->second);  // FLOAT / DOUBLE: the patterns (the keys are internal)
    if (type) *type = it->second.type;
    return CUBIT_OK;
}
