// CDNA4 (gfx950) kernels of the bitmap-indexed scan filter.
//
//   K1+K2  eval_decode_pairs — AND/OR/ANDNOT over K bitvectors fused with the
//                          bitvector → int64 row-id compaction. Replaces the per-vector
//                          selection narrowing of RowGroup::TemplatedScan
//                          (src/storage/table/row_group.cpp:537-550 → ColumnSegment::
//                          FilterSelection, column_segment.cpp:378-522) and the row-id
//                          synthesis start+current_row+sel[i] (row_group.cpp:573-580).
//          eval_count_kernel — the same evaluation for count(*) / bitvector materialisation.
//          order_* — optional pass that lays the per-tile runs out in row order.
//   K0     compare_bitvector — predicate → bitvector over a raw column, the comparison
//                          semantics of TemplatedFilterSelection (column_segment.cpp:261-349).
//   K3     gather / gather_sum_product — probe columns at row ids
//                          (ColumnData::FilterScan / FetchRow, column_data.cpp:305-309,452-461).
//   K4     visibility / update_mask — MVCC delta → bitvectors
//                          (ChunkVectorInfo::TemplatedGetSelVector chunk_info.cpp:123-161,
//                           UpdateInfo::UpdatesForTransaction update_info.hpp:44-55).
//
// Bandwidth-bound integer work: no MFMA. Loads are 16 B per lane (dwordx4), a wave moves
// 1 KiB per load instruction; row ids are staged in LDS and written as contiguous runs.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "../../include/cubit_gpu.h"
#include "cubit_internal.hpp"

namespace cubit {

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// Inclusive wave64 prefix sum of a uint32 with DPP (GFX9 row shifts, then row_bcast:15 / :31
// across the four 16-lane rows): six v_add with a DPP operand, no LDS traffic (the 64-bit
// __shfl_up scan above is twelve ds_bpermute). Lanes whose DPP source is outside the row, and
// rows outside row_mask, add `old` = 0.
__device__ __forceinline__ uint32_t wave_incl_scan32(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return x;
}

// Sum over the wave of values below 2^41 (look-back counts): two DPP scans of 24-bit low and high
// parts, the totals read from lane 63 — no ds_bpermute round trips. Every lane must be active.
__device__ __forceinline__ uint64_t wave_sum_flags(uint64_t x) {
    const uint32_t lo = wave_incl_scan32((uint32_t)x & 0xffffffu);
    const uint32_t hi = wave_incl_scan32((uint32_t)(x >> 24));
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 24) +
           (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// Claim-ticket layout (kTicketWords words, context-owned, zero between launches): word 0 =
// running claim counter; word kTicketStride·(1+g) = arrivals of workgroup group g
// (blockIdx % 8, one group per XCD under round-robin dispatch); word kTicketStride·9 =
// arrived groups. Counters sit 512 B apart: atomics on one line serialise (≈88/µs,
// MI355X_MICROARCH.md "dequeue"), and a flat arrival counter put a 512-atomic tail on
// every launch.
//
// finish_ticket is called by thread 0 of every workgroup after its last claim has RETURNED
// (every claim is a returning atomic whose value the caller consumed, so it is performed
// before the arrival is issued). `mine` = the rows this workgroup contributed. An arrival
// carries them: counter += (1 << kArriveShift) | mine, so the arrival count sits in the top
// 16 bits and the running row sum in the low 48. The last workgroup of a group adds the
// group's sum to the top counter; the last group holds the grand total in the value its
// returning atomic gave back, publishes it to *count and re-arms the ticket for the next
// launch on the stream (stream order guarantees that launch sees the zeroes). Two dependent
// atomics from the last arrival to the count, and no kernel has to claim on the running
// counter (word 0) just to be counted: count(*) and the fused sum only arrive.
// No __threadfence(): an agent-scope release on gfx950 writes back L2 (measured +18 µs on
// the decode); only the atomics need ordering, and they are coherent on their own.
constexpr int kArriveShift = 48;
__device__ __forceinline__ void finish_ticket(uint64_t* ticket, uint64_t* count, uint64_t mine) {
    constexpr unsigned long long kArrive = 1ull << kArriveShift, kValue = kArrive - 1;
    const uint32_t G = gridDim.x;
    const uint32_t groups = G < kTicketGroups ? G : kTicketGroups;
    const uint32_t g = blockIdx.x % groups;
    const uint32_t members = G / groups + (g < G % groups ? 1u : 0u);
    unsigned long long* gc = reinterpret_cast<unsigned long long*>(ticket + kTicketStride * (1 + g));
    const unsigned long long og = atomicAdd(gc, kArrive | (unsigned long long)mine);
    if ((og >> kArriveShift) != (unsigned long long)(members - 1)) return;
    const unsigned long long group_sum = (og & kValue) + mine;
    unsigned long long* top = reinterpret_cast<unsigned long long*>(ticket + kTicketStride * (1 + kTicketGroups));
    const unsigned long long ot = atomicAdd(top, kArrive | group_sum);
    if ((ot >> kArriveShift) != (unsigned long long)(groups - 1)) return;
    *count = (ot & kValue) + group_sum;
    atomicExch(reinterpret_cast<unsigned long long*>(ticket), 0ull);
    for (uint32_t i = 0; i < groups; ++i)
        atomicExch(reinterpret_cast<unsigned long long*>(ticket + kTicketStride * (1 + i)), 0ull);
    atomicExch(top, 0ull);
}

__device__ __forceinline__ uint64_t apply_op(uint32_t op, uint64_t a, uint64_t b) {
    return op == OP_AND ? (a & b) : (op == OP_OR ? (a | b) : (a & ~b));
}

// Evaluate the program on NW words per thread. Leaves are loaded by the caller
// (compile-time indexed); the stack is 4 deep and shifted with constant indices so it stays
// in VGPRs.
// FORM (template): FORM_POSTFIX interprets the postfix program; FORM_CONJ = AND of the
// (possibly complemented) leaves; FORM_DNF = OR over groups of AND-ed literals; FORM_CNF =
// AND over groups of OR-ed literals. The last three are branch-free on the data.
template <int K, int NW, int FORM = FORM_POSTFIX>
__device__ __forceinline__ void eval_words(const EvalProgram& prog, const u64x2 (&v)[K][NW / 2],
                                           uint64_t (&r)[NW]) {
    if (FORM == FORM_CONJ) {
        // leaf 0 initialises r; each complemented leaf is a uniform branch, so a word costs
        // one AND (or AND-NOT, v_bfi_b32) per 32 bits instead of an XOR and an AND
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((prog.negate >> k) & 1u) {
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    const uint64_t x = (j & 1) ? v[k][j >> 1].y : v[k][j >> 1].x;
                    r[j] = k == 0 ? ~x : (r[j] & ~x);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    const uint64_t x = (j & 1) ? v[k][j >> 1].y : v[k][j >> 1].x;
                    r[j] = k == 0 ? x : (r[j] & x);
                }
            }
        }
        return;
    }
    if (FORM == FORM_DNF || FORM == FORM_CNF) {
        constexpr bool DNF = FORM == FORM_DNF;
        uint64_t cur[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) r[j] = DNF ? 0ull : ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint64_t neg = ((prog.negate >> k) & 1u) ? ~0ull : 0ull;
            const bool opens = k == 0 || ((prog.gstart >> k) & 1u);
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const u64x2 p = v[k][j >> 1];
                const uint64_t x = ((j & 1) ? p.y : p.x) ^ neg;
                if (k == 0) {
                    cur[j] = x;
                } else if (opens) {
                    r[j] = DNF ? (r[j] | cur[j]) : (r[j] & cur[j]);
                    cur[j] = x;
                } else {
                    cur[j] = DNF ? (cur[j] & x) : (cur[j] | x);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) r[j] = DNF ? (r[j] | cur[j]) : (r[j] & cur[j]);
        return;
    }
    uint64_t s0[NW], s1[NW], s2[NW], s3[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) s0[j] = s1[j] = s2[j] = s3[j] = 0;
    int op_i = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t neg = ((prog.negate >> k) & 1u) ? ~0ull : 0ull;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            s3[j] = s2[j];
            s2[j] = s1[j];
            s1[j] = s0[j];
            const u64x2 p = v[k][j >> 1];
            s0[j] = ((j & 1) ? p.y : p.x) ^ neg;
        }
        const int nops = (int)((prog.nops >> (4 * k)) & 15u);
        for (int t = 0; t < nops; ++t) {
            const uint32_t op = (prog.ops >> (2 * op_i++)) & 3u;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                s0[j] = apply_op(op, s1[j], s0[j]);
                s1[j] = s2[j];
                s2[j] = s3[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) r[j] = s0[j];
}

// Word j of a thread in a tile: pair p = j/2 holds words p·2·THREADS + 2t + {0,1}, so every
// dwordx4 wave-load reads a contiguous 1 KiB.
template <int THREADS>
__device__ __forceinline__ uint64_t word_index(uint64_t tile_word0, int j, int t) {
    return tile_word0 + (uint64_t)(j >> 1) * (2 * THREADS) + 2 * t + (j & 1);
}

template <int NW, int THREADS>
__device__ __forceinline__ void tail_mask(const EvalArgs& a, uint64_t tile_word0, int t, uint64_t (&r)[NW]) {
    // uniform: only the tile that holds the last word (or lies past it) has bits to clear
    if (tile_word0 + (uint64_t)THREADS * NW < a.n_words) return;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint64_t gw = word_index<THREADS>(tile_word0, j, t);
        if (gw >= a.n_words) r[j] = 0;
        else if (gw == a.n_words - 1 && (a.n_rows & 63)) r[j] &= (1ull << (a.n_rows & 63)) - 1;
    }
}

// A tile's result words (materialised subtrees, narrowing masks). SAUX >= 0: buffer stores with
// those cache-policy bits through a descriptor over the tile (tile_word0 is uniform), as the
// decode's copy-out (emit_ids); SAUX < 0: plain stores.
template <int PAIRS, int THREADS, int SAUX = -1>
__device__ __forceinline__ void store_words(uint64_t* out, uint64_t tile_word0, int t, const uint64_t (&r)[2 * PAIRS]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (SAUX >= 0) {
        const uint64_t tw = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(tile_word0 >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)tile_word0);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(out + tw), (short)0, PAIRS * THREADS * 16, 0x00020000);
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            u64x2 o;
            o.x = r[2 * p];
            o.y = r[2 * p + 1];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, (int)((uint32_t)(p * THREADS + t) * 16u),
                                                   0, SAUX < 0 ? 0 : SAUX);
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) {
        u64x2 o;
        o.x = r[2 * p];
        o.y = r[2 * p + 1];
        reinterpret_cast<u64x2*>(out + tile_word0)[p * THREADS + t] = o;
    }
}

// tile_word0 is uniform: each leaf's tile base goes into a buffer descriptor built from
// SGPRs (readfirstlane), and every load is `buffer_load_dwordx4 v, v_off32, s[rsrc] offen nt`
// with one 32-bit per-thread offset shared by all leaves — no 64-bit VGPR address per leaf
// and pair (MI355X guide T8). The descriptor covers exactly the tile's bytes.
template <int K, int PAIRS, int THREADS>
__device__ __forceinline__ void load_tile(const EvalArgs& a, uint64_t tile_word0, int t, u64x2 (&v)[K][PAIRS]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t tw = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(tile_word0 >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)tile_word0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.prog.leaf[k] + tw), (short)0, PAIRS * THREADS * 16, 0x00020000);
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)(p * THREADS + t) * 16u, 0, 2);
            v[k][p] = __builtin_bit_cast(u64x2, x);
        }
    }
}

// rowids[base + i] = row0 + st[i] for i < n, ids at or past `capacity` dropped (base and n are
// workgroup-uniform; n ≤ 2^28 so the byte range fits a buffer descriptor). 16-byte stores from
// the first ALIGN-byte boundary on, the ids before it one per thread. SAUX >= 0: buffer stores through
// a descriptor built from SGPRs with cache-policy bits SAUX — sc1 (16, write-through) measured
// 64.4 µs against 70.1 µs for plain global stores in the decode's read/write floor at SF100 Q6
// (scripts/balbench.hip, profiles/r02e_balbench_cache_policy.txt); SAUX < 0: plain stores.
template <int THREADS, int SAUX, int ALIGN = 16>
__device__ __forceinline__ void emit_ids(int64_t* rowids, uint64_t capacity, const uint32_t* st, uint32_t n,
                                         uint64_t base, int64_t row0, int t) {
    typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t room = capacity > base ? capacity - base : 0;
    const uint32_t lim = (uint32_t)(room < (uint64_t)n ? room : (uint64_t)n);
    if (lim == 0) return;
    int64_t* out = rowids + base;
    static_assert(ALIGN == 16 || ALIGN == 128, "16-byte stores, optionally from a 128-byte line boundary on");
    const uint32_t head = min(lim, (uint32_t)(((ALIGN - (reinterpret_cast<uintptr_t>(out) & (ALIGN - 1))) & (ALIGN - 1)) >> 3));
    if (SAUX < 0) {
        if (t < (int)head) out[t] = row0 + (int64_t)st[t];
        for (uint32_t i = head + 2 * t; i < lim; i += 2 * THREADS) {
            if (i + 1 < lim) {
                i64x2 val;
                val.x = row0 + (int64_t)st[i];
                val.y = row0 + (int64_t)st[i + 1];
                *reinterpret_cast<i64x2*>(out + i) = val;
            } else {
                out[i] = row0 + (int64_t)st[i];
            }
        }
        return;
    }
    const uint64_t ob = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)out >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)out);
    const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane(lim) * 8u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)ob, (short)0, (int)nb, 0x00020000);
    if (t < (int)head)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, row0 + (int64_t)st[t]), rs, (int)(t * 8), 0,
                                              SAUX < 0 ? 0 : SAUX);
    for (uint32_t i = head + 2 * t; i < lim; i += 2 * THREADS) {
        if (i + 1 < lim) {
            i64x2 val;
            val.x = row0 + (int64_t)st[i];
            val.y = row0 + (int64_t)st[i + 1];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), rs, (int)(i * 8u), 0, SAUX < 0 ? 0 : SAUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, row0 + (int64_t)st[i]), rs, (int)(i * 8u), 0,
                                                  SAUX < 0 ? 0 : SAUX);
        }
    }
}

// The prefixed decode's side output (cubit_row_list.hpp): list[base + i] = the low 16 bits of st[i] for
// i < n. Written once per bitvector, by the scan that builds its row list.
template <int THREADS>
__device__ __forceinline__ void emit_list(uint16_t* list, const uint32_t* st, uint32_t n, uint64_t base, int t) {
    for (uint32_t i = t; i < n; i += THREADS) list[base + i] = row_list_encode(st[i]);
}

// The i-th tile of a launch: entry i of the planner's live-tile list (zonemap skip) or i itself.
// i is uniform, so the list entry is a scalar load; callers fetch it one tile ahead.
__device__ __forceinline__ uint32_t tile_at(const EvalArgs& a, uint32_t i) { return a.live ? a.live[i] : i; }

// ------------------------------------------------------------------ K1: count / materialise

// count(*) of the program and/or its result bitvector. Persistent: workgroup g takes tiles
// g, g+G, …, two tiles in flight (register double buffer: the loads of tile i+2 are issued
// as soon as tile i is evaluated), keeps its count in registers and claims once at the end
// (one returning atomic per workgroup).
template <int K, int PAIRS, int FORM = FORM_POSTFIX, int SAUX = -1>
__global__ __launch_bounds__(512, 4) void eval_count_kernel(EvalArgs a) {
    constexpr int THREADS = 512, NW = 2 * PAIRS;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    const int t = threadIdx.x;
    const uint32_t G = gridDim.x;
    uint64_t c = 0;
    u64x2 v0[K][PAIRS], v1[K][PAIRS];
    // i indexes the launch's tiles (tile_at: every tile, or the live-tile list)
    uint32_t i = blockIdx.x;
    const uint32_t n = a.num_tiles;
    if (i < n) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile_at(a, i) * TILE_WORDS, t, v0);
    if (i + G < n) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile_at(a, i + G) * TILE_WORDS, t, v1);
    auto step = [&](u64x2 (&v)[K][PAIRS], uint32_t ii) {
        const uint32_t ahead = ii + 2 * G;
        const uint32_t ahead_tile = ahead < n ? tile_at(a, ahead) : 0;  // list entry fetched before the eval
        const uint64_t tile_word0 = (uint64_t)tile_at(a, ii) * TILE_WORDS;
        uint64_t r[NW];
        eval_words<K, NW, FORM>(a.prog, v, r);
        if (ahead < n) load_tile<K, PAIRS, THREADS>(a, (uint64_t)ahead_tile * TILE_WORDS, t, v);
        tail_mask<NW, THREADS>(a, tile_word0, t, r);
        if (a.result_words) store_words<PAIRS, THREADS, SAUX>(a.result_words, tile_word0, t, r);
#pragma unroll
        for (int j = 0; j < NW; ++j) c += __popcll(r[j]);
    };
    while (i < n) {
        step(v0, i);
        i += G;
        if (i >= n) break;
        step(v1, i);
        i += G;
    }
    __shared__ uint64_t s_part[THREADS / 64];
    c = wave_sum(c);
    if ((t & 63) == 0) s_part[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) s += s_part[w];
        // one arrival carries the count: no returning claim per workgroup (512 of them on one
        // word queued ≈5.8 µs at the end of every count launch, ≈88 per µs)
        finish_ticket(a.ticket, a.count, s);
    }
}

// ------------------------------------------------------------------ K1+K2: evaluate + decode

// Per-tile-claim evaluate + decode (round-1 production kernel, now kept as the reference
// variant in scripts/kbench.hip; the library launches eval_decode_pairs below).
// Persistent, software-pipelined evaluate + decode. Workgroup g takes tiles g, g+G, g+2G, …
// (static striding: per-tile work is uniform up to the decode). Per tile:
//   evaluate the tile whose leaves landed → per-pair bit counts → block scan →
//   ONE returning atomicAdd on the running count claims the tile's output range →
//   issue the NEXT tile's loads (they fly during the rest of this iteration) →
//   decode the set bits into LDS as 32-bit tile-local offsets (each thread's run is
//   ascending and runs are in word order) → copy the run out coalesced as int64 row ids.
// Output: per-tile ascending runs, runs in claim order — the shape of DuckDB's parallel scan,
// whose morsels reach the sink in nondeterministic order with a batch index
// (table_scan.cpp:179-189). dir[2·tile] / dir[2·tile+1] = the run's start / length, so
// reading runs in tile order yields the ascending sequence (order_runs does that on device).
// There is no inter-workgroup wait: a claim is one atomic, so no prefix chain serialises the
// tiles (a decoupled look-back over ~10^4 tiles measured 1.7× slower).
// Per-pair counts are packed as FB-bit fields so one 64-bit scan covers several pairs
// (a pair-chunk holds at most THREADS·128 set bits).
// CLAIM / DECODE = false are diagnostic builds (scripts/kbench.hip). __launch_bounds__: two workgroups per CU (2·THREADS/256 waves per SIMD) caps
// VGPRs at 128.
template <int K, int PAIRS, int STAGE, int THREADS, bool CLAIM = true, bool DECODE = true, int FORM = FORM_POSTFIX>
__global__ __launch_bounds__(THREADS, 2 * THREADS / 256) void eval_decode_tiles(EvalArgs a, uint64_t* __restrict__ dir) {
    constexpr int NW = 2 * PAIRS;
    constexpr int FB = (THREADS * 128 < 65536) ? 16 : 32;
    constexpr int FPW = 64 / FB;
    constexpr uint64_t FMASK = (FB == 16) ? 0xffffull : 0xffffffffull;
    constexpr int NPK = (PAIRS + FPW - 1) / FPW;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr int NWAVES = THREADS / 64;
    static_assert(TILE_WORDS * 64 < (1ull << 32), "tile-local offsets are 32-bit");
    __shared__ uint64_t s_wave_tot[NWAVES][NPK];
    __shared__ uint64_t s_off;
    __shared__ uint32_t s_stage[STAGE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    uint32_t tile = blockIdx.x;
    uint64_t mine = 0;  // thread 0: rows claimed by this workgroup
    u64x2 v[K][PAIRS];
    if (tile < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile * TILE_WORDS, t, v);
    while (tile < a.num_tiles) {
        const uint64_t tile_word0 = (uint64_t)tile * TILE_WORDS;
        uint64_t r[NW];
        eval_words<K, NW, FORM>(a.prog, v, r);
        tail_mask<NW, THREADS>(a, tile_word0, t, r);
        if (a.result_words) store_words<PAIRS, THREADS>(a.result_words, tile_word0, t, r);
        uint64_t packed[NPK], incl[NPK];
#pragma unroll
        for (int q = 0; q < NPK; ++q) packed[q] = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p)
            packed[p / FPW] |= (uint64_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1])) << (FB * (p % FPW));
#pragma unroll
        for (int q = 0; q < NPK; ++q) {
            incl[q] = wave_incl_scan(packed[q], lane);
            if (lane == 63) s_wave_tot[wave][q] = incl[q];
        }
        __syncthreads();  // A: wave totals visible
        uint64_t block_tot[NPK], wave_pre[NPK];
#pragma unroll
        for (int q = 0; q < NPK; ++q) {
            uint64_t wp = 0, bt = 0;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) {
                const uint64_t x = s_wave_tot[w][q];
                if (w < wave) wp += x;
                bt += x;
            }
            block_tot[q] = bt;
            wave_pre[q] = wp;
        }
        uint64_t pair_base[PAIRS];
        uint64_t tile_count = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            pair_base[p] = tile_count;
            tile_count += (block_tot[p / FPW] >> (FB * (p % FPW))) & FMASK;
        }
        uint64_t claimed = 0;
        if (t == 0 && tile_count) {  // not wave-aggregated: built with -amdgpu-atomic-optimizer-strategy=None
            claimed = CLAIM ? atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)tile_count)
                            : (uint64_t)tile * (TILE_WORDS * 64 / 50);  // diag: ~2 % density, disjoint runs
            mine += tile_count;
        }
        const uint32_t next = tile + gridDim.x;
        if (next < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)next * TILE_WORDS, t, v);  // prefetch
        const bool stage = tile_count <= (uint64_t)STAGE;
        const bool write = DECODE && tile_count && a.rowids;
        if (!stage || !write) {
            if (t == 0) {
                s_off = claimed;
                if (dir) {
                    dir[2 * tile] = tile_count ? claimed : 0;
                    dir[2 * tile + 1] = tile_count;
                }
            }
            __syncthreads();
        }
        const uint64_t direct_off = s_off;
        const int64_t row0 = a.row_base + (int64_t)(tile_word0 * 64);
        if (write) {
#pragma unroll
            for (int p = 0; p < PAIRS; ++p) {
                uint64_t off = pair_base[p] +
                               (((wave_pre[p / FPW] + incl[p / FPW] - packed[p / FPW]) >> (FB * (p % FPW))) & FMASK);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    uint64_t w = r[2 * p + e];
                    const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                    while (w) {
                        const uint32_t b = (uint32_t)__builtin_ctzll(w);
                        if (stage) {
                            s_stage[off] = wrow + b;
                        } else {
                            const uint64_t g = direct_off + off;
                            if (g < a.capacity) a.rowids[g] = row0 + (int64_t)(wrow + b);
                        }
                        ++off;
                        w &= w - 1;
                    }
                }
            }
        }
        if (stage && write) {
            if (t == 0) {
                s_off = claimed;
                if (dir) {
                    dir[2 * tile] = claimed;
                    dir[2 * tile + 1] = tile_count;
                }
            }
            __syncthreads();  // B: staged run and its offset visible
            const uint64_t off0 = s_off;
            // 16-byte stores (a wave writes 1 KiB per instruction); one leading 8-byte element
            // when the run starts off a 16-byte boundary
            typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
            int64_t* out = a.rowids + off0;
            const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(out) >> 3) & 1);
            const uint64_t room = a.capacity > off0 ? a.capacity - off0 : 0;
            const uint32_t n = (uint32_t)tile_count;
            if (t == 0 && head && room) out[0] = row0 + (int64_t)s_stage[0];
            for (uint32_t i = head + 2 * t; i < n; i += 2 * THREADS) {
                if (i + 1 < n && i + 1 < room) {
                    i64x2 val;
                    val.x = row0 + (int64_t)s_stage[i];
                    val.y = row0 + (int64_t)s_stage[i + 1];
                    *reinterpret_cast<i64x2*>(out + i) = val;
                } else if (i < room) {
                    out[i] = row0 + (int64_t)s_stage[i];
                }
            }
        }
        __syncthreads();  // C: stage / s_off / s_wave_tot free for the next tile
        tile = next;
    }
    if (t == 0) finish_ticket(a.ticket, a.count, mine);
}

__device__ uint64_t* g_diag_times;  // DIAG & 4 builds only (scripts/kbench.hip)

// Pair-claimed evaluate + decode: one returning atomic per PAIR of tiles, issued one unit
// before its result is needed, so the claim latency is covered by the next tile's work.
// Per pair (tiles A = u, B = u + G of this workgroup's walk):
//   unit A: wait A's leaves → eval → block scan → copy out the PREVIOUS pair (its claim
//           returned meanwhile) → prefetch B → decode A into the pair's stage
//   unit B: wait B's leaves → eval → block scan → claim cnt(A)+cnt(B) → prefetch the next A →
//           decode B into the stage right after A's run
// Stage entries are 32-bit row offsets from tile A's first row (tile B sits G·TILE_ROWS
// further), so the pair's output is ONE contiguous run of cnt(A)+cnt(B) ids, copied out with
// 16-byte stores (measured: 16 B/lane stores cut this read/write mix's floor from 81 to 77 µs).
// Copy-out stores are issued before the prefetch they precede, so the wait for the prefetched
// leaves (vmcnt counts stores too) does not add a store round trip. A tile with more than
// STAGE hits claims on its own and writes straight to the output (dense path).
template <int K, int PAIRS, int STAGE, int THREADS, int DIAG = 0, int FORM = FORM_POSTFIX, int WG_PER_CU = 2,
          bool DSTAGE = true, int SAUX = 16>
__global__ __launch_bounds__(THREADS, WG_PER_CU * THREADS / 256) void eval_decode_pairs(EvalArgs a,
                                                                                       uint64_t* __restrict__ dir) {
    // DIAG (scripts/kbench.hip only): bit 0 = no claim (fixed pair offsets), bit 1 = uniform
    // fake decode (same LDS traffic, no per-bit loop), bit 2 = record each workgroup's start
    // and end (s_memrealtime, 100 MHz) into g_diag_times[2·blockIdx + {0, 1}]
    constexpr int NW = 2 * PAIRS;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr uint64_t TILE_ROWS = TILE_WORDS * 64;
    constexpr int NWAVES = THREADS / 64;
    constexpr bool EARLY = K <= 4;
    static_assert(TILE_WORDS * 64 < (1ull << 32), "tile-local offsets are 32-bit");
    static_assert(PAIRS <= 2, "pair counts are scanned as 16-bit fields of one uint32");
    __shared__ uint32_t s_wave_tot[2][NWAVES];
    __shared__ uint64_t s_off;        // claimed base of the pair being copied out
    __shared__ uint64_t s_dense_off;  // claimed base of a dense tile
    __shared__ uint32_t s_stage[2][2 * STAGE];
    __shared__ uint32_t s_tile_a[2], s_tile_b[2], s_cnt_a[2], s_cnt_b[2], s_dense[2];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const uint32_t G = gridDim.x;
    // B's rows as offsets from A's first row must fit 32 bits
    if ((uint64_t)G * TILE_ROWS + TILE_ROWS >= (1ull << 32)) __builtin_trap();
    const bool write_ids = a.rowids != nullptr;
    if ((DIAG & 4) && t == 0) g_diag_times[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    uint64_t pend_claim = 0;  // thread 0: the previous pair's claimed base
    uint64_t mine = 0;        // thread 0: rows claimed by this workgroup (carried by its arrival)

    u64x2 v[K][PAIRS];
    uint32_t tile = blockIdx.x;
    if (tile < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile * TILE_WORDS, t, v);

    // evaluate the tile in v → r, block scan → per-pair offsets within the tile, tile count
    // publish the previous pair's claim (thread 0, before a barrier): base + directory entries
    auto publish = [&](int sp) {
        s_off = pend_claim;
        if (dir) {
            // staged tiles (dense ones wrote their own entry); empty tiles get {0, 0}
            const uint32_t ca = s_cnt_a[sp], cb = s_cnt_b[sp];
            if (!(s_dense[sp] & 1)) {
                dir[2 * s_tile_a[sp]] = ca ? pend_claim : 0;
                dir[2 * s_tile_a[sp] + 1] = ca;
            }
            if (!(s_dense[sp] & 2) && s_tile_b[sp] < a.num_tiles) {
                dir[2 * s_tile_b[sp]] = cb ? pend_claim + ca : 0;
                dir[2 * s_tile_b[sp] + 1] = cb;
            }
        }
    };

    // evaluate the tile in v → r; with EARLY, issue the loads of tile `prefetch` into v right
    // away (v is dead once evaluated: the longest prefetch distance one register set allows;
    // K ≤ 4 only — at K ≥ 5 the leaves in flight beside the scan state spill, measured
    // 92 vs 88 µs, so the loads wait until after the copy-out / claim);
    // block scan → per-pair offsets within the tile, tile count
    auto eval_scan = [&](uint32_t tl, int par, uint64_t (&r)[NW], uint32_t (&pair_off)[PAIRS],
                         int publish_sp, uint32_t prefetch) -> uint64_t {
        const uint64_t tile_word0 = (uint64_t)tl * TILE_WORDS;
        eval_words<K, NW, FORM>(a.prog, v, r);
        if (EARLY && prefetch < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)prefetch * TILE_WORDS, t, v);
        tail_mask<NW, THREADS>(a, tile_word0, t, r);
        if (a.result_words) store_words<PAIRS, THREADS>(a.result_words, tile_word0, t, r);
        // pair counts as 16-bit fields of one uint32 (a wave's total per pair ≤ 8,192), DPP scan
        uint32_t packed = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p)
            packed |= (uint32_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1])) << (16 * p);
        const uint32_t incl = wave_incl_scan32(packed);
        if (lane == 63) s_wave_tot[par][wave] = incl;
        if (publish_sp >= 0 && t == 0) publish(publish_sp);
        __syncthreads();
        uint32_t wave_pre[2] = {0, 0}, block_tot[2] = {0, 0};
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
            const uint32_t x = s_wave_tot[par][w];
            const uint32_t lo = x & 0xffffu, hi = x >> 16;
            if (w < wave) {
                wave_pre[0] += lo;
                wave_pre[1] += hi;
            }
            block_tot[0] += lo;
            block_tot[1] += hi;
        }
        const uint32_t excl = incl - packed;
        // in-tile offsets and counts fit 32 bits (≤ TILE_WORDS·64 < 2^32, static_assert below)
        uint32_t tile_count = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            pair_off[p] = tile_count + wave_pre[p] + ((excl >> (16 * p)) & 0xffffu);
            tile_count += block_tot[p];
        }
        return tile_count;
    };

    // rowids[base + i] = row0 + st[i] for i < n: 16-byte stores (the first id alone when the
    // output is not 16-byte aligned there), bounded by the capacity
    auto emit = [&](const uint32_t* st, uint32_t n, uint64_t base, int64_t row0) {
        emit_ids<THREADS, SAUX>(a.rowids, a.capacity, st, n, base, row0, t);
    };

    // decode r into stage sp at stage_base with row offsets + delta; a dense tile claims on its
    // own and leaves through the other stage (copied out already) in rounds of 2·STAGE ids.
    // Returns the staged count (0 for a dense tile).
    auto decode = [&](uint32_t tl, int sp, uint32_t stage_base, uint32_t delta, const uint64_t (&r)[NW],
                      const uint32_t (&pair_off)[PAIRS], uint64_t tile_count) -> uint32_t {
        if (tile_count <= (uint64_t)STAGE) {
            if (DIAG & 2) {
                for (uint32_t i = t; i < (uint32_t)tile_count; i += THREADS) s_stage[sp][stage_base + i] = delta + i * 53;
            } else if (write_ids) {
#pragma unroll
                for (int p = 0; p < PAIRS; ++p) {
                    uint32_t off = stage_base + (uint32_t)pair_off[p];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        uint64_t w = r[2 * p + e];
                        const uint32_t wrow = delta + (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                        while (w) {
                            s_stage[sp][off++] = wrow + (uint32_t)__builtin_ctzll(w);
                            w &= w - 1;
                        }
                    }
                }
            }
            return (uint32_t)tile_count;
        }
        // dense tile: its own claim, direct writes
        const int64_t row0 = a.row_base + (int64_t)((uint64_t)tl * TILE_ROWS);
        if (t == 0) {
            const uint64_t c = atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)tile_count);
            mine += tile_count;
            s_dense_off = c;
            if (dir) {
                dir[2 * tl] = c;
                dir[2 * tl + 1] = tile_count;
            }
        }
        __syncthreads();  // also: every thread is done with the copy-out of stage sp ^ 1
        const uint64_t base = s_dense_off;
        if (write_ids && DSTAGE) {
            // stage sp ^ 1 was copied out before this pair's first barrier and is next written
            // by the next pair, behind its own barrier
            uint32_t* st = s_stage[sp ^ 1];
            constexpr uint32_t CAP = 2 * STAGE;
            for (uint32_t r0 = 0; r0 < (uint32_t)tile_count; r0 += CAP) {
                const uint32_t r1 = min((uint32_t)tile_count, r0 + CAP);
#pragma unroll
                for (int p = 0; p < PAIRS; ++p) {
                    uint32_t off = pair_off[p];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        uint64_t w = r[2 * p + e];
                        const uint32_t c = (uint32_t)__popcll(w);
                        const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                        if (off < r1 && off + c > r0) {
                            uint32_t k = off;
                            for (; k < r0; ++k) w &= w - 1;  // the word straddles the round's start
                            for (; w && k < r1; ++k) {
                                st[k - r0] = wrow + (uint32_t)__builtin_ctzll(w);
                                w &= w - 1;
                            }
                        }
                        off += c;
                    }
                }
                __syncthreads();
                emit(st, r1 - r0, base + r0, row0);
                __syncthreads();
            }
        } else if (write_ids) {
#pragma unroll
            for (int p = 0; p < PAIRS; ++p) {
                uint64_t off = base + pair_off[p];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    uint64_t w = r[2 * p + e];
                    const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                    while (w) {
                        if (off < a.capacity) a.rowids[off] = row0 + (int64_t)(wrow + (uint32_t)__builtin_ctzll(w));
                        ++off;
                        w &= w - 1;
                    }
                }
            }
        }
        __syncthreads();  // s_dense_off (and the scratch stage) free again
        return 0;
    };

    // copy out stage sp (one contiguous run of cnt_a + cnt_b ids) at the claimed base, which
    // thread 0 published before the barrier that precedes this call. No barrier of its own:
    // stage sp is next written two units later and s_off next published one pair later,
    // both behind barriers every thread passes after this copy.
    auto copy_out = [&](int sp) {
        const uint64_t base = s_off;
        const uint32_t n = s_cnt_a[sp] + s_cnt_b[sp];
        if (write_ids && n)
            emit_ids<THREADS, SAUX>(a.rowids, a.capacity, s_stage[sp], n, base,
                                    a.row_base + (int64_t)((uint64_t)s_tile_a[sp] * TILE_ROWS), t);
    };

    bool pending = false;  // a claimed pair waits for copy-out (uniform)
    uint32_t pair = 0;
    while (tile < a.num_tiles) {
        const int sp = (int)(pair & 1);
        // ---- unit A
        uint64_t r[NW];
        uint32_t off[PAIRS];
        const uint32_t tile_b = tile + G;
        const uint64_t cnt_a_all = eval_scan(tile, 0, r, off, pending ? (sp ^ 1) : -1, tile_b);
        if (pending) copy_out(sp ^ 1);
        if (!EARLY && tile_b < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile_b * TILE_WORDS, t, v);
        const uint32_t ca = decode(tile, sp, 0, 0, r, off, cnt_a_all);
        // ---- unit B
        uint32_t cb = 0;
        uint32_t next = tile_b;
        bool dense_b = false;
        if (tile_b < a.num_tiles) {
            next = tile_b + G;
            const uint64_t cnt_b_all = eval_scan(tile_b, 1, r, off, -1, next);
            dense_b = cnt_b_all > (uint64_t)STAGE;
            const uint32_t staged_b = cnt_b_all <= (uint64_t)STAGE ? (uint32_t)cnt_b_all : 0;
            if (t == 0 && (ca + staged_b)) {
                pend_claim = (DIAG & 1) ? (uint64_t)tile * 5400
                                        : atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)(ca + staged_b));
                mine += ca + staged_b;
            }
            if (!EARLY && next < a.num_tiles) load_tile<K, PAIRS, THREADS>(a, (uint64_t)next * TILE_WORDS, t, v);
            cb = decode(tile_b, sp, ca, G * (uint32_t)TILE_ROWS, r, off, cnt_b_all);
        } else if (t == 0 && ca) {
            pend_claim = atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)ca);
            mine += ca;
        }
        if (t == 0) {
            s_tile_a[sp] = tile;
            s_tile_b[sp] = tile_b;
            s_cnt_a[sp] = ca;
            s_cnt_b[sp] = cb;
            s_dense[sp] = (cnt_a_all > (uint64_t)STAGE ? 1u : 0u) | (dense_b ? 2u : 0u);
        }
        __syncthreads();  // this pair's stage and counts complete
        pending = true;
        tile = next;
        ++pair;
    }
    if (pending) {
        const int sp = (int)((pair - 1) & 1);
        if (t == 0) publish(sp);
        __syncthreads();
        copy_out(sp);
    }
    if (t == 0) finish_ticket(a.ticket, a.count, mine);
    if ((DIAG & 4) && t == 0) g_diag_times[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
}

// Run-claimed evaluate + decode: the workgroup keeps decoding tiles into one LDS stage (a
// *run*) until the next tile would not fit (or the run holds MAXT tiles), then claims the whole
// run with ONE returning atomic and switches to the other stage; the claim returns while the
// next tile is evaluated, and the closed run is copied out (16-byte stores) after that tile's
// scan barrier. The claim count follows the output volume (≈ q / RUN_CAP + workgroups) instead
// of the tile count (pairs: one per two tiles), and a tile costs one block barrier instead of
// one and a half. A stage entry is the row's offset from the run's first tile row (a run spans
// fewer than 2^32 / TILE_ROWS tiles so that fits 32 bits), so the copy-out adds one base per run.
// With a live-tile list (zonemap skip) the workgroup walks list entries g, g+G, … instead of
// tiles; runs, offsets and the directory are per tile as before, skipped tiles keep the {0, 0}
// entries the host cleared. Tiles with more than RUN_CAP hits claim on
// their own and write straight to the output (dense path). The directory gets {start, len} per
// tile ({0, 0} for empty tiles) as with pairs.
// Workgroup g takes tiles g, g+G, … (static striding). A dynamic hand-out of the last third of
// the tiles from per-XCD heads (scripts/kbench.hip) evened the workgroups' end
// times (spread 25 → 14 µs) but slowed every workgroup more than that gained: its dequeue is a
// returning atomic that the next wait on the leaf loads (vmcnt counts in order) also waits for.
template <int K, int PAIRS, int RUN_CAP, int THREADS, int FORM = FORM_POSTFIX, int MAXT = 16, bool STAMP = false,
          bool DSTAGE = true, int SAUX = 16, int ALIGN = 16, int EARLY_AT = 4>
__global__ __launch_bounds__(THREADS, 2 * THREADS / 256) void eval_decode_runs(EvalArgs a, uint64_t* __restrict__ dir) {
    // STAMP (scripts/kbench.hip only): each workgroup's start / end (s_memrealtime) into g_diag_times
    if (STAMP && threadIdx.x == 0) g_diag_times[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    constexpr int NW = 2 * PAIRS;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr uint64_t TILE_ROWS = TILE_WORDS * 64;
    static_assert(MAXT <= 64, "directory entries per run");
    constexpr int NWAVES = THREADS / 64;
    constexpr bool EARLY = K <= EARLY_AT;  // next tile's loads before the copy-out (K <= 4) or after it
    // per-wave totals of the pair counts, two 16-bit fields (a wave's total per pair is at most
    // 64 lanes × 128 bits = 8,192)
    static_assert(PAIRS <= 2, "pair counts are scanned as 16-bit fields of one uint32");
    __shared__ uint32_t s_wave_tot[2][NWAVES];
    __shared__ uint64_t s_off;        // claimed base of the run being copied out
    __shared__ uint64_t s_dense_off;  // claimed base of a dense tile
    __shared__ uint32_t s_stage[2][RUN_CAP];
    __shared__ uint32_t s_rt[2][MAXT], s_ro[2][MAXT], s_rc[2][MAXT];  // run tiles: tile, offset, count
    __shared__ uint32_t s_rn[2], s_rfill[2], s_rfirst[2];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const uint32_t G = gridDim.x;
    // a stage entry (tile - run's first tile)·TILE_ROWS + row must fit 32 bits
    constexpr uint32_t kMaxSpan = (uint32_t)((1ull << 32) / TILE_ROWS);
    const bool write_ids = a.rowids != nullptr;
    uint64_t pend_claim = 0;  // thread 0: the closed run's claimed base
    uint64_t mine = 0;        // thread 0: rows claimed by this workgroup

    u64x2 v[K][PAIRS];
    // i indexes the launch's tiles (every tile, or the live-tile list of the zonemap skip);
    // tile / next_tile are the current and the next tile, the list entry after them is fetched
    // one unit ahead
    const uint32_t n_idx = a.num_tiles;
    uint32_t i = blockIdx.x;
    uint32_t tile = i < n_idx ? tile_at(a, i) : 0;
    uint32_t next_tile = i + G < n_idx ? tile_at(a, i + G) : 0;
    if (i < n_idx) load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile * TILE_WORDS, t, v);

    // rowids[base + i] = row0 + st[i] for i < n: 16-byte stores (the first id alone when the
    // output is not 16-byte aligned there), bounded by the capacity
    auto emit = [&](const uint32_t* st, uint32_t n, uint64_t base, int64_t row0) {
        emit_ids<THREADS, SAUX, ALIGN>(a.rowids, a.capacity, st, n, base, row0, t);
    };
    // copy out closed run rs at s_off (published before the preceding barrier) and write its
    // directory entries
    auto copy_out = [&](int rs) {
        const uint64_t base = s_off;
        const uint32_t n = s_rfill[rs];
        const uint32_t nt = s_rn[rs];
        if (dir && t < (int)nt) {
            dir[2 * s_rt[rs][t]] = s_rc[rs][t] ? base + s_ro[rs][t] : 0;
            dir[2 * s_rt[rs][t] + 1] = s_rc[rs][t];
        }
        if (write_ids && n) emit(s_stage[rs], n, base, a.row_base + (int64_t)((uint64_t)s_rfirst[rs] * TILE_ROWS));
    };

    int rs = 0;              // the open run's stage
    uint32_t fill = 0, rn = 0, rfirst = 0;  // open run: entries, tiles, first tile (uniform)
    bool pending = false;    // a closed run (stage rs ^ 1) waits for its claim and copy-out
    uint32_t u = 0;
    while (i < n_idx) {
        const int par = (int)(u & 1);
        const uint64_t tile_word0 = (uint64_t)tile * TILE_WORDS;
        const bool has_next = i + G < n_idx;
        const uint32_t after = i + 2 * G < n_idx ? tile_at(a, i + 2 * G) : 0;
        uint64_t r[NW];
        eval_words<K, NW, FORM>(a.prog, v, r);
        if (EARLY && has_next) load_tile<K, PAIRS, THREADS>(a, (uint64_t)next_tile * TILE_WORDS, t, v);
        tail_mask<NW, THREADS>(a, tile_word0, t, r);
        if (a.result_words) store_words<PAIRS, THREADS>(a.result_words, tile_word0, t, r);
        uint32_t packed = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p)
            packed |= (uint32_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1])) << (16 * p);
        const uint32_t incl = wave_incl_scan32(packed);
        if (lane == 63) s_wave_tot[par][wave] = incl;
        if (pending && t == 0) s_off = pend_claim;  // the closed run's claim returned meanwhile
        __syncthreads();
        uint32_t wave_pre[2] = {0, 0}, block_tot[2] = {0, 0};
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
            const uint32_t x = s_wave_tot[par][w];
            const uint32_t lo = x & 0xffffu, hi = x >> 16;
            if (w < wave) {
                wave_pre[0] += lo;
                wave_pre[1] += hi;
            }
            block_tot[0] += lo;
            block_tot[1] += hi;
        }
        const uint32_t excl = incl - packed;  // per field: no borrow (incl ≥ packed field-wise)
        uint32_t pair_off[PAIRS];
        uint32_t tile_count = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            pair_off[p] = tile_count + wave_pre[p] + ((excl >> (16 * p)) & 0xffffu);
            tile_count += block_tot[p];
        }
        const bool dense = tile_count > (uint32_t)RUN_CAP;
        // close the open run when this tile does not fit (claimed after the previous run's
        // copy-out: issuing the claim before it measured 3 µs slower at K = 5)
        const bool close = !dense && rn > 0 &&
                           (fill + tile_count > (uint32_t)RUN_CAP || rn == (uint32_t)MAXT || tile - rfirst >= kMaxSpan);
        const bool copied = pending;
        if (pending) {
            copy_out(rs ^ 1);
            pending = false;
        }
        if (!EARLY && has_next) load_tile<K, PAIRS, THREADS>(a, (uint64_t)next_tile * TILE_WORDS, t, v);
        const int64_t row0 = a.row_base + (int64_t)tile_word0 * 64;
        if (dense) {
            // dense tile: its own claim, direct writes
            if (t == 0) {
                const uint64_t c = atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)tile_count);
                mine += tile_count;
                s_dense_off = c;
                if (dir) {
                    dir[2 * tile] = c;
                    dir[2 * tile + 1] = tile_count;
                }
            }
            __syncthreads();  // also: every thread is done with the copy-out of stage rs ^ 1
            const uint64_t base = s_dense_off;
            if (write_ids && DSTAGE) {
                // in rounds of RUN_CAP ids through the free stage (rs ^ 1; the open run keeps
                // stage rs): each thread decodes its bits whose tile-local index falls in the
                // round, then the round leaves as 16-byte stores
                uint32_t* st = s_stage[rs ^ 1];
                for (uint32_t r0 = 0; r0 < tile_count; r0 += (uint32_t)RUN_CAP) {
                    const uint32_t r1 = min(tile_count, r0 + (uint32_t)RUN_CAP);
#pragma unroll
                    for (int p = 0; p < PAIRS; ++p) {
                        uint32_t off = pair_off[p];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            uint64_t w = r[2 * p + e];
                            const uint32_t c = (uint32_t)__popcll(w);
                            const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                            if (off < r1 && off + c > r0) {
                                uint32_t k = off;
                                for (; k < r0; ++k) w &= w - 1;  // the word straddles the round's start
                                for (; w && k < r1; ++k) {
                                    st[k - r0] = wrow + (uint32_t)__builtin_ctzll(w);
                                    w &= w - 1;
                                }
                            }
                            off += c;
                        }
                    }
                    __syncthreads();
                    emit(st, r1 - r0, base + r0, row0);
                    __syncthreads();
                }
            } else if (write_ids) {
#pragma unroll
                for (int p = 0; p < PAIRS; ++p) {
                    uint64_t off = base + pair_off[p];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        uint64_t w = r[2 * p + e];
                        const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                        while (w) {
                            if (off < a.capacity) a.rowids[off] = row0 + (int64_t)(wrow + (uint32_t)__builtin_ctzll(w));
                            ++off;
                            w &= w - 1;
                        }
                    }
                }
            }
            __syncthreads();  // s_dense_off (and the scratch stage) free again
        } else {
            if (close) {
                // one claim for the whole run (returns during the next tile)
                if (t == 0) {
                    s_rn[rs] = rn;
                    s_rfill[rs] = fill;
                    s_rfirst[rs] = rfirst;
                    pend_claim = 0;
                    if (fill) {
                        pend_claim = atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)fill);
                        mine += fill;
                    }
                }
                pending = true;
                rs ^= 1;
                fill = 0;
                rn = 0;
                // the stage we switch to was copied out in this unit: every thread must be done
                if (copied) __syncthreads();
            }
            if (rn == 0) rfirst = tile;
            if (tile_count && write_ids) {
                const uint32_t delta = (tile - rfirst) * (uint32_t)TILE_ROWS;
#pragma unroll
                for (int p = 0; p < PAIRS; ++p) {
                    uint32_t off = fill + pair_off[p];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        uint64_t w = r[2 * p + e];
                        const uint32_t wrow = delta + (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                        while (w) {
                            s_stage[rs][off++] = wrow + (uint32_t)__builtin_ctzll(w);
                            w &= w - 1;
                        }
                    }
                }
            }
            if (t == 0) {
                s_rt[rs][rn] = tile;
                s_ro[rs][rn] = fill;
                s_rc[rs][rn] = tile_count;
            }
            fill += tile_count;
            ++rn;
        }
        i += G;
        tile = next_tile;
        next_tile = after;
        ++u;
    }
    // drain: the closed run (if any), then the open one
    if (pending) {
        if (t == 0) s_off = pend_claim;
        __syncthreads();
        copy_out(rs ^ 1);
    }
    if (rn > 0) {
        if (t == 0) {
            s_rn[rs] = rn;
            s_rfill[rs] = fill;
            s_rfirst[rs] = rfirst;
            uint64_t c = 0;
            if (fill) {
                c = atomicAdd(reinterpret_cast<unsigned long long*>(a.ticket), (unsigned long long)fill);
                mine += fill;
            }
            pend_claim = c;
        }
        __syncthreads();  // s_off may still be read by the copy-out above
        if (t == 0) s_off = pend_claim;
        __syncthreads();
        copy_out(rs);
    }
    if (t == 0) finish_ticket(a.ticket, a.count, mine);
    if (STAMP && t == 0) g_diag_times[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
}

// ------------------------------------------------------------------ K1+K2 for small partitions

// One tile per workgroup, output offsets by look-back instead of a claim. For partitions whose
// tiles fit the co-resident grid (WPC workgroups per CU: SF100 split over 8 GPUs = 572 tiles,
// SURVEY config 2 = 768), where the claim kernels are latency-bound: every workgroup of those
// takes its one claim at about the same moment, and one word serves ≈ 88 returning atomics per µs
// (MI355X_MICROARCH.md "dequeue"), so the last claim of 572 returns ≈ 6.5 µs after the first.
// Here each workgroup
//   loads and evaluates its tile → block scan → publishes the tile's count in its own flag word
//   (agent-scope store; the word carries the launch's epoch in its high bits, so flags are never
//   reset) → decodes its rows into LDS (the flags of its predecessors land meanwhile) → sums the
//   counts of every earlier workgroup, each thread polling one or two flags (agent-scope loads,
//   MI355X_MICROARCH.md hand-off table row 1; the whole window in one round trip once they are
//   published) → copies its run out at that offset and writes its directory entry. The last
//   workgroup writes the count: no arrival ticket either. A workgroup waits only on lower block
//   indices, which are dispatched before it, so the walk completes whatever the residency.
// A tile with more rows than the stage leaves through it in rounds after the offset is known.
// A poll that exceeds the spin limit (EvalArgs::spin_limit, kLookbackSpins by default) does not
// fail the scan: the thread stops waiting and flags the workgroup, which then walks the earlier
// flags once more without waiting and counts every tile still unpublished from its bitvectors
// itself (lookback_recount — the same program over the same words, so the same count). No
// workgroup ever waits on another without bound, every workgroup writes its run, and the last
// one's count is the true count whatever the dispatch order: the kernel has no failure exit for
// the host to miss.
// Runs land in tile order, so the output is one ascending array: ordered scans take this kernel
// at any size up to kLookbackMaxTiles (SF100, 4,578 tiles: 68.5 µs against 95 µs for the
// run-claimed decode plus the ordering pass; scripts/smallbench.hip).
constexpr int kFlagCntBits = 20;  // a tile holds ≤ 131,072 rows
constexpr uint32_t kLookbackSpins = 1u << 22;

// The expiry path of the look-back (workgroup-uniform call): the rows of tiles 0 … b-1 of the
// launch, each taken from its published flag when it is there now, else counted by the whole
// workgroup from the tile's bitvectors (load_tile / eval_words / tail_mask, as the tile's own
// workgroup does). s_list holds THREADS entries, s_n and s_sum are scratch.
template <int K, int FORM, int THREADS, int PAIRS>
__device__ uint64_t lookback_recount(const EvalArgs& a, uint32_t b, int t, uint32_t* s_list, uint32_t* s_n,
                                     uint64_t* s_sum) {
    constexpr int NWAVES = THREADS / 64;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * 2 * PAIRS;
    constexpr uint64_t kCntMask = (1ull << kFlagCntBits) - 1;
    uint64_t acc = 0;
    for (uint32_t j0 = 0; j0 < b; j0 += THREADS) {
        const uint32_t j = j0 + (uint32_t)t;
        __syncthreads();  // the previous round's list is consumed
        if (t == 0) *s_n = 0;
        __syncthreads();
        if (j < b) {
            const uint64_t f = __hip_atomic_load(a.flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((f >> kFlagCntBits) == a.epoch) acc += f & kCntMask;
            else s_list[atomicAdd(s_n, 1u)] = j;
        }
        __syncthreads();
        const uint32_t n_miss = *s_n;
#pragma unroll 1
        for (uint32_t i = 0; i < n_miss; ++i) {
            // one word pair per thread at a time (half the registers of the tile's own pass:
            // this runs while that pass's words are still live)
#pragma unroll 1
            for (int h = 0; h < PAIRS; ++h) {
                const uint64_t w0 = (uint64_t)tile_at(a, s_list[i]) * TILE_WORDS + (uint64_t)h * 2 * THREADS;
                u64x2 v[K][1];
                load_tile<K, 1, THREADS>(a, w0, t, v);
                uint64_t r[2];
                eval_words<K, 2, FORM>(a.prog, v, r);
                tail_mask<2, THREADS>(a, w0, t, r);
                acc += (uint64_t)(__popcll(r[0]) + __popcll(r[1]));
            }
        }
    }
    acc = wave_sum_flags(acc);
    __syncthreads();
    if ((t & 63) == 0) s_sum[t >> 6] = acc;
    __syncthreads();
    uint64_t total = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) total += s_sum[w];
    return total;
}
// DBG (diagnostic builds, scripts/smallbench.hip; 0 in the library): 1 no spin, 2 no ids, 4 no
// sleep, 8 no flag loads, 16 no LDS decode, 64 the staging loop without its LDS stores, 128 the
// staging by rank (stage_by_rank) instead of the per-lane loop.
// Measured and not kept (scripts/smallbench.hip; profiles/r03e_*, r03g_*, r03h_*): eight copies of
// every flag, each reader on its own; a two-level walk (groups of 64 tiles + group totals); flag
// loads issued before the LDS decode; a decoupled look-back (aggregate, then inclusive-prefix flags,
// walks that stop at the nearest prefix) — slower at every size measured, 573 to 4,578 tiles (at
// 4,578 the sum over every earlier flag costs 68.5 µs, the decoupled walk 91 µs).
// Diagnostic (DBG 128): a wave's set bits of one word pair handed out by rank instead of by
// word — lane l's two words are words 2l, 2l+1 of the wave's slice, `inc` its inclusive count
// in the slice, `wtot` the slice's total and `base` its first stage slot; `row0` is the slice's
// first row in the tile. Each lane takes ids k = lane, lane + 64, … : the owning lane by a binary
// search over the lanes' inclusive counts (LDS), the word by its popcount, the bit by a popcount
// walk over halves (no pdep on CDNA4). Trips per wave: ⌈wtot / 64⌉ instead of the largest
// per-lane popcount of each word. Uses s_words' wave region for the words and s_inc's.
template <int THREADS>
__device__ __forceinline__ void stage_by_rank(uint64_t w0, uint64_t w1, uint32_t inc, uint32_t wtot, uint32_t base,
                                              uint32_t row0, uint64_t* s_words, uint32_t* s_inc, uint32_t* s_stage,
                                              int lane, int wave) {
    uint64_t* sw = s_words + (uint32_t)wave * 128u;
    uint32_t* si = s_inc + (uint32_t)wave * 64u;
    sw[2 * lane] = w0;
    sw[2 * lane + 1] = w1;
    si[lane] = inc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (uint32_t k = (uint32_t)lane; k < wtot; k += 64u) {
        // owner: the number of lanes whose inclusive count is <= k
        uint32_t l = 0;
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1)
            if (si[l + step - 1] <= k) l += step;
        const uint32_t ex = l ? si[l - 1] : 0u;
        uint32_t rk = k - ex;
        const uint64_t a0 = sw[2 * l], a1 = sw[2 * l + 1];
        const uint32_t c0 = (uint32_t)__popcll(a0);
        const bool second = rk >= c0;
        uint64_t w = second ? a1 : a0;
        rk -= second ? c0 : 0u;
        uint32_t x = (uint32_t)w, pos = 0;
        uint32_t c = (uint32_t)__popc(x);
        if (rk >= c) {
            rk -= c;
            x = (uint32_t)(w >> 32);
            pos = 32;
        }
#pragma unroll
        for (uint32_t h = 16; h; h >>= 1) {
            c = (uint32_t)__popc(x & ((1u << h) - 1u));
            if (rk >= c) {
                rk -= c;
                x >>= h;
                pos += h;
            }
        }
        s_stage[base + k] = row0 + (2u * l + (second ? 1u : 0u)) * 64u + pos;
    }
    __builtin_amdgcn_wave_barrier();
}

// PRE: an instantiation for launches with EvalArgs::tile_prefix only. Nothing is published or
// waited for, so a dense tile's result words stay in registers and neither s_words nor the
// recount's list take LDS: four workgroups share a CU where three did.
template <int K, int FORM, int STAGE, int WPC, int SAUX = 16, int DBG = 0, int THREADS = 512, bool PRE = false>
__global__ __launch_bounds__(THREADS, WPC * THREADS / 256) void eval_decode_lookback(EvalArgs a,
                                                                                    uint64_t* __restrict__ dir) {
    constexpr int PAIRS = 2, NW = 2 * PAIRS, NWAVES = THREADS / 64;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr uint64_t kCntMask = (1ull << kFlagCntBits) - 1;
    __shared__ uint32_t s_wave_tot[NWAVES];
    __shared__ uint64_t s_pre[NWAVES];
    __shared__ uint32_t s_expired;
    __shared__ uint32_t s_list_n;
    __shared__ uint32_t s_list_scratch[PRE ? 1 : THREADS];
    __shared__ uint32_t s_stage[STAGE];
    // a dense tile's result words, kept here across the look-back walk (16 KiB: three workgroups
    // per CU still fit the 160 KiB) instead of being read and evaluated a second time
    __shared__ uint64_t s_words[PRE ? 1 : (uint32_t)THREADS * 2 * PAIRS];
    static_assert(!PRE || !(DBG & 128), "the by-rank stage uses s_words");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t b = blockIdx.x;
    const uint32_t tile = tile_at(a, b);
    const uint64_t tile_word0 = (uint64_t)tile * TILE_WORDS;
    const bool write_ids = a.rowids != nullptr;
    const uint32_t spin_limit = a.spin_limit ? a.spin_limit : kLookbackSpins;
    // with per-tile counts known up front (a single index leaf: EvalArgs::tile_prefix) the
    // offset is one load, issued here so that it lands while the tile is read and decoded, and
    // no workgroup publishes or waits
    const bool prefixed = PRE || a.tile_prefix != nullptr;
    const uint64_t known_base = prefixed ? a.tile_prefix[tile] : 0;
    // the row list's side output never passes the tile's own slice of the list
    const bool listed = PRE && a.list_off != nullptr;
    const uint64_t known_next = listed ? a.tile_prefix[tile + 1] : 0;
    if (t == 0) s_expired = 0;
    u64x2 v[K][PAIRS];
    load_tile<K, PAIRS, THREADS>(a, tile_word0, t, v);
    uint64_t r[NW];
    eval_words<K, NW, FORM>(a.prog, v, r);
    tail_mask<NW, THREADS>(a, tile_word0, t, r);
    if (a.result_words) store_words<PAIRS, THREADS>(a.result_words, tile_word0, t, r);
    uint32_t packed = 0;
#pragma unroll
    for (int p = 0; p < PAIRS; ++p)
        packed |= (uint32_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1])) << (16 * p);
    const uint32_t incl = wave_incl_scan32(packed);
    if (lane == 63) s_wave_tot[wave] = incl;
    __syncthreads();
    uint32_t wave_pre[2] = {0, 0}, block_tot[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const uint32_t x = s_wave_tot[w];
        const uint32_t lo = x & 0xffffu, hi = x >> 16;
        if (w < wave) {
            wave_pre[0] += lo;
            wave_pre[1] += hi;
        }
        block_tot[0] += lo;
        block_tot[1] += hi;
    }
    const uint32_t excl = incl - packed;
    uint32_t pair_off[PAIRS];
    uint32_t tile_count = 0;
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) {
        pair_off[p] = tile_count + wave_pre[p] + ((excl >> (16 * p)) & 0xffffu);
        tile_count += block_tot[p];
    }
    if (t == 0 && !prefixed)
        __hip_atomic_store(a.flags + b, (a.epoch << kFlagCntBits) | (uint64_t)tile_count, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    const bool staged = tile_count <= (uint32_t)STAGE;
    if (!PRE && !staged && write_ids && !(DBG & 2)) {
#pragma unroll
        for (int j = 0; j < NW; ++j) s_words[(uint32_t)j * THREADS + t] = r[j];
    }
    if (!PRE && (DBG & 128) && staged && write_ids && tile_count) {
        // every lane takes ids lane, lane + 64, … of its wave's slice of each pair
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            const uint32_t inc = (incl >> (16 * p)) & 0xffffu;
            const uint32_t wtot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            stage_by_rank<THREADS>(r[2 * p], r[2 * p + 1], inc, wtot, pair_off[p] - (inc - (uint32_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1]))),
                                   (uint32_t)(p * 2 * THREADS + 2 * wave * 64) * 64u, s_words, s_list_scratch, s_stage,
                                   lane, wave);
        }
    } else if (!(DBG & 16) && staged && write_ids && tile_count) {
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            uint32_t off = pair_off[p];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uint64_t w = r[2 * p + e];
                const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                if (DBG & 64) {  // diagnostic: the loop without its LDS stores (positions summed)
                    uint32_t acc = 0;
                    while (w) {
                        acc += wrow + (uint32_t)__builtin_ctzll(w) + off++;
                        w &= w - 1;
                    }
                    if (acc == 0xffffffffu) s_stage[0] = acc;
                    continue;
                }
                while (w) {
                    s_stage[off++] = wrow + (uint32_t)__builtin_ctzll(w);
                    w &= w - 1;
                }
            }
        }
    }
    // look-back over every earlier workgroup's flag
    uint64_t pre = 0;
    for (uint32_t j = t; !prefixed && j < b && !(DBG & 8); j += THREADS) {
        uint64_t f = __hip_atomic_load(a.flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t spins = 0;
        bool gave_up = false;
        while (!(DBG & 1) && (f >> kFlagCntBits) != a.epoch) {
            // stop waiting once this thread's limit is reached or another thread of the workgroup
            // gave up: the workgroup recounts every flag below anyway, so no further flag is
            // worth a wait (without this each remaining unpublished flag cost another full limit)
            if (++spins >= spin_limit || *static_cast<volatile uint32_t*>(&s_expired)) {
                s_expired = 1;
                gave_up = true;
                break;
            }
            if (!(DBG & 4)) __builtin_amdgcn_s_sleep(2);
            f = __hip_atomic_load(a.flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (gave_up) break;  // `pre` is replaced by the recount
        pre += f & kCntMask;
    }
    pre = wave_sum_flags(pre);
    if (lane == 0) s_pre[wave] = pre;
    __syncthreads();  // also: the stage is complete
    uint64_t base = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) base += s_pre[w];
    if (prefixed) {
        base = known_base;
    } else if (!PRE && s_expired) {
        // some earlier tile was not published within the limit: every flag once more, the
        // missing tiles counted here (s_pre and s_wave_tot are free again; s_stage is not)
        base = lookback_recount<K, FORM, THREADS, PAIRS>(a, b, t, s_list_scratch, &s_list_n, s_pre);
    }
    const int64_t row0 = a.row_base + (int64_t)(tile_word0 * 64);
    if (t == 0) {
        if (dir) {
            dir[2 * tile] = tile_count ? base : 0;
            dir[2 * tile + 1] = tile_count;
        }
        if (b == gridDim.x - 1) *a.count = base + tile_count;
        if (listed) a.list_lo[tile] = block_tot[0];
    }
    if (!write_ids || !tile_count || (DBG & 2)) return;
    const uint32_t list_n = listed && known_next > base ? (uint32_t)min((uint64_t)tile_count, known_next - base) : 0;
    if (staged) {
        emit_ids<THREADS, SAUX>(a.rowids, a.capacity, s_stage, tile_count, base, row0, t);
        if (listed) emit_list<THREADS>(a.list_off, s_stage, list_n, base, t);
        return;
    }
    // dense tile: rounds of STAGE ids through the stage, its result words back from s_words (no
    // word is held in registers across the look-back walk and its expiry recount; reading and
    // evaluating the tile a second time instead cost 39.2 vs 30.7 µs for 673 dense tiles)
    if (!PRE) {
#pragma unroll
        for (int j = 0; j < NW; ++j) r[j] = s_words[(uint32_t)j * THREADS + t];
    }
    for (uint32_t r0 = 0; r0 < tile_count; r0 += (uint32_t)STAGE) {
        const uint32_t r1 = min(tile_count, r0 + (uint32_t)STAGE);
        if (r0) __syncthreads();  // the previous round's copy-out is done
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            uint32_t off = pair_off[p];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uint64_t w = r[2 * p + e];
                const uint32_t c = (uint32_t)__popcll(w);
                const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                if (off < r1 && off + c > r0) {
                    uint32_t k = off;
                    for (; k < r0; ++k) w &= w - 1;  // the word straddles the round's start
                    for (; w && k < r1; ++k) {
                        s_stage[k - r0] = wrow + (uint32_t)__builtin_ctzll(w);
                        w &= w - 1;
                    }
                }
                off += c;
            }
        }
        __syncthreads();
        emit_ids<THREADS, SAUX>(a.rowids, a.capacity, s_stage, r1 - r0, base + r0, row0, t);
        if (listed && r0 < list_n) emit_list<THREADS>(a.list_off, s_stage, min(r1, list_n) - r0, base + r0, t);
    }
}

// Row ids, tile directory and count of a bitvector from its row list (cubit_row_list.hpp), exactly as
// the prefixed decode above writes them: one workgroup per tile, ids row_base + tile * 131,072 + offset
// at rowids[prefix[tile] + i], those at or past `capacity` dropped, dir = {count ? prefix[tile] : 0,
// count} for every tile. Reads 2 bytes per id where the decode reads the bitvector; the stores follow
// emit_ids (16-byte sc1 buffer stores from the first 16-byte boundary on).
template <int THREADS, int SAUX>
__global__ __launch_bounds__(THREADS) void decode_row_list_kernel(RowListArgs a, uint64_t* __restrict__ dir) {
    typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int t = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const uint64_t base = a.prefix[tile];
    const uint64_t next = a.prefix[tile + 1];
    const uint32_t n = next > base ? (uint32_t)min(next - base, (uint64_t)kRowListTileRows) : 0;
    const uint32_t lo = a.lo_cnt[tile];
    if (t == 0) {
        if (dir) {
            dir[2 * tile] = n ? base : 0;
            dir[2 * tile + 1] = n;
        }
        if (tile == gridDim.x - 1) *a.count = base + n;
    }
    const uint64_t room = a.capacity > base ? a.capacity - base : 0;
    const uint32_t lim = (uint32_t)(room < (uint64_t)n ? room : (uint64_t)n);
    if (!a.rowids || lim == 0) return;
    const int64_t row0 = a.row_base + (int64_t)((uint64_t)tile * kRowListTileRows);
    int64_t* out = a.rowids + base;
    const uint16_t* src = a.off + base;
    const uint32_t head = min(lim, (uint32_t)(((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) >> 3));
    const uint64_t ob = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)out >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)out);
    const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane(lim) * 8u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)ob, (short)0, (int)nb, 0x00020000);
    auto id = [&](uint32_t i) { return row0 + (int64_t)row_list_decode(src[i], i, lo); };
    if (t < (int)head) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, id((uint32_t)t)), rs, t * 8, 0, SAUX);
    for (uint32_t i = head + 2 * t; i < lim; i += 2 * THREADS) {
        if (i + 1 < lim) {
            i64x2 val;
            val.x = id(i);
            val.y = id(i + 1);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), rs, (int)(i * 8u), 0, SAUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, id(i)), rs, (int)(i * 8u), 0, SAUX);
        }
    }
}

// A decoded value in the segments' own T when T is narrower than the column's values
// (BpGroup::tnorm, uniform per group): mod 2^bits, then sign- or zero-extended — T's
// wrap-around arithmetic (a UINT32 DELTA_FOR run that wraps, an INT16 CONSTANT_DELTA that
// steps by -3) carried out in the wider U
template <typename U>
__device__ __forceinline__ U bp_norm(U v, uint32_t tn) {
    if (!tn) return v;
    typedef typename std::conditional<sizeof(U) == 8, int64_t, int32_t>::type S;
    const uint32_t sh = (uint32_t)(sizeof(U) * 8) - (tn & 0x7fu);
    return (tn & 0x80u) ? (U)((S)(v << sh) >> sh) : (U)((U)(v << sh) >> sh);
}

// ------------------------------------------------------------------ K1+K3: fused filter + probe-sum

__device__ __forceinline__ void add128(uint64_t& lo, int64_t& hi, __int128 x) {
    const uint64_t xl = (uint64_t)x;
    const int64_t xh = (int64_t)(x >> 64);
    const uint64_t nl = lo + xl;
    hi += xh + (nl < lo ? 1 : 0);
    lo = nl;
}

// SELECT sum(a * b) WHERE <program>: evaluate a tile, decode its set bits into LDS (row
// offset, and — when b is decoded from its index — which of the M decode leaves miss the row,
// as M bits above the 17-bit tile-local offset, so b = v0 + Σ delta[m] over those bits is
// rebuilt in full int64 at the gather), then gather a (and b) for the
// staged rows with several loads in flight per thread, accumulating in 128 bits
// (DECIMAL(38,4) storage, Q6's sum(l_extendedprice * l_discount)). No row ids are written.
// Persistent like eval_decode_pairs; per-workgroup partials are summed by sum_partials_kernel;
// the qualifying-row count goes through the claim ticket.
template <int K, int M, int FORM>
__global__ __launch_bounds__(512, 4) void eval_sum_product(EvalArgs a, SumArgs s) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4, STAGE = 4096;
    constexpr int FB = 32;  // THREADS * 128 ≥ 65536
    constexpr uint64_t FMASK = 0xffffffffull;
    constexpr int FPW = 2;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr int NWAVES = THREADS / 64;
    __shared__ uint64_t s_wave_tot[NWAVES];
    // s_row: tile-local row offset (bits 0..16) | decode-leaf miss bits (bits kMissShift..)
    constexpr int kMissShift = 24;
    static_assert(TILE_WORDS * 64 <= (1u << kMissShift) && M <= 32 - kMissShift, "s_row packing");
    __shared__ uint32_t s_row[STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint64_t acc_lo = 0;
    int64_t acc_hi = 0;
    uint64_t total = 0;

    // b decoded from its range index: v0 plus the deltas of the leaves that miss the row (full
    // int64 — b may be any BIGINT / DECIMAL(18,x) storage value)
    auto decoded_b = [&](uint32_t miss) -> int64_t {
        uint64_t v = (uint64_t)s.v0;  // modular: v0 + Σ deltas lands on a stored value
#pragma unroll
        for (int m = 0; m < M; ++m)
            if ((miss >> m) & 1u) v += (uint64_t)s.delta[m];
        return (int64_t)v;
    };
    // a from its BITPACKING segments: the group records of the current tile (the groups from the
    // one holding the tile's first row on; 2,048 rows each inside a segment, so a tile of 131,072
    // rows spans 64 of them, a few more where segments end mid-vector) are staged in LDS at the
    // start of the tile, so a gathered value costs one load of its packed words, like the plain
    // column's one load of its value
    constexpr int NREC = 96;
    __shared__ int32_t s_gst[NREC];   // group's first row - the tile's first row
    __shared__ uint32_t s_gcnt[NREC];
    __shared__ uint64_t s_gbase[NREC], s_gaux[NREC], s_goff[NREC];
    __shared__ uint8_t s_gmode[NREC], s_gw[NREC], s_gtn[NREC];
    uint32_t tile_g0 = 0, tile_ng = 0;  // staged records: groups tile_g0 … tile_g0 + tile_ng - 1
    uint64_t tile_row0 = 0;
    auto stage_groups = [&](uint64_t row0) {
        tile_row0 = row0;
        const uint64_t n_vec = (a.n_rows + 2047) / 2048;
        const uint64_t v0 = row0 >> 11;
        tile_g0 = s.a_vgroup[v0 < n_vec ? v0 : n_vec - 1];
        tile_ng = (uint32_t)min<uint64_t>((uint64_t)NREC, s.a_n_groups - tile_g0);
        if (t < (int)tile_ng) {
            const BpGroup& gr = s.a_groups[tile_g0 + t];
            s_gst[t] = (int32_t)((int64_t)gr.row_start - (int64_t)row0);
            s_gcnt[t] = gr.count;
            s_gbase[t] = gr.base;
            s_gaux[t] = gr.aux;
            s_goff[t] = gr.words_off;
            s_gmode[t] = gr.mode;
            s_gtn[t] = gr.tnorm;
            s_gw[t] = (uint8_t)gr.width;
        }
    };
    // a[r], from the plain column or from its BITPACKING group (group record → packed bits)
    auto load_a = [&](uint64_t r) -> int64_t {
        if (!s.a_bytes) return __builtin_nontemporal_load(s.a + r);
        const int64_t rl = (int64_t)r - (int64_t)tile_row0;
        int32_t g = (int32_t)((rl - (int64_t)s_gst[0]) >> 11);  // exact inside one segment
        if (g >= (int32_t)tile_ng) g = (int32_t)tile_ng - 1;
        while (g > 0 && rl < (int64_t)s_gst[g]) --g;
        while (g + 1 < (int32_t)tile_ng && rl >= (int64_t)s_gst[g] + (int64_t)s_gcnt[g]) ++g;
        if (rl < (int64_t)s_gst[g] || rl >= (int64_t)s_gst[g] + (int64_t)s_gcnt[g])
            return __builtin_nontemporal_load(s.a_plain + r);  // past the staged groups
        const uint64_t i = (uint64_t)(rl - (int64_t)s_gst[g]);
        const uint32_t mode = s_gmode[g], tn = s_gtn[g];
        const uint64_t base = s_gbase[g];
        if (mode == 2) return (int64_t)bp_norm<uint64_t>(base, tn);
        if (mode == 3) return (int64_t)bp_norm<uint64_t>(base + s_gaux[g] * i, tn);
        if (mode != 5) return __builtin_nontemporal_load(s.a_plain + r);  // DELTA_FOR: needs its prefix
        const uint32_t w = s_gw[g];
        if (w == 0) return (int64_t)bp_norm<uint64_t>(base, tn);
        const uint32_t* words = reinterpret_cast<const uint32_t*>(s.a_bytes + s_goff[g]);
        const uint64_t bit = i * w;
        const uint32_t wi = (uint32_t)(bit >> 5), off = (uint32_t)(bit & 31);
        uint64_t x = ((uint64_t)__builtin_nontemporal_load(words + wi) |
                      (off + w > 32 ? (uint64_t)__builtin_nontemporal_load(words + wi + 1) << 32 : 0ull)) >> off;
        if (off + w > 64) x |= (uint64_t)__builtin_nontemporal_load(words + wi + 2) << (64 - off);
        if (w < 64) x &= (1ull << w) - 1;
        return (int64_t)bp_norm<uint64_t>(x + base, tn);
    };
    auto accumulate = [&](int64_t row, int64_t bval_decoded) {
        const uint64_t r = (uint64_t)(row - a.row_base);
        if (s.a_valid && !((s.a_valid[r >> 6] >> (r & 63)) & 1ull)) return;
        int64_t bv = bval_decoded;
        if (M == 0 && s.b) {  // gathered b (b = nullptr with M = 0: the filter pins b to v0 alone)
            if (s.b_valid && !((s.b_valid[r >> 6] >> (r & 63)) & 1ull)) return;
            bv = s.b[r];
        }
        add128(acc_lo, acc_hi, (__int128)load_a(r) * (__int128)bv);
    };

    u64x2 v[K][PAIRS];
    u64x2 dv[M > 0 ? M : 1][PAIRS];
    // i indexes the launch's tiles (every tile, or the zonemap skip's live-tile list)
    const uint32_t n_idx = a.num_tiles;
    uint32_t i = blockIdx.x;
    uint32_t tile = i < n_idx ? tile_at(a, i) : 0;
    auto load_decode = [&](uint64_t tile_word0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const u64x2* base = reinterpret_cast<const u64x2*>(s.dleaf[m] + tile_word0);
#pragma unroll
            for (int p = 0; p < PAIRS; ++p) dv[m][p] = __builtin_nontemporal_load(base + p * THREADS + t);
        }
    };
    if (i < n_idx) {
        load_tile<K, PAIRS, THREADS>(a, (uint64_t)tile * TILE_WORDS, t, v);
        load_decode((uint64_t)tile * TILE_WORDS);
    }
    while (i < n_idx) {
        const uint64_t tile_word0 = (uint64_t)tile * TILE_WORDS;
        const bool has_next = i + gridDim.x < n_idx;
        const uint32_t next = has_next ? tile_at(a, i + gridDim.x) : 0;
        // (read at the gathers, behind the "stage complete" barrier; the previous tile's gathers
        // finished behind the barrier that ends its iteration)
        if (s.a_bytes) stage_groups(tile_word0 * 64);
        uint64_t r[NW];
        eval_words<K, NW, FORM>(a.prog, v, r);
        tail_mask<NW, THREADS>(a, tile_word0, t, r);
        if (has_next) load_tile<K, PAIRS, THREADS>(a, (uint64_t)next * TILE_WORDS, t, v);
        uint64_t packed = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p)
            packed |= (uint64_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1])) << (FB * (p % FPW));
        const uint64_t incl = wave_incl_scan(packed, lane);
        if (lane == 63) s_wave_tot[wave] = incl;
        __syncthreads();
        uint64_t wp = 0, bt = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
            const uint64_t x = s_wave_tot[w];
            if (w < wave) wp += x;
            bt += x;
        }
        uint64_t pair_off[PAIRS];
        uint64_t tile_count = 0;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            pair_off[p] = tile_count + (((wp + incl - packed) >> (FB * (p % FPW))) & FMASK);
            tile_count += (bt >> (FB * (p % FPW))) & FMASK;
        }
        total += tile_count;
        const int64_t row0 = a.row_base + (int64_t)(tile_word0 * 64);
        const bool staged = tile_count <= (uint64_t)STAGE;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            uint32_t off = (uint32_t)pair_off[p];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uint64_t w = r[2 * p + e];
                const uint32_t wrow = (uint32_t)((p * 2 * THREADS + 2 * t + e) * 64);
                while (w) {
                    const uint32_t b = (uint32_t)__builtin_ctzll(w);
                    uint32_t miss = 0;  // bit m: the row is not in decode leaf m (b >= v_{m+1})
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const u64x2 d = dv[m][p];
                        const uint64_t dw = e ? d.y : d.x;
                        miss |= (uint32_t)(((dw >> b) & 1ull) ^ 1ull) << m;
                    }
                    if (staged) {
                        s_row[off] = (wrow + b) | (miss << kMissShift);
                    } else {
                        accumulate(row0 + (int64_t)(wrow + b), decoded_b(miss));  // dense tile: direct
                    }
                    ++off;
                    w &= w - 1;
                }
            }
        }
        if (M > 0 && has_next) load_decode((uint64_t)next * TILE_WORDS);
        __syncthreads();  // stage complete
        if (staged) {
            // 4 gathers in flight per thread per round
            for (uint32_t i = t; i < (uint32_t)tile_count; i += 4 * THREADS) {
                int64_t av[4], bvv[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t k = i + u * THREADS;
                    ok[u] = k < (uint32_t)tile_count;
                    const uint32_t sr = ok[u] ? s_row[k] : 0u;
                    const uint64_t rr = (uint64_t)(row0 - a.row_base) + (sr & ((1u << kMissShift) - 1));
                    // line-granular gathers, no reuse: nontemporal like the leaf loads
                    av[u] = ok[u] ? load_a(rr) : 0;
                    bvv[u] = M > 0 ? (ok[u] ? decoded_b(sr >> kMissShift) : 0) : (ok[u] ? (s.b ? __builtin_nontemporal_load(s.b + rr) : s.v0) : 0);
                    if (ok[u] && s.a_valid && !((s.a_valid[rr >> 6] >> (rr & 63)) & 1ull)) ok[u] = false;
                    if (M == 0 && ok[u] && s.b_valid && !((s.b_valid[rr >> 6] >> (rr & 63)) & 1ull)) ok[u] = false;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (ok[u]) add128(acc_lo, acc_hi, (__int128)av[u] * (__int128)bvv[u]);
            }
        }
        __syncthreads();  // stage / wave totals free
        i += gridDim.x;
        tile = next;
    }
    // block reduce of the 128-bit partial sums
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t olo = __shfl_xor(acc_lo, d, 64);
        const int64_t ohi = __shfl_xor(acc_hi, d, 64);
        const uint64_t nlo = acc_lo + olo;
        acc_hi = acc_hi + ohi + (nlo < acc_lo ? 1 : 0);
        acc_lo = nlo;
    }
    __shared__ uint64_t s_lo[NWAVES];
    __shared__ int64_t s_hi[NWAVES];
    if (lane == 0) {
        s_lo[wave] = acc_lo;
        s_hi[wave] = acc_hi;
    }
    __syncthreads();
    if (t == 0) {
        uint64_t lo = 0;
        int64_t hi = 0;
        for (int w = 0; w < NWAVES; ++w) add128(lo, hi, ((__int128)s_hi[w] << 64) | (unsigned __int128)s_lo[w]);
        s.partials[2 * blockIdx.x] = (int64_t)lo;
        s.partials[2 * blockIdx.x + 1] = hi;
        finish_ticket(a.ticket, a.count, total);
    }
}

__global__ __launch_bounds__(256) void sum_product_arrays_kernel(const int64_t* __restrict__ x,
                                                                 const int64_t* __restrict__ y,
                                                                 const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                                 int64_t* __restrict__ partials) {
    __shared__ __int128 s_part[4];
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t lo = 0;
    int64_t hi = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        add128(lo, hi, (__int128)x[i] * (__int128)y[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t olo = __shfl_xor(lo, d, 64);
        const int64_t ohi = __shfl_xor(hi, d, 64);
        const uint64_t nlo = lo + olo;
        hi = hi + ohi + (nlo < lo ? 1 : 0);
        lo = nlo;
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ((__int128)hi << 64) | lo;
    __syncthreads();
    if (threadIdx.x == 0) {
        const __int128 tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        partials[2 * blockIdx.x] = (int64_t)(uint64_t)tot;
        partials[2 * blockIdx.x + 1] = (int64_t)(tot >> 64);
    }
}

// ------------------------------------------------------------------ row-order pass

// One launch: workgroup w moves the runs of tiles [tpw·w, tpw·w + tpw) to their row-order
// position (tpw = tiles per workgroup, 1..8: at least ~1,024 workgroups when there are tiles
// for them).
// The position is the sum of the run lengths of every earlier tile, which the workgroup
// reads from the directory itself (16 B per tile, L2-resident: ≤ 37 KB at SF100, read with
// every thread's loads in flight), so no separate scan launch and no single-workgroup scan
// precede the copy. The copy keeps four 8-byte loads in flight per thread.
// MODE (scripts/balbench.hip compares them): 0 plain loads and stores, 1 nontemporal loads and
// sc1 (write-through) buffer stores, 2 nontemporal loads and plain stores.
template <int MODE = 0>
__global__ __launch_bounds__(256) void order_runs_kernel(const uint64_t* __restrict__ dir, uint32_t n_tiles,
                                                         uint32_t tpw, const int64_t* __restrict__ src,
                                                         uint64_t capacity, int64_t* __restrict__ dst) {
    constexpr int THREADS = 256;
    __shared__ uint64_t s_part[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t t0 = blockIdx.x * tpw;
    uint64_t acc = 0;
#pragma unroll 4
    for (uint32_t i = t; i < t0; i += THREADS) acc += dir[2 * i + 1];
    acc = wave_sum(acc);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    uint64_t d = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) d += s_part[w];
    const uint32_t t1 = t0 + tpw < n_tiles ? t0 + tpw : n_tiles;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const uint64_t so = dir[2 * tile], n = dir[2 * tile + 1];
        // MODE 1: this tile's destination run through a descriptor from SGPRs (≤ 131,072 ids)
        const uint64_t lim = d < capacity ? min(n, capacity - d) : 0;
        const uintptr_t dp = reinterpret_cast<uintptr_t>(dst + d);
        const uint64_t db = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(dp >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)dp);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)db, (short)0, (int)((uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)lim) * 8u), 0x00020000);
        for (uint64_t i = t; i < n; i += 4 * THREADS) {
            int64_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t j = i + (uint64_t)u * THREADS;
                v[u] = (j < n && so + j < capacity) ? (MODE ? __builtin_nontemporal_load(src + so + j) : src[so + j]) : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t j = i + (uint64_t)u * THREADS;
                if (j < n && so + j < capacity && d + j < capacity) {
                    if (MODE == 1)
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[u]), rs, (int)(j * 8u), 0, 16);
                    else
                        dst[d + j] = v[u];
                }
            }
        }
        d += n;
    }
}

// ------------------------------------------------------------------ K0: compare → bitvector

// K0: predicate → bitvector over a raw column, for M keys in one read of the column (M = 1:
// a constant with no index key at query time; M = kMultiKeys: index build — range L(k),
// equality E(k) or bins [k, k2)). A wave handles 64 consecutive words; 16 rows per lane are
// loaded ahead, then every key's predicate is one ballot per word, kept by lane j for word j,
// and each key's 64 words leave as one 512-byte store. Bytes per pass: n·w_c read + M·n/8
// written, instead of M·(n·w_c + n/8). Comparison semantics are TemplatedFilterSelection's
// (column_segment.cpp:261-349): NULL rows never qualify.
// CMP 0..5 = EQ NE LT LE GT GE (CUBIT_CMP_*); 6 = c <= v < c2 (bin of a CUBIT_INDEX_BINS index)
template <int CMP, typename CT>
__device__ __forceinline__ bool cmp_v(CT v, CT c, CT c2) {
    if (CMP == 0) return v == c;
    if (CMP == 1) return v != c;
    if (CMP == 2) return v < c;
    if (CMP == 3) return v <= c;
    if (CMP == 4) return v > c;
    if (CMP == 5) return v >= c;
    return v >= c && v < c2;
}

template <typename T, typename CT, int CMP, int M, int FK = 0>
__global__ __launch_bounds__(256) void compare_bitvectors_kernel(const T* __restrict__ col,
                                                                 const uint64_t* __restrict__ validity,
                                                                 uint64_t n_rows, uint64_t n_words_padded,
                                                                 MultiKeyArgs a) {
    // CT: compare type (int32 when the column and every key fit 32 bits: one VALU compare)
    static_assert(M >= 1 && M <= kMultiKeys, "keys per pass");
    constexpr int JB = 16;
    const int lane = threadIdx.x & 63;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t w0 = wave_id * 64; w0 < n_words_padded; w0 += n_waves * 64) {
        uint32_t lo[M], hi[M];  // lane j keeps word j of every key
#pragma unroll
        for (int k = 0; k < M; ++k) lo[k] = hi[k] = 0;
        for (int jb = 0; jb < 64; jb += JB) {
            CT v[JB];
            bool ok[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const uint64_t row = (w0 + jb + j) * 64 + lane;
                ok[j] = row < n_rows;
                v[j] = ok[j] ? (CT)key_of<FK>(__builtin_nontemporal_load(col + row)) : (CT)0;  // streamed once: nt
                if (validity) ok[j] = ok[j] && ((validity[w0 + jb + j] >> lane) & 1ull);
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                // every key's ballot for word jb + j (uniform, SGPRs), then lane jb + j alone
                // moves them into its registers under the exec mask: per (word, key) one
                // compare and two moves
                // (keys past a.m repeat the last key: the host pads them, their words are not stored)
                const uint64_t okm = __ballot(ok[j]);
                uint64_t b[M];
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const CT c = (CT)a.c[k], c2 = (CT)a.c2[k];
                    b[k] = __ballot(cmp_v<CMP, CT>(v[j], c, c2)) & okm;
                }
                if (lane == jb + j) {
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        lo[k] = (uint32_t)b[k];
                        hi[k] = (uint32_t)(b[k] >> 32);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < M; ++k)
            if (k < (int)a.m) a.out[k][w0 + lane] = ((uint64_t)hi[k] << 32) | lo[k];
    }
}

template <typename T, typename CT, int M, int FK = 0>
hipError_t launch_compare_multi_t(const T* col, const uint64_t* validity, uint64_t n_rows, int cmp,
                                  const MultiKeyArgs& a, hipStream_t stream) {
    const uint64_t nw = padded_words(n_rows);
    const uint64_t waves = nw / 64;
    const uint64_t blocks = std::min<uint64_t>((waves + 3) / 4, 8192);
    const dim3 grid((unsigned)std::max<uint64_t>(blocks, 1)), block(256);
#define CUBIT_CMP_CASE(C)                                                                                       \
    case C:                                                                                                     \
        hipLaunchKernelGGL((compare_bitvectors_kernel<T, CT, C, M, FK>), grid, block, 0, stream, col, validity, n_rows, nw, a); \
        break;
    if constexpr (M == 1) {  // a query-time constant: every comparison
        switch (cmp) {
            CUBIT_CMP_CASE(0)
            CUBIT_CMP_CASE(1)
            CUBIT_CMP_CASE(2)
            CUBIT_CMP_CASE(3)
            CUBIT_CMP_CASE(4)
            CUBIT_CMP_CASE(5)
            CUBIT_CMP_CASE(6)
        default: return hipErrorInvalidValue;
        }
    } else {  // index build: L(k) = v < k, E(k) = v == k, bins k <= v < k2
        switch (cmp) {
            CUBIT_CMP_CASE(0)
            CUBIT_CMP_CASE(2)
            CUBIT_CMP_CASE(6)
        default: return hipErrorInvalidValue;
        }
    }
#undef CUBIT_CMP_CASE
    return hipGetLastError();
}

// Candidate check (binned range index): a query-time constant c that is not an index key
// falls in one bin [k_lo, k_hi) of the range index. Its rows are cand = L(k_hi) \ L(k_lo)
// (L(k) = valid rows with v < k; no k_lo → ∅, no k_hi → every valid row), and only they
// need the raw value:
//   v <  c  =  L(k_lo) ∪ {r ∈ cand : v[r] < c}
//   v == c  =           {r ∈ cand : v[r] == c}
// Per word: two bitvector words read, the column read at the candidate rows only, one word
// written — instead of K0's read of the whole column. Each thread owns two consecutive
// words (16-byte loads and stores), so a wave's bitvector traffic is 1 KiB per instruction;
// the candidate values are gathered per set bit (line-granular reads of the column where a
// line holds a candidate). Comparison semantics are TemplatedFilterSelection's
// (column_segment.cpp:261-349); NULL rows are never candidates.
template <typename T, typename CT, int CMP, int FK = 0>
__global__ __launch_bounds__(256) void candidate_check_kernel(const T* __restrict__ col,
                                                              const uint64_t* __restrict__ validity,
                                                              const uint64_t* __restrict__ lo_bv,
                                                              const uint64_t* __restrict__ hi_bv, uint64_t n_rows,
                                                              uint64_t n_words_padded, CT c,
                                                              uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_words = (n_rows + 63) / 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * p < n_words_padded; p += stride) {
        const uint64_t w0 = 2 * p;
        u64x2 lo = {0ull, 0ull}, hi;
        if (lo_bv) lo = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(lo_bv) + p);
        if (hi_bv) {
            hi = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(hi_bv) + p);
        } else {
            // every valid row of the partition: full words, the tail word's rows, nothing past it
            hi.x = w0 < n_words ? ~0ull : 0ull;
            hi.y = w0 + 1 < n_words ? ~0ull : 0ull;
            if (w0 + 1 == n_words && (n_rows & 63)) hi.x = (1ull << (n_rows & 63)) - 1;
            if (w0 + 2 == n_words && (n_rows & 63)) hi.y = (1ull << (n_rows & 63)) - 1;
            if (validity) {
                const u64x2 vw = reinterpret_cast<const u64x2*>(validity)[p];
                hi.x &= vw.x;
                hi.y &= vw.y;
            }
        }
        u64x2 res;
        res.x = CMP == 2 ? lo.x : 0ull;
        res.y = CMP == 2 ? lo.y : 0ull;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            uint64_t cand = e ? (hi.y & ~lo.y) : (hi.x & ~lo.x);
            uint64_t hit = 0;
            const T* base = col + (w0 + e) * 64;
            while (cand) {
                const int b = __builtin_ctzll(cand);
                const CT v = (CT)key_of<FK>(base[b]);
                if (CMP == 2 ? v < c : v == c) hit |= 1ull << b;
                cand &= cand - 1;
            }
            if (e) res.y |= hit;
            else res.x |= hit;
        }
        reinterpret_cast<u64x2*>(out)[p] = res;
    }
}

// Selection narrowing: RowGroup::TemplatedScan evaluates each filter column after the first
// only at the rows the earlier ones kept (ColumnData::Select over the shared SelectionVector,
// row_group.cpp:537-550). For a constant comparison on a column without a usable index inside a
// conjunction: out = mask ∩ valid ∩ {r : lo <= v[r] <= hi, complemented when neg}, the column
// read only at the mask's rows (line-granular gathers, as the candidate check). Each thread owns
// two consecutive words (16-byte loads and stores).
template <typename T, int FK = 0>
__global__ __launch_bounds__(256) void masked_compare_kernel(const T* __restrict__ col,
                                                             const uint64_t* __restrict__ validity,
                                                             const uint64_t* __restrict__ mask, uint64_t n_words_padded,
                                                             T lo, T hi, int neg, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * p < n_words_padded; p += stride) {
        const uint64_t w0 = 2 * p;
        u64x2 m = reinterpret_cast<const u64x2*>(mask)[p];
        if (validity) {
            const u64x2 vw = reinterpret_cast<const u64x2*>(validity)[p];
            m.x &= vw.x;
            m.y &= vw.y;
        }
        u64x2 res = {0ull, 0ull};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            uint64_t cand = e ? m.y : m.x;
            uint64_t hit = 0;
            const T* base = col + (w0 + e) * 64;
            while (cand) {
                const int b = __builtin_ctzll(cand);
                const T v = key_of<FK>(base[b]);
                if (((v >= lo) & (v <= hi)) != (neg != 0)) hit |= 1ull << b;
                cand &= cand - 1;
            }
            if (e) res.y = hit;
            else res.x = hit;
        }
        reinterpret_cast<u64x2*>(out)[p] = res;
    }
}

template <typename T, typename CT, int FK = 0>
hipError_t launch_candidate_t(const T* col, const uint64_t* validity, const uint64_t* lo_bv, const uint64_t* hi_bv,
                              uint64_t n_rows, int cmp, CT c, uint64_t* out, hipStream_t stream) {
    const uint64_t nw = padded_words(n_rows);
    const dim3 grid((unsigned)std::min<uint64_t>((nw / 2 + 255) / 256, 8192)), block(256);
    if (cmp == 2)
        hipLaunchKernelGGL((candidate_check_kernel<T, CT, 2, FK>), grid, block, 0, stream, col, validity, lo_bv, hi_bv,
                           n_rows, nw, c, out);
    else if (cmp == 0)
        hipLaunchKernelGGL((candidate_check_kernel<T, CT, 0, FK>), grid, block, 0, stream, col, validity, lo_bv, hi_bv,
                           n_rows, nw, c, out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// every key (and bin end) an int32: an int32 column compares in 32 bits
bool keys_fit32(const MultiKeyArgs& a, int cmp) {
    for (uint32_t k = 0; k < a.m; ++k)
        if (a.c[k] < INT32_MIN || a.c[k] > INT32_MAX ||
            (cmp == kCmpBetween && (a.c2[k] < INT32_MIN || a.c2[k] > INT32_MAX)))
            return false;
    return true;
}

template <int M>
hipError_t launch_compare_m(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int cmp,
                            const MultiKeyArgs& a, hipStream_t stream) {
    // FLOAT / DOUBLE: the patterns' keys (FLOAT keys are int32, so are the planner's keys for it)
    if (type == kTypeFloat)
        return keys_fit32(a, cmp) ? launch_compare_multi_t<int32_t, int32_t, M, 1>(static_cast<const int32_t*>(col),
                                                                                   validity, n_rows, cmp, a, stream)
                                  : launch_compare_multi_t<int32_t, int64_t, M, 1>(static_cast<const int32_t*>(col),
                                                                                   validity, n_rows, cmp, a, stream);
    if (type == kTypeDouble)
        return launch_compare_multi_t<int64_t, int64_t, M, 2>(static_cast<const int64_t*>(col), validity, n_rows, cmp, a,
                                                              stream);
    if (type == kTypeUInt64) {
        // the keys v ^ 2^63 order as the raw values do unsigned: un-key the constants once and
        // compare the 64 bits unsigned (no per-value XOR in the loop)
        MultiKeyArgs u = a;
        for (int k = 0; k < kMultiKeys; ++k) {
            u.c[k] = (int64_t)((uint64_t)u.c[k] ^ 0x8000000000000000ull);
            u.c2[k] = (int64_t)((uint64_t)u.c2[k] ^ 0x8000000000000000ull);
        }
        return launch_compare_multi_t<uint64_t, uint64_t, M>(static_cast<const uint64_t*>(col), validity, n_rows, cmp, u,
                                                             stream);
    }
    if (type_is32(type) && keys_fit32(a, cmp))
        return launch_compare_multi_t<int32_t, int32_t, M>(static_cast<const int32_t*>(col), validity, n_rows, cmp, a,
                                                           stream);
    if (type_is32(type))
        return launch_compare_multi_t<int32_t, int64_t, M>(static_cast<const int32_t*>(col), validity, n_rows, cmp, a,
                                                           stream);
    return launch_compare_multi_t<int64_t, int64_t, M>(static_cast<const int64_t*>(col), validity, n_rows, cmp, a,
                                                       stream);
}

// ------------------------------------------------------------------ bit-sliced index
//
// A bit-sliced index (O'Neil & Quass 1997; Rinfret, O'Neil & O'Neil 2001) holds one bitvector per
// bit of u = (uint64)key - (uint64)base: bit r of slice s = valid(r) && ((u_r >> s) & 1). Any
// comparison with a constant is then a ripple of AND / OR / ANDNOT over 64-row words from the top
// slice down: no unpack, no per-row compare, b/8 bytes read per row for a b-bit span.

// Build: bitslice_build_kernel follows compare_bitvectors_kernel — a wave takes 64 words, 16 words'
// values are loaded ahead, each (word, slice) is one ballot kept by lane j for word j, and every
// slice's 64 words leave as one 512-byte store. A pass makes at most kMultiKeys slices (the bits
// s0 … s0 + m - 1 of u, taken once per value as a 32-bit window), so b slices cost ⌈b/16⌉ reads of
// the column: ⌈b/16⌉·n·w_c bytes read + b·n/8 written.
struct SliceBuildArgs {
    uint64_t* out[kMultiKeys];
    int64_t base;
    uint32_t s0, m;
};

template <typename T, int M, int FK = 0>
__global__ __launch_bounds__(256) void bitslice_build_kernel(const T* __restrict__ col,
                                                             const uint64_t* __restrict__ validity, uint64_t n_rows,
                                                             uint64_t n_words_padded, SliceBuildArgs a) {
    static_assert(M >= 1 && M <= kMultiKeys, "slices per pass");
    constexpr int JB = 16;
    const int lane = threadIdx.x & 63;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t w0 = wave_id * 64; w0 < n_words_padded; w0 += n_waves * 64) {
        uint32_t lo[M], hi[M];  // lane j keeps word j of every slice
#pragma unroll
        for (int k = 0; k < M; ++k) lo[k] = hi[k] = 0;
        for (int jb = 0; jb < 64; jb += JB) {
            uint32_t v[JB];  // bits s0 … s0 + 31 of u
            bool ok[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const uint64_t row = (w0 + jb + j) * 64 + lane;
                ok[j] = row < n_rows;
                const int64_t key = ok[j] ? (int64_t)key_of<FK>(__builtin_nontemporal_load(col + row)) : a.base;
                v[j] = (uint32_t)(((uint64_t)key - (uint64_t)a.base) >> a.s0);
                if (validity) ok[j] = ok[j] && ((validity[w0 + jb + j] >> lane) & 1ull);
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const uint64_t okm = __ballot(ok[j]);
                uint64_t b[M];
#pragma unroll
                for (int k = 0; k < M; ++k) b[k] = __ballot((v[j] >> k) & 1u) & okm;
                if (lane == jb + j) {
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        lo[k] = (uint32_t)b[k];
                        hi[k] = (uint32_t)(b[k] >> 32);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < M; ++k)
            if (k < (int)a.m) a.out[k][w0 + lane] = ((uint64_t)hi[k] << 32) | lo[k];
    }
}

// After a merge: the words holding a merged row, sliced again. A wave walks 64 records (rows
// ascend); the first record of each 64-row word makes the wave load that word's 64 values and
// ballot every slice, lane 0 storing the word. The build kernel restricted to those words.
template <typename T, int FK = 0>
__global__ __launch_bounds__(256) void bitslice_reslice_kernel(const int64_t* __restrict__ rows, uint64_t m,
                                                               const T* __restrict__ col,
                                                               const uint64_t* __restrict__ validity, uint64_t n_rows,
                                                               int64_t base, uint32_t n_slices, SliceSet sl) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i0 = wave_id * 64; i0 < m; i0 += n_waves * 64) {
        const uint64_t i1 = i0 + 64 < m ? i0 + 64 : m;
        for (uint64_t i = i0; i < i1; ++i) {
            const uint64_t r = (uint64_t)rows[i];
            if (r >= n_rows) continue;
            const uint64_t word = r >> 6;
            if (i > 0 && ((uint64_t)rows[i - 1] >> 6) == word) continue;  // this word is done
            const uint64_t row = word * 64 + lane;
            bool ok = row < n_rows;
            const int64_t key = ok ? (int64_t)key_of<FK>(col[row]) : base;
            const uint64_t u = (uint64_t)key - (uint64_t)base;
            if (validity) ok = ok && ((validity[word] >> lane) & 1ull);
            const uint64_t okm = __ballot(ok);
            for (uint32_t s = 0; s < n_slices; ++s) {
                const uint64_t bits = __ballot((u >> s) & 1ull) & okm;
                if (lane == 0) sl.s[s][word] = bits;
            }
        }
    }
}

// Compare: out = valid ∧ (lo <= u <= hi), u read from the slices; `negate` complements under
// valid (!=). One pass from slice b - 1 down to 0 carrying, per word, (gt, eq) against lo and
// (lt, eq) against hi: at a slice w, a 1 bit of lo keeps eq only where w is 1, a 0 bit moves
// eq ∧ w to gt; hi mirrored. lo and hi are kernel arguments, so the branch on each constant bit
// is scalar. Shaped like candidate_check_kernel: each thread owns two consecutive words (16-byte
// loads and one 16-byte store), and a chunk of up to 8 slices is loaded (streamed once:
// non-temporal) before the ripple consumes it. LO / HI: the sides the bound needs (lo > 0,
// hi < 2^b - 1). Traffic: (b + 1 [+ 1 with validity])·n/8 bytes.
template <bool LO, bool HI, int CNT>
__device__ __forceinline__ void ripple_chunk(const SliceSet& sl, int top, uint64_t p, uint64_t lo, uint64_t hi,
                                             u64x2& gt, u64x2& eql, u64x2& lt, u64x2& eqh) {
    u64x2 w[CNT];
#pragma unroll
    for (int j = 0; j < CNT; ++j) w[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(sl.s[top - j]) + p);
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
        const int s = top - j;
        if (LO) {
            if ((lo >> s) & 1ull) {
                eql &= w[j];
            } else {
                gt |= eql & w[j];
                eql &= ~w[j];
            }
        }
        if (HI) {
            if ((hi >> s) & 1ull) {
                lt |= eqh & ~w[j];
                eqh &= w[j];
            } else {
                eqh &= ~w[j];
            }
        }
    }
}

template <bool LO, bool HI>
__global__ __launch_bounds__(256) void bitslice_compare_kernel(SliceSet sl, uint32_t n_slices,
                                                               const uint64_t* __restrict__ validity, uint64_t n_rows,
                                                               uint64_t n_words_padded, uint64_t lo, uint64_t hi,
                                                               int negate, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_words = (n_rows + 63) / 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * p < n_words_padded; p += stride) {
        const uint64_t w0 = 2 * p;
        // the valid rows: full words, the tail word's rows, nothing past it (validity is read only
        // below n_words: a caller's mask need not be padded)
        u64x2 valid;
        valid.x = w0 < n_words ? ~0ull : 0ull;
        valid.y = w0 + 1 < n_words ? ~0ull : 0ull;
        if (w0 + 1 == n_words && (n_rows & 63)) valid.x = (1ull << (n_rows & 63)) - 1;
        if (w0 + 2 == n_words && (n_rows & 63)) valid.y = (1ull << (n_rows & 63)) - 1;
        if (validity) {
            if (w0 + 1 < n_words) valid &= reinterpret_cast<const u64x2*>(validity)[p];
            else if (w0 < n_words) valid.x &= validity[w0];
        }
        u64x2 res = valid;
        if ((LO || HI) && w0 < n_words) {
            u64x2 gt = {0ull, 0ull}, lt = {0ull, 0ull}, eql = {~0ull, ~0ull}, eqh = {~0ull, ~0ull};
            int top = (int)n_slices - 1;
            switch (n_slices & 7u) {  // the top slices that fill no chunk of 8, then whole chunks
            case 1: ripple_chunk<LO, HI, 1>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 2: ripple_chunk<LO, HI, 2>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 3: ripple_chunk<LO, HI, 3>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 4: ripple_chunk<LO, HI, 4>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 5: ripple_chunk<LO, HI, 5>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 6: ripple_chunk<LO, HI, 6>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            case 7: ripple_chunk<LO, HI, 7>(sl, top, p, lo, hi, gt, eql, lt, eqh); break;
            default: break;
            }
            top -= (int)(n_slices & 7u);
            for (; top >= 7; top -= 8) ripple_chunk<LO, HI, 8>(sl, top, p, lo, hi, gt, eql, lt, eqh);
            if (LO) res &= gt | eql;
            if (HI) res &= lt | eqh;
        }
        if (negate) res = valid & ~res;
        reinterpret_cast<u64x2*>(out)[p] = res;
    }
}

// ---- what the kernels that answer a query from the slices share (eval_slice_aggregate,
// eval_slice_select, eval_slice_aggregate_grouped and the reductions beside them)

// The tile prologue: r = the program over the thread's NW words of the tile (K = 0: every row), cut at
// n_rows. (The decode and sum kernels pipeline load_tile across tiles and keep their own.)
template <int K, int FORM, int NW, int THREADS>
__device__ __forceinline__ void eval_tile(const EvalArgs& a, uint64_t tile_word0, int t, uint64_t (&r)[NW]) {
    if constexpr (K > 0) {
        u64x2 v[K][NW / 2];
        load_tile<K, NW / 2, THREADS>(a, tile_word0, t, v);
        eval_words<K, NW, FORM>(a.prog, v, r);
    } else {
#pragma unroll
        for (int j = 0; j < NW; ++j) r[j] = ~0ull;
    }
    tail_mask<NW, THREADS>(a, tile_word0, t, r);
}

// Pair p of the thread's words of a bitvector that is not a program leaf (a validity, a group leaf),
// complemented when neg. whole (uniform): the tile lies below the last word; the tile that holds the
// last word reads nothing at or past n_words (a caller's bitvector need not be padded).
template <int THREADS>
__device__ __forceinline__ u64x2 load_pair(const uint64_t* bv, bool neg, bool whole, uint64_t tile_word0, int p, int t,
                                           uint64_t n_words) {
    u64x2 e;
    if (whole) {
        e = reinterpret_cast<const u64x2*>(bv + tile_word0)[p * THREADS + t];
    } else {
        const uint64_t gw = word_index<THREADS>(tile_word0, 2 * p, t);
        e.x = gw < n_words ? bv[gw] : 0ull;
        e.y = gw + 1 < n_words ? bv[gw + 1] : 0ull;
    }
    return neg ? ~e : e;
}

// The partial aggregate a thread, a wave, a workgroup and the finishing wave carry: the 128-bit sum,
// the least and greatest offset, the valid rows and (ROWS) the rows. Exact integer adds and unsigned
// min / max, so any order of merges gives the same. In memory it is kSlots words in that order (the
// ungrouped workspace keeps the first kAggPartial and counts the rows through the ticket).
template <bool ROWS>
struct AggPartial {
    static constexpr int kSlots = ROWS ? 6 : 5;
    U128 sum{0, 0};
    uint64_t mn = ~0ull, mx = 0, valid = 0, rows = 0;
    __device__ __forceinline__ void merge(const AggPartial& o) {
        sum = u128_add(sum, o.sum);
        mn = o.mn < mn ? o.mn : mn;
        mx = o.mx > mx ? o.mx : mx;
        valid += o.valid;
        if (ROWS) rows += o.rows;
    }
    // butterfly: every lane ends with the wave's partial
    __device__ __forceinline__ void wave_reduce() {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            AggPartial o;
            o.sum.lo = __shfl_xor(sum.lo, d, 64);
            o.sum.hi = __shfl_xor(sum.hi, d, 64);
            o.mn = __shfl_xor(mn, d, 64);
            o.mx = __shfl_xor(mx, d, 64);
            o.valid = __shfl_xor(valid, d, 64);
            if (ROWS) o.rows = __shfl_xor(rows, d, 64);
            merge(o);
        }
    }
    template <typename W>
    __device__ __forceinline__ void store(W* s, int slots = kSlots) const {
        s[0] = (W)sum.lo;
        s[1] = (W)sum.hi;
        s[2] = (W)mn;
        s[3] = (W)mx;
        s[4] = (W)valid;
        if (ROWS && slots > 5) s[5] = (W)rows;
    }
    template <typename W>
    __device__ __forceinline__ static AggPartial load(const W* s) {
        AggPartial r;
        r.sum = U128{(uint64_t)s[0], (uint64_t)s[1]};
        r.mn = (uint64_t)s[2];
        r.mx = (uint64_t)s[3];
        r.valid = (uint64_t)s[4];
        if (ROWS) r.rows = (uint64_t)s[5];
        return r;
    }
    // the per-wave LDS fold: after each wave's lane 0 stored its partial at s + wave·stride and a
    // barrier, the sum over the n waves
    __device__ __forceinline__ static AggPartial fold(const uint64_t* s, int n, int stride) {
        AggPartial r;
        for (int w = 0; w < n; ++w) r.merge(load(s + w * stride));
        return r;
    }
    // The four result values {sum lo, sum hi, min, max} of the finishing wave. from_slices: the sum
    // is Σ 2^s·c_s and the offsets count from `base` (slice_agg_combine); else the sum is the values'
    // and the offsets count from INT64_MIN.
    __device__ __forceinline__ void result(uint32_t ops, int type, int64_t base, int from_slices, int64_t r[4]) const {
        if (from_slices) {
            slice_agg_combine(type, base, valid, sum, mn, mx, ops, r);
        } else {
            slice_agg_combine(type, INT64_MIN, valid, U128{0, 0}, mn, mx, ops & ~kAggSum, r);
            if (ops & kAggSum) {
                r[0] = (int64_t)sum.lo;
                r[1] = (int64_t)sum.hi;
            }
        }
    }
};

// Aggregate: SUM / MIN / MAX / COUNT of the column over the rows a program keeps, from the slices
// alone (O'Neil & Quass 1997 §3; Rinfret et al. 2001). Fused evaluate + aggregate in the eval_*
// family: persistent workgroups walk tiles of one zone (load_tile / eval_words / tail_mask, live-tile
// lists, every program form; K = 0: every row below n_rows), F stays in registers and no bitvector
// is written. Per pair of words Fv = F ∧ valid, then the slices are streamed once from the top
// down in chunks of up to 8 loaded before use (16-byte non-temporal loads, as ripple_chunk):
//   SUM     per chunk Σ_j popc(Fv ∧ w_j)·2^j is at most 2^15, shifted to the chunk's lowest slice
//           and added to the thread's 128-bit running sum Σ_s 2^s·c_s — exact at any partition size
//           (the whole sum stays below 2^64 · rows);
//   MIN/MAX the candidate ripple per word, cand = (cand ∧ ¬w) if that is non-empty (bit 0) else cand
//           (bit 1), MAX mirrored, with selects; the word's offset is built a bit per slice and
//           reduced unsigned per thread, wave, workgroup. A word with Fv = 0 yields 2^b - 1 / 0,
//           which can win only when no row qualifies.
// A pair whose Fv is zero across the whole wave skips its slice loads (a wave-uniform branch).
// Traffic: (b + K [+ 1 with validity])·n/8 bytes read over the live zones, nothing written.
template <bool SUM, bool MINMAX, int CNT>
__device__ __forceinline__ void agg_chunk(const SliceSet& sl, int top, uint64_t pi, const u64x2& f, U128& acc,
                                          u64x2& cmin, u64x2& cmax, u64x2& omin, u64x2& omax) {
    u64x2 w[CNT];
#pragma unroll
    for (int j = 0; j < CNT; ++j) w[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(sl.s[top - j]) + pi);
    if (SUM) {
        uint32_t local = 0;  // Horner from the chunk's top slice: ≤ 128·(2^CNT - 1)
#pragma unroll
        for (int j = 0; j < CNT; ++j) local = (local << 1) + (uint32_t)(__popcll(f.x & w[j].x) + __popcll(f.y & w[j].y));
        acc = u128_add(acc, u128_shl(local, (uint32_t)(top - CNT + 1)));
    }
    if (MINMAX) {
#pragma unroll
        for (int j = 0; j < CNT; ++j) {
            const u64x2 tn = cmin & ~w[j], tx = cmax & w[j];
            const bool nx = tn.x != 0, ny = tn.y != 0, xx = tx.x != 0, xy = tx.y != 0;
            cmin.x = nx ? tn.x : cmin.x;
            cmin.y = ny ? tn.y : cmin.y;
            cmax.x = xx ? tx.x : cmax.x;
            cmax.y = xy ? tx.y : cmax.y;
            omin.x = (omin.x << 1) | (nx ? 0ull : 1ull);
            omin.y = (omin.y << 1) | (ny ? 0ull : 1ull);
            omax.x = (omax.x << 1) | (xx ? 1ull : 0ull);
            omax.y = (omax.y << 1) | (xy ? 1ull : 0ull);
        }
    }
}

template <int K, int FORM, bool SUM, bool MINMAX>
__global__ __launch_bounds__(512, 4) void eval_slice_aggregate(EvalArgs a, SliceAggArgs g) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    constexpr int NWAVES = THREADS / 64;
    using Partial = AggPartial<true>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    Partial part;
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        u64x2 fv[PAIRS];
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            fv[p].x = r[2 * p];
            fv[p].y = r[2 * p + 1];
        }
        if (g.validity) {
            const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
#pragma unroll
            for (int p = 0; p < PAIRS; ++p) fv[p] &= load_pair<THREADS>(g.validity, false, whole, tile_word0, p, t, a.n_words);
        }
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            part.rows += (uint64_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1]));
            part.valid += (uint64_t)(__popcll(fv[p].x) + __popcll(fv[p].y));
        }
        if (!SUM && !MINMAX) continue;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            const u64x2 f = fv[p];
            if (__ballot((f.x | f.y) != 0) == 0) continue;  // no qualifying row in the wave's 128 words
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            u64x2 cmin = f, cmax = f, omin = {0ull, 0ull}, omax = {0ull, 0ull};
            int top = (int)g.n_slices - 1;
            switch (g.n_slices & 7u) {  // the top slices that fill no chunk of 8, then whole chunks
            case 1: agg_chunk<SUM, MINMAX, 1>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 2: agg_chunk<SUM, MINMAX, 2>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 3: agg_chunk<SUM, MINMAX, 3>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 4: agg_chunk<SUM, MINMAX, 4>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 5: agg_chunk<SUM, MINMAX, 5>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 6: agg_chunk<SUM, MINMAX, 6>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            case 7: agg_chunk<SUM, MINMAX, 7>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax); break;
            default: break;
            }
            top -= (int)(g.n_slices & 7u);
            for (; top >= 7; top -= 8) agg_chunk<SUM, MINMAX, 8>(g.slices, top, pi, f, part.sum, cmin, cmax, omin, omax);
            if (MINMAX) {
                // (a word of the pair without a qualifying row gives 2^b - 1 / 0: never below / above
                // the other word's offset)
                const uint64_t lo = omin.x < omin.y ? omin.x : omin.y, hi = omax.x > omax.y ? omax.x : omax.y;
                part.mn = lo < part.mn ? lo : part.mn;
                part.mx = hi > part.mx ? hi : part.mx;
            }
        }
    }
    // wave, then workgroup
    part.wave_reduce();
    __shared__ uint64_t s_part[NWAVES][Partial::kSlots];
    if (lane == 0) part.store(s_part[wave]);
    __syncthreads();
    if (t == 0) {
        const Partial s = Partial::fold(&s_part[0][0], NWAVES, Partial::kSlots);
        s.store(g.workspace + (uint64_t)kAggPartial * blockIdx.x, kAggPartial);
        finish_ticket(a.ticket, a.count, s.rows);
    }
}

// The column path's reduction: x[i] = the probed value of qualifying row i as the ABI carries it
// (FLOAT / DOUBLE patterns, UINT64 bits; 0 at NULL rows), valid bit i its NULL-ness. The sum adds
// the values (UINT64 unsigned, every other type signed) in 128 bits; min / max go through the
// comparison key, kept as the unsigned-ordered key ^ 2^63 — an offset from base INT64_MIN, so the
// finishing wave maps them as it maps the slices' offsets.
__global__ __launch_bounds__(256) void aggregate_arrays_kernel(const int64_t* __restrict__ x,
                                                               const uint64_t* __restrict__ valid,
                                                               const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                               uint32_t ops, int type, int64_t* __restrict__ workspace) {
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    using Partial = AggPartial<false>;
    Partial part;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (valid && !((valid[i >> 6] >> (i & 63)) & 1ull)) continue;
        const int64_t v = x[i];
        ++part.valid;
        if (ops & kAggSum) part.sum = u128_add(part.sum, U128{(uint64_t)v, type == kTypeUInt64 || v >= 0 ? 0ull : ~0ull});
        const uint64_t off = (uint64_t)value_key(type, v) ^ 0x8000000000000000ull;
        part.mn = off < part.mn ? off : part.mn;
        part.mx = off > part.mx ? off : part.mx;
    }
    part.wave_reduce();
    __shared__ uint64_t s_part[4][Partial::kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part.store(s_part[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial::fold(&s_part[0][0], 4, Partial::kSlots).store(workspace + (uint64_t)kAggPartial * blockIdx.x);
        // count_rows for the finishing wave (a scan that counted into the slot itself left it there)
        if (blockIdx.x == 0 && d_count != agg_count_slot(workspace)) *agg_count_slot(workspace) = n;
    }
}

// One wave combines the workgroups' partials (beside sum_partials_kernel: a strided share per lane,
// then a butterfly) and writes the six result slots (AggPartial::result has from_slices).
__global__ __launch_bounds__(64) void aggregate_finish_kernel(const int64_t* __restrict__ workspace, int nblocks,
                                                              uint32_t ops, int type, int64_t base, int from_slices,
                                                              int64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    using Partial = AggPartial<false>;
    Partial part;
    for (int b = lane; b < nblocks; b += 64) part.merge(Partial::load(workspace + (uint64_t)kAggPartial * b));
    part.wave_reduce();
    if (lane == 0) {
        int64_t r[4];
        part.result(ops, type, base, from_slices, r);
        out[0] = r[0];
        out[1] = r[1];
        out[2] = r[2];
        out[3] = r[3];
        out[4] = (int64_t)part.valid;
        out[5] = (int64_t)workspace[(uint64_t)kAggPartial * kAggMaxGrid];
    }
}

// Sum of a product: Σ a·b over the rows a program keeps, from the two columns' slices alone
// (cubit_program.hpp has the arithmetic; Rinfret et al. 2001). The tile walk, the program and the live
// tiles are eval_slice_aggregate's. Per pair of words V = F ∧ valid_a ∧ valid_b; a group of up to
// kProductInner slices of the inner operand (the one with fewer slices) is loaded and kept as
// M_j = V ∧ B_j, and the outer operand's slices stream past them from the top down in chunks of
// kProductChunk loaded before use (16-byte non-temporal loads, as agg_chunk). Per chunk and per j a
// Horner popcount over the chunk gives local_j ≤ 128·(2^8 - 1); Σ_j local_j·2^j < 2^23 goes to the
// thread's 128-bit cross accumulator with one shifted add. Σ of the outer offsets accumulates from
// popc(V ∧ A_i) in the first pass, Σ of the inner offsets from popc(M_j). An inner operand wider
// than kProductInner takes further groups, each streaming the outer slices again. The top chunk may
// reach above the outer slices, and a group above the inner ones: a slice that does not exist reads as
// zero. A pair whose V is zero across the wave loads nothing more (a wave-uniform branch).
// Traffic: (K + validities + n_in + n_out·passes)·n/8 bytes over the live zones, nothing written;
// n_in·n_out AND + popcount pairs per 64 rows.
constexpr int kProductChunk = 8;
// a partial: {cross lo, hi, Σ outer offsets lo, hi, Σ inner offsets lo, hi, valid rows}; exact adds,
// so any order of merges gives the same
__device__ __forceinline__ void product_merge(uint64_t* into, const uint64_t* from) {
#pragma unroll
    for (int k = 0; k < 6; k += 2) {
        const U128 s = u128_add(U128{into[k], into[k + 1]}, U128{from[k], from[k + 1]});
        into[k] = s.lo;
        into[k + 1] = s.hi;
    }
    into[6] += from[6];
}
__device__ __forceinline__ void product_wave_reduce(uint64_t (&part)[kProductPartial]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint64_t o[kProductPartial];
#pragma unroll
        for (int k = 0; k < kProductPartial; ++k) o[k] = __shfl_xor(part[k], d, 64);
        product_merge(part, o);
    }
}

template <int K, int FORM>
__global__ __launch_bounds__(512, 4) void eval_slice_sum_product(EvalArgs a, SliceProductArgs g) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    static_assert(PAIRS == 2, "the pair loop selects between two pairs");
    constexpr int NWAVES = THREADS / 64;
    constexpr int NI = (int)kProductInner, NC = kProductChunk;
    static_assert(NI <= 8 && NC <= 8, "Σ_j local_j·2^j stays inside 32 bits");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    U128 cross{0, 0}, s_out{0, 0}, s_in{0, 0};
    uint64_t c_valid = 0, c_rows = 0;
    const int n_out = (int)g.n_outer, n_in = (int)g.n_inner;
    const int top0 = (n_out + NC - 1) / NC * NC - 1;  // the top chunk's highest slot (-1: no outer slice)
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
        // one pair at a time (p is uniform, so the selects are scalar): both pairs' masks and chunks
        // in flight would not fit the register file
#pragma unroll 1
        for (int p = 0; p < PAIRS; ++p) {
            u64x2 v;
            v.x = p ? r[2] : r[0];
            v.y = p ? r[3] : r[1];
            c_rows += (uint64_t)(__popcll(v.x) + __popcll(v.y));
            if (__ballot((v.x | v.y) != 0) == 0) continue;  // no qualifying row in the wave's 128 words
            if (g.valid_a) v &= load_pair<THREADS>(g.valid_a, false, whole, tile_word0, p, t, a.n_words);
            if (g.valid_b) v &= load_pair<THREADS>(g.valid_b, false, whole, tile_word0, p, t, a.n_words);
            c_valid += (uint64_t)(__popcll(v.x) + __popcll(v.y));
            if (__ballot((v.x | v.y) != 0) == 0) continue;
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            int g0 = 0;
            do {
                const int cnt = n_in - g0 < NI ? n_in - g0 : NI;
                u64x2 m[NI];
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    m[j] = u64x2{0ull, 0ull};
                    if (j < cnt) m[j] = v & __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.inner.s[g0 + j]) + pi);
                }
                uint32_t li = 0;
#pragma unroll
                for (int j = 0; j < NI; ++j) li += (uint32_t)(__popcll(m[j].x) + __popcll(m[j].y)) << j;
                s_in = u128_add(s_in, u128_shl_wide(li, (uint32_t)g0));
#pragma unroll 1
                for (int top = top0; top >= 0; top -= NC) {
                    u64x2 w[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        w[c] = u64x2{0ull, 0ull};
                        if (top - c < n_out)
                            w[c] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.outer.s[top - c]) + pi);
                    }
                    const uint32_t low = (uint32_t)(top - NC + 1);
                    if (g0 == 0) {
                        uint32_t lo = 0;
#pragma unroll
                        for (int c = 0; c < NC; ++c) lo = (lo << 1) + (uint32_t)(__popcll(v.x & w[c].x) + __popcll(v.y & w[c].y));
                        s_out = u128_add(s_out, u128_shl(lo, low));
                    }
                    uint32_t comb = 0;
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        if (j >= cnt) continue;  // uniform
                        uint32_t l = 0;  // Horner from the chunk's top slice
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            l = (l << 1) + (uint32_t)(__popcll(m[j].x & w[c].x) + __popcll(m[j].y & w[c].y));
                        comb += l << j;
                    }
                    cross = u128_add(cross, u128_shl_wide(comb, low + (uint32_t)g0));
                }
                g0 += NI;
            } while (g0 < n_in);
        }
    }
    // wave, then workgroup
    uint64_t part[kProductPartial] = {cross.lo, cross.hi, s_out.lo, s_out.hi, s_in.lo, s_in.hi, c_valid};
    product_wave_reduce(part);
    c_rows = wave_sum(c_rows);
    __shared__ uint64_t s_part[NWAVES][kProductPartial + 1];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kProductPartial; ++k) s_part[wave][k] = part[k];
        s_part[wave][kProductPartial] = c_rows;
    }
    __syncthreads();
    if (t == 0) {
        uint64_t rows = s_part[0][kProductPartial];
        for (int w = 1; w < NWAVES; ++w) {
            product_merge(s_part[0], s_part[w]);
            rows += s_part[w][kProductPartial];
        }
        int64_t* o = g.workspace + (uint64_t)kProductPartial * blockIdx.x;
#pragma unroll
        for (int k = 0; k < kProductPartial; ++k) o[k] = (int64_t)s_part[0][k];
        finish_ticket(a.ticket, a.count, rows);
    }
}

// One wave combines the workgroups' partials and writes {sum_lo, sum_hi} (slice_product_combine),
// with out_slots = 4 also {count_valid, count_rows}; count_out (optional) gets the rows as well.
__global__ __launch_bounds__(64) void slice_product_finish_kernel(const int64_t* __restrict__ workspace, int nblocks,
                                                                  int64_t base_outer, int64_t base_inner,
                                                                  int64_t* __restrict__ out, int out_slots,
                                                                  uint64_t* __restrict__ count_out) {
    const int lane = threadIdx.x;
    uint64_t part[kProductPartial] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = lane; b < nblocks; b += 64)
        product_merge(part, reinterpret_cast<const uint64_t*>(workspace) + (uint64_t)kProductPartial * b);
    product_wave_reduce(part);
    if (lane == 0) {
        int64_t r[2];
        slice_product_combine(base_outer, base_inner, part[6], U128{part[0], part[1]}, U128{part[2], part[3]},
                              U128{part[4], part[5]}, r);
        const uint64_t rows = (uint64_t)workspace[(uint64_t)kAggPartial * kAggMaxGrid];
        out[0] = r[0];
        out[1] = r[1];
        if (out_slots >= 4) {
            out[2] = (int64_t)part[6];
            out[3] = (int64_t)rows;
        }
        if (count_out) *count_out = rows;
    }
}

// Select: the k-th smallest / largest value (or quantile_disc) of the column over the rows a program
// keeps, from the slices alone — a radix select over the offsets, most significant slices first,
// kSelectChunk slices per pass (cubit_program.hpp has the step logic, shared with the CPU).
//   pass 0     eval_slice_select, in the eval_* family as eval_slice_aggregate: F in registers,
//              C = F ∧ valid written to the candidate bitvector (every word of every evaluated tile),
//              count_rows through the ticket, and the first chunk histogrammed: per pair of words
//              the popcounts of the 2^cnt AND-combinations of C with the chunk's slices and their
//              complements, formed depth-first so one mask per level is live;
//   pass p > 0 slice_select_narrow reads C, loads the previous chunk again and the next one (all
//              loads before use), keeps the rows whose previous chunk equals the bucket the step
//              chose (read from the device state; uniform), writes C back in place (one thread per
//              word) and histograms the next chunk.
// After each pass one workgroup (select_step_kernel) sums the workgroups' partial histograms and applies
// select_step; after the last it writes the six result slots. The chosen bucket's count after the
// last chunk is count_equal, so the candidates are not narrowed by the last chunk. Counters are
// exact 64-bit integers reduced by wave, then workgroup, then per-workgroup partials: no atomics per
// row, no workgroup waits on another, the stream orders the passes. A pair whose C is zero across
// the wave skips its slice loads. Traffic: (K [+ 1] + 1 + 2b - d_last + 2·(passes - 1))·n/8 bytes
// over the live zones.
// The counters of a histogram: 64 bits per bucket, or — the grouped kernels, which keep a histogram per
// group — 16-bit fields, two per register. A thread adds at most the 64·NW = 256 rows it holds of a
// tile to one field, so the grouped kernels fold the fields into 64-bit counters every
// kSelectFoldTiles tiles (and at the end), before a field can wrap.
template <int IDX>
__device__ __forceinline__ void select_hist_add(uint64_t (&h)[1 << kSelectChunk], uint32_t px) {
    h[IDX] += px;
}
constexpr uint32_t kSelectFoldTiles = 128;
static_assert((uint64_t)kSelectFoldTiles * 4 * 64 <= 0xffffu, "a 16-bit field holds a thread's rows between two folds");
struct PackedHist {
    uint32_t v[(1 << kSelectChunk) / 2];
};
template <int IDX>
__device__ __forceinline__ void select_hist_add(PackedHist& h, uint32_t px) {
    h.v[IDX >> 1] += px << (16 * (IDX & 1));
}
template <int CNT, int J, int IDX, typename H>
__device__ __forceinline__ void select_hist_rec(const u64x2 (&w)[CNT > 0 ? CNT : 1], const u64x2& x, uint32_t px, H& h) {
    if constexpr (J == CNT) {
        select_hist_add<IDX>(h, px);
    } else {
        const u64x2 one = x & w[J];
        const uint32_t p1 = (uint32_t)(__popcll(one.x) + __popcll(one.y));
        select_hist_rec<CNT, J + 1, 2 * IDX + 1>(w, one, p1, h);
        const u64x2 zero = x & ~w[J];
        select_hist_rec<CNT, J + 1, 2 * IDX>(w, zero, px - p1, h);
    }
}
// the chunk whose top slice is `top` (w[0]), CNT slices: bucket = the chunk's bits, top slice first
template <int CNT>
__device__ __forceinline__ void select_hist_chunk(const SliceSet& sl, int top, uint64_t pi, const u64x2& c,
                                                  uint64_t (&h)[1 << kSelectChunk]) {
    u64x2 w[CNT > 0 ? CNT : 1];
#pragma unroll
    for (int j = 0; j < CNT; ++j) w[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(sl.s[top - j]) + pi);
    select_hist_rec<CNT, 0, 0>(w, c, (uint32_t)(__popcll(c.x) + __popcll(c.y)), h);
}

// wave, then workgroup, then this workgroup's partials (nb counters at workspace + nb·blockIdx.x)
template <int NWAVES>
__device__ __forceinline__ void select_hist_publish(uint64_t (&h)[1 << kSelectChunk], int64_t* workspace, int t) {
    constexpr int NB = 1 << kSelectChunk;
    __shared__ uint64_t s_hist[NWAVES][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) h[i] = wave_sum(h[i]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NB; ++i) s_hist[t >> 6][i] = h[i];
    }
    __syncthreads();
    if (t < NB) {
        uint64_t s = 0;
        for (int w = 0; w < NWAVES; ++w) s += s_hist[w][t];
        workspace[(uint64_t)NB * blockIdx.x + t] = (int64_t)s;
    }
}

template <int K, int FORM>
__global__ __launch_bounds__(512, 2) void eval_slice_select(EvalArgs a, SliceSelectArgs g) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    constexpr int NWAVES = THREADS / 64;
    const int t = threadIdx.x;
    uint64_t c_rows = 0;
    uint64_t h[1 << kSelectChunk];
#pragma unroll
    for (int i = 0; i < (1 << kSelectChunk); ++i) h[i] = 0;
    const int cnt0 = (int)select_first_chunk(g.n_slices, kSelectChunk), top = (int)g.n_slices - 1;
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        u64x2 fv[PAIRS];
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            fv[p].x = r[2 * p];
            fv[p].y = r[2 * p + 1];
        }
        // (load_pair's words, spelled out: read through load_pair this kernel compiles to 132 VGPRs and
        // three waves per SIMD in 13 instantiations that have four this way)
        if (g.validity) {
            if (tile_word0 + TILE_WORDS <= a.n_words) {  // uniform: the whole tile lies below the last word
#pragma unroll
                for (int p = 0; p < PAIRS; ++p)
                    fv[p] &= reinterpret_cast<const u64x2*>(g.validity + tile_word0)[p * THREADS + t];
            } else {  // the tile holding the last word: nothing at or past n_words is read
#pragma unroll
                for (int p = 0; p < PAIRS; ++p) {
                    const uint64_t gw = word_index<THREADS>(tile_word0, 2 * p, t);
                    fv[p].x &= gw < a.n_words ? g.validity[gw] : 0ull;
                    fv[p].y &= gw + 1 < a.n_words ? g.validity[gw + 1] : 0ull;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            c_rows += (uint64_t)(__popcll(r[2 * p]) + __popcll(r[2 * p + 1]));
            const u64x2 c = fv[p];
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            reinterpret_cast<u64x2*>(g.cand)[pi] = c;  // the tile lies inside the padded candidate words
            if (__ballot((c.x | c.y) != 0) == 0) continue;  // no candidate in the wave's 128 words
            switch (cnt0) {  // uniform
            case 1: select_hist_chunk<1>(g.slices, top, pi, c, h); break;
            case 2: select_hist_chunk<2>(g.slices, top, pi, c, h); break;
            case 3: select_hist_chunk<3>(g.slices, top, pi, c, h); break;
            case 4: select_hist_chunk<4>(g.slices, top, pi, c, h); break;
            default: select_hist_chunk<0>(g.slices, top, pi, c, h); break;  // no slice: one bucket, the rows
            }
        }
    }
    select_hist_publish<NWAVES>(h, g.workspace, t);
    c_rows = wave_sum(c_rows);
    __shared__ uint64_t s_rows[NWAVES];
    if ((t & 63) == 0) s_rows[t >> 6] = c_rows;
    __syncthreads();
    if (t == 0) {
        uint64_t cr = 0;
        for (int w = 0; w < NWAVES; ++w) cr += s_rows[w];
        finish_ticket(a.ticket, a.count, cr);
    }
}

// PC: the previous chunk's slices (its lowest at prev_low); the next chunk is whole, its lowest slice
// at prev_low - kSelectChunk. a: the tile list of pass 0 (num_tiles, live).
template <int PC>
__global__ __launch_bounds__(512, 2) void slice_select_narrow(EvalArgs a, SliceSelectArgs g, uint32_t prev_low) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4, NC = (int)kSelectChunk;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    constexpr int NWAVES = THREADS / 64;
    const int t = threadIdx.x;
    uint64_t h[1 << kSelectChunk];
#pragma unroll
    for (int i = 0; i < (1 << kSelectChunk); ++i) h[i] = 0;
    const SelectState* st = select_state(g.workspace);
    if (st->found) {  // uniform; a select without a row leaves the candidates and the histogram alone
        const uint32_t want = (uint32_t)(st->prefix >> prev_low);  // the previous chunk's bucket in its low PC bits
        const int ptop = (int)prev_low + PC - 1, ntop = (int)prev_low - 1;
        const uint32_t n_idx = a.num_tiles;
        for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
            const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
#pragma unroll
            for (int p = 0; p < PAIRS; ++p) {
                const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
                u64x2 c = reinterpret_cast<const u64x2*>(g.cand)[pi];
                if (__ballot((c.x | c.y) != 0) == 0) continue;  // no candidate in the wave's 128 words
                u64x2 pw[PC], w[NC];
#pragma unroll
                for (int j = 0; j < PC; ++j)
                    pw[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.slices.s[ptop - j]) + pi);
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    w[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.slices.s[ntop - j]) + pi);
#pragma unroll
                for (int j = 0; j < PC; ++j) {
                    if ((want >> (PC - 1 - j)) & 1u) c &= pw[j];
                    else c &= ~pw[j];
                }
                reinterpret_cast<u64x2*>(g.cand)[pi] = c;
                select_hist_rec<NC, 0, 0>(w, c, (uint32_t)(__popcll(c.x) + __popcll(c.y)), h);
            }
        }
    }
    select_hist_publish<NWAVES>(h, g.workspace, t);
}

// The array select's pass (the column path): x / valid / d_count as aggregate_arrays_kernel reads
// them. A row's comparison key ^ 2^63 orders unsigned (an offset from base INT64_MIN); the pass
// histograms bits [shift, shift + 8) of the rows whose higher bits equal the state's prefix into 256
// LDS counters per workgroup and leaves them as the workgroup's partials.
__global__ __launch_bounds__(256) void select_arrays_kernel(const int64_t* __restrict__ x,
                                                            const uint64_t* __restrict__ valid,
                                                            const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                            int type, uint32_t shift, int first,
                                                            int64_t* __restrict__ workspace) {
    constexpr int NB = 1 << kSelectArrayBits;
    static_assert(NB == 256, "one counter per thread");
    __shared__ unsigned long long s_h[NB];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n = min(*d_count, max_n);
    const SelectState* st = select_state(workspace);
    if (first || st->found) {  // uniform
        // (the first pass takes every valid row: the state is not set yet)
        const uint64_t hi_mask = first ? 0ull : ~0ull << (shift + kSelectArrayBits);
        const uint64_t prefix = first ? 0ull : st->prefix & hi_mask;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        const uint32_t lane = threadIdx.x & 63u;
        // a wave walks 64 consecutive rows with every lane active (the bound is on the wave's first
        // row), so the ballots below see the whole wave
        for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
            const uint64_t i = i0 + lane;
            bool take = i < n && (!valid || ((valid[i0 >> 6] >> lane) & 1ull));
            uint32_t bucket = 0;
            if (take) {
                const uint64_t off = (uint64_t)value_key(type, x[i]) ^ 0x8000000000000000ull;
                take = (off & hi_mask) == prefix;
                bucket = (uint32_t)(off >> shift) & (NB - 1);
            }
            const uint64_t m = __ballot(take);
            if (m == 0) continue;
            // a wave whose rows all fall into one bucket (the passes above a narrow column's span,
            // heavy ties) adds its count once: 64 atomics on one LDS address serialise
            const uint32_t lead = (uint32_t)__shfl((int)bucket, __ffsll((unsigned long long)m) - 1, 64);
            if (__ballot(take && bucket == lead) == m) {
                if (lane == 0) atomicAdd(&s_h[lead], (unsigned long long)__popcll(m));
            } else if (take) {
                atomicAdd(&s_h[bucket], 1ull);
            }
        }
    }
    __syncthreads();
    workspace[(uint64_t)NB * blockIdx.x + threadIdx.x] = (int64_t)s_h[threadIdx.x];
    if (first && blockIdx.x == 0 && threadIdx.x == 0) *select_count_slot(workspace) = n;  // count_rows
}

// One workgroup after each pass: sums the nblocks partial histograms of nb buckets (a power of two,
// at most 256) — thread t takes bucket t mod nb of every (1024 / nb)-th workgroup, so the loads of
// one bucket spread over 4 … 1024 threads and a lane issues nblocks·nb/1024 of them — and thread 0
// applies select_step to the device state; `last` writes the six result slots.
constexpr int kSelectStepThreads = 1024;
__global__ __launch_bounds__(kSelectStepThreads) void select_step_kernel(int64_t* __restrict__ workspace, int nblocks,
                                                                         uint32_t nb, uint32_t low, int first, int last,
                                                                         int mode, uint64_t k, double q, int type,
                                                                         int64_t base, int64_t* __restrict__ out) {
    __shared__ uint64_t s_part[kSelectStepThreads];
    __shared__ uint64_t s_counts[1 << kSelectArrayBits];
    const uint32_t lane = threadIdx.x;
    const uint32_t groups = (uint32_t)kSelectStepThreads / nb, j = lane % nb;
    uint64_t sum = 0;
    for (uint32_t b = lane / nb; b < (uint32_t)nblocks; b += groups) sum += (uint64_t)workspace[(uint64_t)nb * b + j];
    s_part[lane] = sum;
    __syncthreads();
    if (lane < nb) {
        uint64_t c = 0;
        for (uint32_t g = 0; g < groups; ++g) c += s_part[g * nb + lane];
        s_counts[lane] = c;
    }
    __syncthreads();
    if (lane == 0) {
        SelectState* st = select_state(workspace);
        SelectState state = *st;
        select_step(&state, first != 0, mode, k, q, s_counts, nb, low);
        *st = state;
        if (last) {
            int64_t r[6];
            select_result(state, type, base, *select_count_slot(workspace), r);
#pragma unroll
            for (int i = 0; i < 6; ++i) out[i] = r[i];
        }
    }
}

// Two ascending runs of distinct row ids (no id in both) merged into one: every element lands at its
// index plus the number of the other run's ids below it (a binary search). *count = na + nb.
__device__ __forceinline__ uint64_t ids_below(const int64_t* __restrict__ v, uint64_t n, int64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void merge_ids_kernel(const int64_t* __restrict__ a, uint64_t na,
                                                        const int64_t* __restrict__ b, uint64_t nb,
                                                        int64_t* __restrict__ out, uint64_t* __restrict__ count) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += stride) {
        if (i < na) out[i + ids_below(b, nb, a[i])] = a[i];
        else out[(i - na) + ids_below(a, na, b[i - na])] = b[i - na];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = na + nb;
}

// GROUP BY: eval_slice_aggregate over a batch of groups per launch. Each group is the AND of one
// equality bitvector per group column, so the tile walk, the program evaluation and the slice stream
// are eval_slice_aggregate's, read once for the whole batch, and per pair of words the batch's group
// leaves are loaded once (16 bytes each) and every group's rows formed in registers as
// m = F ∧ E1_a ∧ E2_b (then ∧ v for the valid rows). A leaf flagged in neg is a group column's
// validity: its complement under F (tail_mask has cleared the bits past n_rows) is the NULL group.
// Per chunk of slices every group adds its Horner popcount sum to its own 128-bit accumulator, and
// with MINMAX runs its own candidate ripple. A pair whose F is zero across the wave loads nothing
// more; one whose groups' valid rows are all zero skips the slices; a group whose mask is zero across
// the wave skips its arithmetic (wave-uniform branches). The batch is NG = kGroupBatchSum groups, or
// kGroupBatchMinMax with MINMAX (the ripple keeps 16 more registers per group): NG × 1 leaves with one
// group column, NG/2 × 2 with TWO. Each group's rows are counted in its partials, so the kernel takes
// no ticket. Traffic: (b + K [+ 1] + the launch's group leaves)·n/8 bytes over the live zones.
// One chunk of CNT slices from `top` down for every live group. GUARD: the chunk may reach above the
// index's slices (the slice count rounded up to the chunk), and a slice that does not exist reads as
// zero: it adds nothing to a sum, leaves a non-empty candidate set as it is (bit 0 of the offset) and
// makes an empty word's MIN offset larger still.
template <int NG, bool MINMAX, int CNT, bool GUARD>
__device__ __forceinline__ void agg_chunk_grouped(const SliceSet& sl, int n_slices, int top, uint64_t pi, uint32_t live,
                                                  const u64x2 (&m)[NG], U128 (&acc)[NG], u64x2 (&cmin)[NG],
                                                  u64x2 (&cmax)[NG], u64x2 (&omin)[NG], u64x2 (&omax)[NG]) {
    u64x2 w[CNT];
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
        if (GUARD && top - j >= n_slices) w[j] = u64x2{0ull, 0ull};
        else w[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(sl.s[top - j]) + pi);
    }
#pragma unroll
    for (int q = 0; q < NG; ++q) {
        if (!((live >> q) & 1u)) continue;  // no valid row of this group in the wave's 128 words
        uint32_t local = 0;  // Horner from the chunk's top slice: ≤ 128·(2^CNT - 1)
#pragma unroll
        for (int j = 0; j < CNT; ++j)
            local = (local << 1) + (uint32_t)(__popcll(m[q].x & w[j].x) + __popcll(m[q].y & w[j].y));
        acc[q] = u128_add(acc[q], u128_shl(local, (uint32_t)(top - CNT + 1)));
        if (MINMAX) {
#pragma unroll
            for (int j = 0; j < CNT; ++j) {
                const u64x2 tn = cmin[q] & ~w[j], tx = cmax[q] & w[j];
                const bool nx = tn.x != 0, ny = tn.y != 0, xx = tx.x != 0, xy = tx.y != 0;
                cmin[q].x = nx ? tn.x : cmin[q].x;
                cmin[q].y = ny ? tn.y : cmin[q].y;
                cmax[q].x = xx ? tx.x : cmax[q].x;
                cmax[q].y = xy ? tx.y : cmax[q].y;
                omin[q].x = (omin[q].x << 1) | (nx ? 0ull : 1ull);
                omin[q].y = (omin[q].y << 1) | (ny ? 0ull : 1ull);
                omax[q].x = (omax[q].x << 1) | (xx ? 1ull : 0ull);
                omax[q].y = (omax[q].y << 1) | (xy ? 1ull : 0ull);
            }
        }
    }
}

template <int K, int FORM, bool TWO, bool MINMAX>
__global__ __launch_bounds__(512, 2) void eval_slice_aggregate_grouped(EvalArgs a, SliceAggArgs g, GroupAggArgs q) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    constexpr int NWAVES = THREADS / 64;
    constexpr int NG = MINMAX ? (int)kGroupBatchMinMax : (int)kGroupBatchSum;
    constexpr int NA = TWO ? NG / 2 : NG;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    U128 acc[NG];
    uint64_t mn[NG], mx[NG], c_rows[NG], c_valid[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        acc[j] = U128{0, 0};
        mn[j] = ~0ull;
        mx[j] = 0;
        c_rows[j] = c_valid[j] = 0;
    }
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
        static_assert(PAIRS == 2, "the pair loop selects between two pairs");
        // one pair at a time (not unrolled: both pairs' masks and slices in flight do not fit the
        // register file; p is uniform, so the selects are scalar)
#pragma unroll 1
        for (int p = 0; p < PAIRS; ++p) {
            u64x2 f;
            f.x = p ? r[2] : r[0];
            f.y = p ? r[3] : r[1];
            if (__ballot((f.x | f.y) != 0) == 0) continue;  // no qualifying row in the wave's 128 words
            u64x2 m[NG];
            if (TWO) {
                u64x2 eb[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    eb[b] = u64x2{0ull, 0ull};
                    if ((uint32_t)b < q.n2)
                        eb[b] = load_pair<THREADS>(q.e2[b], (q.neg2 >> b) & 1u, whole, tile_word0, p, t, a.n_words);
                }
#pragma unroll
                for (int x = 0; x < NA; ++x) {
                    u64x2 ea = {0ull, 0ull};
                    if ((uint32_t)x < q.n1)
                        ea = f & load_pair<THREADS>(q.e1[x], (q.neg1 >> x) & 1u, whole, tile_word0, p, t, a.n_words);
                    m[2 * x] = ea & eb[0];
                    m[2 * x + 1] = ea & eb[1];
                }
            } else {
#pragma unroll
                for (int x = 0; x < NA; ++x) {
                    m[x] = u64x2{0ull, 0ull};
                    if ((uint32_t)x < q.n1)
                        m[x] = f & load_pair<THREADS>(q.e1[x], (q.neg1 >> x) & 1u, whole, tile_word0, p, t, a.n_words);
                }
            }
            if (g.validity) {
                const u64x2 vv = load_pair<THREADS>(g.validity, false, whole, tile_word0, p, t, a.n_words);
#pragma unroll
                for (int j = 0; j < NG; ++j) {
                    c_rows[j] += (uint64_t)(__popcll(m[j].x) + __popcll(m[j].y));
                    m[j] &= vv;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NG; ++j) c_rows[j] += (uint64_t)(__popcll(m[j].x) + __popcll(m[j].y));
            }
            uint32_t live = 0;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                c_valid[j] += (uint64_t)(__popcll(m[j].x) + __popcll(m[j].y));
                if (__ballot((m[j].x | m[j].y) != 0) != 0) live |= 1u << j;
            }
            if (live == 0) continue;
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            u64x2 cmin[NG], cmax[NG], omin[NG], omax[NG];
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                cmin[j] = cmax[j] = m[j];
                omin[j] = omax[j] = u64x2{0ull, 0ull};
            }
            // the top slices that fill no chunk of 4 as one guarded chunk, then whole chunks (chunks of
            // 8, as the ungrouped kernel takes them, spill beside a batch of masks and accumulators)
            const int ns = (int)g.n_slices, rem = ns & 3;
            int top = ns - rem - 1;
            if (rem > 0)
                agg_chunk_grouped<NG, MINMAX, 4, true>(g.slices, ns, top + 4, pi, live, m, acc, cmin, cmax, omin, omax);
#pragma unroll 1
            for (; top >= 3; top -= 4)
                agg_chunk_grouped<NG, MINMAX, 4, false>(g.slices, ns, top, pi, live, m, acc, cmin, cmax, omin, omax);
            if (MINMAX) {
#pragma unroll
                for (int j = 0; j < NG; ++j) {
                    if (!((live >> j) & 1u)) continue;
                    // (a word of the pair without a row of the group gives 2^b - 1 / 0: never below /
                    // above another word's offset)
                    const uint64_t lo = omin[j].x < omin[j].y ? omin[j].x : omin[j].y;
                    const uint64_t hi = omax[j].x > omax[j].y ? omax[j].x : omax[j].y;
                    mn[j] = lo < mn[j] ? lo : mn[j];
                    mx[j] = hi > mx[j] ? hi : mx[j];
                }
            }
        }
    }
    // wave, then workgroup, per group
    using Partial = AggPartial<true>;
    static_assert(Partial::kSlots == kGroupPartial, "the grouped workspace holds whole partials");
    __shared__ uint64_t s_part[NWAVES][NG][kGroupPartial];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        Partial part{acc[j], mn[j], mx[j], c_valid[j], c_rows[j]};
        part.wave_reduce();
        if (lane == 0) part.store(s_part[wave][j]);
    }
    __syncthreads();
    if (t < NG)
        Partial::fold(&s_part[0][t][0], NWAVES, NG * kGroupPartial)
            .store(q.partials + ((uint64_t)t * gridDim.x + blockIdx.x) * kGroupPartial);
}

// The column path per group: x / valid as aggregate_arrays_kernel's, and per group column the probed
// value and its validity. Each row's group values map to slots by binary search over the columns'
// ascending slot keys (a NULL value: the column's NULL slot), and the row is accumulated into its
// group in LDS: the value's two 32-bit halves go to two 64-bit LDS sums (the high half signed, or
// unsigned for UINT64), which cannot wrap within kGroupFlushIters iterations of 256 rows; every so
// many iterations, and at the end, a thread per group folds them into the group's 128-bit sum. Min /
// max go through the comparison key as an unsigned offset from INT64_MIN, as above. The partials
// are the grouped slice kernel's.
constexpr uint32_t kGroupFlushIters = 64;
__device__ __forceinline__ int group_slot_of(const GroupColArgs& gc, int c, uint64_t i) {
    if (gc.valid[c] && !((gc.valid[c][i >> 6] >> (i & 63)) & 1ull)) return gc.null_slot[c];
    const int64_t key = value_key(gc.type[c], gc.v[c][i]);
    const int64_t* keys = gc.keys[c];
    uint32_t lo = 0, hi = gc.n_keys[c];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < gc.n_keys[c] && keys[lo] == key ? (int)lo : -1;
}

__global__ __launch_bounds__(256) void aggregate_arrays_grouped_kernel(const int64_t* __restrict__ x,
                                                                       const uint64_t* __restrict__ valid,
                                                                       GroupColArgs gc, uint32_t n_groups,
                                                                       const uint64_t* __restrict__ d_count,
                                                                       uint64_t max_n, uint32_t ops, int type,
                                                                       int64_t* __restrict__ partials) {
    // per group: {Σ low halves, Σ high halves, sum lo, sum hi, min, max, valid rows, rows}
    __shared__ unsigned long long s_acc[CUBIT_AGG_MAX_GROUPS][8];
    const uint64_t n = min(*d_count, max_n);
    const bool uns = type == kTypeUInt64;
    for (uint32_t q = threadIdx.x; q < n_groups; q += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_acc[q][k] = k == 4 ? ~0ull : 0ull;
    }
    __syncthreads();
    auto fold = [&]() {
        for (uint32_t q = threadIdx.x; q < n_groups; q += blockDim.x) {
            const uint64_t l = s_acc[q][0], h = s_acc[q][1];
            // Σ = l + h·2^32, h sign-extended unless the column is unsigned
            const U128 hh{h << 32, uns ? h >> 32 : (uint64_t)((int64_t)h >> 32)};
            const U128 s = u128_add(U128{s_acc[q][2], s_acc[q][3]}, u128_add(U128{l, 0}, hh));
            s_acc[q][0] = s_acc[q][1] = 0;
            s_acc[q][2] = s.lo;
            s_acc[q][3] = s.hi;
        }
    };
    uint32_t iters = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        if (i < n) {
            const int s1 = group_slot_of(gc, 0, i);
            const int s2 = gc.n_cols > 1 ? group_slot_of(gc, 1, i) : 0;
            if (s1 >= 0 && s2 >= 0) {
                unsigned long long* acc = s_acc[(uint32_t)s1 * gc.n2 + (uint32_t)s2];
                atomicAdd(&acc[7], 1ull);
                if (!valid || ((valid[i >> 6] >> (i & 63)) & 1ull)) {
                    const int64_t v = x[i];
                    atomicAdd(&acc[6], 1ull);
                    if (ops & kAggSum) {
                        atomicAdd(&acc[0], (unsigned long long)(uint32_t)v);
                        atomicAdd(&acc[1], uns ? (unsigned long long)((uint64_t)v >> 32) : (unsigned long long)(v >> 32));
                    }
                    const unsigned long long off = (uint64_t)value_key(type, v) ^ 0x8000000000000000ull;
                    atomicMin(&acc[4], off);
                    atomicMax(&acc[5], off);
                }
            }
        }
        if (++iters == kGroupFlushIters) {  // uniform: the loop bounds are the workgroup's
            __syncthreads();
            fold();
            __syncthreads();
            iters = 0;
        }
    }
    __syncthreads();
    fold();
    for (uint32_t q = threadIdx.x; q < n_groups; q += blockDim.x) {
        int64_t* part = partials + ((uint64_t)q * gridDim.x + blockIdx.x) * kGroupPartial;
        part[0] = (int64_t)s_acc[q][2];
        part[1] = (int64_t)s_acc[q][3];
        part[2] = (int64_t)s_acc[q][4];
        part[3] = (int64_t)s_acc[q][5];
        part[4] = (int64_t)s_acc[q][6];
        part[5] = (int64_t)s_acc[q][7];
    }
}

// One wave per group (slot) combines the workgroups' partials as aggregate_finish_kernel does and
// writes the group's six result slots; a group without a qualifying row gets six zeros, one whose
// rows are all NULL its count_rows alone. group: the group of each slot (kNoGroup: none), or null
// when slot = group.
__global__ __launch_bounds__(64) void aggregate_grouped_finish_kernel(const int64_t* __restrict__ partials, int nblocks,
                                                                      GroupAggArgs q, int identity, uint32_t ops,
                                                                      int type, int64_t base, int from_slices,
                                                                      int64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    const uint32_t slot = blockIdx.x;
    const uint32_t group = identity ? slot : q.group[slot < kGroupBatchSum ? slot : 0];
    if (group == kNoGroup) return;
    using Partial = AggPartial<true>;
    Partial part;
    for (int b = lane; b < nblocks; b += 64) part.merge(Partial::load(partials + ((uint64_t)slot * nblocks + b) * kGroupPartial));
    part.wave_reduce();
    if (lane == 0) {
        int64_t r[4] = {0, 0, 0, 0};
        if (part.valid != 0) part.result(ops, type, base, from_slices, r);
        int64_t* o = out + (uint64_t)group * 6;
        o[0] = r[0];
        o[1] = r[1];
        o[2] = r[2];
        o[3] = r[3];
        o[4] = (int64_t)part.valid;
        o[5] = (int64_t)part.rows;
    }
}

// GROUP BY for the select: the radix select of eval_slice_select / slice_select_narrow for a batch of
// NG = kGroupBatchSelect groups over ONE candidate bitvector. The groups of a call are pairwise
// disjoint row sets (one equality leaf per group column, the NULL slot the complemented validity under
// F), so C = ∪_g C_g keeps every group's candidates apart: group g's are C ∧ E_g.
//   pass 0     eval_slice_select_grouped: F in registers, the batch's group leaves loaded once per pair
//              of words (as eval_slice_aggregate_grouped), per group M_g = F ∧ E1 ∧ E2 counted into
//              count_rows_g, C_g = M_g ∧ valid, C = ∪ C_g written to the candidate bitvector (every word
//              of every evaluated tile) and the first chunk histogrammed per group over C_g;
//   pass p > 0 slice_select_narrow_grouped reads C, loads the group leaves, the previous chunk and
//              the next (all loads before use), keeps C' = C ∧ ∪_g (E_g ∧ [previous chunk = group g's
//              chosen bucket]) — the bucket read from the group's device state, uniform; a group whose
//              found is 0 keeps nothing — writes C' back in place (one thread per word) and histograms
//              the next chunk per group.
// After each pass select_step_grouped_kernel sums the workgroups' partials per slot and applies
// select_step to each slot's state; after the last it writes the six result slots of each group. A
// batch runs through all its passes before the next starts, so each batch's pass 0 rewrites the
// candidate bitvector whole. Counters: per thread and group the 2^4 buckets as 16-bit fields
// (PackedHist) and a 32-bit row count, folded by wave_sum into the wave's 64-bit LDS counters every
// kSelectFoldTiles tiles and at the end; then workgroup, then the workgroup's partials. Exact integers,
// no atomics, no workgroup waits on another, the stream orders the passes. A pair whose F (or C) is
// zero across the wave loads nothing more; a group whose rows are zero across the wave skips its
// arithmetic. Traffic per launch: (K [+ 1] + 1 + 2b - d_last + 2·(passes - 1) + leaves·passes)·n/8
// bytes over the live zones.
template <int NG>
__device__ __forceinline__ void select_group_zero(uint64_t (*s_hist)[NG][kSelectSlotCols], int nwaves, int t, int threads) {
    uint64_t* flat = &s_hist[0][0][0];
    for (int i = t; i < nwaves * NG * (int)kSelectSlotCols; i += threads) flat[i] = 0;
    __syncthreads();
}
// the thread's packed counters into its wave's LDS counters (every lane active); the fields restart
template <int NG>
__device__ __forceinline__ void select_group_fold(PackedHist (&h)[NG], uint32_t (&c_rows)[NG / 2],
                                                  uint64_t (&s_wave)[NG][kSelectSlotCols], int lane) {
#pragma unroll
    for (int j = 0; j < NG; ++j) {
#pragma unroll
        for (int i = 0; i < (1 << kSelectChunk) / 2; ++i) {
            const uint64_t lo = wave_sum((uint64_t)(h[j].v[i] & 0xffffu)), hi = wave_sum((uint64_t)(h[j].v[i] >> 16));
            if (lane == 0) {
                s_wave[j][2 * i] += lo;
                s_wave[j][2 * i + 1] += hi;
            }
            h[j].v[i] = 0;
        }
    }
    // the rows: two groups' 16-bit fields per register, as the buckets
#pragma unroll
    for (int j = 0; j < NG / 2; ++j) {
        const uint64_t lo = wave_sum((uint64_t)(c_rows[j] & 0xffffu)), hi = wave_sum((uint64_t)(c_rows[j] >> 16));
        if (lane == 0) {
            s_wave[2 * j][1 << kSelectChunk] += lo;
            s_wave[2 * j + 1][1 << kSelectChunk] += hi;
        }
        c_rows[j] = 0;
    }
}
// the waves' counters into this workgroup's partials (NG·kSelectSlotCols words at its index)
template <int NG>
__device__ __forceinline__ void select_group_publish(uint64_t (*s_hist)[NG][kSelectSlotCols], int nwaves,
                                                     int64_t* workspace, int t, int threads) {
    __syncthreads();
    constexpr int COLS = NG * (int)kSelectSlotCols;
    const uint64_t* flat = &s_hist[0][0][0];
    for (int i = t; i < COLS; i += threads) {
        uint64_t s = 0;
        for (int w = 0; w < nwaves; ++w) s += flat[w * COLS + i];
        workspace[(uint64_t)COLS * blockIdx.x + i] = (int64_t)s;
    }
}
// the batch's group leaves of pair p: ea[x] (zero past q.n1) and, TWO, eb[0 … 1] (zero past q.n2)
template <int NA, bool TWO, int THREADS>
__device__ __forceinline__ void load_group_leaves(const GroupAggArgs& q, bool whole, uint64_t tile_word0, int p, int t,
                                                  uint64_t n_words, u64x2 (&ea)[NA], u64x2 (&eb)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        eb[b] = u64x2{~0ull, ~0ull};
        if (TWO) {
            eb[b] = u64x2{0ull, 0ull};
            if ((uint32_t)b < q.n2) eb[b] = load_pair<THREADS>(q.e2[b], (q.neg2 >> b) & 1u, whole, tile_word0, p, t, n_words);
        }
    }
#pragma unroll
    for (int x = 0; x < NA; ++x) {
        ea[x] = u64x2{0ull, 0ull};
        if ((uint32_t)x < q.n1) ea[x] = load_pair<THREADS>(q.e1[x], (q.neg1 >> x) & 1u, whole, tile_word0, p, t, n_words);
    }
}

template <int K, int FORM, bool TWO>
__global__ __launch_bounds__(512, 2) void eval_slice_select_grouped(EvalArgs a, SliceSelectArgs g, GroupAggArgs q) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    static_assert(PAIRS == 2, "the pair loop selects between two pairs");
    static_assert(NW * 64 == 256, "the rows of a tile a thread adds to one field (kSelectFoldTiles)");
    constexpr int NWAVES = THREADS / 64;
    constexpr int NG = (int)kGroupBatchSelect, NA = TWO ? NG / 2 : NG, NB = TWO ? 2 : 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ uint64_t s_hist[NWAVES][NG][kSelectSlotCols];
    select_group_zero<NG>(s_hist, NWAVES, t, THREADS);
    static_assert(NG % 2 == 0, "two groups' row counts share a register");
    PackedHist h[NG];
    uint32_t c_rows[NG / 2];  // 16-bit fields, folded with the buckets
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        c_rows[j >> 1] = 0;
#pragma unroll
        for (int i = 0; i < (1 << kSelectChunk) / 2; ++i) h[j].v[i] = 0;
    }
    // The first chunk is taken as kSelectChunk slices from top0 down: it may reach above the index's
    // slices (it holds n_slices mod 4 of them, or none), and a slice that does not exist reads as zero,
    // so the bucket is the chunk's bits all the same.
    const int top0 = (int)select_chunk_low(g.n_slices, kSelectChunk, 0) + (int)kSelectChunk - 1;
    uint32_t since = 0;
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
        // one pair at a time, as eval_slice_aggregate_grouped (p is uniform, so the selects are scalar)
#pragma unroll 1
        for (int p = 0; p < PAIRS; ++p) {
            u64x2 f;
            f.x = p ? r[2] : r[0];
            f.y = p ? r[3] : r[1];
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            if (__ballot((f.x | f.y) != 0) == 0) {  // no qualifying row in the wave's 128 words: no candidate
                reinterpret_cast<u64x2*>(g.cand)[pi] = u64x2{0ull, 0ull};
                continue;
            }
            u64x2 ea[NA], eb[2];
            load_group_leaves<NA, TWO, THREADS>(q, whole, tile_word0, p, t, a.n_words, ea, eb);
            u64x2 vv = {~0ull, ~0ull};
            if (g.validity) vv = load_pair<THREADS>(g.validity, false, whole, tile_word0, p, t, a.n_words);
            // C = ∪_g F ∧ E1_a ∧ E2_b ∧ valid = F ∧ valid ∧ (∪ E1) ∧ (∪ E2)
            u64x2 ua = ea[0];
#pragma unroll
            for (int x = 1; x < NA; ++x) ua |= ea[x];
            if (TWO) ua &= eb[0] | eb[1];
            const u64x2 c = f & vv & ua;
            reinterpret_cast<u64x2*>(g.cand)[pi] = c;  // the tile lies inside the padded candidate words
            const bool none = __ballot((c.x | c.y) != 0) == 0;  // no candidate in the wave's 128 words: no slice is read
            u64x2 w[kSelectChunk];
#pragma unroll
            for (int s = 0; s < (int)kSelectChunk; ++s) {
                w[s] = u64x2{0ull, 0ull};
                if (!none && top0 - s < (int)g.n_slices)
                    w[s] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.slices.s[top0 - s]) + pi);
            }
#pragma unroll
            for (int x = 0; x < NA; ++x) {
#pragma unroll
                for (int y = 0; y < NB; ++y) {
                    const int j = NB * x + y;
                    u64x2 m = f & ea[x] & eb[y];
                    if (__ballot((m.x | m.y) != 0) == 0) continue;  // no row of this group in the wave's 128 words
                    c_rows[j >> 1] += (uint32_t)(__popcll(m.x) + __popcll(m.y)) << (16 * (j & 1));
                    m &= vv;
                    if (__ballot((m.x | m.y) != 0) == 0) continue;
                    select_hist_rec<(int)kSelectChunk, 0, 0>(w, m, (uint32_t)(__popcll(m.x) + __popcll(m.y)), h[j]);
                }
            }
        }
        if (++since == kSelectFoldTiles) {  // uniform: the tile loop is the workgroup's
            select_group_fold<NG>(h, c_rows, s_hist[wave], lane);
            since = 0;
        }
    }
    select_group_fold<NG>(h, c_rows, s_hist[wave], lane);
    select_group_publish<NG>(s_hist, NWAVES, g.workspace, t, THREADS);
}

// PC: the previous chunk's slices (its lowest at prev_low); the next chunk is whole, its lowest slice
// at prev_low - kSelectChunk. a: the tile list of pass 0 (num_tiles, live); q: the batch of pass 0.
template <int PC, bool TWO>
__global__ __launch_bounds__(512, 2) void slice_select_narrow_grouped(EvalArgs a, SliceSelectArgs g, GroupAggArgs q,
                                                                      uint32_t prev_low) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4, NC = (int)kSelectChunk;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(NW * 64 == 256, "the rows of a tile a thread adds to one field (kSelectFoldTiles)");
    constexpr int NWAVES = THREADS / 64;
    constexpr int NG = (int)kGroupBatchSelect, NA = TWO ? NG / 2 : NG, NB = TWO ? 2 : 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ uint64_t s_hist[NWAVES][NG][kSelectSlotCols];
    select_group_zero<NG>(s_hist, NWAVES, t, THREADS);
    PackedHist h[NG];
    uint32_t c_rows[NG / 2];  // (not counted here: the fold adds zeros)
    uint32_t want[NG], alive = 0;  // uniform: each group's bucket of the previous chunk in its low PC bits
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        c_rows[j >> 1] = 0;
#pragma unroll
        for (int i = 0; i < (1 << kSelectChunk) / 2; ++i) h[j].v[i] = 0;
        const SelectState* st = select_group_state(g.workspace, (uint32_t)j);
        want[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(st->prefix >> prev_low));
        if (__builtin_amdgcn_readfirstlane((int)(st->found != 0))) alive |= 1u << j;
    }
    if (alive) {  // uniform; a batch without a found group leaves the candidates and the histograms alone
        const int ptop = (int)prev_low + PC - 1, ntop = (int)prev_low - 1;
        uint32_t since = 0;
        const uint32_t n_idx = a.num_tiles;
        for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
            const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
            const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
#pragma unroll 1
            for (int p = 0; p < PAIRS; ++p) {
                const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
                const u64x2 c = reinterpret_cast<const u64x2*>(g.cand)[pi];
                if (__ballot((c.x | c.y) != 0) == 0) continue;  // no candidate in the wave's 128 words
                u64x2 ea[NA], eb[2], pw[PC], w[NC];
                load_group_leaves<NA, TWO, THREADS>(q, whole, tile_word0, p, t, a.n_words, ea, eb);
#pragma unroll
                for (int s = 0; s < PC; ++s)
                    pw[s] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.slices.s[ptop - s]) + pi);
#pragma unroll
                for (int s = 0; s < NC; ++s)
                    w[s] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.slices.s[ntop - s]) + pi);
                u64x2 keep = {0ull, 0ull};
#pragma unroll
                for (int x = 0; x < NA; ++x) {
#pragma unroll
                    for (int y = 0; y < NB; ++y) {
                        const int j = NB * x + y;
                        if (!((alive >> j) & 1u)) continue;  // uniform: the group has no such row
                        u64x2 m = c & ea[x] & eb[y];
#pragma unroll
                        for (int s = 0; s < PC; ++s) {
                            if ((want[j] >> (PC - 1 - s)) & 1u) m &= pw[s];
                            else m &= ~pw[s];
                        }
                        keep |= m;
                        if (__ballot((m.x | m.y) != 0) == 0) continue;
                        select_hist_rec<NC, 0, 0>(w, m, (uint32_t)(__popcll(m.x) + __popcll(m.y)), h[j]);
                    }
                }
                reinterpret_cast<u64x2*>(g.cand)[pi] = keep;
            }
            if (++since == kSelectFoldTiles) {  // uniform
                select_group_fold<NG>(h, c_rows, s_hist[wave], lane);
                since = 0;
            }
        }
    }
    select_group_fold<NG>(h, c_rows, s_hist[wave], lane);
    select_group_publish<NG>(s_hist, NWAVES, g.workspace, t, THREADS);
}

// The column path's pass: x / valid as select_arrays_kernel reads them, the group columns as
// aggregate_arrays_grouped_kernel's. Every row maps to its slot (group_slot_of); pass 0 counts the
// slot's rows; a valid row whose key ^ 2^63 has the slot's prefix above bit shift + 4 adds one to the
// slot's bucket of bits [shift, shift + 4) — per-(slot, bucket) LDS counters, CUBIT_AGG_MAX_GROUPS × 2^4 of
// 64 bits (32 KB). Rows off their slot's prefix, and rows of a slot whose found is 0, are ignored.
__global__ __launch_bounds__(256) void select_arrays_grouped_kernel(const int64_t* __restrict__ x,
                                                                    const uint64_t* __restrict__ valid,
                                                                    GroupColArgs gc, uint32_t n_groups,
                                                                    const uint64_t* __restrict__ d_count,
                                                                    uint64_t max_n, int type, uint32_t shift, int first,
                                                                    int64_t* __restrict__ workspace) {
    constexpr uint32_t NB = 1u << kSelectGroupArrayBits;
    static_assert(NB + 1 == kSelectSlotCols, "a slot's buckets, then its rows");
    __shared__ unsigned long long s_h[CUBIT_AGG_MAX_GROUPS][kSelectSlotCols];
    __shared__ uint64_t s_prefix[CUBIT_AGG_MAX_GROUPS];
    __shared__ uint32_t s_found[CUBIT_AGG_MAX_GROUPS];
    const uint64_t hi_mask = first ? 0ull : ~0ull << (shift + kSelectGroupArrayBits);
    for (uint32_t s = threadIdx.x; s < n_groups; s += blockDim.x) {
#pragma unroll
        for (uint32_t b = 0; b < kSelectSlotCols; ++b) s_h[s][b] = 0;
        // (the first pass takes every valid row: the states are not set yet)
        const SelectState* st = select_group_state(workspace, s);
        s_prefix[s] = first ? 0ull : st->prefix & hi_mask;
        s_found[s] = first || st->found ? 1u : 0u;
    }
    __syncthreads();
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int s1 = group_slot_of(gc, 0, i);
        const int s2 = gc.n_cols > 1 ? group_slot_of(gc, 1, i) : 0;
        if (s1 < 0 || s2 < 0) continue;
        const uint32_t slot = (uint32_t)s1 * gc.n2 + (uint32_t)s2;
        if (slot >= n_groups) continue;
        if (first) atomicAdd(&s_h[slot][NB], 1ull);
        if (!s_found[slot] || (valid && !((valid[i >> 6] >> (i & 63)) & 1ull))) continue;
        const uint64_t off = (uint64_t)value_key(type, x[i]) ^ 0x8000000000000000ull;
        if ((off & hi_mask) != s_prefix[slot]) continue;
        atomicAdd(&s_h[slot][(uint32_t)(off >> shift) & (NB - 1)], 1ull);
    }
    __syncthreads();
    const uint32_t cols = n_groups * kSelectSlotCols;
    const unsigned long long* flat = &s_h[0][0];
    for (uint32_t c = threadIdx.x; c < cols; c += blockDim.x) workspace[(uint64_t)cols * blockIdx.x + c] = (int64_t)flat[c];
}

// One workgroup after each pass of either path: sums the nblocks partials of n_slots · kSelectSlotCols
// counters — thread t takes column t mod cols of every (1024 / cols)-th workgroup when the columns are
// fewer than the threads, else every 1024-th column of every workgroup, so the loads spread as
// select_step_kernel's — then one thread per slot applies select_step to the slot's state (`first`
// also keeps the slot's rows), and `last` writes select_result to out + 6·group[slot] (q.group; the
// slot itself with identity; kNoGroup: nothing). A slot without a row writes six zeros.
__global__ __launch_bounds__(kSelectStepThreads) void select_step_grouped_kernel(
    int64_t* __restrict__ workspace, int nblocks, uint32_t n_slots, uint32_t low, int first, int last, int mode, uint64_t k,
    double quantile, int type, int64_t base, GroupAggArgs q, int identity, int64_t* __restrict__ out) {
    constexpr uint32_t NB = 1u << kSelectChunk;
    __shared__ uint64_t s_part[kSelectStepThreads];
    __shared__ uint64_t s_counts[CUBIT_AGG_MAX_GROUPS * kSelectSlotCols];
    const uint32_t lane = threadIdx.x, cols = n_slots * kSelectSlotCols;
    if (cols < (uint32_t)kSelectStepThreads) {
        const uint32_t stripes = (uint32_t)kSelectStepThreads / cols, j = lane % cols, s0 = lane / cols;
        uint64_t sum = 0;
        if (s0 < stripes)
            for (uint32_t b = s0; b < (uint32_t)nblocks; b += stripes) sum += (uint64_t)workspace[(uint64_t)cols * b + j];
        s_part[lane] = sum;
        __syncthreads();
        if (lane < cols) {
            uint64_t c = 0;
            for (uint32_t s = 0; s < stripes; ++s) c += s_part[s * cols + lane];
            s_counts[lane] = c;
        }
    } else {
        for (uint32_t j = lane; j < cols; j += (uint32_t)kSelectStepThreads) {
            uint64_t sum = 0;
            for (uint32_t b = 0; b < (uint32_t)nblocks; ++b) sum += (uint64_t)workspace[(uint64_t)cols * b + j];
            s_counts[j] = sum;
        }
    }
    __syncthreads();
    if (lane < n_slots) {
        const uint64_t* counts = s_counts + lane * kSelectSlotCols;
        SelectState* st = select_group_state(workspace, lane);
        SelectState state = *st;
        select_step(&state, first != 0, mode, k, quantile, counts, NB, low);
        *st = state;
        uint64_t* rows = select_group_rows(workspace, lane);
        if (first) *rows = counts[NB];
        const uint32_t group = identity ? lane : q.group[lane < kGroupBatchSum ? lane : 0];
        if (last && group != kNoGroup) {
            int64_t r[6];
            select_result(state, type, base, *rows, r);
#pragma unroll
            for (int i = 0; i < 6; ++i) out[(uint64_t)group * 6 + i] = r[i];
        }
    }
}

// GROUP BY for the sum of a product: eval_slice_sum_product's loop nest per group over a rectangle of
// kProductGroupBatch groups, formed as eval_slice_aggregate_grouped forms them (m = F ∧ E1_a ∧ E2_b,
// the NULL slot the complemented validity; rows counted, then ∧ valid_a ∧ valid_b). The inner group's
// slices stay unmasked in registers; per chunk of kProductGroupChunk outer slices and per live group
// the chunk is masked once (wq = m ∧ w) and every inner slice takes its Horner popcount over it. A
// pair whose F is zero across the wave loads nothing more, one whose groups' valid rows are all zero
// skips the slices, a group whose mask is zero across the wave skips its arithmetic (wave-uniform
// branches). Partials are group-major, kProductGroupPartial words: the ungrouped seven, then the rows.
// Traffic: (K + validities + n_in + n_out·passes + the launch's group leaves)·n/8 bytes per launch.
constexpr int kProductGroupChunk = 4;
__device__ __forceinline__ void product_merge_rows(uint64_t* into, const uint64_t* from) {
    product_merge(into, from);
    into[7] += from[7];
}
template <int K, int FORM, bool TWO>
__global__ __launch_bounds__(512, 2) void eval_slice_sum_product_grouped(EvalArgs a, SliceProductArgs g, GroupAggArgs q) {
    constexpr int THREADS = 512, PAIRS = 2, NW = 4;
    constexpr uint64_t TILE_WORDS = (uint64_t)THREADS * NW;
    static_assert(TILE_WORDS == kAggTileWords, "a tile is one zone");
    static_assert(PAIRS == 2, "the pair loop selects between two pairs");
    constexpr int NWAVES = THREADS / 64;
    constexpr int NG = (int)kProductGroupBatch, NA = TWO ? NG / 2 : NG;
    constexpr int NI = (int)kProductInner, NC = kProductGroupChunk;
    static_assert(NG <= (int)kGroupBatchSum, "GroupAggArgs holds the batch");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    U128 cross[NG], s_out[NG], s_in[NG];
    uint64_t c_valid[NG], c_rows[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        cross[j] = s_out[j] = s_in[j] = U128{0, 0};
        c_valid[j] = c_rows[j] = 0;
    }
    const int n_out = (int)g.n_outer, n_in = (int)g.n_inner;
    const int top0 = (n_out + NC - 1) / NC * NC - 1;
    const uint32_t n_idx = a.num_tiles;
    for (uint32_t i = blockIdx.x; i < n_idx; i += gridDim.x) {
        const uint64_t tile_word0 = (uint64_t)tile_at(a, i) * TILE_WORDS;
        uint64_t r[NW];
        eval_tile<K, FORM, NW, THREADS>(a, tile_word0, t, r);
        const bool whole = tile_word0 + TILE_WORDS <= a.n_words;
#pragma unroll 1
        for (int p = 0; p < PAIRS; ++p) {
            u64x2 f;
            f.x = p ? r[2] : r[0];
            f.y = p ? r[3] : r[1];
            if (__ballot((f.x | f.y) != 0) == 0) continue;  // no qualifying row in the wave's 128 words
            u64x2 m[NG];
            if (TWO) {
                u64x2 eb[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    eb[b] = u64x2{0ull, 0ull};
                    if ((uint32_t)b < q.n2)
                        eb[b] = load_pair<THREADS>(q.e2[b], (q.neg2 >> b) & 1u, whole, tile_word0, p, t, a.n_words);
                }
#pragma unroll
                for (int x = 0; x < NA; ++x) {
                    u64x2 ea = {0ull, 0ull};
                    if ((uint32_t)x < q.n1)
                        ea = f & load_pair<THREADS>(q.e1[x], (q.neg1 >> x) & 1u, whole, tile_word0, p, t, a.n_words);
                    m[2 * x] = ea & eb[0];
                    m[2 * x + 1] = ea & eb[1];
                }
            } else {
#pragma unroll
                for (int x = 0; x < NA; ++x) {
                    m[x] = u64x2{0ull, 0ull};
                    if ((uint32_t)x < q.n1)
                        m[x] = f & load_pair<THREADS>(q.e1[x], (q.neg1 >> x) & 1u, whole, tile_word0, p, t, a.n_words);
                }
            }
            u64x2 vv = {~0ull, ~0ull};
            if (g.valid_a) vv &= load_pair<THREADS>(g.valid_a, false, whole, tile_word0, p, t, a.n_words);
            if (g.valid_b) vv &= load_pair<THREADS>(g.valid_b, false, whole, tile_word0, p, t, a.n_words);
            uint32_t live = 0;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                c_rows[j] += (uint64_t)(__popcll(m[j].x) + __popcll(m[j].y));
                m[j] &= vv;
                c_valid[j] += (uint64_t)(__popcll(m[j].x) + __popcll(m[j].y));
                if (__ballot((m[j].x | m[j].y) != 0) != 0) live |= 1u << j;
            }
            if (live == 0) continue;
            const uint64_t pi = (tile_word0 >> 1) + (uint64_t)(p * THREADS + t);
            int g0 = 0;
            do {
                const int cnt = n_in - g0 < NI ? n_in - g0 : NI;
                u64x2 b[NI];
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    b[j] = u64x2{0ull, 0ull};
                    if (j < cnt) b[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.inner.s[g0 + j]) + pi);
                }
#pragma unroll
                for (int x = 0; x < NG; ++x) {
                    if (!((live >> x) & 1u)) continue;
                    uint32_t li = 0;
#pragma unroll
                    for (int j = 0; j < NI; ++j) li += (uint32_t)(__popcll(m[x].x & b[j].x) + __popcll(m[x].y & b[j].y)) << j;
                    s_in[x] = u128_add(s_in[x], u128_shl_wide(li, (uint32_t)g0));
                }
#pragma unroll 1
                for (int top = top0; top >= 0; top -= NC) {
                    u64x2 w[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        w[c] = u64x2{0ull, 0ull};
                        if (top - c < n_out)
                            w[c] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(g.outer.s[top - c]) + pi);
                    }
                    const uint32_t low = (uint32_t)(top - NC + 1);
#pragma unroll
                    for (int x = 0; x < NG; ++x) {
                        if (!((live >> x) & 1u)) continue;  // no valid row of this group in the wave's 128 words
                        u64x2 wq[NC];
#pragma unroll
                        for (int c = 0; c < NC; ++c) wq[c] = m[x] & w[c];
                        if (g0 == 0) {
                            uint32_t lo = 0;
#pragma unroll
                            for (int c = 0; c < NC; ++c) lo = (lo << 1) + (uint32_t)(__popcll(wq[c].x) + __popcll(wq[c].y));
                            s_out[x] = u128_add(s_out[x], u128_shl(lo, low));
                        }
                        uint32_t comb = 0;
#pragma unroll
                        for (int j = 0; j < NI; ++j) {
                            if (j >= cnt) continue;  // uniform
                            uint32_t l = 0;
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                l = (l << 1) + (uint32_t)(__popcll(b[j].x & wq[c].x) + __popcll(b[j].y & wq[c].y));
                            comb += l << j;
                        }
                        cross[x] = u128_add(cross[x], u128_shl_wide(comb, low + (uint32_t)g0));
                    }
                }
                g0 += NI;
            } while (g0 < n_in);
        }
    }
    // wave, then workgroup, per group
    __shared__ uint64_t s_part[NWAVES][NG][kProductGroupPartial];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        uint64_t part[kProductPartial] = {cross[j].lo, cross[j].hi, s_out[j].lo, s_out[j].hi,
                                          s_in[j].lo,  s_in[j].hi,  c_valid[j]};
        product_wave_reduce(part);
        const uint64_t rows = wave_sum(c_rows[j]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kProductPartial; ++k) s_part[wave][j][k] = part[k];
            s_part[wave][j][7] = rows;
        }
    }
    __syncthreads();
    if (t < NG) {
        for (int w = 1; w < NWAVES; ++w) product_merge_rows(s_part[0][t], s_part[w][t]);
        int64_t* o = q.partials + ((uint64_t)t * gridDim.x + blockIdx.x) * kProductGroupPartial;
#pragma unroll
        for (int k = 0; k < kProductGroupPartial; ++k) o[k] = (int64_t)s_part[0][t][k];
    }
}

// The column path per group: xa / xb = the probed values of qualifying row i (0 at NULL rows), va / vb
// their validity (null: all valid), the group columns as aggregate_arrays_grouped_kernel's. Each valid
// row's 128-bit product goes to its group in LDS as four 32-bit limbs, each added to a 64-bit sum
// that cannot wrap below 2^32 rows a workgroup; Σ_k limb_k·2^(32k) modulo 2^128 is the exact
// two's-complement sum. The partials are the grouped slice kernel's, the sum in the cross slots.
__global__ __launch_bounds__(256) void sum_product_arrays_grouped_kernel(const int64_t* __restrict__ xa,
                                                                         const uint64_t* __restrict__ va,
                                                                         const int64_t* __restrict__ xb,
                                                                         const uint64_t* __restrict__ vb,
                                                                         GroupColArgs gc, uint32_t n_groups,
                                                                         const uint64_t* __restrict__ d_count,
                                                                         uint64_t max_n, int64_t* __restrict__ partials) {
    // per group: {limb 0 … 3, valid rows, rows}
    __shared__ unsigned long long s_acc[CUBIT_AGG_MAX_GROUPS][6];
    const uint64_t n = min(*d_count, max_n);
    for (uint32_t q = threadIdx.x; q < n_groups; q += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_acc[q][k] = 0ull;
    }
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const int s1 = group_slot_of(gc, 0, i);
        const int s2 = gc.n_cols > 1 ? group_slot_of(gc, 1, i) : 0;
        if (s1 < 0 || s2 < 0) continue;
        unsigned long long* acc = s_acc[(uint32_t)s1 * gc.n2 + (uint32_t)s2];
        atomicAdd(&acc[5], 1ull);
        if (va && !((va[i >> 6] >> (i & 63)) & 1ull)) continue;
        if (vb && !((vb[i >> 6] >> (i & 63)) & 1ull)) continue;
        atomicAdd(&acc[4], 1ull);
        const unsigned __int128 pr = (unsigned __int128)((__int128)xa[i] * (__int128)xb[i]);
        const uint64_t lo = (uint64_t)pr, hi = (uint64_t)(pr >> 64);
        atomicAdd(&acc[0], (unsigned long long)(uint32_t)lo);
        atomicAdd(&acc[1], (unsigned long long)(lo >> 32));
        atomicAdd(&acc[2], (unsigned long long)(uint32_t)hi);
        atomicAdd(&acc[3], (unsigned long long)(hi >> 32));
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < n_groups; q += blockDim.x) {
        U128 s{s_acc[q][0], s_acc[q][2]};
        s = u128_add(s, U128{s_acc[q][1] << 32, s_acc[q][1] >> 32});
        s.hi += s_acc[q][3] << 32;
        int64_t* part = partials + ((uint64_t)q * gridDim.x + blockIdx.x) * kProductGroupPartial;
        part[0] = (int64_t)s.lo;
        part[1] = (int64_t)s.hi;
        part[2] = part[3] = part[4] = part[5] = 0;
        part[6] = (int64_t)s_acc[q][4];
        part[7] = (int64_t)s_acc[q][5];
    }
}

// One wave per group (slot) combines the workgroups' partials (slice_product_combine; the column
// path passes zero bases and sums) and writes the group's four result slots {sum_lo, sum_hi,
// count_valid, count_rows}: four zeros for a group without a qualifying row. group: as
// aggregate_grouped_finish_kernel's.
__global__ __launch_bounds__(64) void sum_product_grouped_finish_kernel(const int64_t* __restrict__ partials, int nblocks,
                                                                        GroupAggArgs q, int identity, int64_t base_outer,
                                                                        int64_t base_inner, int64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    const uint32_t slot = blockIdx.x;
    const uint32_t group = identity ? slot : q.group[slot < kGroupBatchSum ? slot : 0];
    if (group == kNoGroup) return;
    uint64_t part[kProductGroupPartial] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = lane; b < nblocks; b += 64)
        product_merge_rows(part, reinterpret_cast<const uint64_t*>(partials) + ((uint64_t)slot * nblocks + b) * kProductGroupPartial);
    uint64_t head[kProductPartial];
#pragma unroll
    for (int k = 0; k < kProductPartial; ++k) head[k] = part[k];
    product_wave_reduce(head);
    const uint64_t rows = wave_sum(part[7]);
    if (lane == 0) {
        int64_t r[2];
        slice_product_combine(base_outer, base_inner, head[6], U128{head[0], head[1]}, U128{head[2], head[3]},
                              U128{head[4], head[5]}, r);
        int64_t* o = out + (uint64_t)group * 4;
        o[0] = r[0];
        o[1] = r[1];
        o[2] = (int64_t)head[6];
        o[3] = (int64_t)rows;
    }
}

// ------------------------------------------------------------------ index build: column stats

// min / max / any-valid of a column (the statistics an index build needs; the reference
// keeps them per segment as BaseStatistics, used by CheckZonemap, row_group.cpp:361-371).
// out[0] = min, out[1] = max (pre-set to INT64_MAX / INT64_MIN), out[2] = valid rows.
template <typename T, int FK = 0>
__global__ __launch_bounds__(256) void column_minmax_kernel(const T* __restrict__ col,
                                                            const uint64_t* __restrict__ validity, uint64_t n,
                                                            int64_t* __restrict__ out) {
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    uint64_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (validity && !((validity[i >> 6] >> (i & 63)) & 1ull)) continue;
        const int64_t v = (int64_t)key_of<FK>(col[i]);
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        ++cnt;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        cnt += __shfl_xor(cnt, d, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicMin(reinterpret_cast<long long*>(out), (long long)mn);
        atomicMax(reinterpret_cast<long long*>(out + 1), (long long)mx);
        atomicAdd(reinterpret_cast<unsigned long long*>(out + 2), (unsigned long long)cnt);
    }
}

// presence bitmap of the valid values: bit (v - vmin) of `bits`. Narrow ranges (≤ 2^16
// values) collect in LDS first so the few global words are OR-ed once per workgroup.
template <typename T, bool LDS, int FK = 0>
__global__ __launch_bounds__(256) void presence_kernel(const T* __restrict__ col, const uint64_t* __restrict__ validity,
                                                       uint64_t n, int64_t vmin, uint64_t range,
                                                       uint64_t* __restrict__ bits) {
    __shared__ uint64_t s_bits[LDS ? 1024 : 1];
    const uint64_t nw = (range + 63) / 64;
    if (LDS) {
        for (uint64_t w = threadIdx.x; w < nw; w += blockDim.x) s_bits[w] = 0;
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (validity && !((validity[i >> 6] >> (i & 63)) & 1ull)) continue;
        const uint64_t off = (uint64_t)((int64_t)key_of<FK>(col[i]) - vmin);
        const uint64_t bit = 1ull << (off & 63);
        if (LDS) {
            if (!(s_bits[off >> 6] & bit)) atomicOr(reinterpret_cast<unsigned long long*>(&s_bits[off >> 6]), bit);
        } else {
            atomicOr(reinterpret_cast<unsigned long long*>(&bits[off >> 6]), bit);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint64_t w = threadIdx.x; w < nw; w += blockDim.x)
            if (s_bits[w]) atomicOr(reinterpret_cast<unsigned long long*>(&bits[w]), s_bits[w]);
    }
}

// ------------------------------------------------------------------ K5: bit-unpack

// One workgroup per DuckDB bitpacking metadata group (BitpackingScanPartial,
// bitpacking.cpp:785-868): CONSTANT, CONSTANT_DELTA (first + i·delta), FOR (unpacked + min)
// and DELTA_FOR (running sum of unpacked + min_delta from delta_offset, a block scan here).
// Packed values are horizontal (fastpforlib fastpack): value i at bits [i·w, (i+1)·w) of
// little-endian 32-bit words. The group's packed words (≤ 2,048·64 bits = 16 KiB) are staged
// in LDS with coalesced loads; thread t then owns the 4-value quads t and t + 256 (values
// 4t..4t+3 and 1024+4t..1024+4t+3), so every wave store is a contiguous 16 B per lane
// (HBM-write-bound: the output is 4–8 B per value, the input w/8). U = unsigned T, the
// reference's wrap-around arithmetic.
constexpr uint32_t kBpMaxWords = 2048 * 64 / 32;  // packed 32-bit words of a 64-bit-wide group

typedef uint32_t bp_u32x4 __attribute__((ext_vector_type(4)));

// The 16-byte-aligned span of a FOR / DELTA_FOR group's packed words (they start 4-aligned; the
// upload pads the bytes by 16): nvec dwordx4 from byte a0, word 0 at s_words[sh]. CONSTANT
// groups have no span.
struct BpSpan {
    uint64_t a0;
    uint32_t sh, nvec;
};
__device__ __forceinline__ BpSpan bp_span(const BpGroup& g) {
    BpSpan sp{0, 0, 0};
    if (g.mode == 4 || g.mode == 5) {
        const uint32_t nwords = (g.count + 31) / 32 * g.width;  // validated on the host against the bytes
        sp.a0 = g.words_off & ~15ull;
        sp.sh = (uint32_t)(g.words_off - sp.a0) / 4;
        sp.nvec = (sp.sh + nwords + 3) / 4;
    }
    return sp;
}

// Unpack one group with 256 threads: thread t produces the 4-value quads t and t + 256 (values
// 4t..4t+3 and 1024+4t..1024+4t+3) and hands each to store_quad(c, v) (c = 0, 1). s_words
// (kBpMaxWords + 8 words, 16-byte aligned) stages the packed words, s_tot holds wave totals.
// STAGED: the caller already landed the group's span in s_words (and synchronised).
template <typename T, typename U, bool STAGED = false, typename Store>
__device__ __forceinline__ void unpack_group(const uint8_t* __restrict__ bytes, const BpGroup& g, uint32_t* s_words,
                                             U* s_tot, Store&& store_quad) {
    constexpr int THREADS = 256, QUADS = 2;
    const int t = threadIdx.x;
    if (g.mode == 2 || g.mode == 3) {  // CONSTANT, CONSTANT_DELTA
        const U base = (U)g.base, d = g.mode == 3 ? (U)g.aux : (U)0;
#pragma unroll
        for (int c = 0; c < QUADS; ++c) {
            U v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = bp_norm<U>((U)(d * (U)(4u * (uint32_t)(t + THREADS * c) + j) + base), g.tnorm);
            store_quad(c, v);
        }
        return;
    }
    const U fr = (U)g.base;
    const uint32_t w = g.width;
    const bool delta = g.mode == 4;
    const U doff = delta ? (U)g.aux : (U)0;
    // packed words start 4-aligned: stage the 16-byte-aligned span that covers them with
    // dwordx4 loads (the upload pads the bytes by 16), word 0 lands at s_words[sh]
    const BpSpan sp = bp_span(g);
    const uint32_t sh = sp.sh;
    if (!STAGED) {
        const bp_u32x4* src = reinterpret_cast<const bp_u32x4*>(bytes + sp.a0);
        bp_u32x4* sw = reinterpret_cast<bp_u32x4*>(s_words);
        for (uint32_t i = t; i < sp.nvec; i += THREADS) sw[i] = __builtin_nontemporal_load(src + i);
        // (a value's window may read one word past its last bit: those bits are masked off)
        __syncthreads();
    }
    U v[QUADS][4];
#pragma unroll
    for (int c = 0; c < QUADS; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = 4u * (uint32_t)(t + THREADS * c) + j;
            uint64_t x = 0;
            if (w && i < g.count) {
                const uint64_t bit = (uint64_t)i * w;
                const uint32_t wi = (uint32_t)(bit >> 5), off = (uint32_t)(bit & 31);
                x = ((uint64_t)s_words[sh + wi] | (uint64_t)s_words[sh + wi + 1] << 32) >> off;
                if (off + w > 64) x |= (uint64_t)s_words[sh + wi + 2] << (64 - off);
                if (w < 64) x &= (1ull << w) - 1;
            }
            v[c][j] = bp_norm<U>((U)x + fr, g.tnorm);
        }
    if (!delta) {
#pragma unroll
        for (int c = 0; c < QUADS; ++c) store_quad(c, v[c]);
        return;
    }
    // DELTA_FOR: inclusive prefix over the group in value order: quad c = 0 covers values
    // 0..1023, c = 1 covers 1024..2047 (carry = the first half's total). Values past count add 0.
    const int lane = t & 63, wave = t >> 6;
    U carry = doff;
#pragma unroll
    for (int c = 0; c < QUADS; ++c) {
        U run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4u * (uint32_t)(t + THREADS * c) + j >= g.count) v[c][j] = 0;
            run += v[c][j];
            v[c][j] = run;
        }
        U incl = run;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const U y = (U)__shfl_up((uint64_t)incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) s_tot[wave] = incl;
        __syncthreads();
        U pre = carry + incl - run, tot = 0;
#pragma unroll
        for (int w2 = 0; w2 < THREADS / 64; ++w2) {
            if (w2 < wave) pre += s_tot[w2];
            tot += s_tot[w2];
        }
        __syncthreads();  // s_tot is rewritten by the next half
        carry += tot;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = bp_norm<U>(v[c][j] + pre, g.tnorm);
        store_quad(c, v[c]);
    }
}

template <typename T, typename U>
__global__ __launch_bounds__(256) void bitunpack_kernel(const uint8_t* __restrict__ bytes,
                                                        const BpGroup* __restrict__ groups, T* __restrict__ out) {
    constexpr int THREADS = 256;
    __shared__ __attribute__((aligned(16))) uint32_t s_words[kBpMaxWords + 8];  // + alignment shift + 3-word window
    __shared__ U s_tot[THREADS / 64];
    const BpGroup g = groups[blockIdx.x];
    const int t = threadIdx.x;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    // 4-byte values leave through a descriptor over dst[0, count) built from SGPRs, as sc1
    // (write-through) 16-byte buffer stores — the store policy the decode's copy-out measured
    // fastest (emit_ids, profiles/r02e_balbench_cache_policy.txt); each store instruction then
    // covers 1 KiB contiguously
    T* dst = out + g.row_start;
    const uintptr_t dp = reinterpret_cast<uintptr_t>(dst);
    const uint64_t db = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(dp >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)dp);
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane(g.count);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)db, (short)0, (int)(cnt * (uint32_t)sizeof(T)), 0x00020000);
    // store quad c of this thread: values 4·(t + 256c) + 0..3
    unpack_group<T, U>(bytes, g, s_words, s_tot, [&](int c, const U (&v)[4]) {
        const uint32_t i0 = 4u * (uint32_t)(t + THREADS * c);
        if (sizeof(T) == 8 && cnt == 2048u) {
            // 8-byte values of a full group (uniform; store_quad runs with every lane active): a
            // wave's 256 values are 2 KiB, lane l owns bytes [32l, 32l + 32). Two lane exchanges
            // make each store instruction cover 1 KiB contiguously — lane l writes wave values
            // 2l, 2l + 1 (from lane l/2) and 128 + 2l, 129 + 2l (from lane 32 + l/2) — so the
            // stores can be sc1 (write-through) without half-line writes
            const int lane = t & 63;
            const bool odd = (lane & 1) != 0;
            const uint32_t wbase = 32u * (uint32_t)(THREADS * c + (t & ~63));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int src = 32 * h + (lane >> 1);
                const unsigned long long e0 = __shfl((unsigned long long)(uint64_t)v[0], src, 64);
                const unsigned long long e1 = __shfl((unsigned long long)(uint64_t)v[1], src, 64);
                const unsigned long long f0 = __shfl((unsigned long long)(uint64_t)v[2], src, 64);
                const unsigned long long f1 = __shfl((unsigned long long)(uint64_t)v[3], src, 64);
                u64x2 o;
                o.x = odd ? f0 : e0;
                o.y = odd ? f1 : e1;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, (int)(wbase + 1024u * h + 16u * lane),
                                                       0, 16);
            }
            return;
        }
        if (i0 + 4 <= cnt) {
            if (sizeof(T) == 4) {
                u32x4 o;
                o.x = (uint32_t)v[0], o.y = (uint32_t)v[1], o.z = (uint32_t)v[2], o.w = (uint32_t)v[3];
                __builtin_amdgcn_raw_buffer_store_b128(o, rs, (int)(i0 * 4u), 0, 16);
            } else {
                // 8-byte values of a partial group: a lane's quad is 32 bytes, so each store
                // instruction covers every other 16 bytes; write-through (sc1) of those half lines
                // measured 3.3 ms instead of 1.0 ms for l_discount, so these stay plain
                u64x2 o0, o1;
                o0.x = (uint64_t)v[0], o0.y = (uint64_t)v[1], o1.x = (uint64_t)v[2], o1.y = (uint64_t)v[3];
                reinterpret_cast<u64x2*>(dst + i0)[0] = o0;
                reinterpret_cast<u64x2*>(dst + i0)[1] = o1;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= cnt) continue;
                if (sizeof(T) == 4)
                    __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v[j], rs, (int)((i0 + j) * 4u), 0, 16);
                else
                    dst[i0 + j] = (T)v[j];
            }
        }
    });
}

// Filter straight from DuckDB BITPACKING segments (the reference's ColumnSegment::Scan →
// BitpackingScanPartial → ColumnSegment::FilterSelection chain, column_segment.cpp:378-522 /
// bitpacking.cpp:779-868, for one constant comparison). The comparison arrives as an inclusive
// range: p = (lo <= v <= hi) XOR neg (the host maps = != < <= > >= and between onto it, clamped
// to T), so testing a value is branch-free. A workgroup takes GPW consecutive groups and lands
// every group's header and packed span in LDS at once, so one load round trip covers GPW
// groups (a group is ~3 KB at 12 bits per value: one group per workgroup waited on its round
// trip). Then, group by group (not unrolled: the code stays small enough for the instruction
// cache — the fully unrolled version ran 18,800 instructions and a quarter of the bandwidth),
// thread t tests values t, t + 256, …, so a wave's 64 consecutive values are one ballot = one
// 64-row bitvector word. A FOR value of ≤ 32 bits comes straight from the staged words (one
// funnel shift); DELTA_FOR and wider FOR groups are unpacked into LDS values first, as
// bitunpack_kernel does. NULL rows never pass (validity, optional). Words wholly inside the
// group are stored; a word a group shares with its neighbour (a group whose rows do not start
// or end on a 64-row boundary) is OR-ed atomically, so `out` must be zero beforehand. Reads
// w/8 bytes per row instead of the plain column's sizeof(T).
template <typename T, typename U, int GPW>
__global__ __launch_bounds__(256) void bitpacked_compare_kernel(const uint8_t* __restrict__ bytes,
                                                                const BpGroup* __restrict__ groups, uint32_t n_groups,
                                                                const uint64_t* __restrict__ validity, T lo, T hi,
                                                                int neg, uint64_t* __restrict__ out) {
    constexpr int THREADS = 256;
    // a group's span: ≤ 2,048·8·sizeof(T) bits + the alignment shift + a 3-word read window
    constexpr uint32_t SPANW = 2048u * 8u * (uint32_t)sizeof(T) / 32u + 8u;
    constexpr int VECS = (int)((SPANW / 4 + THREADS - 1) / THREADS);
    static_assert(sizeof(BpGroup) % 4 == 0, "headers copied as words");
    constexpr int HDRW = (int)(sizeof(BpGroup) / 4);
    __shared__ __attribute__((aligned(16))) uint32_t s_words[GPW][SPANW];
    __shared__ __attribute__((aligned(16))) T s_vals[2048];
    __shared__ U s_tot[THREADS / 64];
    __shared__ BpGroup s_hdr[GPW];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const uint32_t wave_u = __builtin_amdgcn_readfirstlane((uint32_t)(t >> 6));
    const uint32_t g0 = blockIdx.x * (uint32_t)GPW;
    const uint32_t ng = min((uint32_t)GPW, n_groups - g0);
    // headers (as words) and spans: every load issued before any lands
    {
        const uint32_t* hsrc = reinterpret_cast<const uint32_t*>(groups + g0);
        uint32_t hw = 0;
        if (t < (int)(ng * HDRW)) hw = hsrc[t];
        BpGroup hg[GPW];
        bp_u32x4 pf[GPW][VECS];
#pragma unroll
        for (int q = 0; q < GPW; ++q) {
            if ((uint32_t)q < ng) {
                hg[q] = groups[g0 + q];
                const BpSpan sp = bp_span(hg[q]);
                const bp_u32x4* src = reinterpret_cast<const bp_u32x4*>(bytes + sp.a0);
#pragma unroll
                for (int k = 0; k < VECS; ++k) {
                    const uint32_t i = (uint32_t)(t + THREADS * k);
                    if (i < sp.nvec) pf[q][k] = src[i];
                }
            }
        }
        if (t < (int)(ng * HDRW)) reinterpret_cast<uint32_t*>(s_hdr)[t] = hw;
#pragma unroll
        for (int q = 0; q < GPW; ++q) {
            if ((uint32_t)q < ng) {
                const BpSpan sp = bp_span(hg[q]);
                bp_u32x4* sw = reinterpret_cast<bp_u32x4*>(s_words[q]);
#pragma unroll
                for (int k = 0; k < VECS; ++k) {
                    const uint32_t i = (uint32_t)(t + THREADS * k);
                    if (i < sp.nvec) sw[i] = pf[q][k];
                }
            }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t q = 0; q < ng; ++q) {
        const BpGroup cur = s_hdr[q];
        const uint32_t* W = s_words[q];
        const uint64_t end = cur.row_start + cur.count;
        // test values t, t + 256, …: the chunk's first value and row are wave-uniform
        auto test_and_store = [&](auto&& value_of) {
#pragma unroll 1
            for (uint32_t i0 = 64u * wave_u; i0 < cur.count; i0 += 256u) {
                const uint32_t i = i0 + (uint32_t)lane;
                bool p = false;
                if (i < cur.count) {
                    const T v = value_of(i);
                    p = ((v >= lo) & (v <= hi)) != (neg != 0);
                    if (validity) {
                        const uint64_t r = cur.row_start + i;
                        p = p && ((validity[r >> 6] >> (r & 63)) & 1ull);
                    }
                }
                const uint64_t bits = __ballot(p);
                const uint64_t r0 = cur.row_start + i0;  // row of bit 0 (uniform)
                const uint32_t sh = (uint32_t)(r0 & 63);
                const uint64_t w0 = r0 >> 6;
                if (lane == 0) {
                    if (sh == 0) {
                        if (r0 + 64 <= end) out[w0] = bits;  // only this group's rows
                        else atomicOr(reinterpret_cast<unsigned long long*>(&out[w0]), (unsigned long long)bits);
                    } else {
                        atomicOr(reinterpret_cast<unsigned long long*>(&out[w0]), (unsigned long long)(bits << sh));
                        const uint64_t hi2 = bits >> (64 - sh);
                        if (hi2) atomicOr(reinterpret_cast<unsigned long long*>(&out[w0 + 1]), (unsigned long long)hi2);
                    }
                }
            }
        };
        if (cur.mode == 5 && cur.width <= 32) {
            // FOR, w ≤ 32: one funnel shift of the two words a value's bits span, a mask, the
            // frame of reference
            const uint32_t w = cur.width, sh = bp_span(cur).sh;
            const uint32_t mask = w == 32 ? ~0u : (1u << w) - 1u;
            const U fr = (U)cur.base;
            test_and_store([&](uint32_t i) -> T {
                const uint32_t bit = i * w, wi = sh + (bit >> 5);  // i·w < 2^16
                const uint32_t x = __builtin_amdgcn_alignbit(W[wi + 1], W[wi], bit & 31) & mask;
                return (T)bp_norm<U>((U)x + fr, cur.tnorm);
            });
        } else if (cur.mode == 2 || cur.mode == 3) {  // CONSTANT, CONSTANT_DELTA: no packed words
            const U base = (U)cur.base, d = cur.mode == 3 ? (U)cur.aux : (U)0;
            test_and_store([&](uint32_t i) -> T { return (T)bp_norm<U>(d * (U)i + base, cur.tnorm); });
        } else {
            // DELTA_FOR (a running sum) or FOR wider than 32 bits: unpack into LDS values first
            unpack_group<T, U, true>(bytes, cur, const_cast<uint32_t*>(W), s_tot, [&](int qq, const U (&v)[4]) {
                const uint32_t i0 = 4u * (uint32_t)(t + THREADS * qq);
                if (sizeof(T) == 4) {
                    bp_u32x4 o;
                    o.x = (uint32_t)v[0], o.y = (uint32_t)v[1], o.z = (uint32_t)v[2], o.w = (uint32_t)v[3];
                    *reinterpret_cast<bp_u32x4*>(&s_vals[i0]) = o;
                } else {
                    u64x2 o0, o1;
                    o0.x = (uint64_t)v[0], o0.y = (uint64_t)v[1], o1.x = (uint64_t)v[2], o1.y = (uint64_t)v[3];
                    reinterpret_cast<u64x2*>(&s_vals[i0])[0] = o0;
                    reinterpret_cast<u64x2*>(&s_vals[i0])[1] = o1;
                }
            });
            __syncthreads();  // values complete
            test_and_store([&](uint32_t i) -> T { return s_vals[i]; });
            __syncthreads();  // s_vals free for the next group
        }
    }
}

// One group's 64-row output words from its values (a FOR group's packed words staged in L,
// CONSTANT / CONSTANT_DELTA from its record): 64 values per step, each lane taking its value's
// bits from the staged words with one funnel shift, one ballot per step = one output word
// (bitpacked_compare_waves).
template <typename T, typename U>
__device__ __forceinline__ void compare_group_words(const BpGroup& cur, const uint32_t* L, bool packed, uint32_t w,
                                                    uint32_t mask, int lane, const uint64_t* __restrict__ validity,
                                                    T lo, T hi, int neg, uint64_t* __restrict__ out) {
    const uint64_t end = cur.row_start + cur.count;
    const U base = (U)cur.base, d = cur.mode == 3 ? (U)cur.aux : (U)0;
    const uint32_t nchunks = (cur.count + 63u) / 64u;  // ≤ 32
    // a group starting on a 64-row boundary keeps step c's word in lane c and stores the words
    // together at the end (one coalesced store; 8-byte stores from lane 0, one per step, cost
    // more than the whole read); other groups store or OR each word as it is made
    const bool aligned = (cur.row_start & 63) == 0;
    uint64_t myword = 0;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t i = c * 64u + (uint32_t)lane;
        bool p = false;
        if (i < cur.count) {
            T v;
            if (packed) {
                const uint32_t bit = i * w, wi = bit >> 5;  // i·w < 2^16
                v = (T)bp_norm<U>((U)(__builtin_amdgcn_alignbit(L[wi + 1], L[wi], bit & 31) & mask) + base, cur.tnorm);
            } else {
                v = (T)bp_norm<U>(d * (U)i + base, cur.tnorm);
            }
            p = ((v >= lo) & (v <= hi)) != (neg != 0);
            if (validity) {
                const uint64_t r = cur.row_start + i;
                p = p && ((validity[r >> 6] >> (r & 63)) & 1ull);
            }
        }
        const uint64_t bits = __ballot(p);
        if (aligned) {
            if ((uint32_t)lane == c) myword = bits;
            continue;
        }
        const uint64_t r0 = cur.row_start + 64ull * c;  // row of bit 0 (uniform)
        const uint32_t sh = (uint32_t)(r0 & 63);
        const uint64_t w0 = r0 >> 6;
        if (lane == 0) {
            if (sh == 0) {
                if (r0 + 64 <= end) out[w0] = bits;  // only this group's rows
                else atomicOr(reinterpret_cast<unsigned long long*>(&out[w0]), (unsigned long long)bits);
            } else {
                atomicOr(reinterpret_cast<unsigned long long*>(&out[w0]), (unsigned long long)(bits << sh));
                const uint64_t hi2 = bits >> (64 - sh);
                if (hi2) atomicOr(reinterpret_cast<unsigned long long*>(&out[w0 + 1]), (unsigned long long)hi2);
            }
        }
    }
    if (aligned && (uint32_t)lane < nchunks) {
        const uint64_t r0 = cur.row_start + 64ull * (uint32_t)lane;
        if (r0 + 64 <= end) out[r0 >> 6] = myword;  // only this group's rows
        else atomicOr(reinterpret_cast<unsigned long long*>(&out[r0 >> 6]), (unsigned long long)myword);
    }
}

// The same filter for columns whose groups are all FOR of ≤ MAXW bits (MAXW ≤ 32), CONSTANT or
// CONSTANT_DELTA (the modes DuckDB's AUTO picks for unsorted integer columns): one wave per group.
// The wave lands its group's packed words in its own LDS slice with coalesced 256-byte loads — all
// of them in flight at once (≤ MAXW per lane), one round trip per group — then tests 64 values per
// step, each lane taking its value's bits from the staged words with one funnel shift. One ballot
// per step = one 64-row output word, stored (or OR-ed where a group's rows share the word with a
// neighbour) by lane 0, as in bitpacked_compare_kernel. Measured before (profiles/r03w_*): the
// same wave layout loading each value's two words from global memory, eight 64-value steps in
// flight: 0.650 ms for a 600 M-row 12-bit column (the LDS kernel above 0.93 ms, K0 0.43 ms).
template <typename T, typename U, int MAXW>
__global__ __launch_bounds__(256) void bitpacked_compare_waves(const uint8_t* __restrict__ bytes,
                                                               const BpGroup* __restrict__ groups, uint32_t n_groups,
                                                               const uint64_t* __restrict__ validity, T lo, T hi,
                                                               int neg, uint64_t* __restrict__ out) {
    static_assert(MAXW >= 1 && MAXW <= 32, "FOR groups of at most 32 bits");
    constexpr uint32_t SLICE = 64u * MAXW + 4u;  // a group's words (2,048·w/32) + the read window
    __shared__ uint32_t s_w[4][SLICE];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.x * 4u + wave;
    if (g >= n_groups) return;  // no workgroup barrier below: each wave works alone
    uint32_t* L = s_w[wave];
    const BpGroup cur = groups[g];
    const bool packed = cur.mode == 5 && cur.width;
    const uint32_t w = packed ? cur.width : 0u;
    const uint32_t mask = w >= 32 ? ~0u : (1u << w) - 1u;
    const uint32_t nwords = packed ? (cur.count + 31u) / 32u * w : 0u;  // ≤ 64·MAXW (host-checked)
    if (packed) {
        const uint32_t* W = reinterpret_cast<const uint32_t*>(bytes + cur.words_off);
        uint32_t x[MAXW];
#pragma unroll
        for (int m = 0; m < MAXW; ++m) {
            const uint32_t k = 64u * (uint32_t)m + (uint32_t)lane;
            x[m] = k < nwords ? __builtin_nontemporal_load(W + k) : 0u;
        }
#pragma unroll
        for (int m = 0; m < MAXW; ++m) L[64u * (uint32_t)m + (uint32_t)lane] = x[m];
        if (lane < 4) L[64u * MAXW + (uint32_t)lane] = 0u;
        // the wave's own LDS writes, read back by other lanes of the same wave: LDS operations of a
        // wave complete in order, so only the compiler must not move the reads above the writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    }
    compare_group_words<T, U>(cur, L, packed, w, mask, lane, validity, lo, hi, neg, out);
}

// ------------------------------------------------------------------ transfer compaction

// out[i] = (int32)(in[i] - offset) for i < min(*d_count, max_n): the DataChunk column of a
// window crosses PCIe at 4 bytes per row when every value of the column lies within 2^31 of the
// offset (the host mirror widens while it fills the chunk). 16-byte loads, 8-byte stores.
// (overflow, optional: set to 1 when some value - offset lies outside int32 — the caller's bound
// did not hold and the compacted copy must not be used)
__global__ __launch_bounds__(256) void narrow_i32_kernel(const int64_t* __restrict__ in, const uint64_t* __restrict__ d_count,
                                                          uint64_t max_n, int64_t offset, int32_t* __restrict__ out,
                                                          uint32_t* __restrict__ overflow) {
    const uint64_t n = min(*d_count, max_n);
    auto fits = [](int64_t d) { return d >= INT32_MIN && d <= INT32_MAX; };
    bool bad = false;
    for (uint64_t i = 2 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 2ull * gridDim.x * blockDim.x) {
        if (i + 1 < n) {
            const u64x2 v = *reinterpret_cast<const u64x2*>(in + i);
            const int64_t dx = (int64_t)((uint64_t)v.x - (uint64_t)offset), dy = (int64_t)((uint64_t)v.y - (uint64_t)offset);
            bad |= !fits(dx) || !fits(dy);
            typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
            i32x2 o;
            o.x = (int32_t)dx;
            o.y = (int32_t)dy;
            *reinterpret_cast<i32x2*>(out + i) = o;
        } else {
            const int64_t d = (int64_t)((uint64_t)in[i] - (uint64_t)offset);
            bad |= !fits(d);
            out[i] = (int32_t)d;
        }
    }
    if (overflow && bad) *overflow = 1u;
}

// Transfer compaction to 1, 2 or 4 bytes: out[i] = (O)(in[i] - offset) as an unsigned O, for a
// column whose values lie in [offset, offset + 2^(8·sizeof O)); `overflow` set when one does not.
// 8 values per thread per step: four 16-byte loads, and the 8 narrowed values packed into one
// 8-byte (bytes), one 16-byte (halves) or two 16-byte (words) stores, so a wave's store covers
// 512 B – 2 KB contiguously — the shape that matters when `out` is page-locked host memory
// written across PCIe (a wave of scattered 1-byte stores ran the link at ~3 GB/s). `in` and
// `out` 16-byte aligned (launch_narrow_unsigned falls back to the scalar form otherwise).
template <typename O>
__global__ __launch_bounds__(256) void narrow_unsigned_kernel(const int64_t* __restrict__ in,
                                                              const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                              int64_t offset, O* __restrict__ out,
                                                              uint32_t* __restrict__ overflow) {
    const uint64_t n = min(*d_count, max_n);
    constexpr uint64_t kMax = sizeof(O) == 4 ? 0xffffffffull : (1ull << (8 * sizeof(O))) - 1;
    bool bad = false;
    for (uint64_t i = 8 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 8ull * gridDim.x * blockDim.x) {
        if (i + 8 <= n) {
            const ulonglong2* src = reinterpret_cast<const ulonglong2*>(in + i);
            uint64_t d[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const ulonglong2 v = src[j];
                d[2 * j] = v.x - (uint64_t)offset;
                d[2 * j + 1] = v.y - (uint64_t)offset;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) bad |= d[j] > kMax;
            if constexpr (sizeof(O) == 1) {
                uint64_t p = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) p |= (d[j] & 0xff) << (8 * j);
                *reinterpret_cast<uint64_t*>(out + i) = p;
            } else if constexpr (sizeof(O) == 2) {
                ulonglong2 p{0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p.x |= (d[j] & 0xffff) << (16 * j);
                    p.y |= (d[4 + j] & 0xffff) << (16 * j);
                }
                *reinterpret_cast<ulonglong2*>(out + i) = p;
            } else {
                ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + i);
                dst[0] = ulonglong2{(d[0] & 0xffffffffull) | (d[1] << 32), (d[2] & 0xffffffffull) | (d[3] << 32)};
                dst[1] = ulonglong2{(d[4] & 0xffffffffull) | (d[5] << 32), (d[6] & 0xffffffffull) | (d[7] << 32)};
            }
        } else {
            for (uint64_t k = i; k < n; ++k) {
                const uint64_t d = (uint64_t)in[k] - (uint64_t)offset;
                bad |= d > kMax;
                out[k] = (O)d;
            }
        }
    }
    if (overflow && bad) *overflow = 1u;
}

// Three bytes per value (a column whose range spans < 2^24, e.g. l_extendedprice in cents):
// value k of the output at bytes [3k, 3k + 3), little-endian. 8 values per thread per step,
// packed into three 8-byte stores (a wave's 1.5 KB contiguous). `in` 16-byte and `out` 8-byte
// aligned (launch_narrow_unsigned falls back to byte stores otherwise).
__global__ __launch_bounds__(256) void narrow_u24_kernel(const int64_t* __restrict__ in,
                                                         const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                         int64_t offset, uint8_t* __restrict__ out,
                                                         uint32_t* __restrict__ overflow) {
    const uint64_t n = min(*d_count, max_n);
    constexpr uint64_t kMax = (1ull << 24) - 1;
    bool bad = false;
    for (uint64_t i = 8 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += 8ull * gridDim.x * blockDim.x) {
        if (i + 8 <= n) {
            const ulonglong2* src = reinterpret_cast<const ulonglong2*>(in + i);
            uint64_t d[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const ulonglong2 v = src[j];
                d[2 * j] = v.x - (uint64_t)offset;
                d[2 * j + 1] = v.y - (uint64_t)offset;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bad |= d[j] > kMax;
                d[j] &= kMax;
            }
            uint64_t* dst = reinterpret_cast<uint64_t*>(out + 3 * i);
            dst[0] = d[0] | (d[1] << 24) | (d[2] << 48);
            dst[1] = (d[2] >> 16) | (d[3] << 8) | (d[4] << 32) | (d[5] << 56);
            dst[2] = (d[5] >> 8) | (d[6] << 16) | (d[7] << 40);
        } else {
            for (uint64_t k = i; k < n; ++k) {
                const uint64_t d = (uint64_t)in[k] - (uint64_t)offset;
                bad |= d > kMax;
                out[3 * k] = (uint8_t)d;
                out[3 * k + 1] = (uint8_t)(d >> 8);
                out[3 * k + 2] = (uint8_t)(d >> 16);
            }
        }
    }
    if (overflow && bad) *overflow = 1u;
}

__global__ __launch_bounds__(256) void narrow_u24_scalar_kernel(const int64_t* __restrict__ in,
                                                                const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                                int64_t offset, uint8_t* __restrict__ out,
                                                                uint32_t* __restrict__ overflow) {
    const uint64_t n = min(*d_count, max_n);
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t d = (uint64_t)in[i] - (uint64_t)offset;
        bad |= d > 0xffffffull;
        out[3 * i] = (uint8_t)d;
        out[3 * i + 1] = (uint8_t)(d >> 8);
        out[3 * i + 2] = (uint8_t)(d >> 16);
    }
    if (overflow && bad) *overflow = 1u;
}

// The same for operands of any alignment: one value per store.
template <typename O>
__global__ __launch_bounds__(256) void narrow_unsigned_scalar_kernel(const int64_t* __restrict__ in,
                                                                     const uint64_t* __restrict__ d_count,
                                                                     uint64_t max_n, int64_t offset, O* __restrict__ out,
                                                                     uint32_t* __restrict__ overflow) {
    const uint64_t n = min(*d_count, max_n);
    constexpr uint64_t kMax = sizeof(O) == 4 ? 0xffffffffull : (1ull << (8 * sizeof(O))) - 1;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t d = (uint64_t)in[i] - (uint64_t)offset;
        bad |= d > kMax;
        out[i] = (O)d;
    }
    if (overflow && bad) *overflow = 1u;
}

// out[i] = in[i] widened: a column registered with a narrower or unsigned type code
// (cubit_table_add_column) is held as INT32 / INT64 values. 4 values per thread per step.
template <typename S, typename D>
__global__ __launch_bounds__(256) void widen_kernel(const S* __restrict__ in, uint64_t n, D* __restrict__ out) {
    const uint64_t stride = 4ull * gridDim.x * blockDim.x;
    for (uint64_t i = 4ull * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += stride) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < n) out[i + j] = (D)in[i + j];
    }
}

// ------------------------------------------------------------------ FLOAT / DOUBLE keys

// A FLOAT / DOUBLE column is held twice: its bit patterns (probes) and their comparison keys
// (key_of<FK>), which every compare kernel reads as a plain INT32 / INT64 column — the per-value key
// in the compare loop made K0 instruction-bound (FLOAT 0.71 ms vs INT32 0.39 ms at 600 M rows).
// One streaming pass, 16-byte loads and stores.
template <int FK, typename T>
__global__ __launch_bounds__(256) void fp_keys_kernel(const T* __restrict__ raw, uint64_t n, T* __restrict__ keys) {
    constexpr int PER = 16 / sizeof(T);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * PER;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * PER; i < n; i += stride) {
        if (i + PER <= n && (reinterpret_cast<uintptr_t>(raw + i) % 16) == 0 && (reinterpret_cast<uintptr_t>(keys + i) % 16) == 0) {
            u64x2 q = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(raw + i));
            T v[PER];
            __builtin_memcpy(v, &q, 16);
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = key_of<FK>(v[k]);
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<u64x2*>(keys + i) = q;
        } else {
            for (uint64_t k = i; k < n && k < i + PER; ++k) keys[k] = key_of<FK>(raw[k]);
        }
    }
}

// out[i] = value_key(type, v[i]): update values (bit patterns) as the keys a merge compares and
// writes into the key column
__global__ __launch_bounds__(256) void value_keys_kernel(const int64_t* __restrict__ v, uint64_t n, int type,
                                                         int64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = value_key(type, v[i]);
}

// raw[rows[i]] = the merged record's bit pattern (0 for a NULL record): the pattern column beside the
// keys a merge rewrote
__global__ __launch_bounds__(256) void scatter_raw_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ v,
                                                          const uint8_t* __restrict__ valids, uint64_t m, int is32,
                                                          void* __restrict__ raw) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int64_t x = (!valids || valids[i]) ? v[i] : 0;
        if (is32) static_cast<int32_t*>(raw)[rows[i]] = (int32_t)x;
        else static_cast<int64_t*>(raw)[rows[i]] = x;
    }
}

// ------------------------------------------------------------------ K3: probe

template <typename T>
__global__ __launch_bounds__(256) void gather_kernel(const T* __restrict__ col, const int64_t* __restrict__ rowids,
                                                     const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                     int64_t row_base, int64_t* __restrict__ out) {
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (int64_t)__builtin_nontemporal_load(col + (__builtin_nontemporal_load(rowids + i) - row_base));
}

// K3 with NULL-ness (ColumnData::FilterScan + Vector::Slice carry the vector's validity with
// its values, column_data.cpp:305-309, vector.cpp:223-258): out[i] = col[r] for a valid row and
// 0 for a NULL one, and bit i of out_valid (LSB-first words over output positions — DuckDB's
// ValidityMask layout) says whether row r is valid. A wave takes 64 consecutive positions, so
// one ballot forms each word and lane 0 stores it: 1 bit per row beside the 8-byte value.
template <typename T>
__global__ __launch_bounds__(256) void gather_valid_kernel(const T* __restrict__ col,
                                                           const uint64_t* __restrict__ validity,
                                                           const int64_t* __restrict__ rowids,
                                                           const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                           int64_t row_base, int64_t* __restrict__ out,
                                                           uint64_t* __restrict__ out_valid) {
    const uint64_t n = min(*d_count, max_n);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // the loop bound is the wave's first position: every lane of a wave runs the ballot together
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + lane;
        bool ok = false;
        if (i < n) {
            const int64_t r = __builtin_nontemporal_load(rowids + i) - row_base;
            ok = !validity || ((validity[r >> 6] >> (r & 63)) & 1ull);
            out[i] = ok ? (int64_t)__builtin_nontemporal_load(col + r) : 0;
        }
        const uint64_t word = __ballot(ok);
        if (lane == 0) out_valid[base >> 6] = word;
    }
}

__global__ __launch_bounds__(256) void gather_sum_product_kernel(const int64_t* __restrict__ x,
                                                                 const int64_t* __restrict__ y,
                                                                 const int64_t* __restrict__ rowids,
                                                                 const uint64_t* __restrict__ d_count, uint64_t max_n,
                                                                 int64_t row_base, int64_t* __restrict__ partials) {
    __shared__ __int128 s_part[4];
    const uint64_t n = min(*d_count, max_n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    __int128 acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = __builtin_nontemporal_load(rowids + i) - row_base;
        acc += (__int128)__builtin_nontemporal_load(x + r) * (__int128)__builtin_nontemporal_load(y + r);
    }
    // wave reduce on the two halves
    uint64_t lo = (uint64_t)acc;
    int64_t hi = (int64_t)(acc >> 64);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t olo = __shfl_xor(lo, d, 64);
        const int64_t ohi = __shfl_xor(hi, d, 64);
        const uint64_t nlo = lo + olo;
        hi = hi + ohi + (nlo < lo ? 1 : 0);
        lo = nlo;
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ((__int128)hi << 64) | lo;
    __syncthreads();
    if (threadIdx.x == 0) {
        __int128 s = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        partials[2 * blockIdx.x] = (int64_t)(uint64_t)s;
        partials[2 * blockIdx.x + 1] = (int64_t)(s >> 64);
    }
}

// Σ of the per-workgroup 128-bit partials: every lane of one wave sums a strided share (its
// loads independent, so they overlap), then a 64-lane butterfly adds the 128-bit values as
// (lo, hi) pairs with carry. (One lane walking 1,024 partials serially took ~80 µs.)
__global__ __launch_bounds__(64) void sum_partials_kernel(const int64_t* __restrict__ partials, int nblocks,
                                                          int64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    __int128 s = 0;
    for (int b = lane; b < nblocks; b += 64)
        s += ((__int128)partials[2 * b + 1] << 64) | (unsigned __int128)(uint64_t)partials[2 * b];
    uint64_t lo = (uint64_t)s;
    int64_t hi = (int64_t)(s >> 64);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t olo = __shfl_xor(lo, d, 64);
        const int64_t ohi = __shfl_xor(hi, d, 64);
        const uint64_t nlo = lo + olo;
        hi = (int64_t)((uint64_t)hi + (uint64_t)ohi + (nlo < lo ? 1u : 0u));
        lo = nlo;
    }
    if (lane == 0) {
        out[0] = (int64_t)lo;
        out[1] = hi;
    }
}

// ------------------------------------------------------------------ zonemaps

// Zone classes of a bitvector (the bitmap form of a segment's min/max statistics,
// NumericStats::CheckZonemap, numeric_stats.cpp:157-228): one workgroup per zone of kZoneWords
// words, each thread ANDs and ORs 8 words (4 coalesced 16-byte loads). Only rows < n_rows count:
// words past the last row are skipped, the last word is masked. out[z - z0] bit 0 = no row set,
// bit 1 = every row set (both for a zone past the last row).
// Zone class of one bitvector per zone (bit 0: no row set, bit 1: every row set) and, with
// cnt, the zone's set rows — the per-tile counts a single-leaf decode takes its output offsets
// from (eval_decode_lookback with EvalArgs::tile_prefix).
__global__ __launch_bounds__(256) void zone_class_kernel(const uint64_t* __restrict__ bv, uint64_t n_rows,
                                                         uint32_t z0, uint8_t* __restrict__ out,
                                                         uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t z = z0 + blockIdx.x;
    const int t = threadIdx.x;
    const uint64_t n_words = (n_rows + 63) / 64;
    const uint64_t last_mask = (n_rows & 63) ? (1ull << (n_rows & 63)) - 1 : ~0ull;
    uint64_t all = ~0ull, any = 0;
    uint32_t ones = 0;
    const uint64_t w0 = (uint64_t)z * kZoneWords;
#pragma unroll
    for (int p = 0; p < (int)(kZoneWords / 512); ++p) {
        const uint64_t gw = w0 + (uint64_t)(p * 256 + t) * 2;
        if (gw >= n_words) continue;
        const u64x2 x = reinterpret_cast<const u64x2*>(bv + w0)[p * 256 + t];
        uint64_t a = x.x, b = x.y;
        uint64_t ma = gw == n_words - 1 ? last_mask : ~0ull;
        if (gw + 1 >= n_words) {  // b is past the last row (or a is the last word)
            all &= a | ~ma;
            any |= a & ma;
            ones += (uint32_t)__popcll(a & ma);
            continue;
        }
        const uint64_t mb = gw + 1 == n_words - 1 ? last_mask : ~0ull;
        all &= (a | ~ma) & (b | ~mb);
        any |= (a & ma) | (b & mb);
        ones += (uint32_t)(__popcll(a & ma) + __popcll(b & mb));
    }
    const uint32_t wsum = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan32(ones), 63);
    if ((t & 63) == 0) s_cnt[t >> 6] = wsum;
    const int none_set = __syncthreads_and(any == 0);
    const int all_set = __syncthreads_and(all == ~0ull);
    if (t == 0) {
        out[blockIdx.x] = (uint8_t)((none_set ? 1 : 0) | (all_set ? 2 : 0));
        if (cnt) cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

// Per-zone statistics of a raw column (the segment statistics CheckZonemap consults,
// numeric_stats.cpp:157-228): min / max over the zone's valid rows and whether any / every row
// is valid. One workgroup per zone; consecutive threads read consecutive 4-row chunks.
template <typename T, int FK = 0>
__global__ __launch_bounds__(256) void column_zone_stats_kernel(const T* __restrict__ col,
                                                                const uint64_t* __restrict__ validity, uint64_t n_rows,
                                                                int64_t* __restrict__ mn, int64_t* __restrict__ mx,
                                                                uint8_t* __restrict__ fl) {
    __shared__ int64_t s_lo[256], s_hi[256];
    __shared__ uint32_t s_n[256];
    const int t = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * kZoneRows;
    const uint64_t r1 = min(n_rows, r0 + kZoneRows);
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    uint32_t nv = 0;
    auto take = [&](int64_t v) {
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        ++nv;
    };
    // four consecutive rows per thread per step (one 16-byte load for INT32, two for INT64; a
    // zone starts on a 131,072-row boundary, so the loads are aligned), four steps in flight
#pragma unroll 4
    for (uint64_t b = r0 + 4u * (uint64_t)t; b < r1; b += 4u * 256u) {
        const uint32_t vb = validity ? (uint32_t)((validity[b >> 6] >> (b & 63)) & 15u) : 15u;
        if (b + 4 <= r1) {
            int64_t x[4];
            if (sizeof(T) == 4) {
                const bp_u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const bp_u32x4*>(col + b));
                x[0] = key_of<FK>((int32_t)q.x), x[1] = key_of<FK>((int32_t)q.y), x[2] = key_of<FK>((int32_t)q.z),
                x[3] = key_of<FK>((int32_t)q.w);
            } else {
                const u64x2 q0 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(col + b));
                const u64x2 q1 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(col + b) + 1);
                x[0] = key_of<FK>((int64_t)q0.x), x[1] = key_of<FK>((int64_t)q0.y), x[2] = key_of<FK>((int64_t)q1.x),
                x[3] = key_of<FK>((int64_t)q1.y);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((vb >> j) & 1u) take(x[j]);
        } else {
            for (uint64_t r = b; r < r1; ++r)
                if ((vb >> (r - b)) & 1u) take((int64_t)key_of<FK>(col[r]));
        }
    }
    s_lo[t] = lo;
    s_hi[t] = hi;
    s_n[t] = nv;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            s_lo[t] = s_lo[t + d] < s_lo[t] ? s_lo[t + d] : s_lo[t];
            s_hi[t] = s_hi[t + d] > s_hi[t] ? s_hi[t + d] : s_hi[t];
            s_n[t] += s_n[t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        mn[blockIdx.x] = s_lo[0];
        mx[blockIdx.x] = s_hi[0];
        fl[blockIdx.x] = (uint8_t)((s_n[0] > 0 ? 1 : 0) | (r1 > r0 && s_n[0] == r1 - r0 ? 2 : 0));
    }
}

// ------------------------------------------------------------------ index build: quantile edges

// One pass of the multi-target radix select that picks a column's equi-depth edges
// (QuantileHistArgs, cubit_internal.hpp). Each thread reads 16 bytes (4 INT32 or 2 INT64 rows) per
// load, kQuantileUnroll loads in flight, nontemporal like K0's column loads (streamed once); a
// workgroup owns 512 × kQuantileUnroll such vectors per step and strides by the grid. The validity
// word is read once per vector (a vector never crosses a 64-row word); NULL rows and rows past
// n_rows are never counted. Counters are the workgroup's own, in LDS: PASS0 the top d bits of u;
// otherwise the next d bits under the row's active prefix, found through s_top (for each value of
// u's top kQuantileTopBits bits, the first active prefix that starts with it: the rows of no
// active prefix leave after one LDS read) and a binary search among the prefixes that share those
// bits (one, unless the targets crowd into a narrow range). A row whose counter would fall outside
// the table is dropped, so a column that changed under the build shows as a wrong total on the
// host, never as a stray LDS write. WAGG: a wave whose rows of one step (64 lanes × kQuantileUnroll
// vectors) all fall into one counter adds their number from one lane (a single-valued or sorted
// column otherwise serialises 64 LDS adds per instruction; measured). At the end
// every non-zero counter is added to the global 64-bit counters with one atomic, 2^d · n_active ≤
// 16,384 per workgroup, instead of one global atomic per row.
constexpr int kQuantileThreads = 512;
constexpr int kQuantileUnroll = 4;
constexpr uint32_t kQuantileTopBits = 11;
static_assert(kQuantileTopBits < kQuantileD0, "every later pass has at least kQuantileTopBits resolved bits");
static_assert((1u << kQuantileD0) <= kQuantileCounters, "pass 0 fits the counters");
constexpr uint32_t kQuantileNone = 0xffffffffu;

template <typename T, int FK, bool PASS0, bool WAGG>
__global__ __launch_bounds__(kQuantileThreads, 4) void quantile_hist_kernel(const T* __restrict__ col,
                                                                            const uint64_t* __restrict__ validity,
                                                                            uint64_t n_rows, bool aligned,
                                                                            QuantileHistArgs a) {
    constexpr int R = 16 / sizeof(T);  // rows per 16-byte vector
    constexpr uint32_t RMASK = (1u << R) - 1;
    __shared__ uint32_t s_cnt[PASS0 ? (1u << kQuantileD0) : kQuantileCounters];
    __shared__ uint64_t s_pre[PASS0 ? 1 : kQuantileMaxActive];
    __shared__ uint16_t s_top[PASS0 ? 1 : (1u << kQuantileTopBits) + 1];
    const uint32_t t = threadIdx.x;
    const uint32_t n_cnt = PASS0 ? 1u << a.d : a.n_active << a.d;
    const uint32_t left = a.bits - a.consumed;  // bits of u not resolved before this pass
    for (uint32_t i = t; i < n_cnt; i += kQuantileThreads) s_cnt[i] = 0;
    if (!PASS0) {
        for (uint32_t i = t; i < a.n_active; i += kQuantileThreads) s_pre[i] = a.prefixes[i];
        __syncthreads();
        const uint32_t psh = a.consumed - kQuantileTopBits;  // prefix → its top bits
        for (uint32_t b = t; b <= (1u << kQuantileTopBits); b += kQuantileThreads) {
            uint32_t lo = 0, hi = a.n_active;  // the first prefix whose top bits are >= b
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((uint32_t)(s_pre[mid] >> psh) < b) lo = mid + 1;
                else hi = mid;
            }
            s_top[b] = (uint16_t)lo;
        }
    }
    __syncthreads();

    // the counter of a valid row's value, or kQuantileNone
    auto bucket = [&](T raw) -> uint32_t {
        const uint64_t u = (uint64_t)(int64_t)key_of<FK>(raw) - (uint64_t)a.vmin;
        if (PASS0) {
            const uint64_t b = u >> (left - a.d);
            return b < n_cnt ? (uint32_t)b : kQuantileNone;
        }
        const uint64_t top = u >> (a.bits - kQuantileTopBits);
        if (top >= (1u << kQuantileTopBits)) return kQuantileNone;  // u past 2^bits
        uint32_t lo = s_top[top], hi = s_top[top + 1];
        if (lo == hi) return kQuantileNone;
        const uint64_t p = u >> left;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_pre[mid] <= p) lo = mid;
            else hi = mid;
        }
        if (s_pre[lo] != p) return kQuantileNone;
        return (lo << a.d) | ((uint32_t)(u >> (left - a.d)) & ((1u << a.d) - 1));
    };
    const uint64_t tile_rows = (uint64_t)kQuantileThreads * kQuantileUnroll * R;
    for (uint64_t r0 = (uint64_t)blockIdx.x * tile_rows; r0 < n_rows; r0 += (uint64_t)gridDim.x * tile_rows) {
        T v[kQuantileUnroll][R];
        uint32_t ok[kQuantileUnroll];
        if (aligned && r0 + tile_rows <= n_rows) {
#pragma unroll
            for (int k = 0; k < kQuantileUnroll; ++k) {
                const uint64_t row = r0 + ((uint64_t)k * kQuantileThreads + t) * R;
                if constexpr (sizeof(T) == 4) {
                    const bp_u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const bp_u32x4*>(col + row));
                    v[k][0] = (T)q.x, v[k][1] = (T)q.y, v[k][2] = (T)q.z, v[k][3] = (T)q.w;
                } else {
                    const u64x2 q = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(col + row));
                    v[k][0] = (T)q.x, v[k][1] = (T)q.y;
                }
                ok[k] = validity ? (uint32_t)(validity[row >> 6] >> (row & 63)) & RMASK : RMASK;
            }
        } else {  // the last tile, or a column that does not start on 16 bytes
#pragma unroll
            for (int k = 0; k < kQuantileUnroll; ++k) {
                const uint64_t row = r0 + ((uint64_t)k * kQuantileThreads + t) * R;
                ok[k] = 0;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const bool in = row + j < n_rows;
                    v[k][j] = in ? __builtin_nontemporal_load(col + row + j) : (T)0;
                    ok[k] |= in ? 1u << j : 0u;
                }
                if (validity && ok[k]) ok[k] &= (uint32_t)(validity[row >> 6] >> (row & 63));
            }
        }
        uint32_t b[kQuantileUnroll][R];
#pragma unroll
        for (int k = 0; k < kQuantileUnroll; ++k)
#pragma unroll
            for (int j = 0; j < R; ++j) b[k][j] = (ok[k] >> j) & 1u ? bucket(v[k][j]) : kQuantileNone;
        if (WAGG) {  // one test per step: every row of the wave in one counter (whole waves get here)
            bool same = true;
#pragma unroll
            for (int k = 0; k < kQuantileUnroll; ++k)
#pragma unroll
                for (int j = 0; j < R; ++j) same = same && b[k][j] == b[0][0];
            const uint32_t b0 = __builtin_amdgcn_readfirstlane(b[0][0]);
            if (__ballot(same && b[0][0] == b0) == ~0ull) {
                if (b0 != kQuantileNone && (t & 63) == 0) atomicAdd(&s_cnt[b0], 64u * kQuantileUnroll * R);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < kQuantileUnroll; ++k)
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (b[k][j] != kQuantileNone) atomicAdd(&s_cnt[b[k][j]], 1u);
    }
    __syncthreads();
    for (uint32_t i = t; i < n_cnt; i += kQuantileThreads) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + i, (unsigned long long)c);
    }
}

// ------------------------------------------------------------------ K4: MVCC

__global__ __launch_bounds__(256) void fill_valid_kernel(uint64_t* __restrict__ words, uint64_t n_rows,
                                                         uint64_t n_words_padded) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t full = n_rows / 64;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words_padded; w += stride) {
        uint64_t v = 0;
        if (w < full) v = ~0ull;
        else if (w == full && (n_rows & 63)) v = (1ull << (n_rows & 63)) - 1;
        words[w] = v;
    }
}

// ------------------------------------------------------------------ index maintenance

// Append (BoundIndex::Append, bound_index.hpp:67-70): splice the n_bits bits of src (bit 0 =
// the first appended row) into dst at bit offset bit_off. One thread per destination word, so
// no word is written twice; the first word keeps its bits below bit_off (the rows already
// there) and the last keeps its bits past the splice (padding, zero). The appended rows'
// bitvector words come from the index-build compare kernel run over the appended slice alone.
__global__ __launch_bounds__(256) void splice_bits_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src,
                                                          uint64_t bit_off, uint64_t n_bits) {
    const uint64_t w0 = bit_off >> 6, w1 = (bit_off + n_bits + 63) >> 6;
    const uint32_t sh = (uint32_t)(bit_off & 63);
    const uint64_t src_words = (n_bits + 63) >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = w0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < w1; d += stride) {
        const uint64_t j = d - w0;  // src word whose low bits land in d (shifted up by sh)
        uint64_t v = j < src_words ? src[j] << sh : 0ull;
        if (sh && j >= 1 && j - 1 < src_words) v |= src[j - 1] >> (64 - sh);
        // bits of d that belong to the splice: rows [max(64d, bit_off), min(64d + 64, bit_off + n_bits))
        const uint64_t lo = d == w0 ? sh : 0;
        const uint64_t end = bit_off + n_bits - 64 * d;  // > 0
        const uint64_t hi = end >= 64 ? 64 : end;
        const uint64_t m = (hi == 64 ? ~0ull : ((1ull << hi) - 1)) & ~((1ull << lo) - 1);
        dst[d] = (dst[d] & ~m) | (v & m);
    }
}

// Merge of committed updates into the base (the checkpoint of update chains, cf.
// UpdateSegment / ColumnData checkpointing; CUBIT merges its update bitvectors the same way):
// row r gets its newest merged value and NULL-ness, and every index bitvector whose predicate
// changes for r changes r's bit. Only the keys whose predicate changes are touched: for a range
// index L(k) = {v < k}, the keys in (min(old, new), max(old, new)] (binary search over the sorted
// keys); for an equality index E(old) and E(new); for bins the old and the new bin.
__device__ __forceinline__ uint32_t upper_key(const int64_t* keys, uint32_t n, int64_t v) {  // first key > v
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Merge by words (cubit_table_merge_updates): the merged records (rows ascending, one per row)
// in chunks of 64 per wave; a wave takes every 64-row word whose first record lies in its chunk
// (a word's records are contiguous, at most 64, and may run into the next chunk), one word at a
// time. The record lanes read the old values, write the new ones and the validity word; then
// every index bitvector whose membership a record can change is rewritten for the word from the
// 64 rows' merged values — one ballot per bitvector — with a plain store: no atomics, no word
// list, and each word is written once however many of its rows changed (flipping bits per record
// through atomics took 140 ms for 6 M records x ~25 range keys at SF100). Range: the keys in
// [min a, max b) of the records' symmetric differences; equality / bins: each record's old and
// new key. Rows past n_rows read as not present.
constexpr uint32_t kMergeLdsKeys = 1024;
constexpr int kMergeBatch = 4;  // words whose 64 values a wave loads together

__global__ __launch_bounds__(256) void merge_words_kernel(const int64_t* __restrict__ rows,
                                                          const int64_t* __restrict__ values,
                                                          const uint8_t* __restrict__ valids, uint64_t m,
                                                          uint64_t n_rows, void* col, int type, uint64_t* validity,
                                                          MergeIndex ix0, MergeIndex ix1) {
    // both indexes' keys and bitvector pointers in LDS (up to kMergeLdsKeys each): a word's
    // rewrite walks its keys one after another, and from global memory each step waited for a
    // dependent load of the key and of the bitvector pointer
    __shared__ int64_t s_keys[2][kMergeLdsKeys];
    __shared__ uint64_t* s_bvs[2][kMergeLdsKeys];
    for (int x = 0; x < 2; ++x) {
        const MergeIndex& ix = x ? ix1 : ix0;
        if (!ix.bvs || ix.n_keys > kMergeLdsKeys) continue;
        for (uint32_t k = threadIdx.x; k < ix.n_keys; k += blockDim.x) {
            s_keys[x][k] = ix.keys[k];
            s_bvs[x][k] = ix.bvs[k];
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
    for (uint64_t i0 = ((uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64) * 64; i0 < m; i0 += waves * 64) {
        // the chunk's records and the next chunk's (a word starting here may run into it), each
        // record loaded once; a word's records then come by shuffles, and the old values of its
        // rows from the one load of the word's 64 values — one round of loads per batch of words
        const uint64_t ic = i0 + lane, inx = i0 + 64 + lane;
        const bool in_c = ic < m, in_n = inx < m;
        const int64_t row_c = in_c ? rows[ic] : -1, row_n = in_n ? rows[inx] : -1;
        const int64_t val_c = in_c ? values[ic] : 0, val_n = in_n ? values[inx] : 0;
        const int ok_c = in_c && (!valids || valids[ic]), ok_n = in_n && (!valids || valids[inx]);
        const int64_t before = i0 > 0 ? rows[i0 - 1] : -1;  // the record ahead of the chunk
        int64_t prev_row = __shfl_up(row_c, 1, 64);
        if (lane == 0) prev_row = before;
        const bool starts_word = in_c && (prev_row < 0 || ((uint64_t)prev_row >> 6) != ((uint64_t)row_c >> 6));
        uint64_t todo = __ballot(starts_word);
        while (todo) {
            uint32_t s[kMergeBatch];
            uint64_t wd[kMergeBatch];
            int nb = 0;
            for (; nb < kMergeBatch && todo; ++nb) {
                s[nb] = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                wd[nb] = (uint64_t)__shfl(row_c, (int)s[nb], 64) >> 6;
            }
            int64_t colv[kMergeBatch];
            uint64_t vw[kMergeBatch];
#pragma unroll
            for (int j = 0; j < kMergeBatch; ++j) {
                colv[j] = 0;
                vw[j] = ~0ull;
                if (j < nb) {
                    const uint64_t row = wd[j] * 64 + lane;
                    if (row < n_rows)
                        colv[j] = value_key(type, type_is32(type) ? (int64_t)static_cast<const int32_t*>(col)[row]
                                                                  : static_cast<const int64_t*>(col)[row]);
                    if (validity) vw[j] = validity[wd[j]];
                }
            }
#pragma unroll
            for (int j = 0; j < kMergeBatch; ++j) {
                if (j >= nb) break;
                const uint64_t word = wd[j];
                // the word's records: chunk lanes s[j] … and on into the next chunk (a prefix)
                const uint32_t cnt = (uint32_t)__popcll(__ballot(in_c && ((uint64_t)row_c >> 6) == word)) +
                                     (uint32_t)__popcll(__ballot(in_n && ((uint64_t)row_n >> 6) == word));
                const uint32_t q = s[j] + lane;  // this lane's record, 0 … 127 over the two chunks
                const int64_t r_a = __shfl(row_c, (int)(q & 63), 64), r_b = __shfl(row_n, (int)(q & 63), 64);
                const int64_t v_a = __shfl(val_c, (int)(q & 63), 64), v_b = __shfl(val_n, (int)(q & 63), 64);
                const int o_a = __shfl(ok_c, (int)(q & 63), 64), o_b = __shfl(ok_n, (int)(q & 63), 64);
                const bool has_rec = lane < cnt;
                const int64_t rrow = q < 64 ? r_a : r_b;
                const int64_t nv = q < 64 ? v_a : v_b;  // as stored (FLOAT / DOUBLE: the bit pattern)
                const int64_t nk = value_key(type, nv);  // as compared (colv holds keys too)
                const bool nvalid = (q < 64 ? o_a : o_b) != 0;
                const uint32_t pos = has_rec ? (uint32_t)(rrow & 63) : 0;
                const int64_t ov = __shfl(colv[j], (int)pos, 64);  // the row's old value
                const uint64_t old_vword = vw[j];
                const bool ovalid = has_rec && ((old_vword >> pos) & 1ull);
                // the records' rows and new NULL-ness as word masks (OR over the wave)
                uint64_t rec_bits = has_rec ? 1ull << pos : 0, new_bits = has_rec && nvalid ? 1ull << pos : 0;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    rec_bits |= __shfl_xor(rec_bits, d, 64);
                    new_bits |= __shfl_xor(new_bits, d, 64);
                }
                const uint64_t vword = (old_vword & ~rec_bits) | new_bits;
                if (has_rec) {
                    if (type_is32(type)) static_cast<int32_t*>(col)[rrow] = nvalid ? (int32_t)nv : 0;
                    else static_cast<int64_t*>(col)[rrow] = nvalid ? nv : 0;
                }
                if (validity && lane == 0) validity[word] = vword;
                // each row's merged value: its record's (records ascend by row: the row's record is
                // the popcount of the record rows below it), else its old value
                const uint64_t row = word * 64 + lane;
                const bool mine = (rec_bits >> lane) & 1ull;
                const int64_t from_rec = __shfl(nk, (int)__popcll(rec_bits & ((1ull << lane) - 1ull)), 64);
                const bool present = row < n_rows && ((vword >> lane) & 1ull);
                const int64_t v = present ? (mine ? from_rec : colv[j]) : 0;
                for (int x = 0; x < 2; ++x) {
                    const MergeIndex& gix = x ? ix1 : ix0;
                    if (!gix.bvs) continue;
                    const uint32_t n = gix.n_keys;
                    const bool lds = n <= kMergeLdsKeys;
                    const MergeIndex ix{lds ? s_keys[x] : gix.keys, lds ? s_bvs[x] : gix.bvs, n, gix.encoding};
                    if (ix.encoding == 0) {  // range: L(k) = {valid, v < k}
                        // the union of the records' flipped key intervals (keys searched in LDS when
                        // cached there: called with the LDS array itself, the searches are ds_reads)
                        auto interval = [&](const int64_t* keys, uint32_t& ra, uint32_t& rb) {
                            ra = n;
                            rb = n;
                            if (ovalid && nvalid) {
                                const int64_t lo = ov < nk ? ov : nk, hi = ov < nk ? nk : ov;
                                ra = upper_key(keys, n, lo);
                                rb = upper_key(keys, n, hi);
                            } else if (ovalid) {
                                ra = upper_key(keys, n, ov);
                            } else if (nvalid) {
                                ra = upper_key(keys, n, nk);
                            }
                        };
                        uint32_t a = n, b = 0;
                        if (has_rec) {
                            uint32_t ra, rb;
                            if (lds) interval(s_keys[x], ra, rb);
                            else interval(gix.keys, ra, rb);
                            if (ra < rb) {
                                a = ra;
                                b = rb;
                            }
                        }
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) {
                            a = min(a, (uint32_t)__shfl_xor((int)a, d, 64));
                            b = max(b, (uint32_t)__shfl_xor((int)b, d, 64));
                        }
                        if (lds) {  // explicit LDS reads (through a generic pointer they issue as flat loads)
                            for (uint32_t k = a; k < b; ++k) {
                                const uint64_t bits = __ballot(present && v < s_keys[x][k]);
                                if (lane == 0) s_bvs[x][k][word] = bits;
                            }
                        } else {
                            for (uint32_t k = a; k < b; ++k) {
                                const uint64_t bits = __ballot(present && v < ix.keys[k]);
                                if (lane == 0) ix.bvs[k][word] = bits;
                            }
                        }
                    } else {  // equality E(k) = {valid, v == k}; bins B_i = {valid, e_i <= v < e_i+1}
                        // each record's old and new bitvector (-1: none), rewritten one record at a time
                        auto which = [&](bool ok, int64_t val) -> int32_t {
                            if (!ok) return -1;
                            const uint32_t k = upper_key(ix.keys, n, val);
                            if (ix.encoding == 1) return (k > 0 && ix.keys[k - 1] == val) ? (int32_t)k - 1 : -1;
                            return (k == 0 || k == n) ? -1 : (int32_t)k - 1;
                        };
                        const int32_t ko = has_rec ? which(ovalid, ov) : -1, kn = has_rec ? which(nvalid, nk) : -1;
                        for (uint32_t jj = 0; jj < cnt; ++jj) {
                            for (int side = 0; side < 2; ++side) {
                                const int32_t k = __shfl(side ? kn : ko, (int)jj, 64);
                                if (k < 0) continue;
                                const bool in = ix.encoding == 1 ? v == ix.keys[k] : (ix.keys[k] <= v && v < ix.keys[k + 1]);
                                const uint64_t bits = __ballot(present && in);
                                if (lane == 0) ix.bvs[k][word] = bits;
                            }
                        }
                    }
                }
            }
        }
    }
}


// A delete is in effect for the reader when UseInsertedVersion(start, tid, delete_id)
// (chunk_info.cpp:11-19): clear that row.
__global__ __launch_bounds__(256) void visibility_kernel(const int64_t* __restrict__ rows,
                                                         const uint64_t* __restrict__ ids, uint64_t n,
                                                         uint64_t start_time, uint64_t tid,
                                                         uint64_t* __restrict__ words) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = ids[i];
        if (id < start_time || id == tid) {
            const uint64_t r = (uint64_t)rows[i];
            atomicAnd(reinterpret_cast<unsigned long long*>(&words[r >> 6]), ~(1ull << (r & 63)));
        }
    }
}

// Rows of insert ranges the reader may not see (UseInsertedVersion false for the range's
// insert id, chunk_info.cpp:11-19, ChunkConstantInfo / ChunkVectorInfo::inserted): clear
// [begin, end) of range blockIdx.y. Ranges are disjoint, so only a range's first and last
// word can be shared with another range (atomicAnd); inner words are stored as 0.
__global__ __launch_bounds__(256) void clear_ranges_kernel(const int64_t* __restrict__ ranges, uint64_t* __restrict__ words) {
    const uint64_t b = (uint64_t)ranges[2 * blockIdx.y], e = (uint64_t)ranges[2 * blockIdx.y + 1];
    if (b >= e) return;
    const uint64_t w0 = b >> 6, w1 = (e - 1) >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = w0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= w1; w += stride) {
        uint64_t clear = ~0ull;
        if (w == w0) clear &= ~0ull << (b & 63);
        if (w == w1 && (e & 63)) clear &= (1ull << (e & 63)) - 1;
        if (w == w0 || w == w1) atomicAnd(reinterpret_cast<unsigned long long*>(&words[w]), ~clear);
        else words[w] = 0;
    }
}

__global__ __launch_bounds__(256) void update_mask_kernel(const int64_t* __restrict__ rows,
                                                          const uint64_t* __restrict__ versions, uint64_t n,
                                                          uint64_t start_time, uint64_t tid,
                                                          uint64_t* __restrict__ mask) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t v = versions[i];
        if (v < start_time || v == tid) {
            const uint64_t r = (uint64_t)rows[i];
            atomicOr(reinterpret_cast<unsigned long long*>(&mask[r >> 6]), 1ull << (r & 63));
        }
    }
}

// Column sync (cubit_table_sync_column): which rows of a column differ from the new contents a
// host engine holds after committed UPDATEs. One streaming pass over the old values, the old
// validity, the new values and the new validity, in the layout of compare_bitvectors_kernel: a
// wave handles 64 consecutive words, lane l reads row l of each word (one coalesced 256- / 512-byte
// load per word and side, 8 words of both sides loaded ahead), the word's "changed" mask is one
// ballot kept by lane j for word j, and the 64 masks leave as one 512-byte plain store. A row
// changed when its NULL-ness differs, or when it is valid on both sides and the stored bits
// differ (FLOAT / DOUBLE: the caller passes the pattern column, so -0.0 → +0.0 is a change); two
// NULLs are equal whatever their slots hold. Rows past n_rows never count and the padding words
// up to n_words_padded are written as 0. The changed rows are counted from the masks: per lane,
// then per wave, then per workgroup (LDS, 4 words), one atomicAdd per workgroup into *counter.
// old_valid / new_valid may be null (every row valid); both are read only below n_words.
// Bytes per pass: n · 2 · sizeof(T) + 3 · n / 8.
template <typename T>
__global__ __launch_bounds__(256) void column_diff_kernel(const T* __restrict__ old_col,
                                                          const uint64_t* __restrict__ old_valid,
                                                          const T* __restrict__ new_col,
                                                          const uint64_t* __restrict__ new_valid, uint64_t n_rows,
                                                          uint64_t n_words, uint64_t n_words_padded,
                                                          uint64_t* __restrict__ changed,
                                                          unsigned long long* __restrict__ counter) {
    constexpr int JB = 8;
    __shared__ uint64_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint64_t cnt = 0;
    for (uint64_t w0 = wave_id * 64; w0 < n_words_padded; w0 += n_waves * 64) {
        uint64_t mine = 0;  // lane j keeps word w0 + j
        if (w0 < n_words) {  // a wave wholly in the padding stores zeros
            for (int jb = 0; jb < 64; jb += JB) {
                T a[JB], b[JB];
                uint64_t va[JB], vb[JB];
                bool in[JB];
#pragma unroll
                for (int j = 0; j < JB; ++j) {
                    const uint64_t w = w0 + jb + j, row = w * 64 + lane;
                    in[j] = row < n_rows;
                    a[j] = in[j] ? __builtin_nontemporal_load(old_col + row) : (T)0;  // streamed once: nt
                    b[j] = in[j] ? __builtin_nontemporal_load(new_col + row) : (T)0;
                    va[j] = old_valid && w < n_words ? old_valid[w] : ~0ull;
                    vb[j] = new_valid && w < n_words ? new_valid[w] : ~0ull;
                }
#pragma unroll
                for (int j = 0; j < JB; ++j) {
                    const bool oa = (va[j] >> lane) & 1ull, ob = (vb[j] >> lane) & 1ull;
                    const uint64_t m = __ballot(in[j] && (oa != ob || (oa && a[j] != b[j])));
                    if (lane == jb + j) mine = m;
                }
            }
        }
        changed[w0 + lane] = mine;
        cnt += (uint64_t)__popcll(mine);
    }
    cnt = wave_sum(cnt);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (total) atomicAdd(counter, (unsigned long long)total);
    }
}

// The changed rows' records for merge_words_kernel, read from the new column and validity at the
// ascending row ids the ordered decode produced: values[i] as the ABI carries a value (INT32 and
// codes sign-extended, a FLOAT pattern zero-extended, 0 for a NULL record) and valids[i] (1 = the
// value, 0 = NULL).
template <typename T>
__global__ __launch_bounds__(256) void sync_gather_kernel(const T* __restrict__ new_col,
                                                          const uint64_t* __restrict__ new_valid,
                                                          const int64_t* __restrict__ rows, uint64_t m,
                                                          int64_t* __restrict__ values, uint8_t* __restrict__ valids) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const uint64_t r = (uint64_t)rows[i];
        const bool ok = !new_valid || ((new_valid[r >> 6] >> (r & 63)) & 1ull);
        values[i] = ok ? (int64_t)new_col[r] : 0;
        valids[i] = ok ? 1 : 0;
    }
}

unsigned grid_for(uint64_t n, unsigned cap = 4096) {
    const uint64_t b = (n + 255) / 256;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, cap));
}

}  // namespace

// production geometry: decode tiles of 512 threads × 2 pairs = 2,048 words (131,072 rows),
// STAGE 4,096 staged ids (16 KiB LDS); count tiles of 256 threads × 8 pairs = 4,096 words.
// Chosen from the interleaved variant sweep in scripts/kbench.hip.
constexpr int kDecodeThreads = 512, kDecodePairs = 2, kDecodeStage = 4096;
// eval_decode_runs: two stages of 9,984 entries (78 KiB; two workgroups per CU fill the 160 KiB)
constexpr int kRunCap = 9984;
// count tiles: 512 threads × 2 pairs = 2,048 words for K ≤ 4, × 1 pair above (two tiles in
// flight must fit the 128-VGPR budget of 4 waves per SIMD)
constexpr int count_pairs(uint32_t k) { return k <= 4 ? 2 : 1; }
constexpr int kCountGrid = 512;   // persistent count grid: 2 workgroups per CU

uint64_t decode_tile_words() { return (uint64_t)kDecodeThreads * 2 * kDecodePairs; }
uint64_t count_tile_words(uint32_t n_leaves) { return 512ull * 2 * (uint64_t)count_pairs(n_leaves); }
int decode_block_threads() { return kDecodeThreads; }

// K × FORM dispatch: f(K, FORM), both std::integral_constant, for a program of 1 … kMaxLeaves leaves
// and the form eval_form gives it; any other leaf count: no call, hipErrorInvalidValue.
template <int K = 1, typename F>
hipError_t dispatch_k_form(const EvalProgram& prog, const F& f) {
    using KC = std::integral_constant<int, K>;
    if constexpr (K > kMaxLeaves) {
        return hipErrorInvalidValue;
    } else {
        if (prog.n_leaves != (uint32_t)K) return dispatch_k_form<K + 1>(prog, f);
        switch (eval_form(prog)) {
        case FORM_CONJ: f(KC{}, std::integral_constant<int, FORM_CONJ>{}); break;
        case FORM_DNF: f(KC{}, std::integral_constant<int, FORM_DNF>{}); break;
        case FORM_CNF: f(KC{}, std::integral_constant<int, FORM_CNF>{}); break;
        default: f(KC{}, std::integral_constant<int, FORM_POSTFIX>{}); break;
        }
        return hipSuccess;
    }
}

// the same with the zero-leaf program (every row): f(0, FORM_CONJ)
template <typename F>
hipError_t dispatch_k0_form(const EvalProgram& prog, const F& f) {
    if (prog.n_leaves != 0) return dispatch_k_form(prog, f);
    f(std::integral_constant<int, 0>{}, std::integral_constant<int, FORM_CONJ>{});
    return hipSuccess;
}
// the persistent grid of a slice kernel: wpc 512-thread workgroups per CU, no more than tiles
unsigned slice_grid(uint32_t num_tiles, int n_cus, unsigned wpc) {
    return std::max(1u, std::min<unsigned>(num_tiles, std::min<unsigned>(wpc * (unsigned)n_cus, kAggMaxGrid)));
}

// production decode (scripts/kbench.hip): the run-claimed kernel wherever a
// workgroup walks three or more tiles — one claim per filled LDS stage instead of one per pair
// (SF100-sized, 1 % / 0.75 % / 0.4 % selected at K = 1 / 2 / 3: 41 / 39 / 44 µs vs 46 / 50 / 57
// µs; K = 5 at 1.9 %: 82 vs 84 µs) — except K = 4, where at Q6's density a run holds two tiles
// and the pair kernel measured as fast or 1 % faster (73.2 vs 74.2 µs); the pair kernel for one
// or two tiles per workgroup (small inputs: one claim per workgroup either way).
// look-back kernel geometry: workgroups per CU (the grid is co-resident up to WPC·CUs tiles) and
// stage entries (32 KiB of LDS per workgroup)
constexpr int lookback_wpc(uint32_t) { return 3; }  // 80 VGPRs: no spill for K ≤ 8 (4 per CU: 64, spills)
constexpr int kLookbackStage = 8192;
// the same kernel for one leaf whose per-tile offsets are known (EvalArgs::tile_prefix; PRE): 32 KiB
// of LDS and 50 VGPRs, so four workgroups per CU, all its 32 wave slots. SF100 Q6 kept as one leaf
// (4,578 tiles of about 2,500 ids): 30.5 µs a step against 35.0 µs with three; a stage of 4,096
// entries measured the same (30.8), one of 2,048 (most tiles in rounds) 37.8
// (profiles/r13_prefixed_decode.txt)
constexpr int kPrefixedWpc = 4;
constexpr int kRowListThreads = 512;  // decode_row_list_kernel: one workgroup per tile
uint32_t lookback_max_tiles(uint32_t n_leaves, int n_cus) {
    return std::min<uint32_t>(kLookbackMaxTiles, (uint32_t)lookback_wpc(n_leaves) * (uint32_t)n_cus);
}

int decode_kernel_for(uint32_t n_leaves, uint32_t num_tiles, unsigned grid, int kernel, bool live, int n_cus,
                      bool prefixed) {
    // known per-tile offsets: one tile per workgroup with no inter-workgroup wait, at any size
    if (prefixed && (kernel == 0 || kernel == 3)) return 3;
    if (kernel == 3 && num_tiles <= kLookbackMaxTiles) return 3;
    if (kernel == 0 && num_tiles <= lookback_max_tiles(n_leaves, n_cus)) return 3;
    // a live-tile list (zonemap skip) needs the run kernel: its stage offsets are taken from the
    // run's first tile, while the pair kernel places tile B G tiles after tile A
    if (live) return 2;
    if (kernel == 1 || kernel == 2) return kernel;
    return num_tiles > 2ull * grid ? 2 : 1;
}

template <int K, int FORM>
void launch_decode_kf(const EvalArgs& a, uint64_t* dir, unsigned grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                      int kernel, int n_cus) {
    const int which = decode_kernel_for(K, a.num_tiles, grid, kernel, a.live != nullptr, n_cus, a.tile_prefix != nullptr);
    if (which == 3 && K == 1 && a.tile_prefix)
        hipExtLaunchKernelGGL((eval_decode_lookback<1, FORM, kLookbackStage, kPrefixedWpc, 16, 0, 512, true>),
                              dim3(a.num_tiles), dim3(512), 0, s, e0, e1, 0, a, dir);
    else if (which == 3)
        hipExtLaunchKernelGGL((eval_decode_lookback<K, FORM, kLookbackStage, lookback_wpc(K)>), dim3(a.num_tiles),
                              dim3(512), 0, s, e0, e1, 0, a, dir);
    else if (which == 2)
        hipExtLaunchKernelGGL((eval_decode_runs<K, kDecodePairs, kRunCap, kDecodeThreads, FORM>), dim3(grid),
                              dim3(kDecodeThreads), 0, s, e0, e1, 0, a, dir);
    else
        hipExtLaunchKernelGGL((eval_decode_pairs<K, kDecodePairs, kDecodeStage, kDecodeThreads, 0, FORM>), dim3(grid),
                              dim3(kDecodeThreads), 0, s, e0, e1, 0, a, dir);
}

template <int K, int FORM>
void launch_count_kf(const EvalArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const unsigned grid = std::min<unsigned>(a.num_tiles, (unsigned)kCountGrid);
    // result words: plain stores. sc1 buffer stores (SAUX 16) measured 37.7 vs 38.8 µs for a K = 2
    // materialise at SF100 size (profiles/r02k_balbench_materialise.txt); not enabled until the GPU
    // suite has run with them
    hipExtLaunchKernelGGL((eval_count_kernel<K, count_pairs(K), FORM>), dim3(grid), dim3(512), 0, s, e0, e1, 0, a);
}

hipError_t launch_eval_decode(const EvalArgs& a, uint64_t* dir, unsigned grid, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1, int kernel, int n_cus) {
    if (decode_kernel_for(a.prog.n_leaves, a.num_tiles, grid, kernel, a.live != nullptr, n_cus,
                          a.tile_prefix != nullptr) == 3 &&
        (a.num_tiles == 0 || (!a.tile_prefix && (a.flags == nullptr || a.epoch == 0))))
        return hipErrorInvalidValue;  // the look-back kernel needs the context's flags and an epoch
    const hipError_t e = dispatch_k_form(a.prog, [&](auto k, auto form) {
        launch_decode_kf<k.value, form.value>(a, dir, grid, s, e0, e1, kernel, n_cus);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_decode_row_list(const RowListArgs& a, uint64_t* dir, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.tiles == 0 || !a.prefix || !a.off || !a.lo_cnt || !a.count) return hipErrorInvalidValue;
    hipExtLaunchKernelGGL((decode_row_list_kernel<kRowListThreads, 16>), dim3(a.tiles), dim3(kRowListThreads), 0, s, e0,
                          e1, 0, a, dir);
    return hipGetLastError();
}

hipError_t launch_eval_count(const EvalArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const hipError_t e = dispatch_k_form(a.prog, [&](auto k, auto form) {
        launch_count_kf<k.value, form.value>(a, s, e0, e1);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_order_runs(const uint64_t* dir, uint32_t n_tiles, uint64_t* dst_off, const int64_t* src,
                             uint64_t capacity, int64_t* dst, hipStream_t s) {
    (void)dst_off;
    if (n_tiles == 0) return hipSuccess;
    const uint32_t tpw = std::max<uint32_t>(1, std::min<uint32_t>(8, n_tiles / 1024));
    const unsigned grid = (n_tiles + tpw - 1) / tpw;
    hipLaunchKernelGGL(order_runs_kernel<0>, dim3(grid), dim3(256), 0, s, dir, n_tiles, tpw, src, capacity, dst);
    return hipGetLastError();
}

hipError_t launch_compare_bitvector(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int cmp,
                                    int64_t constant, uint64_t* out_words, hipStream_t stream, int64_t constant2) {
    MultiKeyArgs a{};
    a.m = 1;
    a.c[0] = constant;
    a.c2[0] = constant2;
    a.out[0] = out_words;
    return launch_compare_m<1>(col, type, validity, n_rows, cmp, a, stream);
}

hipError_t launch_candidate_check(const void* col, int type, const uint64_t* validity, const uint64_t* lo_bv,
                                  const uint64_t* hi_bv, uint64_t n_rows, int cmp, int64_t constant,
                                  uint64_t* out_words, hipStream_t stream) {
    if (type == kTypeFloat)
        return constant >= INT32_MIN && constant <= INT32_MAX
                   ? launch_candidate_t<int32_t, int32_t, 1>(static_cast<const int32_t*>(col), validity, lo_bv, hi_bv,
                                                             n_rows, cmp, (int32_t)constant, out_words, stream)
                   : launch_candidate_t<int32_t, int64_t, 1>(static_cast<const int32_t*>(col), validity, lo_bv, hi_bv,
                                                             n_rows, cmp, constant, out_words, stream);
    if (type == kTypeDouble)
        return launch_candidate_t<int64_t, int64_t, 2>(static_cast<const int64_t*>(col), validity, lo_bv, hi_bv, n_rows,
                                                       cmp, constant, out_words, stream);
    if (type == kTypeUInt64)  // unsigned compare against the un-keyed constant
        return launch_candidate_t<uint64_t, uint64_t>(static_cast<const uint64_t*>(col), validity, lo_bv, hi_bv, n_rows,
                                                      cmp, (uint64_t)constant ^ 0x8000000000000000ull, out_words, stream);
    if (type_is32(type) && constant >= INT32_MIN && constant <= INT32_MAX)
        return launch_candidate_t<int32_t, int32_t>(static_cast<const int32_t*>(col), validity, lo_bv, hi_bv, n_rows,
                                                    cmp, (int32_t)constant, out_words, stream);
    if (type_is32(type))
        return launch_candidate_t<int32_t, int64_t>(static_cast<const int32_t*>(col), validity, lo_bv, hi_bv, n_rows,
                                                    cmp, constant, out_words, stream);
    return launch_candidate_t<int64_t, int64_t>(static_cast<const int64_t*>(col), validity, lo_bv, hi_bv, n_rows, cmp,
                                                constant, out_words, stream);
}

hipError_t launch_compare_bitvectors(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int cmp,
                                     const MultiKeyArgs& args, hipStream_t stream) {
    if (args.m == 0) return hipSuccess;
    if (args.m > (uint32_t)kMultiKeys) return hipErrorInvalidValue;
    MultiKeyArgs a = args;
    for (uint32_t k = a.m; k < (uint32_t)kMultiKeys; ++k) {  // the kernel evaluates every slot
        a.c[k] = a.c[a.m - 1];
        a.c2[k] = a.c2[a.m - 1];
        a.out[k] = nullptr;
    }
    // the smallest key count that covers m: the ballots per word grow with it
    if (a.m == 1) return launch_compare_m<1>(col, type, validity, n_rows, cmp, a, stream);
    if (a.m <= 4) return launch_compare_m<4>(col, type, validity, n_rows, cmp, a, stream);
    if (a.m <= 8) return launch_compare_m<8>(col, type, validity, n_rows, cmp, a, stream);
    return launch_compare_m<kMultiKeys>(col, type, validity, n_rows, cmp, a, stream);
}

namespace {
template <typename T, int FK>
void bitslice_build_pass(const T* col, const uint64_t* validity, uint64_t n_rows, const SliceBuildArgs& a,
                         hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const uint64_t nw = padded_words(n_rows);
    const uint64_t blocks = std::min<uint64_t>((nw / 64 + 3) / 4, 8192);
    const dim3 grid((unsigned)std::max<uint64_t>(blocks, 1)), block(256);
    // the smallest slice count that covers m: the ballots per word grow with it
    if (a.m <= 4)
        hipExtLaunchKernelGGL((bitslice_build_kernel<T, 4, FK>), grid, block, 0, stream, e0, e1, 0, col, validity, n_rows,
                              nw, a);
    else if (a.m <= 8)
        hipExtLaunchKernelGGL((bitslice_build_kernel<T, 8, FK>), grid, block, 0, stream, e0, e1, 0, col, validity, n_rows,
                              nw, a);
    else
        hipExtLaunchKernelGGL((bitslice_build_kernel<T, kMultiKeys, FK>), grid, block, 0, stream, e0, e1, 0, col,
                              validity, n_rows, nw, a);
}
}  // namespace

hipError_t launch_bitslice_build(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t base,
                                 uint32_t n_slices, const SliceSet& out, hipStream_t stream, hipEvent_t ev0,
                                 hipEvent_t ev1) {
    if (n_slices > kMaxSlices) return hipErrorInvalidValue;
    for (uint32_t s0 = 0; s0 < n_slices; s0 += kMultiKeys) {
        SliceBuildArgs a{};
        a.base = base;
        a.s0 = s0;
        a.m = std::min<uint32_t>(kMultiKeys, n_slices - s0);
        for (uint32_t k = 0; k < a.m; ++k) a.out[k] = out.s[s0 + k];
        hipEvent_t e0 = s0 == 0 ? ev0 : nullptr, e1 = s0 + kMultiKeys >= n_slices ? ev1 : nullptr;
        if (type == kTypeFloat)
            bitslice_build_pass<int32_t, 1>(static_cast<const int32_t*>(col), validity, n_rows, a, stream, e0, e1);
        else if (type == kTypeDouble)
            bitslice_build_pass<int64_t, 2>(static_cast<const int64_t*>(col), validity, n_rows, a, stream, e0, e1);
        else if (type == kTypeUInt64)
            bitslice_build_pass<int64_t, 3>(static_cast<const int64_t*>(col), validity, n_rows, a, stream, e0, e1);
        else if (type_is32(type))
            bitslice_build_pass<int32_t, 0>(static_cast<const int32_t*>(col), validity, n_rows, a, stream, e0, e1);
        else
            bitslice_build_pass<int64_t, 0>(static_cast<const int64_t*>(col), validity, n_rows, a, stream, e0, e1);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_bitslice_reslice(const int64_t* rows, uint64_t m, const void* col, int type, const uint64_t* validity,
                                   uint64_t n_rows, int64_t base, uint32_t n_slices, const SliceSet& slices,
                                   hipStream_t stream) {
    if (n_slices > kMaxSlices) return hipErrorInvalidValue;
    if (m == 0 || n_slices == 0) return hipSuccess;
    const dim3 grid(grid_for(m)), block(256);  // a wave per 64 records
#define CUBIT_RESLICE(T, FK)                                                                                        \
    hipLaunchKernelGGL((bitslice_reslice_kernel<T, FK>), grid, block, 0, stream, rows, m, static_cast<const T*>(col), \
                       validity, n_rows, base, n_slices, slices)
    if (type == kTypeFloat) CUBIT_RESLICE(int32_t, 1);
    else if (type == kTypeDouble) CUBIT_RESLICE(int64_t, 2);
    else if (type == kTypeUInt64) CUBIT_RESLICE(int64_t, 3);
    else if (type_is32(type)) CUBIT_RESLICE(int32_t, 0);
    else CUBIT_RESLICE(int64_t, 0);
#undef CUBIT_RESLICE
    return hipGetLastError();
}

hipError_t launch_bitslice_compare(const SliceSet& slices, uint32_t n_slices, const uint64_t* validity, uint64_t n_rows,
                                   uint64_t lo, uint64_t hi, int negate, uint64_t* out, hipStream_t stream,
                                   hipEvent_t ev0, hipEvent_t ev1) {
    if (n_slices > kMaxSlices) return hipErrorInvalidValue;
    const uint64_t max = n_slices >= 64 ? ~0ull : (1ull << n_slices) - 1;
    // an interval that holds no offset is the complement of the one that holds them all
    if (lo > hi || lo > max) {
        lo = 0;
        hi = max;
        negate = !negate;
    }
    if (hi > max) hi = max;
    const bool need_lo = lo != 0, need_hi = hi != max;
    const uint64_t nw = padded_words(n_rows);
    const dim3 grid((unsigned)std::min<uint64_t>((nw / 2 + 255) / 256, 8192)), block(256);
#define CUBIT_SLICED(L, H)                                                                                         \
    hipExtLaunchKernelGGL((bitslice_compare_kernel<L, H>), grid, block, 0, stream, ev0, ev1, 0, slices, n_slices, \
                          validity, n_rows, nw, lo, hi, negate ? 1 : 0, out)
    if (need_lo && need_hi) CUBIT_SLICED(true, true);
    else if (need_lo) CUBIT_SLICED(true, false);
    else if (need_hi) CUBIT_SLICED(false, true);
    else CUBIT_SLICED(false, false);
#undef CUBIT_SLICED
    return hipGetLastError();
}

// SUM-only, MIN/MAX-only and both are kernels of their own (the ops are resolved outside the slice
// loop: a SUM pays no ripple, a MIN / MAX no popcounts); a call for the counts alone runs the SUM form
template <int K, int FORM>
void launch_slice_aggregate_kf(const EvalArgs& a, const SliceAggArgs& g, uint32_t ops, unsigned grid, hipStream_t s,
                               hipEvent_t e0, hipEvent_t e1) {
    const bool minmax = (ops & (kAggMin | kAggMax)) != 0;
    if (!minmax)
        hipExtLaunchKernelGGL((eval_slice_aggregate<K, FORM, true, false>), dim3(grid), dim3(512), 0, s, e0, e1, 0, a, g);
    else if (ops & kAggSum)
        hipExtLaunchKernelGGL((eval_slice_aggregate<K, FORM, true, true>), dim3(grid), dim3(512), 0, s, e0, e1, 0, a, g);
    else
        hipExtLaunchKernelGGL((eval_slice_aggregate<K, FORM, false, true>), dim3(grid), dim3(512), 0, s, e0, e1, 0, a, g);
}

hipError_t launch_eval_slice_aggregate(EvalArgs a, const SliceAggArgs& g, uint32_t ops, int type, int64_t base,
                                       int n_cus, LaunchShape* shape,
                                       int64_t* out, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    if (g.n_slices > kMaxSlices || a.num_tiles == 0 || !g.workspace || !a.ticket) return hipErrorInvalidValue;
    a.count = agg_count_slot(g.workspace);
    const unsigned grid = slice_grid(a.num_tiles, n_cus, 2);  // two workgroups per CU, as the fused sum's
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    hipError_t e = dispatch_k0_form(a.prog, [&](auto k, auto form) {
        launch_slice_aggregate_kf<k.value, form.value>(a, g, ops, grid, stream, ev0, ev1);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(aggregate_finish_kernel, dim3(1), dim3(64), 0, stream, g.workspace, (int)grid, ops, type, base, 1,
                       out);
    return hipGetLastError();
}

hipError_t launch_eval_slice_sum_product(EvalArgs a, const SliceProductArgs& g, int64_t base_outer, int64_t base_inner,
                                         int n_cus, LaunchShape* shape,
                                         int64_t* out, int out_slots, uint64_t* count_out, hipStream_t stream,
                                         hipEvent_t ev0, hipEvent_t ev1) {
    if (g.n_outer > kMaxSlices || g.n_inner > g.n_outer || a.num_tiles == 0 || !g.workspace || !a.ticket)
        return hipErrorInvalidValue;
    a.count = agg_count_slot(g.workspace);
    // two workgroups per CU, as the aggregate's; the workspace holds kProductMaxGrid partials
    const unsigned grid = std::min(slice_grid(a.num_tiles, n_cus, 2), kProductMaxGrid);
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    hipError_t e = dispatch_k0_form(a.prog, [&](auto k, auto form) {
        hipExtLaunchKernelGGL((eval_slice_sum_product<k.value, form.value>), dim3(grid), dim3(512), 0, stream, ev0, ev1, 0,
                              a, g);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(slice_product_finish_kernel, dim3(1), dim3(64), 0, stream, g.workspace, (int)grid, base_outer,
                       base_inner, out, out_slots, count_out);
    return hipGetLastError();
}

hipError_t launch_aggregate_arrays(const int64_t* x, const uint64_t* valid, const uint64_t* d_count, uint64_t max_n,
                                   uint32_t ops, int type, int64_t* workspace, int64_t* out, hipStream_t stream) {
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((max_n + 2047) / 2048, kAggMaxGrid));
    hipLaunchKernelGGL(aggregate_arrays_kernel, dim3(grid), dim3(256), 0, stream, x, valid, d_count, max_n, ops, type,
                       workspace);
    hipLaunchKernelGGL(aggregate_finish_kernel, dim3(1), dim3(64), 0, stream, workspace, (int)grid, ops, type,
                       (int64_t)0, 0, out);
    return hipGetLastError();
}

hipError_t launch_slice_select(EvalArgs a, const SliceSelectArgs& g, int mode, uint64_t k, double q, int type,
                               int64_t base, int n_cus, LaunchShape* shape,
                               int64_t* out, hipStream_t stream, uint32_t* n_passes,
                               hipEvent_t ev0, hipEvent_t ev1) {
    if (g.n_slices > kMaxSlices || a.num_tiles == 0 || !g.workspace || !g.cand || !a.ticket) return hipErrorInvalidValue;
    a.count = select_count_slot(g.workspace);
    const unsigned grid = slice_grid(a.num_tiles, n_cus, 2);  // as the aggregate's
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    const uint32_t bits = g.n_slices, passes = select_passes(bits, kSelectChunk);
    if (n_passes) *n_passes = passes;
    hipError_t e = dispatch_k0_form(a.prog, [&](auto kk, auto form) {
        hipExtLaunchKernelGGL((eval_slice_select<kk.value, form.value>), dim3(grid), dim3(512), 0, stream, ev0, nullptr, 0,
                              a, g);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t low = select_chunk_low(bits, kSelectChunk, p);
        if (p > 0) {
            const uint32_t pc = select_chunk_bits(bits, kSelectChunk, p - 1), plow = select_chunk_low(bits, kSelectChunk, p - 1);
#define CUBIT_NARROW(PC) \
    hipLaunchKernelGGL((slice_select_narrow<PC>), dim3(grid), dim3(512), 0, stream, a, g, plow)
            if (pc == 1) CUBIT_NARROW(1);
            else if (pc == 2) CUBIT_NARROW(2);
            else if (pc == 3) CUBIT_NARROW(3);
            else CUBIT_NARROW(4);
#undef CUBIT_NARROW
        }
        const bool last = p + 1 == passes;
        // (the partials hold 2^kSelectChunk counters per workgroup whatever the chunk; those past
        // 2^cnt are zero)
        hipExtLaunchKernelGGL(select_step_kernel, dim3(1), dim3(kSelectStepThreads), 0, stream, nullptr, last ? ev1 : nullptr, 0,
                              g.workspace, (int)grid, 1u << kSelectChunk, low, p == 0 ? 1 : 0, last ? 1 : 0, mode, k, q,
                              type, base, out);
    }
    return hipGetLastError();
}

hipError_t launch_select_arrays(const int64_t* x, const uint64_t* valid, const uint64_t* d_count, uint64_t max_n,
                                int mode, uint64_t k, double q, int type, int64_t* workspace, int64_t* out,
                                hipStream_t stream, uint32_t* n_passes) {
    if (!workspace) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((max_n + 2047) / 2048, kSelectArrayGrid));
    constexpr uint32_t passes = 64 / kSelectArrayBits;
    if (n_passes) *n_passes = passes;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 64 - (p + 1) * kSelectArrayBits;
        hipLaunchKernelGGL(select_arrays_kernel, dim3(grid), dim3(256), 0, stream, x, valid, d_count, max_n, type, shift,
                           p == 0 ? 1 : 0, workspace);
        hipLaunchKernelGGL(select_step_kernel, dim3(1), dim3(kSelectStepThreads), 0, stream, workspace, (int)grid, 1u << kSelectArrayBits,
                           shift, p == 0 ? 1 : 0, p + 1 == passes ? 1 : 0, mode, k, q, type, INT64_MIN, out);
    }
    return hipGetLastError();
}

hipError_t launch_slice_select_grouped(const EvalArgs& a, const SliceSelectArgs& g, const GroupAggArgs& q, int mode,
                                       uint64_t k, double quantile, int type, int64_t base,
                                       int n_cus, LaunchShape* shape, int64_t* out,
                                       hipStream_t stream, uint32_t* n_passes, hipEvent_t ev0, hipEvent_t ev1) {
    constexpr uint32_t limit = kGroupBatchSelect;
    if (g.n_slices > kMaxSlices || a.num_tiles == 0 || !g.workspace || !g.cand || q.n2 > 2 || q.n1 == 0 ||
        q.n1 > (q.n2 ? limit / 2 : limit))
        return hipErrorInvalidValue;
    // one workgroup per CU: at the kernels' register count a CU holds one
    const unsigned grid = slice_grid(a.num_tiles, n_cus, 1);
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    const bool two = q.n2 != 0;
    const uint32_t bits = g.n_slices, passes = select_passes(bits, kSelectChunk);
    if (n_passes) *n_passes = passes;
    hipError_t e = dispatch_k0_form(a.prog, [&](auto kk, auto form) {
        if (two)
            hipExtLaunchKernelGGL((eval_slice_select_grouped<kk.value, form.value, true>), dim3(grid), dim3(512), 0, stream,
                                  ev0, nullptr, 0, a, g, q);
        else
            hipExtLaunchKernelGGL((eval_slice_select_grouped<kk.value, form.value, false>), dim3(grid), dim3(512), 0, stream,
                                  ev0, nullptr, 0, a, g, q);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t low = select_chunk_low(bits, kSelectChunk, p);
        if (p > 0) {
            const uint32_t pc = select_chunk_bits(bits, kSelectChunk, p - 1), plow = select_chunk_low(bits, kSelectChunk, p - 1);
#define CUBIT_NARROW(PC)                                                                                              \
    if (two) hipLaunchKernelGGL((slice_select_narrow_grouped<PC, true>), dim3(grid), dim3(512), 0, stream, a, g, q, plow); \
    else hipLaunchKernelGGL((slice_select_narrow_grouped<PC, false>), dim3(grid), dim3(512), 0, stream, a, g, q, plow)
            if (pc == 1) { CUBIT_NARROW(1); }
            else if (pc == 2) { CUBIT_NARROW(2); }
            else if (pc == 3) { CUBIT_NARROW(3); }
            else { CUBIT_NARROW(4); }
#undef CUBIT_NARROW
        }
        const bool last = p + 1 == passes;
        hipExtLaunchKernelGGL(select_step_grouped_kernel, dim3(1), dim3(kSelectStepThreads), 0, stream, nullptr,
                              last ? ev1 : nullptr, 0, g.workspace, (int)grid, limit, low, p == 0 ? 1 : 0, last ? 1 : 0, mode, k,
                              quantile, type, base, q, 0, out);
    }
    return hipGetLastError();
}

hipError_t launch_select_arrays_grouped(const int64_t* x, const uint64_t* valid, const GroupColArgs& gc, uint32_t n_groups,
                                        const uint64_t* d_count, uint64_t max_n, int mode, uint64_t k, double quantile,
                                        int type, int64_t* workspace, int64_t* out, hipStream_t stream, uint32_t* n_passes) {
    if (n_groups == 0 || n_groups > CUBIT_AGG_MAX_GROUPS || !workspace) return hipErrorInvalidValue;
    const unsigned grid =
        (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((max_n + 2047) / 2048, select_group_col_grid(n_groups)));
    constexpr uint32_t passes = 64 / kSelectGroupArrayBits;
    if (n_passes) *n_passes = passes;
    GroupAggArgs none{};
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 64 - (p + 1) * kSelectGroupArrayBits;
        hipLaunchKernelGGL(select_arrays_grouped_kernel, dim3(grid), dim3(256), 0, stream, x, valid, gc, n_groups, d_count,
                           max_n, type, shift, p == 0 ? 1 : 0, workspace);
        hipLaunchKernelGGL(select_step_grouped_kernel, dim3(1), dim3(kSelectStepThreads), 0, stream, workspace, (int)grid,
                           n_groups, shift, p == 0 ? 1 : 0, p + 1 == passes ? 1 : 0, mode, k, quantile, type, INT64_MIN, none, 1,
                           out);
    }
    return hipGetLastError();
}

hipError_t launch_merge_ids(const int64_t* a, uint64_t na, const int64_t* b, uint64_t nb, int64_t* out, uint64_t* count,
                            hipStream_t stream) {
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((na + nb + 255) / 256, 4096));
    hipLaunchKernelGGL(merge_ids_kernel, dim3(grid), dim3(256), 0, stream, a, na, b, nb, out, count);
    return hipGetLastError();
}

// the grouped slice kernel's forms: one or two group columns, with or without the MIN / MAX ripple
// (a MIN / MAX call computes the sums too and the finishing wave drops them)
template <int K, int FORM>
void launch_slice_aggregate_grouped_kf(const EvalArgs& a, const SliceAggArgs& g, const GroupAggArgs& q, bool minmax,
                                       unsigned grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const bool two = q.n2 != 0;
#define CUBIT_GROUPED(TWO, MM)                                                                                       \
    hipExtLaunchKernelGGL((eval_slice_aggregate_grouped<K, FORM, TWO, MM>), dim3(grid), dim3(512), 0, s, e0, e1, 0, a, g, q)
    if (two && minmax) CUBIT_GROUPED(true, true);
    else if (two) CUBIT_GROUPED(true, false);
    else if (minmax) CUBIT_GROUPED(false, true);
    else CUBIT_GROUPED(false, false);
#undef CUBIT_GROUPED
}

hipError_t launch_eval_slice_aggregate_grouped(const EvalArgs& a, const SliceAggArgs& g, const GroupAggArgs& q,
                                               uint32_t ops, int type, int64_t base, int n_cus, LaunchShape* shape,
                                               int64_t* out,
                                               hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    const bool minmax = (ops & (kAggMin | kAggMax)) != 0;
    const uint32_t limit = minmax ? kGroupBatchMinMax : kGroupBatchSum;
    if (g.n_slices > kMaxSlices || a.num_tiles == 0 || !q.partials || q.n2 > 2 || q.n1 == 0 ||
        q.n1 > (q.n2 ? limit / 2 : limit))
        return hipErrorInvalidValue;
    const unsigned grid = slice_grid(a.num_tiles, n_cus, 1);  // one workgroup per CU at the kernel's register count
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    hipError_t e = dispatch_k0_form(a.prog, [&](auto k, auto form) {
        launch_slice_aggregate_grouped_kf<k.value, form.value>(a, g, q, minmax, grid, stream, ev0, ev1);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(aggregate_grouped_finish_kernel, dim3(limit), dim3(64), 0, stream, q.partials, (int)grid, q, 0, ops,
                       type, base, 1, out);
    return hipGetLastError();
}

hipError_t launch_aggregate_arrays_grouped(const int64_t* x, const uint64_t* valid, const GroupColArgs& gc,
                                           uint32_t n_groups, const uint64_t* d_count, uint64_t max_n, uint32_t ops,
                                           int type, int64_t* partials, int64_t* out, hipStream_t stream) {
    if (n_groups == 0 || n_groups > CUBIT_AGG_MAX_GROUPS || !partials) return hipErrorInvalidValue;
    // a workgroup takes kGroupFlushIters iterations of 256 rows before the grid grows
    const unsigned grid = (unsigned)std::max<uint64_t>(
        1, std::min<uint64_t>((max_n + 256ull * kGroupFlushIters - 1) / (256ull * kGroupFlushIters), kGroupColGrid));
    hipLaunchKernelGGL(aggregate_arrays_grouped_kernel, dim3(grid), dim3(256), 0, stream, x, valid, gc, n_groups, d_count,
                       max_n, ops, type, partials);
    GroupAggArgs none{};
    hipLaunchKernelGGL(aggregate_grouped_finish_kernel, dim3(n_groups), dim3(64), 0, stream, partials, (int)grid, none, 1,
                       ops, type, (int64_t)0, 0, out);
    return hipGetLastError();
}

hipError_t launch_eval_slice_sum_product_grouped(const EvalArgs& a, const SliceProductArgs& g, const GroupAggArgs& q,
                                                 int64_t base_outer, int64_t base_inner, int n_cus, LaunchShape* shape,
                                                 int64_t* out,
                                                 hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    constexpr uint32_t limit = kProductGroupBatch;
    if (g.n_outer > kMaxSlices || g.n_inner > g.n_outer || a.num_tiles == 0 || !q.partials || q.n2 > 2 || q.n1 == 0 ||
        q.n1 > (q.n2 ? limit / 2 : limit))
        return hipErrorInvalidValue;
    const unsigned grid = slice_grid(a.num_tiles, n_cus, 1);  // one workgroup per CU at the kernel's register count
    if (shape) *shape = LaunchShape{grid, a.num_tiles};
    const bool two = q.n2 != 0;
    hipError_t e = dispatch_k0_form(a.prog, [&](auto k, auto form) {
        if (two)
            hipExtLaunchKernelGGL((eval_slice_sum_product_grouped<k.value, form.value, true>), dim3(grid), dim3(512), 0,
                                  stream, ev0, ev1, 0, a, g, q);
        else
            hipExtLaunchKernelGGL((eval_slice_sum_product_grouped<k.value, form.value, false>), dim3(grid), dim3(512), 0,
                                  stream, ev0, ev1, 0, a, g, q);
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sum_product_grouped_finish_kernel, dim3(limit), dim3(64), 0, stream, q.partials, (int)grid, q, 0,
                       base_outer, base_inner, out);
    return hipGetLastError();
}

hipError_t launch_sum_product_arrays_grouped(const int64_t* xa, const uint64_t* va, const int64_t* xb, const uint64_t* vb,
                                             const GroupColArgs& gc, uint32_t n_groups, const uint64_t* d_count,
                                             uint64_t max_n, int64_t* partials, int64_t* out, hipStream_t stream) {
    if (n_groups == 0 || n_groups > CUBIT_AGG_MAX_GROUPS || !partials) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((max_n + 16383) / 16384, kProductColGrid));
    hipLaunchKernelGGL(sum_product_arrays_grouped_kernel, dim3(grid), dim3(256), 0, stream, xa, va, xb, vb, gc, n_groups,
                       d_count, max_n, partials);
    GroupAggArgs none{};
    hipLaunchKernelGGL(sum_product_grouped_finish_kernel, dim3(n_groups), dim3(64), 0, stream, partials, (int)grid, none, 1,
                       (int64_t)0, (int64_t)0, out);
    return hipGetLastError();
}

hipError_t launch_column_minmax(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t* out3,
                                hipStream_t stream) {
    const dim3 grid(grid_for(n_rows, 2048)), block(256);
    if (type == kTypeFloat)
        hipLaunchKernelGGL((column_minmax_kernel<int32_t, 1>), grid, block, 0, stream, static_cast<const int32_t*>(col),
                           validity, n_rows, out3);
    else if (type == kTypeDouble)
        hipLaunchKernelGGL((column_minmax_kernel<int64_t, 2>), grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, n_rows, out3);
    else if (type == kTypeUInt64)
        hipLaunchKernelGGL((column_minmax_kernel<int64_t, 3>), grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, n_rows, out3);
    else if (type_is32(type))
        hipLaunchKernelGGL(column_minmax_kernel<int32_t>, grid, block, 0, stream, static_cast<const int32_t*>(col),
                           validity, n_rows, out3);
    else
        hipLaunchKernelGGL(column_minmax_kernel<int64_t>, grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, n_rows, out3);
    return hipGetLastError();
}

hipError_t launch_presence(const void* col, int type, const uint64_t* validity, uint64_t n_rows, int64_t vmin,
                           uint64_t range, uint64_t* bits, hipStream_t stream) {
    const dim3 grid(grid_for(n_rows, 2048)), block(256);
    const bool lds = range <= 65536;
#define CUBIT_PRESENCE(T, L, FK)                                                                                   \
    hipLaunchKernelGGL((presence_kernel<T, L, FK>), grid, block, 0, stream, static_cast<const T*>(col), validity, \
                       n_rows, vmin, range, bits)
    if (type == kTypeFloat) {  // a FLOAT column's keys span less than 2^32 (a DOUBLE's are sorted on the host)
        if (lds) CUBIT_PRESENCE(int32_t, true, 1);
        else CUBIT_PRESENCE(int32_t, false, 1);
    } else if (type == kTypeDouble) {
        if (lds) CUBIT_PRESENCE(int64_t, true, 2);
        else CUBIT_PRESENCE(int64_t, false, 2);
    } else if (type == kTypeUInt64) {
        if (lds) CUBIT_PRESENCE(int64_t, true, 3);
        else CUBIT_PRESENCE(int64_t, false, 3);
    } else if (type_is32(type)) {
        if (lds) CUBIT_PRESENCE(int32_t, true, 0);
        else CUBIT_PRESENCE(int32_t, false, 0);
    } else {
        if (lds) CUBIT_PRESENCE(int64_t, true, 0);
        else CUBIT_PRESENCE(int64_t, false, 0);
    }
#undef CUBIT_PRESENCE
    return hipGetLastError();
}

hipError_t launch_quantile_hist(const void* col, int type, const uint64_t* validity, uint64_t n_rows,
                                const QuantileHistArgs& a, int n_cus, hipStream_t stream, hipEvent_t ev0,
                                hipEvent_t ev1, bool wave_agg) {
    const bool pass0 = a.consumed == 0;
    if (a.bits > 64 || !a.counts || (uint64_t)a.consumed + a.d > a.bits) return hipErrorInvalidValue;
    if (pass0 ? a.d != std::min(a.bits, kQuantileD0)
              : a.consumed < kQuantileD0 || a.d == 0 || !a.prefixes || a.n_active == 0 ||
                    a.n_active > kQuantileMaxActive || ((uint64_t)a.n_active << a.d) > kQuantileCounters)
        return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    const bool is32 = type_is32(type);
    const uint64_t tile_rows = (uint64_t)kQuantileThreads * kQuantileUnroll * (is32 ? 4 : 2);
    const uint64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
    // two workgroups per CU (the LDS of a later pass allows no more; four in pass 0); more only where
    // a workgroup's share would reach the 2^32 rows a 32-bit LDS counter holds
    const uint64_t per_cu = pass0 ? 4 : 2;
    const uint64_t blocks =
        std::max<uint64_t>(std::min<uint64_t>(tiles, per_cu * (uint64_t)std::max(n_cus, 1)), (n_rows >> 31) + 1);
    const dim3 grid((unsigned)blocks), block(kQuantileThreads);
    const bool aligned = reinterpret_cast<uintptr_t>(col) % 16 == 0;
#define CUBIT_QHIST_W(T, FK, P0, W)                                                                              \
    hipExtLaunchKernelGGL((quantile_hist_kernel<T, FK, P0, W>), grid, block, 0, stream, ev0, ev1, 0,             \
                          static_cast<const T*>(col), validity, n_rows, aligned, a)
#define CUBIT_QHIST(T, FK)                                 \
    do {                                                   \
        if (pass0 && wave_agg) CUBIT_QHIST_W(T, FK, true, true);    \
        else if (pass0) CUBIT_QHIST_W(T, FK, true, false);          \
        else if (wave_agg) CUBIT_QHIST_W(T, FK, false, true);       \
        else CUBIT_QHIST_W(T, FK, false, false);                    \
    } while (0)
    // FLOAT / DOUBLE columns come as their key columns (key_type), as to the compare kernels
    if (type_is_fp(type)) return hipErrorInvalidValue;
    if (type == kTypeUInt64) CUBIT_QHIST(int64_t, 3);
    else if (is32) CUBIT_QHIST(int32_t, 0);
    else CUBIT_QHIST(int64_t, 0);
#undef CUBIT_QHIST
#undef CUBIT_QHIST_W
    return hipGetLastError();
}

hipError_t launch_narrow_i32(const int64_t* in, const uint64_t* d_count, uint64_t max_n, int64_t offset, int32_t* out,
                             hipStream_t stream, uint32_t* overflow) {
    if (max_n == 0) return hipSuccess;
    hipLaunchKernelGGL(narrow_i32_kernel, dim3(grid_for((max_n + 1) / 2)), dim3(256), 0, stream, in, d_count, max_n,
                       offset, out, overflow);
    return hipGetLastError();
}

template <typename O>
static void narrow_unsigned_launch(const int64_t* in, const uint64_t* d_count, uint64_t max_n, int64_t offset, O* out,
                                   uint32_t* overflow, hipStream_t stream) {
    const bool aligned = reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (aligned)
        hipLaunchKernelGGL(narrow_unsigned_kernel<O>, dim3(grid_for((max_n + 7) / 8)), dim3(256), 0, stream, in, d_count,
                           max_n, offset, out, overflow);
    else
        hipLaunchKernelGGL(narrow_unsigned_scalar_kernel<O>, dim3(grid_for(max_n)), dim3(256), 0, stream, in, d_count,
                           max_n, offset, out, overflow);
}

hipError_t launch_narrow_unsigned(const int64_t* in, const uint64_t* d_count, uint64_t max_n, int64_t offset, int width,
                                  void* out, uint32_t* overflow, hipStream_t stream) {
    if (max_n == 0) return hipSuccess;
    if (width == 1)
        narrow_unsigned_launch(in, d_count, max_n, offset, static_cast<uint8_t*>(out), overflow, stream);
    else if (width == 2)
        narrow_unsigned_launch(in, d_count, max_n, offset, static_cast<uint16_t*>(out), overflow, stream);
    else if (width == 4)
        narrow_unsigned_launch(in, d_count, max_n, offset, static_cast<uint32_t*>(out), overflow, stream);
    else if (width == 3) {
        uint8_t* o = static_cast<uint8_t*>(out);
        if (reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(o) % 8 == 0)
            hipLaunchKernelGGL(narrow_u24_kernel, dim3(grid_for((max_n + 7) / 8)), dim3(256), 0, stream, in, d_count,
                               max_n, offset, o, overflow);
        else
            hipLaunchKernelGGL(narrow_u24_scalar_kernel, dim3(grid_for(max_n)), dim3(256), 0, stream, in, d_count, max_n,
                               offset, o, overflow);
    } else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_widen(const void* in, int src_type, uint64_t n, void* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(grid_for((n + 3) / 4)), block(256);
    switch (src_type) {
    case CUBIT_TYPE_INT8:
        hipLaunchKernelGGL((widen_kernel<int8_t, int32_t>), grid, block, 0, stream, static_cast<const int8_t*>(in), n,
                           static_cast<int32_t*>(out));
        break;
    case CUBIT_TYPE_INT16:
        hipLaunchKernelGGL((widen_kernel<int16_t, int32_t>), grid, block, 0, stream, static_cast<const int16_t*>(in), n,
                           static_cast<int32_t*>(out));
        break;
    case CUBIT_TYPE_UINT8:
        hipLaunchKernelGGL((widen_kernel<uint8_t, int32_t>), grid, block, 0, stream, static_cast<const uint8_t*>(in), n,
                           static_cast<int32_t*>(out));
        break;
    case CUBIT_TYPE_UINT16:
        hipLaunchKernelGGL((widen_kernel<uint16_t, int32_t>), grid, block, 0, stream, static_cast<const uint16_t*>(in), n,
                           static_cast<int32_t*>(out));
        break;
    case CUBIT_TYPE_UINT32:
        hipLaunchKernelGGL((widen_kernel<uint32_t, int64_t>), grid, block, 0, stream, static_cast<const uint32_t*>(in), n,
                           static_cast<int64_t*>(out));
        break;
    case CUBIT_TYPE_UINT64:  // the bits as they are; the caller checks every valid value is below 2^63
        hipLaunchKernelGGL((widen_kernel<uint64_t, int64_t>), grid, block, 0, stream, static_cast<const uint64_t*>(in), n,
                           static_cast<int64_t*>(out));
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fp_keys(const void* raw, int type, uint64_t n, void* keys, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (type == kTypeFloat)
        hipLaunchKernelGGL((fp_keys_kernel<1, int32_t>), dim3(grid_for((n + 3) / 4)), dim3(256), 0, stream,
                           static_cast<const int32_t*>(raw), n, static_cast<int32_t*>(keys));
    else if (type == kTypeDouble)
        hipLaunchKernelGGL((fp_keys_kernel<2, int64_t>), dim3(grid_for((n + 1) / 2)), dim3(256), 0, stream,
                           static_cast<const int64_t*>(raw), n, static_cast<int64_t*>(keys));
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_value_keys(const int64_t* v, uint64_t n, int type, int64_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(value_keys_kernel, dim3(grid_for(n)), dim3(256), 0, stream, v, n, type, out);
    return hipGetLastError();
}

hipError_t launch_scatter_raw(const int64_t* rows, const int64_t* v, const uint8_t* valids, uint64_t m, int type,
                              void* raw, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_raw_kernel, dim3(grid_for(m)), dim3(256), 0, stream, rows, v, valids, m,
                       type_is32(type) ? 1 : 0, raw);
    return hipGetLastError();
}

hipError_t launch_gather(const void* col, int type, const int64_t* rowids, const uint64_t* d_count, uint64_t max_n,
                         int64_t row_base, int64_t* out, hipStream_t stream) {
    const dim3 grid(grid_for(max_n, 8192)), block(256);
    // the values as stored: a FLOAT pattern zero-extended, a DOUBLE pattern as it is
    if (type == kTypeFloat)
        hipLaunchKernelGGL(gather_kernel<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t*>(col), rowids,
                           d_count, max_n, row_base, out);
    else if (type_is32(type))
        hipLaunchKernelGGL(gather_kernel<int32_t>, grid, block, 0, stream, static_cast<const int32_t*>(col), rowids,
                           d_count, max_n, row_base, out);
    else
        hipLaunchKernelGGL(gather_kernel<int64_t>, grid, block, 0, stream, static_cast<const int64_t*>(col), rowids,
                           d_count, max_n, row_base, out);
    return hipGetLastError();
}

hipError_t launch_gather_valid(const void* col, int type, const uint64_t* validity, const int64_t* rowids,
                               const uint64_t* d_count, uint64_t max_n, int64_t row_base, int64_t* out,
                               uint64_t* out_valid, hipStream_t stream) {
    const dim3 grid(grid_for(max_n, 8192)), block(256);
    if (type == kTypeFloat)
        hipLaunchKernelGGL(gather_valid_kernel<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t*>(col),
                           validity, rowids, d_count, max_n, row_base, out, out_valid);
    else if (type_is32(type))
        hipLaunchKernelGGL(gather_valid_kernel<int32_t>, grid, block, 0, stream, static_cast<const int32_t*>(col),
                           validity, rowids, d_count, max_n, row_base, out, out_valid);
    else
        hipLaunchKernelGGL(gather_valid_kernel<int64_t>, grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, rowids, d_count, max_n, row_base, out, out_valid);
    return hipGetLastError();
}

hipError_t launch_gather_sum_product(const int64_t* x, const int64_t* y, const int64_t* rowids,
                                     const uint64_t* d_count, uint64_t max_n, int64_t row_base, int64_t* partials,
                                     int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(gather_sum_product_kernel, dim3(kSumBlocks), dim3(256), 0, stream, x, y, rowids, d_count, max_n,
                       row_base, partials);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, stream, partials, kSumBlocks, out);
    return hipGetLastError();
}

unsigned sum_product_grid(unsigned n_cus) { return std::min<unsigned>(2 * n_cus, (unsigned)kSumBlocks); }

hipError_t launch_eval_sum_product(const EvalArgs& a, const SumArgs& s, unsigned grid, int64_t* out, hipStream_t st) {
    if (!s.b && s.n_decode > (uint32_t)kMaxDecode) return hipErrorInvalidValue;
    hipError_t e = dispatch_k_form(a.prog, [&](auto k, auto form) {
#define CUBIT_SUM(M) hipLaunchKernelGGL((eval_sum_product<k.value, M, form.value>), dim3(grid), dim3(512), 0, st, a, s)
        switch (s.b ? 0 : s.n_decode) {  // M: the values b is decoded from (0: gathered)
        case 0: CUBIT_SUM(0); break;
        case 1: CUBIT_SUM(1); break;
        case 2: CUBIT_SUM(2); break;
        default: CUBIT_SUM(3); break;
        }
#undef CUBIT_SUM
    });
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, st, s.partials, (int)grid, out);
    return hipGetLastError();
}

hipError_t launch_sum_product_arrays(const int64_t* x, const int64_t* y, const uint64_t* d_count, uint64_t max_n,
                                     int64_t* partials, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(sum_product_arrays_kernel, dim3(kSumBlocks), dim3(256), 0, stream, x, y, d_count, max_n,
                       partials);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, stream, partials, kSumBlocks, out);
    return hipGetLastError();
}

hipError_t launch_bitunpack(const uint8_t* bytes, const BpGroup* groups, uint64_t n_groups, int type, void* out,
                            hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_groups == 0) return hipSuccess;
    if (n_groups > 0x7fffffffull) return hipErrorInvalidValue;
    if (type == 0)
        hipExtLaunchKernelGGL((bitunpack_kernel<int32_t, uint32_t>), dim3((unsigned)n_groups), dim3(256), 0, stream,
                              start, stop, 0, bytes, groups, static_cast<int32_t*>(out));
    else
        hipExtLaunchKernelGGL((bitunpack_kernel<int64_t, uint64_t>), dim3((unsigned)n_groups), dim3(256), 0, stream,
                              start, stop, 0, bytes, groups, static_cast<int64_t*>(out));
    return hipGetLastError();
}

// ------------------------------------------------------------------ dictionary encode
// Strings (bytes + offsets, in device memory) → codes of an order-preserving dictionary (its
// entries sorted, bytes + offsets on the device): one lane per string, a binary search comparing
// bytes as unsigned then lengths (string_t's order, the host dictionary's). A NULL row gets code
// 0; a valid string the dictionary lacks gets -1 and counts into *missing.
__device__ __forceinline__ int dict_cmp(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb) {
    const uint64_t m = na < nb ? na : nb;
    for (uint64_t i = 0; i < m; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : na > nb ? 1 : 0;
}

__global__ __launch_bounds__(256) void dict_encode_kernel(const uint8_t* __restrict__ bytes,
                                                          const uint64_t* __restrict__ offs, uint64_t n,
                                                          const uint64_t* __restrict__ validity,
                                                          const uint8_t* __restrict__ dbytes,
                                                          const uint64_t* __restrict__ doffs, uint64_t dn,
                                                          int32_t* __restrict__ codes,
                                                          unsigned long long* __restrict__ missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t miss = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (validity && !((validity[i >> 6] >> (i & 63)) & 1ull)) {
            codes[i] = 0;
            continue;
        }
        const uint8_t* s = bytes + offs[i];
        const uint64_t ns = offs[i + 1] - offs[i];
        uint64_t lo = 0, hi = dn;  // first entry >= s
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (dict_cmp(dbytes + doffs[mid], doffs[mid + 1] - doffs[mid], s, ns) < 0) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo < dn && dict_cmp(dbytes + doffs[lo], doffs[lo + 1] - doffs[lo], s, ns) == 0;
        codes[i] = found ? (int32_t)lo : -1;
        miss += found ? 0u : 1u;
    }
    // one add per wave that saw a miss
    for (int o = 32; o > 0; o >>= 1) miss += __shfl_down(miss, o, 64);
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(missing, (unsigned long long)miss);
}

hipError_t launch_dict_encode(const uint8_t* bytes, const uint64_t* offs, uint64_t n, const uint64_t* validity,
                              const uint8_t* dbytes, const uint64_t* doffs, uint64_t dn, int32_t* codes,
                              unsigned long long* missing, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(dict_encode_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bytes, offs, n, validity, dbytes,
                       doffs, dn, codes, missing);
    return hipGetLastError();
}

// ------------------------------------------------------------------ RLE expand
// DuckDB RLE segments (src/storage/compression/rle.cpp) expanded into a plain column. The host
// has parsed every segment into runs — the run values (already widened to the column's type) and
// each run's end row (exclusive, cumulative over the partition; zero-length runs, which the
// reference writes after a run of exactly 65,535 rows, repeat the previous end). Workgroups take
// 2,048-row tiles in turn; a tile's runs, from its first row's through its last row's, are known
// beforehand (rle_tile_first_kernel, a lane per tile). A tile inside one run or across one
// boundary is filled straight from those two runs; otherwise its runs are staged in LDS and each
// lane finds the run of its first of 8 consecutive rows by binary search and walks on from it.
// Every lane writes its 8 rows as 16-byte stores.
// tile_first[b] = the first run ending past row 2,048·b (b = 0 … tiles; n_runs past the end): one
// lane per tile, so the dependent loads of the searches overlap across the whole grid
__global__ __launch_bounds__(256) void rle_tile_first_kernel(const uint64_t* __restrict__ ends, uint64_t n_runs,
                                                             uint64_t n_tiles, uint64_t* __restrict__ tile_first) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_tiles) return;
    const uint64_t r = b * 2048;
    uint64_t lo = 0, hi = n_runs;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (ends[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    tile_first[b] = lo;
}

template <typename T, int PER>
__device__ __forceinline__ void rle_store(T* __restrict__ out, uint64_t r0, uint64_t t1, const T (&v)[PER]) {
    if (r0 + PER <= t1) {  // 32 / 64 contiguous bytes per lane, 16-byte stores
        using V = __attribute__((ext_vector_type(4))) uint32_t;
        V* o = reinterpret_cast<V*>(out + r0);
#pragma unroll
        for (int q = 0; q < (int)(PER * sizeof(T) / 16); ++q) {
            V w;
            __builtin_memcpy(&w, reinterpret_cast<const char*>(v) + 16 * q, 16);
            o[q] = w;
        }
    } else {
        for (int k = 0; k < PER && r0 + k < t1; ++k) out[r0 + k] = v[k];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void rle_expand_kernel(const T* __restrict__ vals, const uint64_t* __restrict__ ends,
                                                         const uint64_t* __restrict__ tile_first, uint64_t n_runs,
                                                         uint64_t n_rows, T* __restrict__ out) {
    constexpr int TILE = 2048, PER = 8, WIN = 2064;  // a tile holds at most 2,048 non-empty runs (+ one empty)
    __shared__ uint64_t s_end[WIN];
    __shared__ T s_val[WIN];
    const uint64_t n_tiles = (n_rows + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // tile-uniform control flow
        const uint64_t t0 = tile * TILE;
        const uint64_t t1 = t0 + TILE < n_rows ? t0 + TILE : n_rows;
        const uint64_t r0 = t0 + (uint64_t)threadIdx.x * PER;
        // the tile's runs: from the first ending past t0 through the first ending past t1 (one
        // more than needed when a run ends at t1 exactly), within the partition's runs
        const uint64_t first = tile_first[tile];
        const uint64_t stop = tile_first[tile + 1] < n_runs ? tile_first[tile + 1] + 1 : n_runs;
        const uint64_t cnt = stop - first;
        T v[PER];
        if (cnt <= 2) {  // inside one run or across one boundary (long runs): no staging
            const uint64_t e0 = ends[first];
            const T a = vals[first], b = cnt == 2 ? vals[first + 1] : a;
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = r0 + k < e0 ? a : b;
            if (r0 < t1) rle_store<T, PER>(out, r0, t1, v);
            continue;
        }
        if (cnt <= (uint64_t)WIN) {
            // the tile's runs in LDS; each lane expands 8 consecutive rows: one search, then a walk
            for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
                s_end[i] = ends[first + i];
                s_val[i] = vals[first + i];
            }
            __syncthreads();
            if (r0 < t1) {
                uint32_t lo = 0, hi = (uint32_t)cnt - 1;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (s_end[mid] > r0) hi = mid;
                    else lo = mid + 1;
                }
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    while (lo + 1 < cnt && s_end[lo] <= r0 + k) ++lo;
                    v[k] = s_val[lo];
                }
                rle_store<T, PER>(out, r0, t1, v);
            }
            __syncthreads();  // the LDS is the next tile's
            continue;
        }
        // more runs than the window (not produced by DuckDB's writer): windows of runs in turn
        uint64_t f = first, row = t0;
        while (row < t1 && f < n_runs) {
            const uint64_t c = n_runs - f < (uint64_t)WIN ? n_runs - f : (uint64_t)WIN;
            for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
                s_end[i] = ends[f + i];
                s_val[i] = vals[f + i];
            }
            __syncthreads();
            const uint64_t covered = s_end[c - 1] < t1 ? s_end[c - 1] : t1;
            for (uint64_t r = row + threadIdx.x; r < covered; r += blockDim.x) {
                uint32_t lo = 0, hi = (uint32_t)c - 1;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (s_end[mid] > r) hi = mid;
                    else lo = mid + 1;
                }
                out[r] = s_val[lo];
            }
            row = covered;
            f += c;
            __syncthreads();
        }
    }
}

hipError_t launch_rle_expand(const void* vals, const uint64_t* ends, uint64_t n_runs, uint64_t n_rows, int type,
                             uint64_t* tile_first, void* out, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_rows == 0) return hipSuccess;
    const uint64_t tiles = (n_rows + 2047) / 2048;
    if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
    // timed from the first kernel's start to the second's end
    hipExtLaunchKernelGGL(rle_tile_first_kernel, dim3((unsigned)((tiles + 1 + 255) / 256)), dim3(256), 0, stream, start,
                          nullptr, 0, ends, n_runs, tiles, tile_first);
    const unsigned grid = (unsigned)std::min<uint64_t>(tiles, 256 * 16);  // 16 workgroups per CU, tiles in turn
    if (type == 0)
        hipExtLaunchKernelGGL(rle_expand_kernel<int32_t>, dim3(grid), dim3(256), 0, stream, nullptr, stop, 0,
                              static_cast<const int32_t*>(vals), ends, tile_first, n_runs, n_rows,
                              static_cast<int32_t*>(out));
    else
        hipExtLaunchKernelGGL(rle_expand_kernel<int64_t>, dim3(grid), dim3(256), 0, stream, nullptr, stop, 0,
                              static_cast<const int64_t*>(vals), ends, tile_first, n_runs, n_rows,
                              static_cast<int64_t*>(out));
    return hipGetLastError();
}

hipError_t launch_masked_compare(const void* col, int type, const uint64_t* validity, const uint64_t* mask,
                                 uint64_t n_rows, int cmp, int64_t constant, uint64_t* out, hipStream_t stream) {
    const uint64_t nw = padded_words(n_rows);
    const CmpRange r = cmp_range(cmp, constant, 0);
    const dim3 grid(grid_for(nw / 2)), block(256);
    if (type_is32(type)) {
        int32_t lo32, hi32;
        r.clamp32(lo32, hi32);
        if (type == kTypeFloat)
            hipLaunchKernelGGL((masked_compare_kernel<int32_t, 1>), grid, block, 0, stream,
                               static_cast<const int32_t*>(col), validity, mask, nw, lo32, hi32, r.neg, out);
        else
            hipLaunchKernelGGL(masked_compare_kernel<int32_t>, grid, block, 0, stream, static_cast<const int32_t*>(col),
                               validity, mask, nw, lo32, hi32, r.neg, out);
    } else if (type == kTypeDouble) {
        hipLaunchKernelGGL((masked_compare_kernel<int64_t, 2>), grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, mask, nw, r.lo, r.hi, r.neg, out);
    } else if (type == kTypeUInt64) {
        hipLaunchKernelGGL(masked_compare_kernel<uint64_t>, grid, block, 0, stream, static_cast<const uint64_t*>(col),
                           validity, mask, nw, (uint64_t)r.lo ^ 0x8000000000000000ull,
                           (uint64_t)r.hi ^ 0x8000000000000000ull, r.neg, out);
    } else {
        hipLaunchKernelGGL(masked_compare_kernel<int64_t>, grid, block, 0, stream, static_cast<const int64_t*>(col),
                           validity, mask, nw, r.lo, r.hi, r.neg, out);
    }
    return hipGetLastError();
}

hipError_t launch_bitpacked_compare(const uint8_t* bytes, const BpGroup* groups, uint64_t n_groups, int type,
                                    const uint64_t* validity, int cmp, int64_t constant, int64_t constant2,
                                    uint64_t* out, hipStream_t stream, int simple_width) {
    if (n_groups == 0) return hipSuccess;
    if (n_groups > 0x7fffffffull) return hipErrorInvalidValue;
    const CmpRange rg = cmp_range(cmp, constant, constant2);
    const int64_t lo = rg.lo, hi = rg.hi;
    const int neg = rg.neg;
    const uint32_t ng = (uint32_t)n_groups;
    if (simple_width > 0) {  // every group FOR ≤ 32 bits / CONSTANT / CONSTANT_DELTA: one wave per group
        const dim3 grid((ng + 3) / 4);
        if (type == 0) {
            int32_t lo32, hi32;
            rg.clamp32(lo32, hi32);
            if (simple_width <= 16)
                hipLaunchKernelGGL((bitpacked_compare_waves<int32_t, uint32_t, 16>), grid, dim3(256), 0, stream, bytes,
                                   groups, ng, validity, lo32, hi32, neg, out);
            else
                hipLaunchKernelGGL((bitpacked_compare_waves<int32_t, uint32_t, 32>), grid, dim3(256), 0, stream, bytes,
                                   groups, ng, validity, lo32, hi32, neg, out);
        } else {
            if (simple_width <= 16)
                hipLaunchKernelGGL((bitpacked_compare_waves<int64_t, uint64_t, 16>), grid, dim3(256), 0, stream, bytes,
                                   groups, ng, validity, lo, hi, neg, out);
            else
                hipLaunchKernelGGL((bitpacked_compare_waves<int64_t, uint64_t, 32>), grid, dim3(256), 0, stream, bytes,
                                   groups, ng, validity, lo, hi, neg, out);
        }
        return hipGetLastError();
    }
    if (type == 0) {
        int32_t lo32, hi32;
        rg.clamp32(lo32, hi32);
        constexpr int GPW = 4;  // groups per workgroup, their loads all in flight together
        hipLaunchKernelGGL((bitpacked_compare_kernel<int32_t, uint32_t, GPW>), dim3((ng + GPW - 1) / GPW), dim3(256),
                           0, stream, bytes, groups, ng, validity, lo32, hi32, neg, out);
    } else {
        constexpr int GPW = 2;  // 16 KiB spans
        hipLaunchKernelGGL((bitpacked_compare_kernel<int64_t, uint64_t, GPW>), dim3((ng + GPW - 1) / GPW), dim3(256),
                           0, stream, bytes, groups, ng, validity, lo, hi, neg, out);
    }
    return hipGetLastError();
}

hipError_t launch_fill_valid(uint64_t* words, uint64_t n_rows, hipStream_t stream) {
    const uint64_t nw = padded_words(n_rows);
    hipLaunchKernelGGL(fill_valid_kernel, dim3(grid_for(nw)), dim3(256), 0, stream, words, n_rows, nw);
    return hipGetLastError();
}

hipError_t launch_zone_classes(const uint64_t* bv, uint64_t n_rows, uint32_t z0, uint32_t nz, uint8_t* out,
                               hipStream_t stream, uint32_t* cnt) {
    if (nz == 0) return hipSuccess;
    hipLaunchKernelGGL(zone_class_kernel, dim3(nz), dim3(256), 0, stream, bv, n_rows, z0, out, cnt);
    return hipGetLastError();
}

hipError_t launch_column_zone_stats(const void* col, int type, const uint64_t* validity, uint64_t n_rows, uint32_t nz,
                                    int64_t* mn, int64_t* mx, uint8_t* fl, hipStream_t stream) {
    if (nz == 0) return hipSuccess;
    if (type == kTypeFloat)
        hipLaunchKernelGGL((column_zone_stats_kernel<int32_t, 1>), dim3(nz), dim3(256), 0, stream,
                           static_cast<const int32_t*>(col), validity, n_rows, mn, mx, fl);
    else if (type == kTypeDouble)
        hipLaunchKernelGGL((column_zone_stats_kernel<int64_t, 2>), dim3(nz), dim3(256), 0, stream,
                           static_cast<const int64_t*>(col), validity, n_rows, mn, mx, fl);
    else if (type == kTypeUInt64)
        hipLaunchKernelGGL((column_zone_stats_kernel<int64_t, 3>), dim3(nz), dim3(256), 0, stream,
                           static_cast<const int64_t*>(col), validity, n_rows, mn, mx, fl);
    else if (type_is32(type))
        hipLaunchKernelGGL(column_zone_stats_kernel<int32_t>, dim3(nz), dim3(256), 0, stream,
                           static_cast<const int32_t*>(col), validity, n_rows, mn, mx, fl);
    else
        hipLaunchKernelGGL(column_zone_stats_kernel<int64_t>, dim3(nz), dim3(256), 0, stream,
                           static_cast<const int64_t*>(col), validity, n_rows, mn, mx, fl);
    return hipGetLastError();
}

hipError_t launch_visibility(const int64_t* del_rows, const uint64_t* del_ids, uint64_t n_del, uint64_t n_rows,
                             uint64_t start_time, uint64_t transaction_id, uint64_t* words, hipStream_t stream,
                             const int64_t* hidden_ranges, uint32_t n_hidden) {
    hipError_t e = launch_fill_valid(words, n_rows, stream);
    if (e != hipSuccess) return e;
    for (uint32_t r0 = 0; r0 < n_hidden; r0 += 65535) {
        const unsigned ny = (unsigned)std::min<uint32_t>(65535, n_hidden - r0);
        hipLaunchKernelGGL(clear_ranges_kernel, dim3(64, ny), dim3(256), 0, stream, hidden_ranges + 2 * (uint64_t)r0,
                           words);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (n_del == 0) return hipSuccess;
    hipLaunchKernelGGL(visibility_kernel, dim3(grid_for(n_del)), dim3(256), 0, stream, del_rows, del_ids, n_del,
                       start_time, transaction_id, words);
    return hipGetLastError();
}

hipError_t launch_splice_bits(uint64_t* dst, const uint64_t* src, uint64_t bit_off, uint64_t n_bits,
                              hipStream_t stream) {
    if (n_bits == 0) return hipSuccess;
    const uint64_t words = ((bit_off + n_bits + 63) >> 6) - (bit_off >> 6);
    hipLaunchKernelGGL(splice_bits_kernel, dim3(grid_for(words)), dim3(256), 0, stream, dst, src, bit_off, n_bits);
    return hipGetLastError();
}

hipError_t launch_merge_words(const int64_t* rows, const int64_t* values, const uint8_t* valids, uint64_t m,
                              uint64_t n_rows, void* col, int type, uint64_t* validity, MergeIndex ix0, MergeIndex ix1,
                              hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(merge_words_kernel, dim3(grid_for(m)), dim3(256), 0, stream, rows, values, valids, m,
                       n_rows, col, type, validity, ix0, ix1);
    return hipGetLastError();
}

hipError_t launch_column_diff(const void* old_col, const uint64_t* old_valid, const void* new_col,
                              const uint64_t* new_valid, int type, uint64_t n_rows, uint64_t* changed,
                              uint64_t* counter, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    const uint64_t nw = padded_words(n_rows), n_words = (n_rows + 63) / 64;
    // the compare kernel's grid: four waves per workgroup, a wave per 64 words
    const dim3 grid((unsigned)std::max<uint64_t>(std::min<uint64_t>((nw / 64 + 3) / 4, 8192), 1)), block(256);
    auto* cnt = reinterpret_cast<unsigned long long*>(counter);
    if (type_is32(type))
        hipExtLaunchKernelGGL(column_diff_kernel<uint32_t>, grid, block, 0, stream, ev0, ev1, 0,
                              static_cast<const uint32_t*>(old_col), old_valid, static_cast<const uint32_t*>(new_col),
                              new_valid, n_rows, n_words, nw, changed, cnt);
    else
        hipExtLaunchKernelGGL(column_diff_kernel<uint64_t>, grid, block, 0, stream, ev0, ev1, 0,
                              static_cast<const uint64_t*>(old_col), old_valid, static_cast<const uint64_t*>(new_col),
                              new_valid, n_rows, n_words, nw, changed, cnt);
    return hipGetLastError();
}

hipError_t launch_sync_gather(const void* new_col, const uint64_t* new_valid, int type, const int64_t* rows, uint64_t m,
                              int64_t* values, uint8_t* valids, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    const dim3 grid(grid_for(m)), block(256);
    if (type == kTypeFloat)  // the pattern zero-extended, as the probe hands it back
        hipLaunchKernelGGL(sync_gather_kernel<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t*>(new_col),
                           new_valid, rows, m, values, valids);
    else if (type_is32(type))
        hipLaunchKernelGGL(sync_gather_kernel<int32_t>, grid, block, 0, stream, static_cast<const int32_t*>(new_col),
                           new_valid, rows, m, values, valids);
    else
        hipLaunchKernelGGL(sync_gather_kernel<int64_t>, grid, block, 0, stream, static_cast<const int64_t*>(new_col),
                           new_valid, rows, m, values, valids);
    return hipGetLastError();
}

hipError_t launch_update_mask(const int64_t* upd_rows, const uint64_t* upd_versions, uint64_t n_upd,
                              uint64_t start_time, uint64_t transaction_id, uint64_t* mask, hipStream_t stream) {
    if (n_upd == 0) return hipSuccess;
    hipLaunchKernelGGL(update_mask_kernel, dim3(grid_for(n_upd)), dim3(256), 0, stream, upd_rows, upd_versions, n_upd,
                       start_time, transaction_id, mask);
    return hipGetLastError();
}

}  // namespace cubit
