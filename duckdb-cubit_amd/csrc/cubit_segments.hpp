// The host arithmetic of DuckDB-segment ingest, free of HIP so a CPU program can run it
// (tests/segment_walk_bounds.cpp): the type table, the BpGroup record the kernels read, and the
// walkers that turn one BITPACKING or RLE segment's bytes into a SegmentPlan, every read bounds-checked.
// A walker reports a refusal as a CUBIT_ERR_* code and a message in the caller's buffer.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cubit_gpu.h"

namespace cubit {

// K5: DuckDB BITPACKING groups → plain values. One record per 2,048-value metadata group
// (mode: 2 CONSTANT, 3 CONSTANT_DELTA, 4 DELTA_FOR, 5 FOR — BitpackingMode).
// The host reads each group's header (the T-sized fields before the packed words) into the
// record, so a workgroup's only dependent load chain is record → packed words.
struct BpGroup {
    uint64_t words_off;  // byte offset of the packed words (FOR / DELTA_FOR)
    uint64_t row_start;  // first row of the group
    uint64_t base;       // CONSTANT value | CONSTANT_DELTA first | FOR minimum | DELTA_FOR min_delta (T bits)
    uint64_t aux;        // CONSTANT_DELTA delta | DELTA_FOR delta_offset (T bits)
    uint32_t count;      // rows in the group (≤ 2,048)
    uint8_t mode;
    // the segments' T when narrower than the column's values (an 8- / 16-bit T in an INT32
    // column, UINT32 in an INT64 column): its bits | 0x80 when signed; 0 = T is the column's
    // type. Decoded values are taken mod 2^bits and sign- or zero-extended (bp_norm), which is
    // T's own wrap-around arithmetic
    uint8_t tnorm;
    uint16_t width;      // bit width of the packed values (FOR / DELTA_FOR)
};
// the layout the kernels were built against
static_assert(sizeof(BpGroup) == 40 && offsetof(BpGroup, words_off) == 0 && offsetof(BpGroup, row_start) == 8 &&
                  offsetof(BpGroup, base) == 16 && offsetof(BpGroup, aux) == 24 && offsetof(BpGroup, count) == 32 &&
                  offsetof(BpGroup, mode) == 36 && offsetof(BpGroup, tnorm) == 37 && offsetof(BpGroup, width) == 38,
              "BpGroup is read by the kernels");

// A CUBIT_TYPE_* code: its value size and signedness, the column type its values are held as
// (INT8, INT16, UINT8, UINT16 → INT32; UINT32 → INT64; UINT64 its bits, keyed; VARCHAR its codes),
// the BpGroup::tnorm that carries T's arithmetic there, and whether the code may name a segment's T.
struct TypeInfo {
    uint32_t size;
    bool sgn;
    int col_type;
    uint8_t tnorm;
    bool segment;
};
// null for an unknown code
inline const TypeInfo* type_info(int type) {
    static const TypeInfo table[] = {
        /* INT32   */ {4, true, CUBIT_TYPE_INT32, 0, true},
        /* INT64   */ {8, true, CUBIT_TYPE_INT64, 0, true},
        /* INT8    */ {1, true, CUBIT_TYPE_INT32, 8 | 0x80, true},
        /* INT16   */ {2, true, CUBIT_TYPE_INT32, 16 | 0x80, true},
        /* UINT8   */ {1, false, CUBIT_TYPE_INT32, 8, true},
        /* UINT16  */ {2, false, CUBIT_TYPE_INT32, 16, true},
        /* UINT32  */ {4, false, CUBIT_TYPE_INT64, 32, true},
        /* UINT64  */ {8, false, CUBIT_TYPE_UINT64, 0, true},
        /* FLOAT   */ {4, true, CUBIT_TYPE_FLOAT, 0, false},
        /* DOUBLE  */ {8, true, CUBIT_TYPE_DOUBLE, 0, false},
        /* VARCHAR */ {4, true, CUBIT_TYPE_VARCHAR, 0, false},
    };
    static_assert(CUBIT_TYPE_INT32 == 0 && CUBIT_TYPE_INT64 == 1 && CUBIT_TYPE_INT8 == 2 && CUBIT_TYPE_INT16 == 3 &&
                      CUBIT_TYPE_UINT8 == 4 && CUBIT_TYPE_UINT16 == 5 && CUBIT_TYPE_UINT32 == 6 &&
                      CUBIT_TYPE_UINT64 == 7 && CUBIT_TYPE_FLOAT == 8 && CUBIT_TYPE_DOUBLE == 9 &&
                      CUBIT_TYPE_VARCHAR == 10, "the table is indexed by type code");
    return type >= 0 && type <= CUBIT_TYPE_VARCHAR ? &table[type] : nullptr;
}
// the type of a segment's T, null for any other code
inline const TypeInfo* segment_type(int type) {
    const TypeInfo* ti = type_info(type);
    return ti && ti->segment ? ti : nullptr;
}

// What a column's segments ask of the device. One run list (values as T widened to int64, each run's
// end row) covers the rows that rle_expand_kernel writes; the BITPACKING groups are unpacked over
// their rows, with the packed runs off the 4-byte alignment copied 16-aligned into `moved`, which
// goes behind the padded bytes; the UNCOMPRESSED spans are copied or widened over theirs.
struct SegmentPlan {
    struct Span {
        uint64_t off, rows, row;  // byte offset, rows, first row
    };
    std::vector<int64_t> vals;
    std::vector<uint64_t> ends;
    std::vector<BpGroup> groups;
    std::vector<uint8_t> moved;
    std::vector<Span> plain;
    uint64_t rows = 0;  // rows covered so far: the next segment's first row
};

inline int refuse(char* err, size_t err_len, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, err_len, fmt, ap);
    va_end(ap);
    return code;
}

// The groups of BITPACKING segment `sg` (at byte `base`, `rows` rows from row p.rows): each group's
// mode, header fields and packed words, bounds-checked (header = end of the metadata words, one word
// per 2,048-row group, highest address first: BitpackingScanState / LoadNextGroup,
// bitpacking.cpp:620-690). A T of 1 or 2 bytes leaves packed runs off the 4-byte alignment the
// kernels' word loads need (the header fields are T-sized, WriteData, :448-451): those are moved, to
// bytes_padded + their offset in p.moved.
inline int walk_bp_segment(const uint8_t* bytes, uint64_t n_bytes, uint64_t base, uint64_t rows, const TypeInfo& ti,
                           uint64_t bytes_padded, uint32_t sg, SegmentPlan& p, char* err, size_t err_len) {
    const uint64_t tsz = ti.size;
    if (base % 8 || base + 8 > n_bytes) return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: bad offset", sg);
    uint64_t meta_end;
    std::memcpy(&meta_end, bytes + base, 8);
    const uint64_t n_groups = (rows + 2047) / 2048;
    if (meta_end > n_bytes - base || meta_end < 8 + 4 * n_groups)
        return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: bad metadata offset", sg);
    for (uint64_t g = 0; g < n_groups; ++g) {
        uint32_t enc;
        std::memcpy(&enc, bytes + base + meta_end - 4 * (g + 1), 4);
        BpGroup bg{};
        const uint32_t mode = enc >> 24;
        const uint64_t data_off = base + (enc & 0x00ffffffu);
        bg.mode = (uint8_t)mode;
        bg.tnorm = ti.tnorm;
        bg.row_start = p.rows + g * 2048;
        bg.count = (uint32_t)std::min<uint64_t>(2048, rows - g * 2048);
        const uint64_t n_fields = mode == 2 ? 1 : (mode == 3 || mode == 5) ? 2 : mode == 4 ? 3 : 0;
        if (n_fields == 0)
            return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u group %llu: mode %u", sg, (unsigned long long)g, mode);
        if (data_off < base + 8 || data_off + n_fields * tsz > n_bytes)
            return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u group %llu: out of bounds", sg, (unsigned long long)g);
        auto field = [&](uint64_t i) {
            uint64_t v = 0;  // T's bits, zero-extended (the kernels work mod 2^bits: bp_norm)
            std::memcpy(&v, bytes + data_off + i * tsz, tsz);
            return v;
        };
        bg.base = field(0);
        uint64_t packed = 0;
        if (mode == 3) {
            bg.aux = field(1);
        } else if (mode == 4 || mode == 5) {
            const uint64_t w = field(1) & 0xff;  // the reference reads the width as a T, uses its low byte
            if (w > 8 * tsz)
                return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u group %llu: width %u", sg, (unsigned long long)g,
                              (unsigned)w);
            bg.width = (uint16_t)w;
            if (mode == 4) bg.aux = field(2);
            packed = ((uint64_t)bg.count + 31) / 32 * 32 * w / 8;
        }
        bg.words_off = data_off + n_fields * tsz;
        if (bg.words_off + packed > n_bytes)
            return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u group %llu: out of bounds", sg, (unsigned long long)g);
        if (packed && bg.words_off % 4) {
            const uint64_t at = p.moved.size();
            p.moved.resize(at + (packed + 15) / 16 * 16, 0);
            std::memcpy(p.moved.data() + at, bytes + bg.words_off, packed);
            bg.words_off = bytes_padded + at;
        }
        p.groups.push_back(bg);
    }
    p.rows += rows;
    return CUBIT_OK;
}

// The runs of RLE segment `sg` (at byte `base`, `rows` rows from row p.rows; rle.cpp
// RLECompressState::FlushSegment, :190-205: 8-byte header = offset of the uint16 run lengths, the run
// values as T from byte 8, the lengths after them): run lengths are read until they cover the
// segment's rows (RLEScanState, :248-277 — zero-length runs, which a run of exactly 65,535 rows
// leaves behind, included), each value widened to int64 with T's sign.
inline int walk_rle_segment(const uint8_t* bytes, uint64_t n_bytes, uint64_t base, uint64_t rows, const TypeInfo& ti,
                            uint32_t sg, SegmentPlan& p, char* err, size_t err_len) {
    const uint64_t tsz = ti.size;
    if (base + 8 > n_bytes) return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: bad offset", sg);
    uint64_t off;
    std::memcpy(&off, bytes + base, 8);
    if (off < 8 || off > n_bytes - base)
        return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: bad run-length offset", sg);
    uint64_t covered = 0;
    for (uint64_t k = 0; covered < rows; ++k) {
        if (8 + (k + 1) * tsz > off || off + 2 * (k + 1) > n_bytes - base)
            return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: runs cover %llu of %llu rows", sg,
                          (unsigned long long)covered, (unsigned long long)rows);
        uint16_t len;
        std::memcpy(&len, bytes + base + off + 2 * k, 2);
        uint64_t raw = 0;  // T's bits, zero-extended, then widened as T
        std::memcpy(&raw, bytes + base + 8 + k * tsz, tsz);
        int64_t v = (int64_t)raw;
        if (ti.sgn && tsz < 8) v = (int64_t)(raw << (64 - 8 * tsz)) >> (64 - 8 * tsz);
        covered += len;
        if (covered > rows) return refuse(err, err_len, CUBIT_ERR_INVALID, "segment %u: runs overrun its rows", sg);
        p.vals.push_back(v);
        p.ends.push_back(p.rows + covered);
    }
    p.rows += rows;
    return CUBIT_OK;
}

}  // namespace cubit
