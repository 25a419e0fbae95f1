// The engine-independent part of the DuckDB extension shim (cubit_extension.cpp): everything
// here works on raw bytes and std containers, so it runs — and is tested — without DuckDB
// (shim/cubit_shim_core_capi.cpp, tests/test_shim_core.py, tests/shim_core_bounds.cpp).
// cubit_gpu.h is used for its CUBIT_* constants and inline helpers only: nothing here calls into
// libcubitgpu. Nothing throws across this interface: a refusal is `false` or a status.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "cubit_gpu.h"

namespace cubit_shim {

// ------------------------------------------------------------------ type table

// DuckDB's PhysicalType as far as the shim distinguishes it (its one switch over PhysicalType maps
// onto this).
enum class Phys { Bool, I8, I16, I32, I64, U8, U16, U32, U64, F32, F64, Varchar, I128, U128, Unsupported };

// What the shim needs to know about a physical type.
//  gpu: the GPU compares its values exactly, carried as int64 — the signed integers up to 64 bits
//    (DATE, TIME, TIMESTAMP*, DECIMAL(≤18) included), BOOLEAN, the unsigned integers up to 32 bits,
//    FLOAT / DOUBLE as their bit patterns (the library compares them with DuckDB's floating-point
//    operators, include/cubit_gpu.h), UBIGINT as its bits (compared unsigned), VARCHAR as int32
//    codes of the table's order-preserving dictionary (constants cross as cubit_strings), and
//    HUGEINT / UHUGEINT as codes of a dictionary over their 16-byte order keys (cubit_key128: the
//    codes are the values' ranks; constants cross as cubit_strings over keys);
//  dict: held as dictionary codes — VARCHAR (the strings), HUGEINT / UHUGEINT (their order keys);
//  wide: uploaded from 8-byte values (INT64, UINT32 widened, UINT64 bits, DOUBLE patterns; else
//    from 4-byte ones);
//  upload_type: the CUBIT_TYPE_* a column is registered as;
//  segment_type: the CUBIT_TYPE_* of a column's BITPACKING segments — the T DuckDB packs its
//    physical type with (bitpacking.cpp:953-977, BOOL as int8_t); -1 for a type whose segments the
//    partition does not read;
//  width: that T's size in bytes (0 without a segment type).
struct PhysTraits {
    bool gpu, dict, wide;
    int upload_type, segment_type, width;
};

constexpr PhysTraits TraitsOf(Phys p) {
    switch (p) {
    case Phys::Bool: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_INT8, 1};
    case Phys::I8: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_INT8, 1};
    case Phys::I16: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_INT16, 2};
    case Phys::I32: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_INT32, 4};
    case Phys::I64: return {true, false, true, CUBIT_TYPE_INT64, CUBIT_TYPE_INT64, 8};
    case Phys::U8: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_UINT8, 1};
    case Phys::U16: return {true, false, false, CUBIT_TYPE_INT32, CUBIT_TYPE_UINT16, 2};
    case Phys::U32: return {true, false, true, CUBIT_TYPE_INT64, CUBIT_TYPE_UINT32, 4};
    case Phys::U64: return {true, false, true, CUBIT_TYPE_UINT64, CUBIT_TYPE_UINT64, 8};  // the bits, compared unsigned
    case Phys::F32: return {true, false, false, CUBIT_TYPE_FLOAT, -1, 0};
    case Phys::F64: return {true, false, true, CUBIT_TYPE_DOUBLE, -1, 0};
    case Phys::Varchar: return {true, true, false, CUBIT_TYPE_INT32, -1, 0};  // codes of a cubit_dict
    case Phys::I128: return {true, true, false, CUBIT_TYPE_INT32, -1, 0};     // codes over the order keys
    case Phys::U128: return {true, true, false, CUBIT_TYPE_INT32, -1, 0};
    case Phys::Unsupported: break;
    }
    return {false, false, false, -1, -1, 0};
}

// ------------------------------------------------------------------ values

inline uint32_t FloatBits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
inline int64_t DoubleBits(double d) {
    int64_t b;
    memcpy(&b, &d, 8);
    return b;
}

template <class T>
inline T LoadAs(const void *data, size_t i) {
    T v;
    memcpy(&v, static_cast<const unsigned char *>(data) + i * sizeof(T), sizeof(T));
    return v;
}

// element i of an array of an integer-backed physical type, as int64
inline int64_t LoadInt64(Phys t, const void *data, size_t i) {
    switch (t) {
    case Phys::Bool: return LoadAs<uint8_t>(data, i) ? 1 : 0;
    case Phys::U8: return LoadAs<uint8_t>(data, i);
    case Phys::U16: return LoadAs<uint16_t>(data, i);
    case Phys::U32: return LoadAs<uint32_t>(data, i);
    case Phys::I8: return LoadAs<int8_t>(data, i);
    case Phys::I16: return LoadAs<int16_t>(data, i);
    case Phys::I32: return LoadAs<int32_t>(data, i);
    case Phys::F32: return FloatBits(LoadAs<float>(data, i));  // the pattern, zero-extended
    case Phys::F64: return DoubleBits(LoadAs<double>(data, i));
    default: return LoadAs<int64_t>(data, i);  // BIGINT; UBIGINT: the bits
    }
}

template <class T>
inline void Narrow(const int64_t *src, void *dst, size_t n) {
    auto d = static_cast<T *>(dst);
    for (size_t i = 0; i < n; i++) {
        d[i] = (T)src[i];
    }
}

// int64 staging → an array of the column's physical type (DATE / INTEGER narrow, BIGINT / DECIMAL /
// DOUBLE patterns copy)
inline void StoreFromInt64(Phys t, void *dst, const int64_t *src, size_t n) {
    switch (t) {
    case Phys::Bool: Narrow<bool>(src, dst, n); break;
    case Phys::U8: Narrow<uint8_t>(src, dst, n); break;
    case Phys::U16: Narrow<uint16_t>(src, dst, n); break;
    case Phys::U32: Narrow<uint32_t>(src, dst, n); break;
    case Phys::I8: Narrow<int8_t>(src, dst, n); break;
    case Phys::I16: Narrow<int16_t>(src, dst, n); break;
    case Phys::I32: Narrow<int32_t>(src, dst, n); break;
    case Phys::F32:  // the 32-bit patterns back into the floats (DOUBLE: the 8-byte copy below)
        for (size_t i = 0; i < n; i++) {
            const uint32_t u = (uint32_t)src[i];
            memcpy(static_cast<unsigned char *>(dst) + 4 * i, &u, 4);
        }
        break;
    default: memcpy(dst, src, n * sizeof(int64_t)); break;
    }
}

// bit r of DuckDB validity words (LSB first)
inline bool RowValid(const uint64_t *words, uint64_t r) {
    return (words[r >> 6] >> (r & 63)) & 1;
}

// ------------------------------------------------------------------ segment images

// One ColumnSegmentInfo row, as far as the attach reads it.
struct SegmentDesc {
    uint64_t start, count;   // segment_start (an absolute row), segment_count
    std::string codec_name;  // compression_type
    bool has_updates, persistent;
    std::string stats;  // segment_stats
};

// CompressionTypeToString of the four codecs the GPU reads.
struct CodecNames {
    std::string bitpacking, rle, constant, uncompressed;
};

// The CUBIT_CODEC_* of every segment of a column when the column can be registered from its
// segments: `descs` (sorted by start) hold rows [0, n_rows) in order without gaps, none has
// in-memory updates, every codec is one the GPU reads — BITPACKING (unpacked), RLE (runs expanded),
// CONSTANT (one value, from the segment's statistics), UNCOMPRESSED (the values) — and every
// segment with bytes is persistent. False otherwise: the caller uploads decoded values.
inline bool PlanSegments(const std::vector<SegmentDesc> &descs, uint64_t n_rows, const CodecNames &names,
                         std::vector<int32_t> &codecs) {
    codecs.clear();
    uint64_t next = 0;
    for (auto &sg : descs) {
        if (sg.has_updates || sg.start != next) {
            return false;
        }
        int32_t codec = -1;
        if (sg.codec_name == names.bitpacking) {
            codec = CUBIT_CODEC_BITPACKING;
        } else if (sg.codec_name == names.rle) {
            codec = CUBIT_CODEC_RLE;
        } else if (sg.codec_name == names.uncompressed) {
            codec = CUBIT_CODEC_UNCOMPRESSED;
        } else if (sg.codec_name == names.constant) {
            codec = CUBIT_CODEC_CONSTANT;
        }
        if (codec < 0 || (codec != CUBIT_CODEC_CONSTANT && !sg.persistent)) {
            return false;
        }
        codecs.push_back(codec);
        next += sg.count;
    }
    return next == n_rows && !descs.empty();
}

// A CONSTANT segment's value: ConstantScanFunction reads NumericStats::Min
// (compression/numeric_constant.cpp); the public ColumnSegmentInfo carries it as text
// ("[Min: v, Max: v][Has Null: …]": numeric_stats.cpp:546, base_statistics.cpp:382), which the
// caller parses back through the column's type (DATE, DECIMAL and BOOL print as literals).
// is_null: an all-NULL segment, any value will do. False when the text is not of that form.
inline bool ConstantMinLiteral(const std::string &stats, std::string &literal, bool &is_null) {
    const auto a = stats.find("[Min: "), b = stats.find(", Max: ");
    if (a != 0 || b == std::string::npos) {
        return false;
    }
    literal = stats.substr(6, b - 6);
    is_null = literal == "NULL";
    return true;
}

// The size in bytes of the segment image at `p` (`count` rows of `width`-byte values), reading no
// byte at or past p + room. A BITPACKING segment's first 8 bytes are the end of its metadata, i.e.
// its size (BitpackingCompressState::FlushSegment); an RLE segment's are the offset of its run
// lengths, which end it (RLECompressState::FlushSegment, rle.cpp:190-205): they are read until
// they cover the segment's rows; an UNCOMPRESSED one is its values from the segment's start
// (FixedSizeScan); a CONSTANT one has no bytes. False when the image does not fit `room`.
inline bool SegmentImageSize(int32_t codec, const uint8_t *p, uint64_t room, uint64_t count, int width, uint64_t &size) {
    size = 0;
    if (codec == CUBIT_CODEC_CONSTANT) {
        return true;
    }
    if (codec == CUBIT_CODEC_UNCOMPRESSED) {
        size = count * (uint64_t)width;
        return size <= room;
    }
    if ((codec != CUBIT_CODEC_BITPACKING && codec != CUBIT_CODEC_RLE) || room < sizeof(size)) {
        return false;
    }
    memcpy(&size, p, sizeof(size));
    if (size < 8 || size > room) {
        return false;  // not a segment header
    }
    if (codec == CUBIT_CODEC_RLE) {
        uint64_t covered = 0, k = 0;
        while (covered < count) {
            if (2 * (k + 1) > room - size) {
                return false;
            }
            uint16_t len;
            memcpy(&len, p + size + 2 * k++, 2);
            covered += len;
        }
        size += 2 * k;
    }
    return true;
}

// The segment images of one column as the cubit_table_add_*_column entry points take them: each
// image at a 16-byte-aligned offset of `bytes`; a CONSTANT segment adds no bytes and keeps its
// offset slot.
struct SegmentImages {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets, rows;
};

// Append the segment at `p` (see SegmentImageSize; p is not read for a CONSTANT segment). False,
// with `images` unchanged, when its image does not fit `room`.
inline bool AppendSegment(SegmentImages &images, int32_t codec, const uint8_t *p, uint64_t room, uint64_t count,
                          int width) {
    uint64_t size = 0;
    if (!SegmentImageSize(codec, p, room, count, width, size)) {
        return false;
    }
    const uint64_t at = (images.bytes.size() + 15) / 16 * 16;
    images.offsets.push_back(at);
    images.rows.push_back(count);
    if (codec != CUBIT_CODEC_CONSTANT) {
        images.bytes.resize(at + size, 0);
        if (size) {
            memcpy(images.bytes.data() + at, p, size);
        }
    }
    return true;
}

// One codec for every segment keeps its own entry point (a BITPACKING column keeps its segments
// for the packed filter); mixed codecs go through cubit_table_add_segment_column.
enum class SegmentEntry { Bitpacked, Rle, Mixed };
inline SegmentEntry ChooseEntry(const std::vector<int32_t> &codecs) {
    auto all = [&](int32_t c) { return std::all_of(codecs.begin(), codecs.end(), [c](int32_t x) { return x == c; }); };
    return all(CUBIT_CODEC_BITPACKING) ? SegmentEntry::Bitpacked : all(CUBIT_CODEC_RLE) ? SegmentEntry::Rle : SegmentEntry::Mixed;
}

// ------------------------------------------------------------------ partitions

// Rows split into one contiguous range per context, boundaries on row groups of 122,880 rows
// (= 1,920 bitvector words, so every partition's validity words are the snapshot's own): at most
// one partition per row group, at least one.
struct PartitionSplit {
    static constexpr uint64_t kRowGroup = 122880;
    uint64_t rows, units, n_parts;
    PartitionSplit(uint64_t rows_p, uint64_t n_contexts)
        : rows(rows_p), units((rows_p + kRowGroup - 1) / kRowGroup),
          n_parts(std::max<uint64_t>(1, std::min<uint64_t>(n_contexts, units))) {
    }
    // partition p holds rows [Begin(p), End(p))
    uint64_t Begin(uint64_t p) const {
        return std::min(rows, units * p / n_parts * kRowGroup);
    }
    uint64_t End(uint64_t p) const {
        return Begin(p + 1);
    }
};

// The row ids [0, rows) a snapshot lacks (absent from `present`, or past its end) as each
// partition's list of local rows; partition p starts at part_base[p] (ascending) and ends where
// the next starts, the last at `rows`.
inline std::vector<std::vector<int64_t>> LocalDeletes(const std::vector<bool> &present, uint64_t rows,
                                                      const std::vector<uint64_t> &part_base) {
    std::vector<std::vector<int64_t>> local(part_base.size());
    size_t p = 0;
    for (uint64_t r = 0; r < rows && !part_base.empty(); r++) {
        if (r < present.size() && present[r]) {
            continue;
        }
        while (p + 1 < part_base.size() && r >= part_base[p + 1]) {
            p++;
        }
        if (r >= part_base[p]) {
            local[p].push_back((int64_t)(r - part_base[p]));
        }
    }
    return local;
}

// ------------------------------------------------------------------ update sync

// After a committed UPDATE of an attached column the shim holds the column's new contents and no
// list of the changed rows. cubit_table_sync_column finds them on the GPU and merges them in
// place, as long as few enough rows changed; past that a rebuild of the partition set is cheaper.
// The changed-row fraction up to which the sync is tried: measured (scripts/sync_timing.py, 612 M
// rows, DESIGN.md §7 has the numbers) — at 1 % the host-form sync takes 0.5-1.2 of a rebuild of the
// column, at 10 % 1.4-3.3 of it.
static constexpr double kDefaultSyncChangedFraction = 0.01;

// Whether an update sync may run in place: the partition set holds rows (part_rows > 0), the
// snapshot covers every one of them (snap_rows >= part_rows: the rows past them are appended as
// usual), row ids did not shrink (a vacuum renumbers them: every row may differ) and no dictionary
// column gained a string (the partitions keep their dictionary). The fraction does not decide
// this: with a fraction of 0 (or below, or NaN) the sync still runs and applies only when no row
// changed. When any partition reports applied = 0 the caller rebuilds.
struct UpdateSyncPlan {
    bool in_place;    // false: rebuild
    double fraction;  // the changed-row fraction, clamped to [0, 1]
    // max_changed of cubit_table_sync_column for a partition of `rows` rows: floor(fraction × rows),
    // never above the rows
    uint64_t MaxChanged(uint64_t rows) const {
        if (fraction >= 1.0) {
            return rows;
        }
        return std::min((uint64_t)((long double)fraction * (long double)rows), rows);
    }
};
inline UpdateSyncPlan PlanUpdateSync(uint64_t part_rows, uint64_t snap_rows, bool ids_shrank, bool new_string,
                                     double fraction) {
    const double f = fraction > 0.0 ? std::min(fraction, 1.0) : 0.0;  // NaN and negatives: 0
    return {part_rows > 0 && snap_rows >= part_rows && !ids_shrank && !new_string, f};
}

// ------------------------------------------------------------------ small helpers

// Every distinct value when the column has at most this many (l_discount 11, l_quantity 50);
// a column with more gets no index unless the attach names one (l_shipdate's 2,526 distinct
// dates would take 2,526 bitvectors, 190 GB at SF100): its comparisons are built from the raw
// column at scan time (K0).
static constexpr size_t kDefaultDistinctIndexMax = 256;

inline bool FewDistinct(const std::vector<int64_t> &v, const std::vector<uint64_t> &valid) {
    std::unordered_set<int64_t> seen;
    for (size_t r = 0; r < v.size(); r++) {
        if (RowValid(valid.data(), r)) {
            seen.insert(v[r]);
            if (seen.size() > kDefaultDistinctIndexMax) {
                return false;
            }
        }
    }
    return true;
}

// The rows a registered column is checked on against the snapshot: the valid rows of a stride over
// the partition's n rows, at most 4,096.
inline std::vector<int64_t> SampleRows(const uint64_t *validity, uint64_t n) {
    std::vector<int64_t> ids;
    const uint64_t stride = std::max<uint64_t>(1, n / 4096);
    for (uint64_t r = 0; r < n && ids.size() < 4096; r += stride) {
        if (RowValid(validity, r)) {
            ids.push_back((int64_t)r);
        }
    }
    return ids;
}

// Strings as the bytes + offsets layout cubit_dict_create / cubit_dict_encode read (string i =
// bytes[offsets[i], offsets[i+1]); an invalid row contributes an empty slot)
inline void PackStrings(const std::vector<std::string> &strs, std::vector<char> &bytes, std::vector<uint64_t> &offsets) {
    bytes.clear();
    offsets.assign(1, 0);
    for (auto &x : strs) {
        bytes.insert(bytes.end(), x.begin(), x.end());
        offsets.push_back(bytes.size());
    }
}

// ------------------------------------------------------------------ index specification

// Index specification of cubit_attach's third argument: `column=encoding[:v1,v2,…]` or
// `column=encoding~count` items separated by ';' — encoding range | equality | bins | sliced (a
// bit-sliced index: no literal list and no count), values as SQL
// literals of the column's type (dates, decimals); `~count` (range and bins only, 2 … 1,024, no
// literal list beside it) asks for that many equi-depth bins, their edges chosen from the column's
// quantiles (cubit_table_build_index_quantiles), e.g.
//   'l_shipdate=range:1994-01-01,1995-01-01;l_shipdate=bins:1992-01-01,1993-01-01,…;l_discount=range'
//   'l_shipdate=range~64;l_extendedprice=bins~256;l_shipdate=sliced'
struct IndexItem {
    std::string name;  // the column, not yet resolved
    int encoding;      // CUBIT_INDEX_RANGE / _EQUALITY / _BINS / _SLICED
    std::vector<std::string> literals;  // not yet cast; empty = every distinct value
    uint32_t quantile_bins = 0;  // `~count`: the equi-depth bins to choose edges for (0 = none asked)
};

enum class SpecStatus { Ok, MissingEquals, UnknownEncoding, BadCount };

static constexpr uint32_t kMinQuantileBins = 2, kMaxQuantileBins = 1024;

// `count` as a decimal number in kMinQuantileBins … kMaxQuantileBins (digits only), or 0
inline uint32_t ParseQuantileBins(const std::string &count) {
    uint32_t v = 0;
    for (char c : count) {
        if (c < '0' || c > '9' || v > kMaxQuantileBins) {
            return 0;
        }
        v = v * 10 + (uint32_t)(c - '0');
    }
    return !count.empty() && v >= kMinQuantileBins && v <= kMaxQuantileBins ? v : 0;
}

// Split on a delimiter as reading a stream up to each delimiter does: no item after a final
// delimiter, none for an empty text.
inline std::vector<std::string> SplitText(const std::string &text, char delimiter) {
    std::vector<std::string> out;
    for (size_t at = 0; at < text.size();) {
        const size_t end = std::min(text.find(delimiter, at), text.size());
        out.push_back(text.substr(at, end - at));
        at = end + 1;
    }
    return out;
}

// Whitespace off both ends, as DuckDB's StringUtil::Trim (string_util.cpp:41-65) — whose right
// trim also takes NUL and bytes of 0x80 and above.
inline void TrimText(std::string &s) {
    auto space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    size_t b = 0, e = s.size();
    while (b < e && space(s[b])) {
        b++;
    }
    while (e > b && ((signed char)s[e - 1] <= 0 || space(s[e - 1]))) {
        e--;
    }
    s = s.substr(b, e - b);
}

// The items of `spec` in order (empty items skipped, whitespace around items, names, encodings and
// literals dropped, encodings in any letter case). At the first malformed item the split stops:
// `items` holds the ones before it, `bad` the offending text — the item without a '=', the
// encoding that is none of the four (`equality~8`, `sliced~8` and `sliced:1` among them: an equality
// index takes no count, a bit-sliced one neither a count nor literals),
// or the count as written, with what follows it (`1025`, `x`, `8:1,2`).
inline SpecStatus SplitIndexSpec(const std::string &spec, std::vector<IndexItem> &items, std::string &bad) {
    items.clear();
    for (auto item : SplitText(spec, ';')) {
        TrimText(item);
        if (item.empty()) {
            continue;
        }
        const auto eq = item.find('=');
        if (eq == std::string::npos) {
            bad = item;
            return SpecStatus::MissingEquals;
        }
        IndexItem ix;
        ix.name = item.substr(0, eq);
        TrimText(ix.name);
        const std::string rest = item.substr(eq + 1);
        const auto colon = rest.find(':');
        std::string enc = rest.substr(0, colon);
        for (auto &c : enc) {
            c = c >= 'A' && c <= 'Z' ? (char)(c - 'A' + 'a') : c;
        }
        // a '~' before any ':' (one inside a literal belongs to the literal) opens the bin count
        const auto tilde = enc.find('~');
        if (tilde != std::string::npos) {
            std::string count = enc.substr(tilde + 1);
            enc = enc.substr(0, tilde);
            TrimText(enc);
            TrimText(count);
            if (enc != "range" && enc != "bins") {
                bad = enc + "~" + count;
                return SpecStatus::UnknownEncoding;
            }
            ix.quantile_bins = ParseQuantileBins(count);
            if (ix.quantile_bins == 0 || colon != std::string::npos) {
                bad = rest.substr(rest.find('~') + 1);
                TrimText(bad);
                return SpecStatus::BadCount;
            }
        }
        TrimText(enc);
        if (enc == "range") {
            ix.encoding = CUBIT_INDEX_RANGE;
        } else if (enc == "equality") {
            ix.encoding = CUBIT_INDEX_EQUALITY;
        } else if (enc == "bins") {
            ix.encoding = CUBIT_INDEX_BINS;
        } else if (enc == "sliced" && colon == std::string::npos) {
            ix.encoding = CUBIT_INDEX_SLICED;
        } else if (enc == "sliced") {
            bad = rest;
            TrimText(bad);
            return SpecStatus::UnknownEncoding;
        } else {
            bad = enc;
            return SpecStatus::UnknownEncoding;
        }
        if (colon != std::string::npos) {
            for (auto lit : SplitText(rest.substr(colon + 1), ',')) {
                TrimText(lit);
                ix.literals.push_back(lit);
            }
        }
        items.push_back(std::move(ix));
    }
    return SpecStatus::Ok;
}

// Integer keys ascending in the column's order and distinct in it (upload_type: the column's
// CUBIT_TYPE_*; FLOAT / DOUBLE patterns and UBIGINT bits by their comparison keys, cubit_fp_key)
inline void SortKeys(int upload_type, std::vector<int64_t> &keys) {
    auto key = [upload_type](int64_t v) { return cubit_fp_key(upload_type, v); };
    std::sort(keys.begin(), keys.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
    keys.erase(std::unique(keys.begin(), keys.end(), [&](int64_t a, int64_t b) { return key(a) == key(b); }), keys.end());
}

// String keys: byte order = DuckDB's string order (string_type.hpp:176-206); HUGEINT / UHUGEINT
// order keys likewise (byte order = the values' order)
inline void SortKeys(std::vector<std::string> &keys) {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
}

// a bins index needs at least two edges
inline bool EnoughKeys(int encoding, size_t n_keys) {
    return encoding != CUBIT_INDEX_BINS || n_keys >= 2;
}

} // namespace cubit_shim
