// Test surface only: cubit_shim_core.hpp behind extern "C", so tests/test_shim_core.py and
// tests/test_gpu_shim_core.py can drive it through ctypes (lib/libcubit_shim_core.so). The shim
// includes the header directly and does not use this file. Text lists cross as fields joined by
// '\x1f' (records by '\x1e'); an output buffer too small for its text makes the call return -1.
#include "cubit_shim_core.hpp"

using namespace cubit_shim;

namespace {

int PutText(const std::string &s, char *out, uint64_t cap) {
    if (s.size() + 1 > cap) {
        return -1;
    }
    memcpy(out, s.c_str(), s.size() + 1);
    return 0;
}

std::string Join(const std::vector<std::string> &parts, char sep) {
    std::string s;
    for (size_t i = 0; i < parts.size(); i++) {
        s += (i ? std::string(1, sep) : std::string()) + parts[i];
    }
    return s;
}

// fields of a joined text, a final empty field included ("" = no field)
std::vector<std::string> Fields(const char *text, uint64_t len, char sep) {
    std::vector<std::string> out;
    if (len == 0) {
        return out;
    }
    std::string cur;
    for (uint64_t i = 0; i < len; i++) {
        if (text[i] == sep) {
            out.push_back(cur);
            cur.clear();
        } else {
            cur += text[i];
        }
    }
    out.push_back(cur);
    return out;
}

} // namespace

extern "C" {

// {gpu, dict, wide, upload_type, segment_type, width} of Phys `phys` (the enum's order)
void csc_traits(int phys, int out[6]) {
    const PhysTraits t = TraitsOf((Phys)phys);
    const int v[6] = {t.gpu, t.dict, t.wide, t.upload_type, t.segment_type, t.width};
    memcpy(out, v, sizeof(v));
}

int64_t csc_load_int64(int phys, const void *data, uint64_t i) {
    return LoadInt64((Phys)phys, data, i);
}

void csc_store_from_int64(int phys, void *dst, const int64_t *src, uint64_t n) {
    StoreFromInt64((Phys)phys, dst, src, n);
}

int csc_row_valid(const uint64_t *words, uint64_t r) {
    return RowValid(words, r);
}

// names: bitpacking, rle, constant, uncompressed. 1 and out_codecs[n] when the segments plan.
int csc_plan_segments(uint32_t n, const uint64_t *start, const uint64_t *count, const char *const *codec_names,
                      const uint8_t *has_updates, const uint8_t *persistent, uint64_t n_rows, const char *const names[4],
                      int32_t *out_codecs) {
    std::vector<SegmentDesc> descs;
    for (uint32_t i = 0; i < n; i++) {
        descs.push_back({start[i], count[i], codec_names[i], has_updates[i] != 0, persistent[i] != 0, ""});
    }
    std::vector<int32_t> codecs;
    if (!PlanSegments(descs, n_rows, CodecNames {names[0], names[1], names[2], names[3]}, codecs)) {
        return 0;
    }
    std::copy(codecs.begin(), codecs.end(), out_codecs);
    return 1;
}

int csc_constant_min_literal(const char *stats, char *literal, uint64_t cap, int *is_null) {
    std::string lit;
    bool null = false;
    if (!ConstantMinLiteral(stats, lit, null)) {
        return 0;
    }
    *is_null = null;
    return PutText(lit, literal, cap) ? -1 : 1;
}

int csc_segment_image_size(int codec, const uint8_t *p, uint64_t room, uint64_t count, int width, uint64_t *size) {
    return SegmentImageSize(codec, p, room, count, width, *size);
}

void *csc_images_new() {
    return new SegmentImages();
}
void csc_images_free(void *im) {
    delete static_cast<SegmentImages *>(im);
}
int csc_images_append(void *im, int codec, const uint8_t *p, uint64_t room, uint64_t count, int width) {
    return AppendSegment(*static_cast<SegmentImages *>(im), codec, p, room, count, width);
}
uint64_t csc_images_n_bytes(void *im) {
    return static_cast<SegmentImages *>(im)->bytes.size();
}
const uint8_t *csc_images_bytes(void *im) {
    return static_cast<SegmentImages *>(im)->bytes.data();
}
uint32_t csc_images_n_segments(void *im) {
    return (uint32_t)static_cast<SegmentImages *>(im)->offsets.size();
}
const uint64_t *csc_images_offsets(void *im) {
    return static_cast<SegmentImages *>(im)->offsets.data();
}
const uint64_t *csc_images_rows(void *im) {
    return static_cast<SegmentImages *>(im)->rows.data();
}

// 0 = cubit_table_add_bitpacked_column, 1 = cubit_table_add_rle_column, 2 = cubit_table_add_segment_column
int csc_choose_entry(const int32_t *codecs, uint32_t n) {
    return (int)ChooseEntry(std::vector<int32_t>(codecs, codecs + n));
}

// n_parts, and bounds[0 … n_parts]: partition p holds rows [bounds[p], bounds[p + 1]) (cap: n_contexts + 2)
uint64_t csc_split_rows(uint64_t rows, uint64_t n_contexts, uint64_t *bounds) {
    const PartitionSplit split(rows, n_contexts);
    for (uint64_t p = 0; p < split.n_parts; p++) {
        bounds[p] = split.Begin(p);
        bounds[p + 1] = split.End(p);
    }
    return split.n_parts;
}

// out_rows (cap: rows): the partitions' lists one after another; out_counts[n_parts]: their lengths
void csc_local_deletes(const uint8_t *present, uint64_t n_present, uint64_t rows, const uint64_t *part_base,
                       uint32_t n_parts, int64_t *out_rows, uint64_t *out_counts) {
    std::vector<bool> pres(n_present);
    for (uint64_t r = 0; r < n_present; r++) {
        pres[r] = present[r] != 0;
    }
    const auto local = LocalDeletes(pres, rows, std::vector<uint64_t>(part_base, part_base + n_parts));
    for (uint32_t p = 0; p < n_parts; p++) {
        out_rows = std::copy(local[p].begin(), local[p].end(), out_rows);
        out_counts[p] = local[p].size();
    }
}

// The update-sync decision; max_changed[i] (n_parts entries, written only when in place) = what
// partition i of part_rows[i] rows passes to cubit_table_sync_column. Returns 1 = in place.
int csc_plan_update_sync(uint64_t gpu_rows, uint64_t snap_rows, int ids_shrank, int new_string, double fraction,
                         const uint64_t *part_rows, uint64_t n_parts, uint64_t *max_changed) {
    const UpdateSyncPlan plan = PlanUpdateSync(gpu_rows, snap_rows, ids_shrank != 0, new_string != 0, fraction);
    for (uint64_t i = 0; plan.in_place && i < n_parts; i++) {
        max_changed[i] = plan.MaxChanged(part_rows[i]);
    }
    return plan.in_place;
}

double csc_default_sync_fraction() {
    return kDefaultSyncChangedFraction;
}

int csc_few_distinct(const int64_t *v, const uint64_t *valid, uint64_t n) {
    return FewDistinct(std::vector<int64_t>(v, v + n), std::vector<uint64_t>(valid, valid + (n + 63) / 64));
}

// out (cap: 4096): the sample's row ids; returns how many
uint64_t csc_sample_rows(const uint64_t *validity, uint64_t n, int64_t *out) {
    const auto ids = SampleRows(validity, n);
    std::copy(ids.begin(), ids.end(), out);
    return ids.size();
}

// strings joined by '\x1f' → bytes (cap: len) and offsets (n + 1); returns n
uint64_t csc_pack_strings(const char *joined, uint64_t len, char *bytes, uint64_t *offsets) {
    std::vector<char> b;
    std::vector<uint64_t> o;
    PackStrings(Fields(joined, len, '\x1f'), b, o);
    std::copy(b.begin(), b.end(), bytes);
    std::copy(o.begin(), o.end(), offsets);
    return o.size() - 1;
}

// items: records "name \x1f encoding \x1f literal…" joined by '\x1e'; bad: the offending text.
// Returns the SpecStatus (0 ok, 1 missing '=', 2 unknown encoding).
int csc_split_index_spec(const char *spec, char *items, uint64_t cap, char *bad, uint64_t bad_cap) {
    std::vector<IndexItem> parsed;
    std::string offending;
    const SpecStatus st = SplitIndexSpec(spec, parsed, offending);
    std::vector<std::string> records;
    for (auto &ix : parsed) {
        std::vector<std::string> f {ix.name, std::to_string(ix.encoding)};
        f.insert(f.end(), ix.literals.begin(), ix.literals.end());
        records.push_back(Join(f, '\x1f'));
    }
    if (PutText(Join(records, '\x1e'), items, cap) || PutText(offending, bad, bad_cap)) {
        return -1;
    }
    return (int)st;
}

// The same split with each item's bin count (`~count`, 0 where none): counts[i] for i < min(cap, *n),
// *n = the items split. Returns the SpecStatus (… 3 bad count); bad as above.
int csc_split_index_spec_counts(const char *spec, uint32_t *counts, uint64_t cap, uint64_t *n, char *bad,
                                uint64_t bad_cap) {
    std::vector<IndexItem> parsed;
    std::string offending;
    const SpecStatus st = SplitIndexSpec(spec, parsed, offending);
    *n = parsed.size();
    for (size_t i = 0; i < parsed.size() && i < cap; i++) {
        counts[i] = parsed[i].quantile_bins;
    }
    if (PutText(offending, bad, bad_cap)) {
        return -1;
    }
    return (int)st;
}

// sorted and deduplicated in place; returns how many remain
uint64_t csc_sort_keys(int upload_type, int64_t *keys, uint64_t n) {
    std::vector<int64_t> k(keys, keys + n);
    SortKeys(upload_type, k);
    std::copy(k.begin(), k.end(), keys);
    return k.size();
}

// keys joined by '\x1f' → sorted, distinct, joined likewise
int csc_sort_string_keys(const char *joined, uint64_t len, char *out, uint64_t cap, uint64_t *out_len) {
    std::vector<std::string> k = Fields(joined, len, '\x1f');
    SortKeys(k);
    const std::string s = Join(k, '\x1f');
    *out_len = s.size();
    return PutText(s, out, cap);
}

int csc_enough_keys(int encoding, uint64_t n_keys) {
    return EnoughKeys(encoding, n_keys);
}
}
