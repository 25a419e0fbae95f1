// Stand-alone bounds check of the library's segment walkers (csrc/cubit_segments.hpp), built by
// tests/test_segment_walk.py with -fsanitize=address,undefined and run as a child process:
//   segment_walk_bounds bp|rle <segment file> <rows> <CUBIT_TYPE_* code of T>
//   segment_walk_bounds types
// bp / rle: for every n from 0 to the segment's size - 1, the first n bytes are copied into a heap
// buffer of exactly n bytes and the walker must refuse, with a message; the sanitizer aborts the
// program if the walker reads a byte past the buffer. With the whole segment it must accept and
// cover the rows. bp then checks the groups (their number, rows contiguous from 0 and summing to
// the segment's, packed words inside the bytes or inside the moved area); rle prints its runs as
// "run <value as int64> <end row>" lines for the test to compare.
// types: one line per type code -1 … 13: "type <code> <size> <signed> <col_type> <tnorm> <segment>",
// or "type <code> none".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "cubit_segments.hpp"

using namespace cubit;

static int walk(bool bp, const uint8_t* buf, uint64_t n, uint64_t rows, const TypeInfo& ti, SegmentPlan& p, char* err,
                size_t err_len) {
    err[0] = 0;
    return bp ? walk_bp_segment(buf, n, 0, rows, ti, (n + 15) / 16 * 16, 3, p, err, err_len)
              : walk_rle_segment(buf, n, 0, rows, ti, 3, p, err, err_len);
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "types") {
        for (int code = -1; code <= 13; ++code) {
            if (const TypeInfo* ti = type_info(code))
                printf("type %d %u %d %d %u %d\n", code, ti->size, (int)ti->sgn, ti->col_type, (unsigned)ti->tnorm,
                       (int)ti->segment);
            else
                printf("type %d none\n", code);
            if ((segment_type(code) != nullptr) != (type_info(code) && type_info(code)->segment)) return 1;
        }
        return 0;
    }
    if (argc != 5) {
        fprintf(stderr, "usage: %s bp|rle <segment file> <rows> <type code> | types\n", argv[0]);
        return 2;
    }
    const bool bp = std::string(argv[1]) == "bp";
    std::vector<uint8_t> seg;
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        perror(argv[2]);
        return 2;
    }
    for (int c; (c = fgetc(f)) != EOF;) seg.push_back((uint8_t)c);
    fclose(f);
    const uint64_t rows = strtoull(argv[3], nullptr, 10);
    const TypeInfo* ti = segment_type(atoi(argv[4]));
    if (!ti) {
        fprintf(stderr, "type %s names no segment type\n", argv[4]);
        return 2;
    }
    char err[192];
    for (uint64_t n = 0; n < seg.size(); n++) {
        std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);  // exactly n bytes: a read past them is caught
        memcpy(buf.get(), seg.data(), n);
        SegmentPlan p;
        const int rc = walk(bp, buf.get(), n, rows, *ti, p, err, sizeof(err));
        if (rc != CUBIT_ERR_INVALID || !err[0] || p.rows != 0) {
            fprintf(stderr, "%llu of %llu bytes: code %d, message '%s', rows %llu\n", (unsigned long long)n,
                    (unsigned long long)seg.size(), rc, err, (unsigned long long)p.rows);
            return 1;
        }
    }
    const uint64_t n = seg.size(), padded = (n + 15) / 16 * 16;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
    memcpy(buf.get(), seg.data(), n);
    SegmentPlan p;
    if (int rc = walk(bp, buf.get(), n, rows, *ti, p, err, sizeof(err))) {
        fprintf(stderr, "the whole segment: code %d, '%s'\n", rc, err);
        return 1;
    }
    if (p.rows != rows || !p.plain.empty() || (bp ? !p.ends.empty() : !p.groups.empty() || !p.moved.empty()) ||
        p.vals.size() != p.ends.size()) {
        fprintf(stderr, "the whole segment: plan covers %llu of %llu rows, or holds another codec's parts\n",
                (unsigned long long)p.rows, (unsigned long long)rows);
        return 1;
    }
    if (bp) {
        uint64_t row = 0;
        if (p.groups.size() != (rows + 2047) / 2048 || p.moved.size() % 16) {
            fprintf(stderr, "%zu groups for %llu rows, %zu moved bytes\n", p.groups.size(), (unsigned long long)rows,
                    p.moved.size());
            return 1;
        }
        for (const BpGroup& g : p.groups) {
            const uint64_t packed = g.mode == 4 || g.mode == 5 ? ((uint64_t)g.count + 31) / 32 * 32 * g.width / 8 : 0;
            const bool in_bytes = g.words_off + packed <= n;
            const bool in_moved = g.words_off >= padded && g.words_off % 16 == 0 && g.words_off + packed <= padded + p.moved.size();
            if (g.row_start != row || g.count == 0 || g.count > 2048 || !(in_bytes || in_moved) ||
                (packed && g.words_off % 4) || g.tnorm != ti->tnorm || g.width > 8 * ti->size) {
                fprintf(stderr, "group at row %llu: row_start %llu, count %u, words_off %llu + %llu of %llu (+%zu moved)\n",
                        (unsigned long long)row, (unsigned long long)g.row_start, g.count,
                        (unsigned long long)g.words_off, (unsigned long long)packed, (unsigned long long)n, p.moved.size());
                return 1;
            }
            row += g.count;
        }
        if (row != rows) {
            fprintf(stderr, "the groups hold %llu of %llu rows\n", (unsigned long long)row, (unsigned long long)rows);
            return 1;
        }
    } else {
        for (size_t k = 0; k < p.ends.size(); ++k)
            printf("run %lld %llu\n", (long long)p.vals[k], (unsigned long long)p.ends[k]);
    }
    printf("refused %llu truncations, accepted %llu bytes: %zu groups, %zu runs, %zu moved bytes\n",
           (unsigned long long)seg.size(), (unsigned long long)seg.size(), p.groups.size(), p.ends.size(), p.moved.size());
    return 0;
}
