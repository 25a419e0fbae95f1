// Stand-alone bounds check of cubit_shim::SegmentImageSize, built by tests/test_shim_core.py with
// -fsanitize=address,undefined and run as a child process:
//   shim_core_bounds <segment file> <codec> <count> <width>
// For every room from 0 to the segment's size - 1, the first `room` bytes are copied into a heap
// buffer of exactly `room` bytes and the call must refuse; the sanitizer aborts the program if the
// call reads a byte past the buffer. With the whole segment it must accept, with the file's size.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "cubit_shim_core.hpp"

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s <segment file> <codec> <count> <width>\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> seg;
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    for (int c; (c = fgetc(f)) != EOF;) {
        seg.push_back((uint8_t)c);
    }
    fclose(f);
    const int codec = atoi(argv[2]), width = atoi(argv[4]);
    const uint64_t count = strtoull(argv[3], nullptr, 10);
    for (uint64_t room = 0; room <= seg.size(); room++) {
        std::unique_ptr<uint8_t[]> buf(new uint8_t[room]);  // exactly `room` bytes: a read past them is caught
        memcpy(buf.get(), seg.data(), room);
        uint64_t size = 0;
        const bool ok = cubit_shim::SegmentImageSize(codec, buf.get(), room, count, width, size);
        if (room < seg.size() && ok) {
            fprintf(stderr, "accepted %llu of %llu bytes (size %llu)\n", (unsigned long long)room,
                    (unsigned long long)seg.size(), (unsigned long long)size);
            return 1;
        }
        if (room == seg.size() && (!ok || size != seg.size())) {
            fprintf(stderr, "the whole segment: ok %d, size %llu of %llu\n", (int)ok, (unsigned long long)size,
                    (unsigned long long)seg.size());
            return 1;
        }
    }
    printf("refused %llu truncations, accepted %llu bytes\n", (unsigned long long)seg.size(),
           (unsigned long long)seg.size());
    return 0;
}
