// The row-list policy and the derived block pool (duckdb-cubit_amd/csrc/cubit_row_list.hpp) on the CPU:
// the byte rule at its edges, the recurrence, budget room and drop-first ordering, the pool's reuse,
// bound and clear, and the off / lo_cnt encoding. Built with AddressSanitizer and UBSan by
// tests/test_row_list_core.py; ends with status 1 at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cubit_derived.hpp"
#include "cubit_row_list.hpp"

using namespace cubit;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

namespace {

void byte_rule() {
    // B = 2,048 words of one tile = 16,384 bytes; L = 2 q + 4 tiles. L = B / 2 at q = 4,094.
    const uint64_t B = 2048 * 8;
    CHECK(row_list_bytes(4094, 1) == B / 2);
    CHECK(row_list_wanted(4094, 1, B));       // L = B / 2
    CHECK(!row_list_wanted(4095, 1, B));      // the next q: L = B / 2 + 2
    // L = B / 2 + 1: L is even, so B / 2 is odd there, which whole words never give; the rule is on
    // bytes all the same (B' = 16,382: B' / 2 = 8,191 = L - 1; B' = 16,386: B' / 2 = L + 1)
    CHECK(!row_list_wanted(4094, 1, B - 2));  // L = B' / 2 + 1
    CHECK(!row_list_wanted(4094, 1, B - 1));  // 2 L <= B' is exact where B' / 2 would round
    CHECK(row_list_wanted(4094, 1, B + 2));
    CHECK(row_list_wanted(0, 1, B));          // an empty bitvector: the counts alone
    CHECK(!row_list_wanted(0, 1, 7));
    // SF100 Q6 as kept: q = 11,421,368 of 600,037,902 rows, 4,578 tiles, 9,388,032 padded words
    const uint64_t tiles = 4578, q = 11421368, b100 = 9388032ull * 8;
    CHECK(row_list_bytes(q, tiles) == 22861048);
    CHECK(row_list_wanted(q, tiles, b100));
    CHECK(!row_list_wanted(b100 / 4, tiles, b100));  // 3.1 % dense: L = B / 2 + 4 tiles
    std::printf("byte rule ok\n");
}

void recurrence() {
    const uint64_t L = 1000;
    // the first decode alone: nothing, whatever else holds
    CHECK(row_list_step(0, false, true, L, UINT64_MAX) == kRowListNone);
    // the second builds when wanted and the room holds the list exactly
    CHECK(row_list_step(1, false, true, L, L) == kRowListBuild);
    CHECK(row_list_step(1, false, true, L, L - 1) == kRowListNone);
    CHECK(row_list_step(1, false, false, L, UINT64_MAX) == kRowListNone);
    CHECK(row_list_step(1, false, true, L, 0) == kRowListNone);  // budget 0: no room, no list
    // later decodes that still have none ask again (room may have come), and a list is read from
    // wherever the counter stands
    CHECK(row_list_step(7, false, true, L, L) == kRowListBuild);
    CHECK(row_list_step(2, true, true, L, 0) == kRowListRead);
    CHECK(row_list_step(0, true, false, L, 0) == kRowListRead);
    // the counter as a table keeps it: scans 1, 2, 3, 4 of one bitvector
    uint64_t solo = 0;
    bool has = false;
    std::vector<int> steps;
    for (int s = 0; s < 4; ++s) {
        const RowListStep st = row_list_step(solo++, has, true, L, 4 * L);
        has |= st == kRowListBuild;
        steps.push_back(st);
    }
    CHECK((steps == std::vector<int>{kRowListNone, kRowListBuild, kRowListRead, kRowListRead}));
    std::printf("recurrence ok\n");
}

void budget() {
    RowListBook<int> book;
    std::vector<int> dropped;
    auto on_drop = [&](int k) { dropped.push_back(k); };
    // room: what the budget leaves beside the kept bitvectors and the lists held
    CHECK(book.room(0, 0) == 0);
    CHECK(book.room(1000, 400) == 600);
    CHECK(book.room(1000, 1000) == 0);
    CHECK(book.room(1000, 1200) == 0);
    book.add(1, 100);
    book.add(2, 200);
    book.add(3, 50);
    CHECK(book.size() == 3 && book.bytes() == 350 && book.has(2) && !book.has(4));
    CHECK(book.room(1000, 400) == 250);
    CHECK(book.room(1000, 650) == 0);
    // nothing goes while bitvectors and lists fit
    CHECK(book.shed(1000, 650, on_drop) == 0 && dropped.empty());
    // a bitvector of 300 more bytes arrives: the oldest lists go until the rest fits; the cache of
    // bitvectors never counted the lists, so none of its entries went for them
    CHECK(book.shed(1000, 950, on_drop) == 2);
    CHECK((dropped == std::vector<int>{1, 2}));
    CHECK(book.size() == 1 && book.bytes() == 50 && book.has(3));
    CHECK(book.shed(1000, 951, on_drop) == 1 && book.size() == 0 && book.bytes() == 0);
    dropped.clear();
    book.add(1, 100);
    book.add(2, 200);
    book.add(1, 120);  // rebuilt: counted once, now the newest
    CHECK(book.size() == 2 && book.bytes() == 320);
    CHECK(book.shed(1000, 800, on_drop) == 1 && (dropped == std::vector<int>{2}));
    CHECK(book.bytes() == 120 && book.has(1));
    // its bitvector's zone map went: the list with it
    CHECK(book.drop(1) && !book.drop(1) && book.bytes() == 0);
    // budget 0 sheds everything
    dropped.clear();
    book.add(5, 10);
    book.add(6, 10);
    CHECK(book.shed(0, 0, on_drop) == 2 && book.size() == 0);
    book.add(7, 10);
    book.clear();
    CHECK(book.size() == 0 && book.bytes() == 0 && book.room(50, 0) == 50);

    // drop-first ordering with the bitvector cache beside it: lists are shed when an entry is
    // inserted, and an eviction finds none left
    DerivedCache<int> cache;
    std::vector<std::string> log;
    auto on_evict = [&](int&) {  // the table's sequence: every list, then the bitvector
        if (book.size()) {
            book.clear();
            log.push_back("lists");
        }
        log.push_back("bitvector");
    };
    cache.set_budget(2000, on_evict);
    DerivedKey a, b, c;
    CHECK(derived_key(1, kDerivedAnd, {{0x10, false}, {0x18, true}}, &a));
    CHECK(derived_key(2, kDerivedAnd, {{0x20, false}, {0x28, true}}, &b));
    CHECK(derived_key(3, kDerivedAnd, {{0x30, false}, {0x38, true}}, &c));
    auto admit = [&](const DerivedKey& k) {
        for (int r = 0; r < 8; ++r) {
            cache.begin_plan(on_evict);
            const bool ok = cache.request(k, 1000);
            if (ok) cache.insert(k, 1000, 1);
            cache.end_plan();
            if (ok) return true;
        }
        return false;
    };
    CHECK(admit(a));
    CHECK(book.room(cache.budget(), cache.bytes()) == 1000);
    book.add(1, 600);
    CHECK(book.room(cache.budget(), cache.bytes()) == 400);
    CHECK(admit(b));  // fits the cache's own count: no eviction
    CHECK(log.empty() && cache.size() == 2);
    dropped.clear();
    CHECK(book.shed(cache.budget(), cache.bytes(), on_drop) == 1);  // but the list's room is gone
    CHECK(book.room(cache.budget(), cache.bytes()) == 0);
    book.add(2, 0);  // (a list of nothing, to see the order)
    CHECK(admit(c));  // evicts a: the lists went first
    CHECK((log == std::vector<std::string>{"lists", "bitvector"}));
    CHECK(book.size() == 0 && cache.size() == 2 && cache.bytes() == 2000);
    std::printf("budget ok\n");
}

// a block: a heap cell, so that a leak, a double free or a use after free is an ASan error
using Handle = std::unique_ptr<int>;

void pool() {
    BlockPool<Handle> p;
    int freed = 0;
    auto on_free = [&](Handle& h) {
        CHECK(h != nullptr);
        h.reset();
        ++freed;
    };
    Handle h;
    CHECK(!p.take(&h) && p.free_blocks() == 0 && p.device_allocs() == 0);
    p.reset(64, 3 * 64, on_free);
    CHECK(p.block_bytes() == 64);
    // nothing waiting: the caller allocates
    CHECK(!p.take(&h));
    Handle x = std::make_unique<int>(1), y = std::make_unique<int>(2), z = std::make_unique<int>(3),
           w = std::make_unique<int>(4);
    for (int i = 0; i < 4; ++i) p.allocated();
    CHECK(p.device_allocs() == 4);
    // blocks come back: three fit the bound, the fourth stays with the caller, as does one of another size
    CHECK(p.give(x, 64) && !x);
    CHECK(p.give(y, 64) && p.give(z, 64));
    CHECK(!p.give(w, 64) && w && *w == 4);
    Handle odd = std::make_unique<int>(9);
    p.reset(64, 4 * 64, on_free);
    CHECK(!p.give(odd, 128) && odd);
    CHECK(p.free_blocks() == 3 && p.free_bytes() == 192 && freed == 0);
    // reuse: the last one in comes out first, and no allocation is counted
    CHECK(p.take(&h) && *h == 3 && p.free_blocks() == 2 && p.device_allocs() == 4);
    CHECK(p.give(h, 64) && p.give(w, 64) && p.free_blocks() == 4);
    // a smaller bound trims, the same size and bound change nothing
    p.reset(64, 4 * 64, on_free);
    CHECK(p.free_blocks() == 4 && freed == 0);
    p.reset(64, 2 * 64, on_free);
    CHECK(p.free_blocks() == 2 && freed == 2);
    // another block size: every free block goes
    p.reset(128, 4 * 128, on_free);
    CHECK(p.free_blocks() == 0 && freed == 4);
    CHECK(p.give(odd, 128) && p.free_blocks() == 1);
    // bound 0: pooling off, nothing kept, nothing accepted
    p.reset(128, 0, on_free);
    CHECK(p.free_blocks() == 0 && freed == 5);
    Handle v = std::make_unique<int>(7);
    CHECK(!p.give(v, 128) && v);
    // clear (table close)
    p.reset(128, 1024, on_free);
    CHECK(p.give(v, 128));
    p.clear(on_free);
    CHECK(p.free_blocks() == 0 && freed == 6);
    // random traffic: blocks out + blocks free = blocks made - blocks freed, the bound always holds
    std::mt19937 rng(7);
    BlockPool<Handle> r;
    int made = 0, gone = 0;
    auto free_r = [&](Handle& b) {
        b.reset();
        ++gone;
    };
    uint64_t bound = 5 * 32;
    r.reset(32, bound, free_r);
    std::vector<Handle> out;
    for (int i = 0; i < 20000; ++i) {
        const unsigned op = rng() % 100;
        if (op < 45) {
            Handle b;
            if (!r.take(&b)) {
                b = std::make_unique<int>(made++);
                r.allocated();
            }
            out.push_back(std::move(b));
        } else if (op < 90 && !out.empty()) {
            Handle b = std::move(out.back());
            out.pop_back();
            if (!r.give(b, 32)) free_r(b);
        } else if (op < 95) {
            bound = (rng() % 8) * 32;
            r.reset(32, bound, free_r);
        } else if (op < 97) {
            r.clear(free_r);
        }
        CHECK(r.free_bytes() <= bound);
        CHECK((int)out.size() + (int)r.free_blocks() == made - gone);
        CHECK(r.device_allocs() == (uint64_t)made);
    }
    for (Handle& b : out) free_r(b);
    r.clear(free_r);
    CHECK(made == gone);
    std::printf("pool ok\n");
}

void round_trip() {
    // one tile holding offsets 0, 65,535, 65,536 and 131,071: two below the half
    const uint32_t offs[] = {0, 65535, 65536, 131071};
    uint16_t enc[4];
    uint32_t lo_cnt = 0;
    for (int i = 0; i < 4; ++i) {
        enc[i] = row_list_encode(offs[i]);
        lo_cnt += offs[i] < kRowListHalf;
    }
    CHECK(lo_cnt == 2 && enc[0] == 0 && enc[1] == 65535 && enc[2] == 0 && enc[3] == 65535);
    for (uint32_t i = 0; i < 4; ++i) CHECK(row_list_decode(enc[i], i, lo_cnt) == offs[i]);
    // all in the lower half, all in the upper half, none
    CHECK(row_list_decode(row_list_encode(65535), 0, 1) == 65535);
    CHECK(row_list_decode(row_list_encode(65536), 0, 0) == 65536);
    CHECK(row_list_decode(row_list_encode(131071), 0, 0) == 131071);
    // every ascending random set of a tile comes back
    std::mt19937 rng(11);
    for (int round = 0; round < 50; ++round) {
        std::vector<uint32_t> set;
        const uint32_t step = 1 + rng() % 97;
        for (uint32_t o = rng() % step; o < kRowListTileRows; o += 1 + rng() % step) set.push_back(o);
        std::vector<uint16_t> e;
        uint32_t lo = 0;
        for (uint32_t o : set) {
            e.push_back(row_list_encode(o));
            lo += o < kRowListHalf;
        }
        for (uint32_t i = 0; i < set.size(); ++i) CHECK(row_list_decode(e[i], i, lo) == set[i]);
    }
    std::printf("round trip ok\n");
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "rule" || what == "all") byte_rule();
    if (what == "recurrence" || what == "all") recurrence();
    if (what == "budget" || what == "all") budget();
    if (what == "pool" || what == "all") pool();
    if (what == "roundtrip" || what == "all") round_trip();
    return 0;
}
