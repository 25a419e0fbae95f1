// The derived-leaf policy (duckdb-cubit_amd/csrc/cubit_derived.hpp) on the CPU: key canonicalisation,
// the admission rule, the LRU order, the budget and the counter bound. Built with AddressSanitizer and
// UBSan by tests/test_derived_core.py; ends with status 1 at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cubit_derived.hpp"

using namespace cubit;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

namespace {

// payload: a heap block standing for the device bitvector (a use after eviction is seen by ASan)
struct Block {
    std::unique_ptr<int> id;
};
using Cache = DerivedCache<Block>;

std::vector<int> g_evicted;
auto on_evict = [](Block& b) { g_evicted.push_back(*b.id); };

DerivedKey key_of(int column, int op, std::vector<DerivedLit> lits) {
    DerivedKey k;
    CHECK(derived_key(column, op, std::move(lits), &k));
    return k;
}
// the interval key number i: two literals of its own
DerivedKey interval(int i) { return key_of(1, kDerivedAnd, {{0x1000u + 16u * i, false}, {0x1008u + 16u * i, true}}); }

// request key until request() says materialise; returns the request number (1-based) that did
int requests_until_admitted(Cache& c, const DerivedKey& k, uint64_t bytes, int limit = 64) {
    for (int r = 1; r <= limit; ++r)
        if (c.request(k, bytes)) return r;
    return -1;
}

std::vector<int> order(const Cache& c) {
    std::vector<int> ids;
    c.for_each([&](const Cache::Entry& e) { ids.push_back(*e.payload.id); });
    return ids;
}

void admission() {
    // uses_so_far * (k - 1) >= k + 1: the first admitted request is ceil((k + 1) / (k - 1)) + 1
    const int expect[] = {0, 0, 4, 3, 3, 3, 3, 3, 3};
    for (int k = 2; k <= 8; ++k) {
        for (uint64_t u = 0; u < 10; ++u) CHECK(derived_admit(u, k) == (u * (k - 1) >= (uint64_t)k + 1));
        int first = -1;
        for (int u = 0; u < 10 && first < 0; ++u)
            if (derived_admit(u, k)) first = u + 1;
        CHECK(first == expect[k]);
        // the same through the cache's counters
        Cache c;
        c.set_budget(1000, on_evict);
        std::vector<DerivedLit> lits;
        for (int i = 0; i < k; ++i) lits.push_back({0x100u + 8u * i, i % 2 == 1});
        const DerivedKey key = key_of(0, kDerivedOr, lits);
        c.begin_plan(on_evict);
        CHECK(requests_until_admitted(c, key, 10) == expect[k]);
        c.end_plan();
    }
    CHECK(!derived_admit(1000, 1) && !derived_admit(1000, 0));
    // a budget of 0, or an entry larger than the budget, never admits (and counts nothing)
    Cache off;
    CHECK(requests_until_admitted(off, interval(0), 10) == -1 && off.counters() == 0);
    off.set_budget(5, on_evict);
    CHECK(requests_until_admitted(off, interval(0), 10) == -1 && off.counters() == 0);
    std::printf("admission ok\n");
}

void keys() {
    const std::vector<DerivedLit> a = {{0x10, false}, {0x20, true}, {0x30, false}};
    const DerivedKey k0 = key_of(3, kDerivedAnd, a);
    std::vector<DerivedLit> p = a;
    std::sort(p.begin(), p.end());
    do {
        CHECK(key_of(3, kDerivedAnd, p) == k0);
        CHECK(!(key_of(3, kDerivedAnd, p) < k0) && !(k0 < key_of(3, kDerivedAnd, p)));
    } while (std::next_permutation(p.begin(), p.end()));
    // a literal met twice counts once
    std::vector<DerivedLit> dup = a;
    dup.push_back(a[1]);
    CHECK(key_of(3, kDerivedAnd, dup) == k0 && key_of(3, kDerivedAnd, dup).lits.size() == 3);
    // a complement flip, another column, another operator, another pointer: other keys
    for (size_t i = 0; i < a.size(); ++i) {
        std::vector<DerivedLit> f = a;
        f[i].second = !f[i].second;
        CHECK(!(key_of(3, kDerivedAnd, f) == k0));
        CHECK(key_of(3, kDerivedAnd, f) < k0 || k0 < key_of(3, kDerivedAnd, f));
        f = a;
        f[i].first += 8;
        CHECK(!(key_of(3, kDerivedAnd, f) == k0));
    }
    CHECK(!(key_of(4, kDerivedAnd, a) == k0));
    CHECK(!(key_of(3, kDerivedOr, a) == k0));
    // fewer than two distinct literals, or a bitvector both plain and complemented: no key
    DerivedKey k;
    CHECK(!derived_key(0, kDerivedAnd, {}, &k));
    CHECK(!derived_key(0, kDerivedAnd, {{0x10, false}}, &k));
    CHECK(!derived_key(0, kDerivedAnd, {{0x10, false}, {0x10, false}}, &k));
    CHECK(!derived_key(0, kDerivedAnd, {{0x10, false}, {0x20, false}, {0x10, true}}, &k));
    std::printf("keys ok\n");
}

Block block(int id) { return Block{std::make_unique<int>(id)}; }

void lru_and_budget() {
    g_evicted.clear();
    Cache c;
    c.set_budget(30, on_evict);  // three entries of 10
    for (int i = 0; i < 3; ++i) {
        c.begin_plan(on_evict);
        CHECK(requests_until_admitted(c, interval(i), 10) == 4);
        CHECK(*c.insert(interval(i), 10, block(i))->id == i);
        c.end_plan();
    }
    CHECK((order(c) == std::vector<int>{2, 1, 0}) && c.bytes() == 30 && c.size() == 3 && c.counters() == 0);
    c.begin_plan(on_evict);
    CHECK(*c.find(interval(0))->id == 0);  // 0 becomes the most recently used
    CHECK(c.find(interval(7)) == nullptr);
    CHECK(c.hits() == 1);
    // a fourth key is due but there is no room: nothing is evicted while the plan is open
    for (int r = 1; r <= 6; ++r) CHECK(!c.request(interval(3), 10));
    c.set_budget(30, on_evict);
    CHECK(g_evicted.empty() && c.size() == 3 && c.bytes() == 30);
    CHECK(*c.find(interval(2))->id == 2);
    CHECK((order(c) == std::vector<int>{2, 0, 1}));
    c.end_plan();
    CHECK(g_evicted.empty());
    // the next plan begins by making the room that was asked for: the least recently used goes
    c.begin_plan(on_evict);
    CHECK((g_evicted == std::vector<int>{1}) && c.bytes() == 20);
    CHECK(c.find(interval(1)) == nullptr);
    CHECK(c.request(interval(3), 10));  // its counter kept counting: admitted at once
    c.insert(interval(3), 10, block(3));
    CHECK((order(c) == std::vector<int>{3, 2, 0}) && c.bytes() == 30);
    c.end_plan();
    // the evicted key counts again from nothing
    c.begin_plan(on_evict);
    for (int r = 1; r <= 3; ++r) CHECK(!c.request(interval(1), 10));
    c.end_plan();
    // a smaller budget takes the cold end at once (no plan open); 0 takes everything
    g_evicted.clear();
    c.set_budget(15, on_evict);
    CHECK((g_evicted == std::vector<int>{0, 2}) && c.bytes() == 10 && (order(c) == std::vector<int>{3}));
    c.set_budget(0, on_evict);
    CHECK((g_evicted == std::vector<int>{0, 2, 3}) && c.bytes() == 0 && c.size() == 0 && c.counters() == 0);
    c.begin_plan(on_evict);
    CHECK(!c.request(interval(3), 10));
    c.end_plan();
    std::printf("lru ok\n");
}

// random traffic: the budget is never exceeded, nothing leaves during a plan, every find returns a live
// payload, and the entries' bytes add up
void soak(unsigned seed) {
    std::mt19937 rng(seed);
    g_evicted.clear();
    Cache c;
    uint64_t budget = 64;
    c.set_budget(budget, on_evict);
    size_t admitted = 0;
    for (int plan = 0; plan < 4000; ++plan) {
        if (rng() % 97 == 0) {
            budget = rng() % 5 == 0 ? 0 : 8 + rng() % 120;
            c.set_budget(budget, on_evict);
            CHECK(c.bytes() <= budget);
        }
        if (rng() % 211 == 0) {
            c.clear(on_evict);
            CHECK(c.size() == 0 && c.bytes() == 0 && c.counters() == 0);
        }
        c.begin_plan(on_evict);
        CHECK(c.bytes() <= budget);
        const size_t evicted_at_begin = g_evicted.size();
        const size_t n = 1 + rng() % 3;
        for (size_t j = 0; j < n; ++j) {
            const int i = (int)(rng() % 12);
            const uint64_t bytes = 8 + 8 * (uint64_t)(i % 3);
            if (Block* b = c.find(interval(i))) {
                CHECK(*b->id == i);
            } else if (c.request(interval(i), bytes)) {
                CHECK(c.bytes() + bytes <= budget);
                c.insert(interval(i), bytes, block(i));
                ++admitted;
            }
            CHECK(c.bytes() <= budget);
            CHECK(g_evicted.size() == evicted_at_begin);
        }
        uint64_t sum = 0;
        c.for_each([&](const Cache::Entry& e) { sum += e.bytes; });
        CHECK(sum == c.bytes());
        c.end_plan();
        CHECK(g_evicted.size() == evicted_at_begin);
    }
    CHECK(admitted > 20 && g_evicted.size() > 10);
    c.clear(on_evict);
}

void counters() {
    Cache c;
    c.set_budget(1 << 20, on_evict);
    c.begin_plan(on_evict);
    for (int i = 0; i < 5000; ++i) {
        CHECK(!c.request(interval(i), 10));
        CHECK(c.counters() <= Cache::kMaxCounters);
    }
    CHECK(c.counters() == 5000 - 4 * (int)Cache::kMaxCounters);
    // a cleared counter starts again: three more requests before the fourth is admitted
    CHECK(!c.request(interval(0), 10) && !c.request(interval(0), 10) && !c.request(interval(0), 10));
    CHECK(c.request(interval(0), 10));
    c.end_plan();
    std::printf("counters ok\n");
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "admission") admission();
    else if (what == "keys") keys();
    else if (what == "lru") lru_and_budget();
    else if (what == "counters") counters();
    else if (what == "soak") {
        for (unsigned s = 1; s <= 20; ++s) soak(s);
        std::printf("soak ok\n");
    } else {
        std::printf("usage: derived_core admission|keys|lru|counters|soak\n");
        return 2;
    }
    return 0;
}
