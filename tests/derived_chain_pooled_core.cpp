// The two costs of a chain's admission (duckdb-cubit_amd/csrc/cubit_derived.hpp) on the CPU: an admitting
// scan that allocates its block pays kDerivedChainCost, one that takes a block of the table's pool pays
// kDerivedChainCostPooled, and the caller of request() says which applies. Built with AddressSanitizer and
// UBSan by tests/test_derived_chain_pooled_core.py; ends with status 1 at the first failed check.
#include <cstdio>
#include <cstdlib>
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

using u128 = unsigned __int128;

// payload: a heap block standing for the device bitvector (a use after eviction is seen by ASan)
struct Block {
    std::unique_ptr<int> id;
};
using Cache = DerivedCache<Block>;

std::vector<int> g_evicted;
auto on_evict = [](Block& b) { g_evicted.push_back(*b.id); };
Block block(int id) { return Block{std::make_unique<int>(id)}; }

// column group number i (an interval of column 1) and chain number i (that interval's literals and a leaf
// of column 2): entries 0 … 5 are groups, 6 … 11 chains
DerivedKey interval(int i) {
    DerivedKey k;
    CHECK(derived_key(1, kDerivedAnd, {{0x1000u + 16u * i, false}, {0x1008u + 16u * i, true}}, &k));
    return k;
}
DerivedKey chain(int i) {
    DerivedKey k;
    CHECK(derived_chain_key({{1, {0x1000u + 16u * i, false}}, {1, {0x1008u + 16u * i, true}}, {2, {0x9000u + 8u * i, false}}}, {}, &k));
    CHECK(derived_is_chain(k));
    return k;
}
DerivedKey entry(int i) { return i < 6 ? interval(i) : chain(i - 6); }

// The request on which the rule first holds when every request passes the same k, B and F: the
// smallest r with (r - 1) * (k - 1) * B >= (k + 1) * B + F, from the inequality itself in 128 bits.
uint64_t admission_request(uint64_t k, uint64_t B, uint64_t F) {
    const u128 buy = (u128)(k + 1) * B + F, step = (u128)(k - 1) * B;
    const u128 uses = (buy + step - 1) / step;
    return (uint64_t)uses + 1;
}

// the first request (1-based) that a fresh counter of `key` is admitted on, every request alike
int first_admitted(Cache& c, const DerivedKey& key, uint64_t bytes, uint64_t k, bool pooled, int limit) {
    for (int r = 1; r <= limit; ++r)
        if (c.request(key, bytes, k, pooled)) return r;
    return -1;
}

void select() {
    const uint64_t max = UINT64_MAX;
    // a fresh cache holds the two constants; the setters reach the slot they name
    {
        Cache c;
        CHECK(c.chain_cost() == kDerivedChainCost && c.chain_cost_pooled() == kDerivedChainCostPooled);
        c.set_chain_cost_pooled(70);
        CHECK(c.chain_cost() == kDerivedChainCost && c.chain_cost_pooled() == 70);
        c.set_chain_cost(200);
        CHECK(c.chain_cost() == 200 && c.chain_cost_pooled() == 200);  // the override of everything
        c.set_chain_cost_pooled(0);
        CHECK(c.chain_cost() == 200 && c.chain_cost_pooled() == 0);
    }
    // pooled selects the pooled cost, for chain keys only. Entries of 10 bytes, k = 3: the allocating cost
    // of 200 admits on request 13 (uses * 2 >= 4 + 20), the pooled cost of 60 on request 6 (4 + 6)
    {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(200);
        c.set_chain_cost_pooled(60);
        c.begin_plan(on_evict);
        CHECK(admission_request(3, 10, 200) == 13 && admission_request(3, 10, 60) == 6);
        CHECK(first_admitted(c, chain(0), 10, 3, false, 40) == 13);
        CHECK(first_admitted(c, chain(1), 10, 3, true, 40) == 6);
        // one counter under both costs: five requests that would allocate, then a block is waiting
        for (int r = 1; r <= 5; ++r) CHECK(!c.request(chain(2), 10, 3, false));
        CHECK(c.request(chain(2), 10, 3, true));
        // and the other way round: due under the pooled cost, the block is gone, it waits for the other
        for (int r = 1; r <= 5; ++r) CHECK(!c.request(chain(3), 10, 3, true));
        for (int r = 6; r <= 12; ++r) CHECK(!c.request(chain(3), 10, 3, false));
        CHECK(c.request(chain(3), 10, 3, false));
        // the column groups keep the count rule whatever `pooled` says
        for (bool pooled : {false, true}) {
            const DerivedKey g = interval(pooled ? 1 : 0);
            CHECK(!c.request(g, 10, 0, pooled) && !c.request(g, 10, 0, pooled) && !c.request(g, 10, 0, pooled));
            CHECK(c.request(g, 10, 0, pooled));
        }
        c.end_plan();
    }
    // UINT64_MAX in either slot never admits through that slot, and does through the other
    {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(0);
        c.set_chain_cost_pooled(max);
        c.begin_plan(on_evict);
        for (int r = 1; r <= 200; ++r) CHECK(!c.request(chain(0), 10, 8, true));
        CHECK(c.request(chain(0), 10, 2, false));
        c.end_plan();
        Cache d;
        d.set_budget(1000, on_evict);
        d.set_chain_cost(max);
        d.set_chain_cost_pooled(0);
        d.begin_plan(on_evict);
        for (int r = 1; r <= 200; ++r) CHECK(!d.request(chain(0), 10, 8, false));
        CHECK(d.request(chain(0), 10, 2, true));
        // set_chain_cost after set_chain_cost_pooled overrides it: never, then the count rule
        d.set_chain_cost(max);
        CHECK(d.chain_cost_pooled() == max);
        for (int r = 1; r <= 200; ++r) CHECK(!d.request(chain(1), 10, 8, true) && !d.request(chain(1), 10, 8, false));
        d.set_chain_cost_pooled(60);
        d.set_chain_cost(0);
        CHECK(d.chain_cost_pooled() == 0 && d.request(chain(1), 10, 2, true));
        d.end_plan();
    }
    std::printf("select ok\n");
}

// the key assertions of derived_chain_core's "cost" section, through the new signature: three arguments
// and set_chain_cost behave as before
void compat() {
    const uint64_t max = UINT64_MAX;
    CHECK(!derived_chain_admit(16, 3, 75'104'256, kDerivedChainCost) && derived_chain_admit(17, 3, 75'104'256, kDerivedChainCost));
    CHECK(Cache().chain_cost() == kDerivedChainCost);
    CHECK(kDerivedChainCost == 2'240'000'000ull);
    // a fresh cache asked with three arguments, or with pooled = false, prices by the allocating constant:
    // SF100 Q6 on its 18th request
    for (int form = 0; form < 2; ++form) {
        Cache c;
        c.set_budget(1ull << 40, on_evict);
        c.begin_plan(on_evict);
        int first = -1;
        for (int r = 1; r <= 40 && first < 0; ++r)
            if (form ? c.request(chain(0), 75'104'256, 3, false) : c.request(chain(0), 75'104'256, 3)) first = r;
        CHECK(first == 18);
        c.end_plan();
    }
    // F = 0 admits a chain by the count rule on k, not on the key's literals, with or without a block waiting
    for (uint64_t k = 2; k <= 5; ++k)
        for (int form = 0; form < 3; ++form) {
            Cache c;
            c.set_budget(1000, on_evict);
            c.set_chain_cost(0);
            CHECK(c.chain_cost() == 0 && c.chain_cost_pooled() == 0);
            c.begin_plan(on_evict);
            int first = -1;
            for (int r = 1; r <= 10 && first < 0; ++r)
                if (form == 0 ? c.request(chain(0), 10, k) : c.request(chain(0), 10, k, form == 2)) first = r;
            CHECK(first == (k == 2 ? 4 : 3));
            c.end_plan();
        }
    // a cost of B * 20 with k = 3: the 13th request, under either value of pooled; k changing between
    // requests is taken as it is at each request
    for (bool pooled : {false, true}) {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(200);
        c.begin_plan(on_evict);
        for (int r = 1; r <= 12; ++r) CHECK(!c.request(chain(0), 10, 3, pooled));
        CHECK(c.request(chain(0), 10, 3, pooled));
        CHECK(!c.request(chain(1), 10, 4) && !c.request(chain(1), 10, 4, pooled) && !c.request(chain(1), 10, 4));
        for (int r = 4; r <= 12; ++r) CHECK(!c.request(chain(1), 10, 3, pooled));
        CHECK(c.request(chain(1), 10, 3));
        CHECK(!c.request(interval(0), 10) && !c.request(interval(0), 10) && !c.request(interval(0), 10));
        CHECK(c.request(interval(0), 10));
        c.end_plan();
    }
    // never: counted, not admitted; a later cost of 0 admits at once
    for (bool pooled : {false, true}) {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(max);
        c.begin_plan(on_evict);
        for (int r = 1; r <= 200; ++r) CHECK(!c.request(chain(0), 10, 8, pooled));
        c.set_chain_cost(0);
        CHECK(c.request(chain(0), 10, 2, pooled));
        c.end_plan();
    }
    std::printf("compat ok\n");
}

// what the committed constants give, derived from them by the rule
void constants() {
    const uint64_t sf100 = 75'104'256, small = 131'072;
    CHECK(kDerivedChainCostPooled < kDerivedChainCost);
    // the helper is the rule: the request before it is refused, it is admitted
    for (uint64_t B : {small, sf100})
        for (uint64_t F : {kDerivedChainCost, kDerivedChainCostPooled}) {
            const uint64_t r = admission_request(3, B, F);
            CHECK(r >= 2 && derived_chain_admit(r - 1, 3, B, F) && !derived_chain_admit(r - 2, 3, B, F));
        }
    const uint64_t big_alloc = admission_request(3, sf100, kDerivedChainCost);
    const uint64_t big_pooled = admission_request(3, sf100, kDerivedChainCostPooled);
    const uint64_t small_alloc = admission_request(3, small, kDerivedChainCost);
    const uint64_t small_pooled = admission_request(3, small, kDerivedChainCostPooled);
    std::printf("admission requests: SF100 Q6 (k = 3, B = %llu) allocating %llu, pooled %llu; 300,001 rows (k = 3, B = %llu) "
                "allocating %llu, pooled %llu\n", (unsigned long long)sf100, (unsigned long long)big_alloc,
                (unsigned long long)big_pooled, (unsigned long long)small, (unsigned long long)small_alloc,
                (unsigned long long)small_pooled);
    CHECK(big_alloc == 18);
    // (a) a 300,001-row table is not admitted within 60 requests from a pooled block, at any k its plans
    // pass (the requests before its column groups are kept count more leaves: up to 6)
    CHECK(small_pooled > 60);
    for (uint64_t k = 2; k <= 6; ++k) CHECK(!derived_chain_admit(59, k, small, kDerivedChainCostPooled));
    // (b) SF100 Q6 from a pooled block is admitted by its 8th request
    CHECK(big_pooled <= 8);
    // and through a fresh cache, which holds the constants: the same requests
    for (uint64_t B : {small, sf100}) {
        Cache c;
        c.set_budget(1ull << 40, on_evict);
        c.begin_plan(on_evict);
        const uint64_t want = B == small ? small_pooled : big_pooled;
        CHECK(first_admitted(c, chain(0), B, 3, true, 100'000) == (int)want);
        c.end_plan();
    }
    std::printf("constants ok\n");
}

// random traffic with `pooled` drawn per request: the bytes held never exceed the budget, and an
// admission with pooled = false never happens below the allocating rule (nor one with pooled = true below
// the pooled rule)
void soak(unsigned seed) {
    std::mt19937 rng(seed);
    g_evicted.clear();
    Cache c;
    uint64_t budget = 64;
    c.set_budget(budget, on_evict);
    c.set_chain_cost(120);
    c.set_chain_cost_pooled(16);
    uint64_t uses[12] = {};  // the requests of each key since its counter last began
    size_t admitted[3] = {0, 0, 0};  // groups, chains allocating, chains pooled
    auto forget = [&] { std::fill(uses, uses + 12, 0); };
    for (int plan = 0; plan < 4000; ++plan) {
        if (rng() % 97 == 0) {
            budget = rng() % 5 == 0 ? 0 : 8 + rng() % 120;
            c.set_budget(budget, on_evict);
            CHECK(c.bytes() <= budget);
            if (budget == 0) forget();
        }
        if (rng() % 211 == 0) {
            c.clear(on_evict);
            CHECK(c.size() == 0 && c.bytes() == 0 && c.counters() == 0);
            forget();
        }
        switch (rng() % 400) {
            case 0: c.set_chain_cost(rng() % 3 == 0 ? UINT64_MAX : rng() % 200); break;
            case 1: c.set_chain_cost_pooled(rng() % 3 == 0 ? UINT64_MAX : rng() % 60); break;
            case 2: c.set_chain_cost(120); c.set_chain_cost_pooled(16); break;
            default: break;
        }
        c.begin_plan(on_evict);
        CHECK(c.bytes() <= budget);
        const size_t evicted_at_begin = g_evicted.size();
        const size_t n = 1 + rng() % 3;
        for (size_t j = 0; j < n; ++j) {
            const int i = (int)(rng() % 12);
            const bool is_chain = i >= 6;
            const uint64_t bytes = 8 + 8 * (uint64_t)(i % 3);
            const uint64_t k = 2 + rng() % 3;
            const bool pooled = rng() % 2;
            if (Block* b = c.find(entry(i))) {
                CHECK(*b->id == i);
                continue;
            }
            const bool counted = budget != 0 && bytes <= budget;
            const uint64_t before = uses[i];
            if (counted) ++uses[i];
            if (c.request(entry(i), bytes, k, pooled)) {
                CHECK(counted && c.bytes() + bytes <= budget);
                if (is_chain) {
                    const uint64_t cost = pooled ? c.chain_cost_pooled() : c.chain_cost();
                    CHECK(cost != UINT64_MAX);
                    CHECK((u128)before * (k - 1) * bytes >= (u128)(k + 1) * bytes + cost);
                } else {
                    CHECK(before >= 3);  // an interval: the fourth request
                }
                c.insert(entry(i), bytes, block(i));
                uses[i] = 0;
                ++admitted[is_chain ? 1 + pooled : 0];
            }
            CHECK(c.bytes() <= budget);
            CHECK(g_evicted.size() == evicted_at_begin);
        }
        uint64_t sum = 0;
        c.for_each([&](const Cache::Entry& e) { sum += e.bytes; });
        CHECK(sum == c.bytes() && c.counters() <= Cache::kMaxCounters);
        c.end_plan();
    }
    CHECK(admitted[0] > 10 && admitted[1] > 3 && admitted[2] > 10 && g_evicted.size() > 10);
    c.clear(on_evict);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "select") select();
    else if (what == "compat") compat();
    else if (what == "constants") constants();
    else if (what == "soak") {
        for (unsigned s = 1; s <= 20; ++s) soak(s);
        std::printf("soak ok\n");
    } else {
        std::printf("usage: derived_chain_pooled_core select|compat|constants|soak\n");
        return 2;
    }
    return 0;
}
