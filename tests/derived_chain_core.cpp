// The chain keys of the derived-leaf policy (duckdb-cubit_amd/csrc/cubit_derived.hpp) on the CPU: the cost
// rule, key canonicalisation, and the LRU, budget and counters that chains share with the column groups.
// Built with AddressSanitizer and UBSan by tests/test_derived_chain_core.py; ends with status 1 at the
// first failed check.
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

// payload: a heap block standing for the device bitvector (a use after eviction is seen by ASan)
struct Block {
    std::unique_ptr<int> id;
};
using Cache = DerivedCache<Block>;

std::vector<int> g_evicted;
auto on_evict = [](Block& b) { g_evicted.push_back(*b.id); };
Block block(int id) { return Block{std::make_unique<int>(id)}; }

DerivedKey group_key(int column, int op, std::vector<DerivedLit> lits) {
    DerivedKey k;
    CHECK(derived_key(column, op, std::move(lits), &k));
    return k;
}
DerivedKey chain_key(const std::vector<ChainLit>& lits, std::vector<DerivedKey> unions = {}) {
    DerivedKey k;
    CHECK(derived_chain_key(lits, std::move(unions), &k));
    CHECK(derived_is_chain(k) && k.op == kDerivedAnd);
    return k;
}
// column group number i (an interval of column 1) and chain number i (that interval's literals and
// a leaf of column 2): entries 0 … 5 are groups, 6 … 11 chains
DerivedKey interval(int i) { return group_key(1, kDerivedAnd, {{0x1000u + 16u * i, false}, {0x1008u + 16u * i, true}}); }
DerivedKey chain(int i) {
    return chain_key({{1, {0x1000u + 16u * i, false}}, {1, {0x1008u + 16u * i, true}}, {2, {0x9000u + 8u * i, false}}});
}
DerivedKey entry(int i) { return i < 6 ? interval(i) : chain(i - 6); }

std::vector<int> order(const Cache& c) {
    std::vector<int> ids;
    c.for_each([&](const Cache::Entry& e) { ids.push_back(*e.payload.id); });
    return ids;
}

void cost() {
    const uint64_t max = UINT64_MAX;
    const uint64_t Bs[] = {8, 131'072, 75'104'256, 1ull << 40};
    const uint64_t Fs[] = {0, 1, 37'504, kDerivedChainCost, 1ull << 50, max - 1, max};
    for (uint64_t B : Bs)
        for (uint64_t F : Fs)
            for (uint64_t k = 0; k <= 9; ++k) {
                bool before = false;
                for (uint64_t u : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 14ull, 15ull, 1000ull, 1ull << 20, 1ull << 40, ~0ull}) {
                    const bool got = derived_chain_admit(u, k, B, F);
                    // the rule itself, in 128 bits
                    const unsigned __int128 rent = (unsigned __int128)u * (k ? k - 1 : 0) * B;
                    const unsigned __int128 buy = (unsigned __int128)(k + 1) * B + F;
                    CHECK(got == (k >= 2 && F != max && rent >= buy));
                    if (F == 0) CHECK(got == derived_admit(u, k));  // the count rule
                    if (F == max) CHECK(!got);                      // never
                    CHECK(got || !before);                          // monotone in the uses
                    before = got;
                }
            }
    // the default cost: SF100 Q6, three leaves of 75 MB, is bought at its 18th request ...
    CHECK(!derived_chain_admit(16, 3, 75'104'256, kDerivedChainCost) && derived_chain_admit(17, 3, 75'104'256, kDerivedChainCost));
    CHECK(Cache().chain_cost() == kDerivedChainCost);
    // ... and a 300,001-row table (one 131,072-byte bitvector) needs thousands of requests
    CHECK(!derived_chain_admit(8'000, 3, 131'072, kDerivedChainCost) && !derived_chain_admit(2'000, 8, 131'072, kDerivedChainCost));
    // through the cache: F = 0 admits a chain by the count rule on k, not on the key's literals
    for (uint64_t k = 2; k <= 5; ++k) {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(0);
        CHECK(c.chain_cost() == 0);
        c.begin_plan(on_evict);
        int first = -1;
        for (int r = 1; r <= 10 && first < 0; ++r)
            if (c.request(chain(0), 10, k)) first = r;
        CHECK(first == (k == 2 ? 4 : 3));
        c.end_plan();
    }
    // a cost of B * 20 with k = 3: uses * 2 >= 4 + 20, the 13th request; k changing between requests
    // is taken as it is at each request
    {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(200);
        c.begin_plan(on_evict);
        for (int r = 1; r <= 12; ++r) CHECK(!c.request(chain(0), 10, 3));
        CHECK(c.request(chain(0), 10, 3));
        CHECK(!c.request(chain(1), 10, 4) && !c.request(chain(1), 10, 4) && !c.request(chain(1), 10, 4));
        for (int r = 4; r <= 12; ++r) CHECK(!c.request(chain(1), 10, 3));  // 4 + 20 > 2 * 11
        CHECK(c.request(chain(1), 10, 3));
        // the column groups keep their own rule whatever the cost
        CHECK(!c.request(interval(0), 10) && !c.request(interval(0), 10) && !c.request(interval(0), 10));
        CHECK(c.request(interval(0), 10));
        c.end_plan();
    }
    // never: counted, not admitted; a later cost of 0 admits at once
    {
        Cache c;
        c.set_budget(1000, on_evict);
        c.set_chain_cost(max);
        c.begin_plan(on_evict);
        for (int r = 1; r <= 200; ++r) CHECK(!c.request(chain(0), 10, 8));
        c.set_chain_cost(0);
        CHECK(c.request(chain(0), 10, 2));
        c.end_plan();
    }
    std::printf("cost ok\n");
}

void keys() {
    const std::vector<ChainLit> a = {{1, {0x10, false}}, {1, {0x20, true}}, {2, {0x30, false}}, {5, {0x40, true}}};
    const DerivedKey u1 = group_key(7, kDerivedOr, {{0x50, false}, {0x58, false}, {0x60, false}});
    const DerivedKey u2 = group_key(8, kDerivedOr, {{0x70, false}, {0x78, false}});
    const DerivedKey k0 = chain_key(a, {u1, u2});
    // every order of the literals and of the unions, and a literal or a union met twice
    std::vector<size_t> p = {0, 1, 2, 3};
    do {
        std::vector<ChainLit> q;
        for (size_t i : p) q.push_back(a[i]);
        CHECK(chain_key(q, {u1, u2}) == k0 && chain_key(q, {u2, u1}) == k0);
        CHECK(!(chain_key(q, {u2, u1}) < k0) && !(k0 < chain_key(q, {u2, u1})));
        q.push_back(a[p[0]]);
        CHECK(chain_key(q, {u2, u1, u2}) == k0);
    } while (std::next_permutation(p.begin(), p.end()));
    // a complement flip, another pointer, a literal more or less, a union more or less: other keys
    for (size_t i = 0; i < a.size(); ++i) {
        std::vector<ChainLit> f = a;
        f[i].lit.second = !f[i].lit.second;
        CHECK(!(chain_key(f, {u1, u2}) == k0));
        f = a;
        f[i].lit.first += 8;
        CHECK(!(chain_key(f, {u1, u2}) == k0));
        f = a;
        f.erase(f.begin() + (long)i);
        CHECK(!(chain_key(f, {u1, u2}) == k0));
    }
    CHECK(!(chain_key(a, {u1}) == k0) && !(chain_key(a) == k0) && !(chain_key(a, {u1}) == chain_key(a)));
    // a union's leaves are not the chain's own literals: a AND (b OR c) is not a AND b AND c
    const DerivedKey flat = chain_key({{1, {0x10, false}}, {7, {0x50, false}}, {7, {0x58, false}}});
    const DerivedKey nested = chain_key({{1, {0x10, false}}}, {group_key(7, kDerivedOr, {{0x50, false}, {0x58, false}})});
    CHECK(!(flat == nested));
    // the column a literal lies on decides only whether there is a chain
    CHECK(chain_key({{1, {0x10, false}}, {2, {0x30, false}}}) == chain_key({{3, {0x30, false}}, {4, {0x10, false}}}));
    // distinct from every column key: of the same literals on any column and either operator
    std::vector<DerivedLit> lits;
    for (const ChainLit& c : a) lits.push_back(c.lit);
    const DerivedKey plain = chain_key(a);
    for (int col : {-1, 0, 1, 2, 5, 7, 1 << 20, INT_MAX})
        for (int op : {kDerivedAnd, kDerivedOr}) {
            const DerivedKey g = group_key(col, op, lits);
            CHECK(!derived_is_chain(g) && !(g == plain) && (g < plain || plain < g));
            CHECK(g.lits == plain.lits);
        }
    // one column alone, or a bitvector both plain and complemented: no chain
    DerivedKey k;
    CHECK(!derived_chain_key({}, {}, &k));
    CHECK(!derived_chain_key({{1, {0x10, false}}, {1, {0x20, true}}}, {}, &k));
    CHECK(!derived_chain_key({}, {u1}, &k));
    CHECK(!derived_chain_key({{7, {0x10, false}}}, {u1}, &k));
    CHECK(derived_chain_key({{1, {0x10, false}}}, {u1}, &k));
    CHECK(derived_chain_key({}, {u1, u2}, &k));
    CHECK(!derived_chain_key({{1, {0x10, false}}, {2, {0x30, false}}, {1, {0x10, true}}}, {}, &k));
    // an AND group or a chain is no union
    CHECK(!derived_chain_key({{1, {0x10, false}}}, {interval(0)}, &k));
    CHECK(!derived_chain_key({{1, {0x10, false}}}, {plain}, &k));
    std::printf("keys ok\n");
}

void lru_shared() {
    g_evicted.clear();
    Cache c;
    c.set_budget(30, on_evict);  // three entries of 10
    c.set_chain_cost(0);
    // a group, a chain, a group
    const int ids[3] = {0, 6, 1};
    for (int i : ids) {
        c.begin_plan(on_evict);
        int first = -1;
        for (int r = 1; r <= 10 && first < 0; ++r)
            if (c.request(entry(i), 10, 3)) first = r;
        CHECK(first == (i < 6 ? 4 : 3));
        c.insert(entry(i), 10, block(i));
        c.end_plan();
    }
    CHECK((order(c) == std::vector<int>{1, 6, 0}) && c.bytes() == 30 && c.size() == 3 && c.chain_size() == 1);
    c.begin_plan(on_evict);
    CHECK(*c.find(entry(0))->id == 0 && c.hits() == 1 && c.chain_hits() == 0);
    CHECK(*c.find(entry(6))->id == 6 && c.hits() == 2 && c.chain_hits() == 1);
    CHECK(c.find(chain(1)) == nullptr && c.hits() == 2 && c.chain_hits() == 1);
    CHECK((order(c) == std::vector<int>{6, 0, 1}));
    // a second chain is due, there is no room: nothing goes while the plan is open
    for (int r = 1; r <= 5; ++r) CHECK(!c.request(entry(7), 10, 3));
    CHECK(g_evicted.empty() && c.size() == 3);
    c.end_plan();
    // the next plan makes room: the least recently used goes, group or chain alike
    c.begin_plan(on_evict);
    CHECK((g_evicted == std::vector<int>{1}) && c.bytes() == 20 && c.chain_size() == 1);
    CHECK(c.request(entry(7), 10, 3));
    c.insert(entry(7), 10, block(7));
    CHECK((order(c) == std::vector<int>{7, 6, 0}) && c.chain_size() == 2);
    // a group is due now: the chain it waits behind is not touched during the plan
    for (int r = 1; r <= 5; ++r) CHECK(!c.request(entry(2), 10));
    c.end_plan();
    c.begin_plan(on_evict);
    CHECK((g_evicted == std::vector<int>{1, 0}) && c.chain_size() == 2);
    // the chain subsumes group 0's literals and outlives the group's eviction
    CHECK(*c.find(entry(6))->id == 6 && c.find(entry(0)) == nullptr);
    CHECK(c.request(entry(2), 10));
    c.insert(entry(2), 10, block(2));
    c.end_plan();
    CHECK((order(c) == std::vector<int>{2, 6, 7}));
    // a smaller budget takes the cold end, chains included; 0 takes everything and its counters
    g_evicted.clear();
    c.set_budget(15, on_evict);
    CHECK((g_evicted == std::vector<int>{7, 6}) && c.chain_size() == 0 && c.size() == 1 && c.bytes() == 10);
    c.begin_plan(on_evict);
    CHECK(!c.request(entry(6), 10, 3) && c.counters() == 1);  // the evicted chain counts from nothing
    c.end_plan();
    c.set_budget(0, on_evict);
    CHECK(c.size() == 0 && c.bytes() == 0 && c.counters() == 0 && c.chain_size() == 0);
    c.begin_plan(on_evict);
    CHECK(!c.request(entry(6), 10, 3) && c.counters() == 0);
    c.end_plan();
    // clear (the bits changed) takes both kinds and keeps the cost setting
    c.set_budget(30, on_evict);
    c.begin_plan(on_evict);
    c.insert(entry(6), 10, block(6));
    c.insert(entry(0), 10, block(0));
    c.end_plan();
    c.clear(on_evict);
    CHECK(c.size() == 0 && c.chain_size() == 0 && c.bytes() == 0 && c.chain_cost() == 0);
    // chains and groups share the counter bound
    Cache d;
    d.set_budget(1 << 20, on_evict);
    d.begin_plan(on_evict);
    for (int i = 0; i < 3000; ++i) {
        CHECK(!d.request(i % 2 ? interval(i) : chain(i), 10, 3));
        CHECK(d.counters() <= Cache::kMaxCounters);
    }
    d.end_plan();
    std::printf("lru ok\n");
}

// random traffic over groups and chains: the budget is never exceeded, nothing leaves during a plan,
// every find returns its own live payload, the bytes and the chain count add up
void soak(unsigned seed) {
    std::mt19937 rng(seed);
    g_evicted.clear();
    Cache c;
    uint64_t budget = 64;
    c.set_budget(budget, on_evict);
    c.set_chain_cost(40);
    size_t admitted[2] = {0, 0};
    uint64_t hits[2] = {0, 0};
    for (int plan = 0; plan < 4000; ++plan) {
        if (rng() % 97 == 0) {
            budget = rng() % 5 == 0 ? 0 : 8 + rng() % 120;
            c.set_budget(budget, on_evict);
            CHECK(c.bytes() <= budget);
        }
        if (rng() % 211 == 0) {
            c.clear(on_evict);
            CHECK(c.size() == 0 && c.bytes() == 0 && c.counters() == 0 && c.chain_size() == 0);
        }
        if (rng() % 301 == 0) c.set_chain_cost(rng() % 3 == 0 ? UINT64_MAX : rng() % 200);
        c.begin_plan(on_evict);
        CHECK(c.bytes() <= budget);
        const size_t evicted_at_begin = g_evicted.size();
        const size_t n = 1 + rng() % 3;
        for (size_t j = 0; j < n; ++j) {
            const int i = (int)(rng() % 12);
            const bool is_chain = i >= 6;
            const uint64_t bytes = 8 + 8 * (uint64_t)(i % 3);
            if (Block* b = c.find(entry(i))) {
                CHECK(*b->id == i);
                ++hits[is_chain];
            } else if (c.request(entry(i), bytes, 2 + rng() % 3)) {
                CHECK(c.bytes() + bytes <= budget);
                CHECK(!is_chain || c.chain_cost() != UINT64_MAX);
                c.insert(entry(i), bytes, block(i));
                ++admitted[is_chain];
            }
            CHECK(c.bytes() <= budget);
            CHECK(g_evicted.size() == evicted_at_begin);
        }
        uint64_t sum = 0;
        size_t chains = 0;
        c.for_each([&](const Cache::Entry& e) {
            sum += e.bytes;
            chains += derived_is_chain(e.key);
            CHECK(derived_is_chain(e.key) == (*e.payload.id >= 6));
        });
        CHECK(sum == c.bytes() && chains == c.chain_size());
        CHECK(c.hits() == hits[0] + hits[1] && c.chain_hits() == hits[1]);
        c.end_plan();
        CHECK(g_evicted.size() == evicted_at_begin);
    }
    CHECK(admitted[0] > 10 && admitted[1] > 10 && g_evicted.size() > 10 && hits[0] > 10 && hits[1] > 10);
    c.clear(on_evict);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "cost") cost();
    else if (what == "keys") keys();
    else if (what == "lru") lru_shared();
    else if (what == "soak") {
        for (unsigned s = 1; s <= 20; ++s) soak(s);
        std::printf("soak ok\n");
    } else {
        std::printf("usage: derived_chain_core cost|keys|lru|soak\n");
        return 2;
    }
    return 0;
}
