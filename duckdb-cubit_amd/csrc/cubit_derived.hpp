// Derived leaves: the policy of keeping a column's repeated leaf combination as one bitvector.
// HIP-free (tests/derived_core.cpp runs it on the CPU); cubit_capi.hip owns the device side.
//
// A scan that combines k >= 2 table-owned bitvectors of one column the same way every time (the
// interval of a RANGE index, L(hi) AND NOT L(lo); the union of EQUALITY or BINS leaves) reads k
// bitvectors where one would do. The combination is named by a canonical key; its requests are
// counted; once keeping it has paid for itself (rent or buy) it is materialised once and later
// scans read that one bitvector. The bitvectors held are bounded by a byte budget, the least
// recently used going first, and nothing is evicted while a plan is being built (a plan holds the
// pointers it has looked up until its kernel is launched).
//
// A second kind of key, the chain, names the derivable literals of one AND chain that lie on two or
// more columns (a repeated WHERE clause: the same conjunction over several indexed columns). It is
// kept by the same cache under the same budget, and bought by cost, not by count: see
// derived_chain_admit.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <list>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

namespace cubit {

enum { kDerivedAnd = 0, kDerivedOr = 1 };

// one literal of a combination: the bitvector and whether it is complemented
using DerivedLit = std::pair<uintptr_t, bool>;

struct DerivedKey {
    int column = -1;
    int op = kDerivedAnd;
    std::vector<DerivedLit> lits;  // sorted, distinct
    bool operator<(const DerivedKey& o) const {
        return std::tie(column, op, lits) < std::tie(o.column, o.op, o.lits);
    }
    bool operator==(const DerivedKey& o) const { return column == o.column && op == o.op && lits == o.lits; }
};

// The canonical key of `lits` combined by `op` on `column`: the order the planner met the literals
// in does not matter, a literal met twice counts once. False when fewer than two distinct literals
// remain, or a bitvector appears both plain and complemented (the group folds to a constant; it is
// left to the evaluator).
inline bool derived_key(int column, int op, std::vector<DerivedLit> lits, DerivedKey* out) {
    std::sort(lits.begin(), lits.end());
    lits.erase(std::unique(lits.begin(), lits.end()), lits.end());
    if (lits.size() < 2) return false;
    for (size_t i = 1; i < lits.size(); ++i)
        if (lits[i].first == lits[i - 1].first) return false;
    out->column = column;
    out->op = op;
    out->lits = std::move(lits);
    return true;
}

// The column of every chain key: no table column has it, so no chain key equals a column's key.
constexpr int kDerivedChainColumn = INT_MIN;

inline bool derived_is_chain(const DerivedKey& k) { return k.column == kDerivedChainColumn; }

// One literal of an AND chain that may join a chain key, with the column it lies on.
struct ChainLit {
    int column;
    DerivedLit lit;
};

// The canonical key of an AND chain over several columns: its plain literals and its unions (each the
// key derived_key gave for an OR group of one column, as an IN-list plans). Always on the base
// bitvectors, never on a kept group's own bitvector, whose address can be handed out again. The
// order of the literals, of the unions and inside a union does not matter. The key holds the sorted
// literals, then per union a separator ({0, true}: no bitvector lies at 0) and the union's literals.
// False when the chain lies on fewer than two columns, or a bitvector appears both plain and
// complemented among the literals.
inline bool derived_chain_key(const std::vector<ChainLit>& chain, std::vector<DerivedKey> unions, DerivedKey* out) {
    std::vector<int> columns;
    std::vector<DerivedLit> lits;
    for (const ChainLit& c : chain) {
        columns.push_back(c.column);
        lits.push_back(c.lit);
    }
    for (const DerivedKey& u : unions) {
        if (u.op != kDerivedOr || derived_is_chain(u)) return false;
        columns.push_back(u.column);
    }
    std::sort(columns.begin(), columns.end());
    if (std::unique(columns.begin(), columns.end()) - columns.begin() < 2) return false;
    std::sort(lits.begin(), lits.end());
    lits.erase(std::unique(lits.begin(), lits.end()), lits.end());
    for (size_t i = 1; i < lits.size(); ++i)
        if (lits[i].first == lits[i - 1].first) return false;
    std::sort(unions.begin(), unions.end());
    unions.erase(std::unique(unions.begin(), unions.end()), unions.end());
    for (const DerivedKey& u : unions) {
        lits.push_back({0, true});
        lits.insert(lits.end(), u.lits.begin(), u.lits.end());
    }
    out->column = kDerivedChainColumn;
    out->op = kDerivedAnd;
    out->lits = std::move(lits);
    return true;
}

// Rent or buy: materialising a combination of k bitvectors costs k reads and one write, and each
// later scan saves k - 1 reads. It is bought on the first request before which renting has
// already cost as much: uses_so_far * (k - 1) >= k + 1, uses_so_far being the requests before this
// one (an interval, k = 2: the fourth request; with a validity leaf, k = 3: the third).
inline bool derived_admit(uint64_t uses_so_far, uint64_t k) { return k >= 2 && uses_so_far * (k - 1) >= k + 1; }

// A chain is bought by cost. Renting has cost uses_so_far * (k - 1) * B bytes so far (k: the leaves the
// plan reads in the chain's place, B: the bytes of one bitvector); buying costs the (k + 1) * B of the
// materialising pass and F, the fixed cost of an admitting scan in byte-equivalents (the allocation,
// the clear, the zone-class pass and its read-back). F = 0 is derived_admit; F = UINT64_MAX never
// buys. A small table (B far below F) needs thousands of requests: a one-off query pays nothing.
inline bool derived_chain_admit(uint64_t uses_so_far, uint64_t k, uint64_t B, uint64_t F) {
    if (k < 2 || F == UINT64_MAX) return false;
    using u128 = unsigned __int128;
    return (u128)uses_so_far * (k - 1) * B >= (u128)(k + 1) * B + F;
}

// F has two values, for the two admitting scans there are. Either is what the cache starts
// with; cubit_table_set_derived_chain_cost replaces both, cubit_table_set_derived_chain_cost_pooled the
// second alone.
//
// kDerivedChainCost: the admitting scan allocates its block, as a table's first admission does. Measured
// on an MI355X at TPC-H SF100 (profiles/r13_admission_cost.txt): the scan that admitted the l_discount
// interval took 413 µs longer than the plain scans after it, 38 µs of them the bits-only pass's own
// 225 MB; the other 376 µs at the 5.97 TB/s of that scan's byte mix. With it SF100 Q6 (k = 3, B = 75 MB)
// is bought at its 18th request; a 300,001-row table (B = 131 KB as allocated) would need some 8,500.
// tests/derived_chain_core.cpp pins the admission points it gives.
//
// kDerivedChainCostPooled: the admitting scan takes a block that waits in the table's pool
// (cubit_row_list.hpp), as every admission after the table's first does while the budget holds a second
// block, and every re-admission after a write. Measured the same way (profiles/r19_admission_cost.txt):
// over 12 pooled admissions at SF100 the admitting scan took 133.0 µs against 65.7 µs for the plain K = 3
// scans before it, 50.3 µs of the difference the bits-only pass's own 300 MB, the other 17 µs at 5.97 TB/s
// 0.101 GB (0.087-0.193; 0.179 GB on an SF100 / 8 partition, where the same microseconds weigh more beside
// a smaller pass). With it SF100 Q6 from a pooled block is bought at its 4th request (with the interval,
// whose slab fills the pool in that plan), an SF100 / 8 partition at its 9th, and the 300,001-row table
// still needs some 385: a one-off query keeps paying nothing.
constexpr uint64_t kDerivedChainCost = 2'240'000'000ull;
constexpr uint64_t kDerivedChainCostPooled = 100'000'000ull;

// The cache of materialised combinations (payload P: whatever owns the bitvector) and the use
// counters of those not materialised yet.
template <class P>
class DerivedCache {
  public:
    static constexpr size_t kMaxCounters = 1024;

    struct Entry {
        DerivedKey key;
        uint64_t bytes = 0;
        P payload{};
    };

    uint64_t budget() const { return budget_; }
    uint64_t bytes() const { return bytes_; }
    size_t size() const { return lru_.size(); }
    uint64_t hits() const { return hits_; }  // of both kinds
    size_t chain_size() const { return chains_; }
    uint64_t chain_hits() const { return chain_hits_; }
    // F of derived_chain_admit for an admission that allocates its block, and for one that takes a
    // pooled block
    uint64_t chain_cost() const { return chain_cost_; }
    uint64_t chain_cost_pooled() const { return chain_cost_pooled_; }
    // Both costs at once (the override: 0 = the count rule, UINT64_MAX = never), or the pooled one
    // alone; counters keep counting under the new value
    void set_chain_cost(uint64_t fixed_bytes) { chain_cost_ = chain_cost_pooled_ = fixed_bytes; }
    void set_chain_cost_pooled(uint64_t fixed_bytes) { chain_cost_pooled_ = fixed_bytes; }
    size_t counters() const { return uses_.size(); }
    bool in_plan() const { return in_plan_; }

    // Entries from the most to the least recently used (tests, statistics).
    template <class F>
    void for_each(F&& f) const {
        for (const Entry& e : lru_) f(e);
    }

    // A plan begins: evictions owed from earlier plans happen now, before any pointer is handed
    // out. on_evict(payload) runs for every entry that goes.
    template <class F>
    void begin_plan(F&& on_evict) {
        in_plan_ = false;
        trim(want_, on_evict);
        want_ = 0;
        in_plan_ = true;
    }
    void end_plan() { in_plan_ = false; }

    // The materialised combination, now the most recently used; null when there is none.
    P* find(const DerivedKey& key) {
        auto it = index_.find(key);
        if (it == index_.end()) return nullptr;
        lru_.splice(lru_.begin(), lru_, it->second);
        ++hits_;
        if (derived_is_chain(key)) ++chain_hits_;
        return &it->second->payload;
    }

    // One more scan planned `key` (k literals, entry_bytes to keep it) and found no entry. True
    // when it is to be materialised now: the admission rule holds and the budget has room. When
    // only room is missing, the least recently used entries go at the next begin_plan and a
    // later request is admitted. A chain key passes k, the leaves the plan reads in its place at
    // this moment (after the column groups took theirs), and is admitted by cost: the pooled cost
    // when the caller says the block this admission would take is waiting, else the allocating one.
    bool request(const DerivedKey& key, uint64_t entry_bytes, uint64_t k = 0, bool pooled = false) {
        if (budget_ == 0 || entry_bytes > budget_) return false;
        auto it = uses_.find(key);
        if (it == uses_.end()) {
            if (uses_.size() >= kMaxCounters) uses_.clear();
            it = uses_.emplace(key, 0).first;
        }
        const uint64_t uses_so_far = it->second++;
        const uint64_t cost = pooled ? chain_cost_pooled_ : chain_cost_;
        if (derived_is_chain(key) ? !derived_chain_admit(uses_so_far, k, entry_bytes, cost)
                                  : !derived_admit(uses_so_far, key.lits.size()))
            return false;
        if (bytes_ + entry_bytes > budget_) {
            want_ = std::max(want_, entry_bytes);
            return false;
        }
        return true;
    }

    // Keep a combination request() admitted (the caller materialised it). Its counter ends.
    P* insert(const DerivedKey& key, uint64_t entry_bytes, P payload) {
        uses_.erase(key);
        lru_.push_front(Entry{key, entry_bytes, std::move(payload)});
        index_[key] = lru_.begin();
        bytes_ += entry_bytes;
        chains_ += derived_is_chain(key);
        return &lru_.front().payload;
    }

    // A new budget (0 = off: every entry and counter goes). Not during a plan.
    template <class F>
    void set_budget(uint64_t b, F&& on_evict) {
        budget_ = b;
        if (b == 0) {
            clear(on_evict);
            return;
        }
        want_ = std::min(want_, b);
        if (!in_plan_) trim(0, on_evict);
    }

    // The bits behind the keys changed: every entry and every counter goes.
    template <class F>
    void clear(F&& on_evict) {
        for (Entry& e : lru_) on_evict(e.payload);
        lru_.clear();
        index_.clear();
        uses_.clear();
        bytes_ = 0;
        chains_ = 0;
        want_ = 0;
    }

  private:
    // evict from the cold end until `room` more bytes fit the budget; an evicted key starts
    // counting again from nothing
    template <class F>
    void trim(uint64_t room, F&& on_evict) {
        if (in_plan_) return;
        room = std::min(room, budget_);
        while (!lru_.empty() && bytes_ + room > budget_) {
            Entry& e = lru_.back();
            on_evict(e.payload);
            bytes_ -= e.bytes;
            chains_ -= derived_is_chain(e.key);
            index_.erase(e.key);
            lru_.pop_back();
        }
    }

    uint64_t budget_ = 0;
    uint64_t bytes_ = 0;
    uint64_t hits_ = 0;
    uint64_t chain_hits_ = 0;
    size_t chains_ = 0;  // entries with a chain key
    uint64_t chain_cost_ = kDerivedChainCost;
    uint64_t chain_cost_pooled_ = kDerivedChainCostPooled;
    uint64_t want_ = 0;  // room a declined admission asked for
    bool in_plan_ = false;
    std::list<Entry> lru_;  // front = most recently used
    std::map<DerivedKey, typename std::list<Entry>::iterator> index_;
    std::map<DerivedKey, uint64_t> uses_;
};

}  // namespace cubit
