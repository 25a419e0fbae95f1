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
#pragma once

#include <algorithm>
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

// Rent or buy: materialising a combination of k bitvectors costs k reads and one write, and each
// later scan saves k - 1 reads. It is bought on the first request before which renting has
// already cost as much: uses_so_far * (k - 1) >= k + 1, uses_so_far being the requests before this
// one (an interval, k = 2: the fourth request; with a validity leaf, k = 3: the third).
inline bool derived_admit(uint64_t uses_so_far, uint64_t k) { return k >= 2 && uses_so_far * (k - 1) >= k + 1; }

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
    uint64_t hits() const { return hits_; }
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
        return &it->second->payload;
    }

    // One more scan planned `key` (k literals, entry_bytes to keep it) and found no entry. True
    // when it is to be materialised now: the admission rule holds and the budget has room. When
    // only room is missing, the least recently used entries go at the next begin_plan and a
    // later request is admitted.
    bool request(const DerivedKey& key, uint64_t entry_bytes) {
        if (budget_ == 0 || entry_bytes > budget_) return false;
        auto it = uses_.find(key);
        if (it == uses_.end()) {
            if (uses_.size() >= kMaxCounters) uses_.clear();
            it = uses_.emplace(key, 0).first;
        }
        const uint64_t uses_so_far = it->second++;
        if (!derived_admit(uses_so_far, key.lits.size())) return false;
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
            index_.erase(e.key);
            lru_.pop_back();
        }
    }

    uint64_t budget_ = 0;
    uint64_t bytes_ = 0;
    uint64_t hits_ = 0;
    uint64_t want_ = 0;  // room a declined admission asked for
    bool in_plan_ = false;
    std::list<Entry> lru_;  // front = most recently used
    std::map<DerivedKey, typename std::list<Entry>::iterator> index_;
    std::map<DerivedKey, uint64_t> uses_;
};

}  // namespace cubit
