// Row lists: the policy of keeping a sparse, repeatedly decoded bitvector's set rows as 16-bit
// offsets beside its per-tile counts. HIP-free (tests/row_list_core.cpp runs it on the CPU);
// cubit_capi.hip owns the device side, cubit_kernels.hip writes and reads the lists.
//
// A decode of one table-owned bitvector alone (an index leaf, a kept group or chain) reads the
// whole bitvector, B bytes, to write 8 bytes per set row. The same rows as ascending offsets within
// each 131,072-row tile take 2 bytes each: the low 16 bits in `off`, tile t's entries at
// prefix[t] .. prefix[t + 1], and per tile the number of entries below row 65,536 in `lo_cnt`,
// which restores the 17th bit (the entries of a tile ascend, so those come first).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define CUBIT_RL_HD __host__ __device__
#else
#define CUBIT_RL_HD
#endif

namespace cubit {

constexpr uint32_t kRowListTileRows = 131072;
constexpr uint32_t kRowListHalf = 65536;

// entry of a tile-local offset, and the offset of entry i of a tile with lo_cnt entries below the half
CUBIT_RL_HD inline uint16_t row_list_encode(uint32_t offset) { return (uint16_t)(offset & 0xffffu); }
CUBIT_RL_HD inline uint32_t row_list_decode(uint16_t off, uint32_t i, uint32_t lo_cnt) {
    return (uint32_t)off + (i >= lo_cnt ? kRowListHalf : 0u);
}

// L: the bytes of a list of q rows over `tiles` tiles
inline uint64_t row_list_bytes(uint64_t q, uint64_t tiles) { return 2 * q + 4 * tiles; }

// The byte rule: a list is wanted only when L <= B / 2, B the bytes of the bitvector's words. At
// L = B a list scan reads as much as a bitvector scan; at B / 2 each list scan saves at least B / 2,
// and the first of them repays the L bytes the building scan wrote on top of its own work.
inline bool row_list_wanted(uint64_t q, uint64_t tiles, uint64_t bitvector_bytes) {
    return 2 * row_list_bytes(q, tiles) <= bitvector_bytes;
}

enum RowListStep { kRowListNone = 0, kRowListBuild = 1, kRowListRead = 2 };

// What the n-th decode of a bitvector alone does (solo_before: such decodes before this one, since the
// bitvector last changed). The first uploads the per-tile prefix only, so a one-off query pays
// nothing; the second writes the list as a side output when the byte rule holds and the list fits
// the room left; every later one reads it. A list that could not be built (no room, rule not met)
// is asked for again by each later decode, which costs a comparison.
inline RowListStep row_list_step(uint64_t solo_before, bool has_list, bool wanted, uint64_t list_bytes, uint64_t room) {
    if (has_list) return kRowListRead;
    if (solo_before < 1 || !wanted || list_bytes > room) return kRowListNone;
    return kRowListBuild;
}

// The lists of one table and their bytes, which count against the table's derived budget beside the
// kept bitvectors (`held`: the bytes those hold). A list is built only into room nobody uses, and
// lists go before any kept bitvector does: shed() runs whenever the bitvectors grow or the budget
// shrinks, and the bitvector cache itself never counts list bytes, so a list cannot push one out.
template <class Key>
class RowListBook {
  public:
    size_t size() const { return lists_.size(); }
    uint64_t bytes() const { return bytes_; }
    bool has(const Key& k) const { return lists_.count(k) != 0; }

    // bytes a new list may take without evicting anything (budget 0: no lists)
    uint64_t room(uint64_t budget, uint64_t held) const {
        return budget > held + bytes_ ? budget - held - bytes_ : 0;
    }

    void add(const Key& k, uint64_t list_bytes) {
        drop(k);
        lists_[k] = Item{list_bytes, ++clock_};
        bytes_ += list_bytes;
    }

    // the list of k goes (its bitvector changed or left); false when there was none
    bool drop(const Key& k) {
        auto it = lists_.find(k);
        if (it == lists_.end()) return false;
        bytes_ -= it->second.bytes;
        lists_.erase(it);
        return true;
    }

    void clear() {
        lists_.clear();
        bytes_ = 0;
    }

    // Drop lists, the oldest first, until bitvectors and lists fit the budget together;
    // on_drop(key) frees each. Returns how many went.
    template <class F>
    size_t shed(uint64_t budget, uint64_t held, F&& on_drop) {
        size_t n = 0;
        while (!lists_.empty() && held + bytes_ > budget) {
            auto oldest = lists_.begin();
            for (auto it = lists_.begin(); it != lists_.end(); ++it)
                if (it->second.stamp < oldest->second.stamp) oldest = it;
            const Key k = oldest->first;
            bytes_ -= oldest->second.bytes;
            lists_.erase(oldest);
            on_drop(k);
            ++n;
        }
        return n;
    }

  private:
    struct Item {
        uint64_t bytes = 0;
        uint64_t stamp = 0;
    };
    std::map<Key, Item> lists_;
    uint64_t bytes_ = 0;
    uint64_t clock_ = 0;
};

// A free list of equally sized device blocks (handle H: whatever owns one). The derived bitvectors
// of a table all have cap_words words, and every write to the table drops them all; the blocks wait
// here instead of going back to the allocator, whose call costs more than the scan that needs the
// block. The blocks kept are bounded by `bound` bytes (the derived budget): give() hands back what
// does not fit, for the caller to free.
//
// Blocks a table's first admission allocates, itself included (cubit_capi.hip, alloc_derived_bv).
constexpr uint64_t kDerivedSlabBlocks = 4;

template <class H>
class BlockPool {
  public:
    uint64_t block_bytes() const { return block_bytes_; }
    size_t free_blocks() const { return free_.size(); }
    uint64_t free_bytes() const { return free_.size() * block_bytes_; }
    uint64_t device_allocs() const { return device_allocs_; }

    // The block size changed (the table's bitvectors grew) or pooling ends (bound 0): every free
    // block goes through on_free.
    template <class F>
    void reset(uint64_t block_bytes, uint64_t bound, F&& on_free) {
        if (block_bytes != block_bytes_ || bound == 0) clear(on_free);
        block_bytes_ = block_bytes;
        bound_ = bound;
        while (!free_.empty() && free_bytes() > bound_) {
            on_free(free_.back());
            free_.pop_back();
        }
    }

    template <class F>
    void clear(F&& on_free) {
        for (H& h : free_) on_free(h);
        free_.clear();
    }

    // A free block into *out; false when there is none (the caller allocates and calls allocated()).
    bool take(H* out) {
        if (free_.empty()) return false;
        *out = std::move(free_.back());
        free_.pop_back();
        return true;
    }
    void allocated() { ++device_allocs_; }

    // A block of `bytes` comes back. False (and h untouched) when it is not of the pool's size or
    // would exceed the bound: the caller frees it.
    bool give(H& h, uint64_t bytes) {
        if (bytes != block_bytes_ || bound_ == 0 || free_bytes() + block_bytes_ > bound_) return false;
        free_.push_back(std::move(h));
        return true;
    }

  private:
    uint64_t block_bytes_ = 0;
    uint64_t bound_ = 0;
    uint64_t device_allocs_ = 0;
    std::vector<H> free_;
};

}  // namespace cubit
