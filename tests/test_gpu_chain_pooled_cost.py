"""A chain's admission is priced by what it would pay: the pooled cost when a block of the table's pool is
waiting for it (cubit_table_set_derived_chain_cost_pooled), the allocating cost when the admitting scan would
have to allocate (the default of cubit_table_set_derived_chain_cost, which also overrides both). That changes
on which request a repeated WHERE clause becomes one kept bitvector and never what a scan returns: every scan
here is compared with the oracle, and the plans, the kept entries and the pool expected at each request are
computed by a model of the rule (uses * (k - 1) * B >= (k + 1) * B + F), not typed in. Tables hold 300,001
rows as in test_gpu_derived_chains.py: three 131,072-row tiles, the last partial and not a multiple of 64;
one bitvector is B = 131,072 bytes as allocated."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.table import Context, CubitTable, padded_words
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 300_001
LEAF_BYTES = padded_words(N) * 8  # B: one table-owned bitvector of a fresh N-row table
NEVER = 2 ** 64 - 1
ALLOCATING = 2_240_000_000  # kDerivedChainCost (cubit_derived.hpp), the cost a fresh table prices an empty pool by
SLAB = 4  # blocks a table's first admission allocates (kDerivedSlabBlocks); the default budget holds more


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """The columns of test_gpu_derived_chains.py (never modified: tests copy what they change)."""
    rng = np.random.default_rng(43)
    a = rng.integers(0, 40, N).astype(np.int32)   # the interval's column (RANGE index, every value a key)
    b = rng.integers(0, 50, N).astype(np.int64)   # a range leaf (RANGE index)
    c = rng.integers(0, 12, N).astype(np.int64)   # EQUALITY index
    d = rng.integers(-1000, 1000, N).astype(np.int64)  # no index
    e = rng.integers(0, 30, N).astype(np.int64)   # a fourth indexed column (RANGE index)
    for x in (a, b, c, d, e):
        x.setflags(write=False)
    return a, b, c, d, e


def make_table(ctx, data):
    t = CubitTable(ctx, N)
    for i, x in enumerate(data):
        t.add_column(i, x)
    t.build_index(0, L.INDEX_RANGE)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_EQUALITY)
    t.build_index(4, L.INDEX_RANGE)
    return t


def interval(lo, hi):
    return F.ConjunctionAndFilter([F.ConstantFilter(">=", lo), F.ConstantFilter("<", hi)])


# 10 <= a < 20 AND b < 24: L(20), NOT L(10) of column 0 (a column group, an interval) and L(24) of column 1
def chain_filter():
    return F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})


def oracle_ids(cols, fs):
    return O.table_scan([O.Column(x) for x in cols], F.serialize(fs), len(cols[0]))


def group_admit(uses, k):
    return k >= 2 and uses * (k - 1) >= k + 1


def chain_admit(uses, k, block, cost):
    return k >= 2 and cost != NEVER and uses * (k - 1) * block >= (k + 1) * block + cost


class Model:
    """What the library is to hold after each request of chain_filter(): the interval of column 0 is a column
    group of two bitvectors kept by count; the chain stands for k bitvectors (three, two once the interval is
    kept) and is kept by cost, the pooled one when a free block waits at its request, which comes after the
    group's in the same plan. An admission takes a free block, else allocates: the table's first SLAB blocks,
    a later one its own block alone."""

    def __init__(self, pooled, allocating=ALLOCATING, block=LEAF_BYTES):
        self.block, self.allocating, self.pooled = block, allocating, pooled
        self.free = self.allocs = 0
        self.hits = self.chain_hits = 0
        self.dropped()

    def dropped(self):
        """A write to the table: every entry and counter goes, the blocks wait in the pool."""
        self.free += getattr(self, "group", False) + getattr(self, "chain", False)
        self.group = self.chain = False
        self.group_uses = self.chain_uses = 0

    def grown(self, block):
        """The bitvectors grew: the entries go and the pool is emptied, its blocks have the old size."""
        self.dropped()
        self.free, self.block = 0, block

    def _take(self):
        if self.free:
            self.free -= 1
        elif self.allocs == 0:
            self.allocs, self.free = SLAB, SLAB - 1
        else:
            self.allocs += 1

    def request(self):
        """One scan: its (K, passes)."""
        if self.chain:
            self.hits += 1
            self.chain_hits += 1
            return (1, 1)
        passes = 1
        if self.group:
            self.hits += 1
        else:
            self.group_uses += 1
            if group_admit(self.group_uses - 1, 2):
                self._take()
                self.group = True
                passes += 1
        k = 2 if self.group else 3
        self.chain_uses += 1
        if chain_admit(self.chain_uses - 1, k, self.block, self.pooled if self.free else self.allocating):
            self._take()
            self.chain = True
            return (1, passes + 1)
        return (k, passes)

    def state(self):
        kept = self.group + self.chain
        return {"derived": (kept, kept * self.block, self.hits), "chains": (int(self.chain), self.chain_hits),
                "pool": (self.free, self.allocs)}


def state(t):
    return {"derived": t.derived_stats(), "chains": t.derived_chain_stats(), "pool": t.derived_pool_stats()}


def scan_against(t, m, fs, ref, times, what=""):
    """`times` scans, each equal to ref and planned as the model says; the requests (1-based, among these) that
    kept the chain."""
    admitted = []
    for i in range(1, times + 1):
        had = m.chain
        want = m.request()
        got = t.scan(fs)
        assert np.array_equal(got, ref), (what, i)
        assert t.last_plan() == want, (what, i, t.last_plan(), want)
        assert state(t) == m.state(), (what, i)
        if m.chain and not had:
            admitted.append(i)
    return admitted


def test_pooled_cost_prices_a_chain_behind_a_kept_group(ctx, data):
    fs = chain_filter()
    ref = oracle_ids(data, fs)
    a, b = data[0], data[1]
    assert np.array_equal(ref, np.flatnonzero((a >= 10) & (a < 20) & (b < 24))) and len(ref) > 1000
    t = make_table(ctx, data)
    t.set_derived_chain_cost_pooled(10 * LEAF_BYTES)
    m = Model(pooled=10 * LEAF_BYTES)
    assert state(t) == m.state() == {"derived": (0, 0, 0), "chains": (0, 0), "pool": (0, 0)}
    # requests 1-3 read three leaves; request 4 keeps the interval, whose admission allocates the slab
    assert scan_against(t, m, fs, ref, 4, "to the group") == []
    assert t.last_plan() == (2, 2) and t.derived_pool_stats() == (SLAB - 1, SLAB)
    # the chain then stands for k = 2 and is kept on the first request r with (r - 1) * B >= 3 B + 10 B
    r = next(r for r in range(5, 100) if (r - 1) * LEAF_BYTES >= 3 * LEAF_BYTES + 10 * LEAF_BYTES)
    assert scan_against(t, m, fs, ref, r - 4 + 2, "to the chain") == [r - 4]
    assert t.last_plan() == (1, 1) and t.derived_chain_stats() == (1, 2)
    assert t.derived_stats()[:2] == (2, 2 * LEAF_BYTES) and t.derived_pool_stats() == (SLAB - 2, SLAB)
    t.close()


def test_an_empty_pool_prices_by_the_allocating_cost(ctx, data):
    a, b = data[0], data[1]
    # one literal on each of two columns: no column group precedes the chain, so nothing fills the pool
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 10), 1: F.ConstantFilter("<", 24)})
    ref = oracle_ids(data, fs)
    assert np.array_equal(ref, np.flatnonzero((a < 10) & (b < 24))) and len(ref) > 1000
    t = make_table(ctx, data)
    t.set_derived_chain_cost_pooled(0)
    assert not any(chain_admit(u, 2, LEAF_BYTES, ALLOCATING) for u in range(30))
    for i in range(30):
        assert np.array_equal(t.scan(fs), ref), i
        assert t.last_plan() == (2, 1), i
    assert t.derived_chain_stats() == (0, 0) and t.derived_stats() == (0, 0, 0) and t.derived_pool_stats() == (0, 0)
    # another filter's interval is admitted on its fourth request and its slab fills the pool
    other = F.TableFilterSet({4: interval(5, 15)})
    ref_o = oracle_ids(data, other)
    assert np.array_equal(ref_o, np.flatnonzero((data[4] >= 5) & (data[4] < 15)))
    for i in range(4):
        assert np.array_equal(t.scan(other), ref_o), i
        assert t.last_plan() == ((2, 1) if i < 3 else (1, 2)), i
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.derived_pool_stats() == (SLAB - 1, SLAB)
    # the chain's counter kept counting: with a block waiting its next request is admitted at once
    assert chain_admit(30, 2, LEAF_BYTES, 0)
    assert np.array_equal(t.scan(fs), ref) and t.last_plan() == (1, 2)
    assert t.derived_chain_stats() == (1, 0) and t.derived_pool_stats() == (SLAB - 2, SLAB)
    assert np.array_equal(t.scan(fs), ref) and t.last_plan() == (1, 1)
    assert t.derived_chain_stats() == (1, 1) and t.derived_stats()[:2] == (2, 2 * LEAF_BYTES)
    t.close()


@pytest.mark.parametrize("pooled", [0, 10 * LEAF_BYTES], ids=["count_rule", "ten_blocks"])
def test_readmission_after_an_append_in_place(ctx, data, pooled):
    fs = chain_filter()
    t = make_table(ctx, data)
    t.set_derived_chain_cost_pooled(pooled)
    m = Model(pooled=pooled)
    ref = oracle_ids(data, fs)
    first = scan_against(t, m, fs, ref, 16, "fresh")
    assert len(first) == 1 and first[0] >= 4  # no block waits before the interval's slab: request 4 at the earliest
    assert state(t)["pool"] == (SLAB - 2, SLAB)
    rng = np.random.default_rng(5)
    n_new = 1000
    add = [rng.integers(0, 40, n_new).astype(np.int32)] + [rng.integers(0, 12, n_new).astype(np.int64) for _ in range(4)]
    t.append({i: x for i, x in enumerate(add)})  # in place: bitvectors are allocated in steps of 1,048,576 rows
    m.dropped()
    assert state(t) == m.state() and state(t)["pool"] == (SLAB, SLAB) and state(t)["derived"][:2] == (0, 0)
    cols = [np.concatenate([x, y]) for x, y in zip(data, add)]
    ref2 = oracle_ids(cols, fs)
    assert len(ref2) > len(ref)
    # the counter starts from zero and every request finds a block waiting: the pooled rule from the first one
    again = scan_against(t, m, fs, ref2, 16, "after the append")
    want = next(r for r in range(1, 100) if chain_admit(r - 1, 3 if r < 4 else 2, LEAF_BYTES, pooled))
    assert again == [want] and want <= first[0] and want > 1
    if pooled == 0:
        assert (first[0], want) == (4, 3)  # the third request is priced as allocating on a fresh table only
    assert state(t)["pool"][1] == SLAB  # no device allocation the second time
    t.close()


def test_growth_empties_the_pool(ctx, data):
    fs = chain_filter()
    t = make_table(ctx, data)
    t.set_derived_chain_cost_pooled(0)
    m = Model(pooled=0)
    assert scan_against(t, m, fs, oracle_ids(data, fs), 5, "fresh") == [4]
    rng = np.random.default_rng(6)
    n_new = 800_000  # past 1,048,576 rows: every bitvector grows and the pooled blocks are of the old size
    add = [rng.integers(0, 40, n_new).astype(np.int32)] + [rng.integers(0, 12, n_new).astype(np.int64) for _ in range(4)]
    t.append({i: x for i, x in enumerate(add)})
    block = padded_words(t.n_rows) * 8
    assert block == 2 * LEAF_BYTES
    m.grown(block)
    assert state(t) == m.state() and state(t)["pool"] == (0, SLAB)
    cols = [np.concatenate([x, y]) for x, y in zip(data, add)]
    ref = oracle_ids(cols, fs)
    # no block waits, and the interval's admission (not the table's first) allocates its own block alone: the
    # chain is priced as allocating at every request, where a waiting block would have bought it on the third
    assert chain_admit(2, 3, block, 0) and not any(chain_admit(u, 2, block, ALLOCATING) for u in range(8))
    assert scan_against(t, m, fs, ref, 8, "after growth") == []
    assert t.last_plan() == (2, 1) and state(t)["pool"] == (0, SLAB + 1) and state(t)["derived"][:2] == (1, block)
    # a write pools the interval's block; the chain's counter starts again and is priced as pooled
    t.column_changed(1)
    m.dropped()
    assert state(t) == m.state() and state(t)["pool"] == (1, SLAB + 1)
    assert scan_against(t, m, fs, ref, 4, "after a write") == [3]
    assert state(t)["pool"] == (0, SLAB + 1)
    t.close()


def test_set_derived_chain_cost_overrides_the_pooled_cost(ctx, data):
    fs = chain_filter()
    ref = oracle_ids(data, fs)
    t = make_table(ctx, data)
    t.set_derived_chain_cost_pooled(0)
    t.set_derived_chain_cost(NEVER)
    m = Model(allocating=NEVER, pooled=NEVER)
    assert scan_against(t, m, fs, ref, 8, "never") == []
    assert t.last_plan() == (2, 1) and state(t)["pool"] == (SLAB - 1, SLAB)  # a block waits and is not taken
    t.set_derived_chain_cost_pooled(10 * LEAF_BYTES)
    m.pooled = 10 * LEAF_BYTES
    assert scan_against(t, m, fs, ref, 1, "ten blocks") == []  # (9 - 1) B < 13 B
    t.set_derived_chain_cost(0)
    m.allocating = m.pooled = 0
    assert scan_against(t, m, fs, ref, 2, "count rule") == [1]
    assert t.last_plan() == (1, 1) and t.derived_chain_stats() == (1, 1)
    t.close()
