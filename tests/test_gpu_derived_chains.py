"""Chains: the derivable literals of one AND chain that lie on two or more columns (a repeated WHERE clause)
are kept as one table-owned bitvector, under the budget and LRU of the column groups of
test_gpu_derived_leaves.py, and bought by cost. That changes how many bitvectors a scan reads and never what
it returns: every scan here is compared with the oracle, before admission, on the admitting scan, after it,
with the literals in another order, beside a K0 leaf, under an OR, under MVCC views that may and may not use
the entry, after every kind of maintenance, and while a budget of one leaf makes a chain and a column group
evict each other. The cost is set to 0 (the count rule: uses * (k - 1) >= k + 1 on the k bitvectors the plan
reads in the chain's place) except where the default is the subject. Tables hold 300,001 rows: three
131,072-row tiles, the last partial and not a multiple of 64."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.table import Context, CubitTable, padded_words, runs_in_row_order
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 300_001
LEAF_BYTES = padded_words(N) * 8  # one table-owned bitvector of a fresh N-row table
TXN = 4611686018427388000
NOT_DELETED = np.uint64(2 ** 64 - 2)
NEVER = 2 ** 64 - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """The columns every test builds its table from (never modified: tests copy what they change)."""
    rng = np.random.default_rng(43)
    a = rng.integers(0, 40, N).astype(np.int32)   # the interval's column (RANGE index, every value a key)
    b = rng.integers(0, 50, N).astype(np.int64)   # a range leaf (RANGE index)
    c = rng.integers(0, 12, N).astype(np.int64)   # the IN-list's column (EQUALITY index)
    d = rng.integers(-1000, 1000, N).astype(np.int64)  # no index: summed, and the K0 leaf
    e = rng.integers(0, 30, N).astype(np.int64)   # a fourth indexed column (RANGE index)
    for x in (a, b, c, d, e):
        x.setflags(write=False)
    return a, b, c, d, e


def make_table(ctx, data, a=None, cost=0):
    a0, b, c, d, e = data
    t = CubitTable(ctx, N)
    for i, x in enumerate((a0 if a is None else a, b, c, d, e)):
        t.add_column(i, x)
    t.build_index(0, L.INDEX_RANGE)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_EQUALITY)
    t.build_index(4, L.INDEX_RANGE)
    if cost is not None:
        t.set_derived_chain_cost(cost)
    return t


def interval(lo, hi):
    return F.ConjunctionAndFilter([F.ConstantFilter(">=", lo), F.ConstantFilter("<", hi)])


def in_list(*vals):
    return F.ConjunctionOrFilter([F.ConstantFilter("=", v) for v in vals])


def ocols(data):
    return [O.Column(x) for x in data]


def oracle_ids(cols, fs, residual=None, n=N, tx=None):
    return O.table_scan(cols, F.serialize(fs, residual), n, tx=tx)


def scan_plans(t, fs, ref, times, residual=None, txn=None, what="", **kw):
    """`times` ordered scans, each equal to ref; their (K, passes)."""
    plans = []
    for i in range(times):
        got = t.scan(fs, residual, txn=txn, **kw)
        plans.append(t.last_plan())
        assert np.array_equal(got, ref), (what, i, plans)
    return plans


def test_three_column_conjunction(ctx, data):
    a, b, c, d, e = data
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24), 2: in_list(3, 5, 9)})
    mask = (a >= 10) & (a < 20) & (b < 24) & np.isin(c, (3, 5, 9))
    ref = oracle_ids(ocols(data), fs)
    assert np.array_equal(ref, np.flatnonzero(mask)) and len(ref) > 1000
    t = make_table(ctx, data)
    assert t.derived_stats() == (0, 0, 0) and t.derived_chain_stats() == (0, 0)
    # L(20), NOT L(10), L(24) and three equality leaves: K = 6. The third scan keeps the union (a group of
    # three: its third request), then the chain, which then stands for four bitvectors (2 * 3 >= 5): two
    # extra bits-only passes. From the fourth scan on the plan is the kept leaf alone.
    assert scan_plans(t, fs, ref, 4) == [(6, 1), (6, 1), (1, 3), (1, 1)]
    assert t.derived_stats() == (2, 2 * LEAF_BYTES, 1) and t.derived_chain_stats() == (1, 1)
    raw = t.scan(fs, ordered=False)
    assert t.last_plan() == (1, 1) and ctx.last_decode_kernel() == L.DECODE_PREFIXED
    directory, _ = ctx.last_tiles()
    assert int(directory[:, 1].sum()) == len(ref)
    assert np.array_equal(runs_in_row_order(raw, directory), ref)
    assert np.array_equal(t.scan(fs, zonemap=False), ref) and t.last_plan() == (1, 1)
    # the same filter written in another order hits the entry
    fs_r = F.TableFilterSet({2: in_list(9, 3, 5), 1: F.ConstantFilter("<", 24),
                             0: F.ConjunctionAndFilter([F.ConstantFilter("<", 20), F.ConstantFilter(">=", 10)])})
    res_r = F.And(F.Cmp(1, "<", 24), F.And(F.Cmp(0, "<", 20), F.Or(F.Cmp(2, "=", 5), F.Cmp(2, "=", 9), F.Cmp(2, "=", 3))),
                  F.Cmp(0, ">=", 10))
    assert scan_plans(t, fs_r, ref, 1) == [(1, 1)]
    assert scan_plans(t, None, ref, 1, residual=res_r) == [(1, 1)]
    assert t.derived_chain_stats() == (1, 5)
    # another constant is another chain: the kept union, L(25), and the interval, which the first three scans
    # requested as a column group and this fourth request keeps
    fs_o = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 25), 2: in_list(3, 5, 9)})
    assert scan_plans(t, fs_o, oracle_ids(ocols(data), fs_o), 2) == [(3, 2), (3, 1)]
    assert t.derived_stats()[:2] == (3, 3 * LEAF_BYTES) and t.derived_chain_stats() == (1, 5)
    # count, sum_product and aggregate through the entry, against a table that never keeps a chain
    plain = make_table(ctx, data, cost=NEVER)
    want_sum = int((d[mask].astype(object) * b[mask].astype(object)).sum())
    for tt in (t, plain):
        assert tt.count(fs) == len(ref)
        assert tt.sum_product(3, 1, fs) == (want_sum, len(ref))
        got = tt.aggregate(3, fs)
        assert got == (int(d[mask].sum()), int(d[mask].min()), int(d[mask].max()), len(ref), len(ref))
        if tt is t:
            assert t.last_plan() == (1, 1)
    assert t.derived_chain_stats() == (1, 8)
    assert plain.derived_chain_stats() == (0, 0) and plain.last_plan()[0] > 1  # its column groups only
    plain.close()
    t.close()


def test_chain_beside_a_k0_leaf(ctx, data):
    a, b, c, d, e = data
    # column 3 has no index: its comparison is a K0 leaf, built per scan, and stays outside the chain
    fs = F.TableFilterSet({0: interval(10, 14), 1: F.ConstantFilter("<", 10), 3: F.ConstantFilter("<", 0)})
    ref = oracle_ids(ocols(data), fs)
    assert np.array_equal(ref, np.flatnonzero((a >= 10) & (a < 14) & (b < 10) & (d < 0))) and len(ref) > 100
    t = make_table(ctx, data)
    t.use_narrowing(False)
    # L(14), NOT L(10), L(10) of column 1 and the K0 leaf; the chain of three is kept by its third request
    assert scan_plans(t, fs, ref, 4) == [(4, 1), (4, 1), (2, 2), (2, 1)]
    assert t.last_narrowed() == 0 and t.last_k0_order() == [3]
    assert t.derived_chain_stats() == (1, 1)
    # narrowing on: the kept leaf (estimated from what it replaced: 0.1 * 0.2 of the rows) is the mask the K0
    # column is read through, and the plan ends as the narrowed leaf
    t.use_narrowing(True)
    assert scan_plans(t, fs, ref, 2) == [(1, 2), (1, 2)]
    assert t.last_narrowed() == 1 and t.last_k0_order() == [3]
    assert t.count(fs) == len(ref)
    assert t.derived_chain_stats() == (1, 4)
    t.use_narrowing(False)
    assert scan_plans(t, fs, ref, 1, zonemap=False) == [(2, 1)]
    assert t.derived_stats()[:2] == (1, LEAF_BYTES)
    t.close()


def test_or_of_two_chains(ctx, data):
    a, b, c, d, e = data
    res = F.Or(F.And(F.Cmp(0, "<", 10), F.Cmp(1, "<", 24)), F.And(F.Cmp(2, "=", 3), F.Cmp(4, "<", 7)))
    ref = oracle_ids(ocols(data), None, res)
    assert np.array_equal(ref, np.flatnonzero(((a < 10) & (b < 24)) | ((c == 3) & (e < 7))))
    t = make_table(ctx, data)
    # each AND is a chain of two bitvectors, kept by its fourth request: two extra passes in one scan
    assert scan_plans(t, None, ref, 5, residual=res) == [(4, 1)] * 3 + [(2, 3), (2, 1)]
    assert t.derived_stats() == (2, 2 * LEAF_BYTES, 2) and t.derived_chain_stats() == (2, 2)
    assert scan_plans(t, None, ref, 1, residual=res, zonemap=False) == [(2, 1)]
    assert t.count(None, res) == len(ref)
    # one of the chains alone, and the two the other way round
    fs_one = F.TableFilterSet({4: F.ConstantFilter("<", 7), 2: F.ConstantFilter("=", 3)})
    assert scan_plans(t, fs_one, np.flatnonzero((c == 3) & (e < 7)), 1) == [(1, 1)]
    res_r = F.Or(F.And(F.Cmp(4, "<", 7), F.Cmp(2, "=", 3)), F.And(F.Cmp(1, "<", 24), F.Cmp(0, "<", 10)))
    assert scan_plans(t, None, ref, 1, residual=res_r) == [(2, 1)]
    assert t.derived_chain_stats() == (2, 9)
    t.close()


def test_mvcc_visibility_leaf_stays_outside(ctx, data):
    a, b, c, d, e = data
    rng = np.random.default_rng(11)
    t = make_table(ctx, data)
    # deletes committed at 4 and an insert range committed at 6
    del_rows = np.sort(rng.choice(N, size=20_000, replace=False)).astype(np.int64)
    t.set_deletes(del_rows, np.full(len(del_rows), 4, dtype=np.uint64))
    deleted = np.full(N, NOT_DELETED, dtype=np.uint64)
    deleted[del_rows] = 4
    inserted = np.zeros(N, dtype=np.uint64)
    inserted[250_000:280_000] = 6
    t.set_inserts(np.array([250_000]), np.array([280_000]), np.array([6], dtype=np.uint64))
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})

    def view(start, tid):
        return L.Txn(start, tid), oracle_ids(ocols(data), fs, tx=O.Mvcc(start, tid, inserted=inserted, deleted=deleted))

    # a reader after both: the chain of three is kept by its third request, the visibility leaf beside it
    late, ref_late = view(10, TXN + 1)
    assert scan_plans(t, fs, ref_late, 4, txn=late, what="late") == [(4, 1), (4, 1), (2, 2), (2, 1)]
    # a reader between them sees the deletes and not the inserted rows: the same entry, another visibility leaf
    mid, ref_mid = view(5, TXN + 2)
    assert len(ref_mid) < len(ref_late)
    assert scan_plans(t, fs, ref_mid, 2, txn=mid, what="mid") == [(2, 1)] * 2
    # a reader before everything: no delete in effect, the insert range hidden
    old, ref_old = view(2, TXN + 3)
    assert not np.array_equal(ref_old, ref_mid)
    assert scan_plans(t, fs, ref_old, 1, txn=old, what="old") == [(2, 1)]
    # no transaction: every row, the kept leaf alone
    ref_all = oracle_ids(ocols(data), fs)
    assert scan_plans(t, fs, ref_all, 1) == [(1, 1)]
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.derived_chain_stats() == (1, 5)
    t.close()


def test_mvcc_views_of_updated_columns(ctx, data):
    a, b, c, d, e = data
    rng = np.random.default_rng(9)
    t = make_table(ctx, data)
    # column 0 updated at version 7, column 1 at version 3
    rows0 = np.sort(rng.choice(N, size=4_000, replace=False)).astype(np.int64)
    vals0 = rng.integers(0, 40, len(rows0)).astype(np.int64)
    vers0 = np.full(len(rows0), 7, dtype=np.uint64)
    rows1 = np.sort(rng.choice(N, size=4_000, replace=False)).astype(np.int64)
    vals1 = rng.integers(0, 50, len(rows1)).astype(np.int64)
    vers1 = np.full(len(rows1), 3, dtype=np.uint64)
    t.set_updates(0, rows0, vals0, vers0)
    t.set_updates(1, rows1, vals1, vers1)
    oc = ocols(data)
    oc[0] = O.Column(a, updates=(rows0, vals0, vers0))
    oc[1] = O.Column(b, updates=(rows1, vals1, vers1))
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24), 2: F.ConstantFilter("=", 3)})

    def view(start, tid):
        return L.Txn(start, tid), oracle_ids(oc, fs, tx=O.Mvcc(start, tid))

    # a snapshot before every update: the chain of all three columns (four bitvectors) by its third request
    old, ref_old = view(2, TXN + 1)
    assert np.array_equal(ref_old, np.flatnonzero((a >= 10) & (a < 20) & (b < 24) & (c == 3)))
    assert scan_plans(t, fs, ref_old, 4, txn=old, what="old") == [(4, 1), (4, 1), (1, 2), (1, 1)]
    assert t.derived_chain_stats() == (1, 1)
    # sees column 1's updates: its leaf is patched and stays outside. The interval is now on its fourth
    # request and kept as a column group; with column 2's leaf it is a smaller chain of two bitvectors,
    # kept by that chain's fourth request
    mid, ref_mid = view(5, TXN + 2)
    assert not np.array_equal(ref_mid, ref_old)
    assert scan_plans(t, fs, ref_mid, 5, txn=mid, what="mid") == [(3, 2), (3, 1), (3, 1), (2, 2), (2, 1)]
    assert t.derived_stats()[:2] == (3, 3 * LEAF_BYTES) and t.derived_chain_stats() == (2, 2)
    # sees column 0's updates too: only column 2 is left, and one column is no chain
    new, ref_new = view(10, TXN + 3)
    assert not np.array_equal(ref_new, ref_mid)
    assert scan_plans(t, fs, ref_new, 4, txn=new, what="new") == [(4, 1)] * 4
    assert t.derived_chain_stats() == (2, 2)
    # the entries are still there for those who may use them
    assert scan_plans(t, fs, ref_old, 1, txn=old, what="old again") == [(1, 1)]
    assert scan_plans(t, fs, ref_mid, 1, txn=mid, what="mid again") == [(2, 1)]
    assert t.derived_chain_stats() == (2, 4)
    t.close()


def test_maintenance_drops_the_entry(ctx, data):
    a, b, c, d, e = data
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})
    admitted = [(3, 1), (3, 1), (1, 2), (1, 1)]
    t = make_table(ctx, data)
    cols = [x.copy() for x in data]

    def check(what):
        assert t.derived_stats()[:2] == (0, 0) and t.derived_chain_stats()[0] == 0, what
        ref = oracle_ids([O.Column(x) for x in cols], fs, n=len(cols[0]))
        assert np.array_equal(ref, np.flatnonzero((cols[0] >= 10) & (cols[0] < 20) & (cols[1] < 24)))
        assert scan_plans(t, fs, ref, 4, what=what) == admitted
        assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.derived_chain_stats()[0] == 1, what
        return ref

    before = check("fresh")
    rng = np.random.default_rng(5)
    # an append in place (bitvectors are allocated in steps of 1,048,576 rows)
    n_new = 50_000
    add = [rng.integers(0, 40, n_new).astype(np.int32)] + [rng.integers(0, 12, n_new).astype(np.int64) for _ in range(4)]
    t.append({i: x for i, x in enumerate(add)})
    cols = [np.concatenate([x, y]) for x, y in zip(cols, add)]
    after = check("append")
    assert len(after) > len(before)
    # update records merged into column 0 and its index
    rows = np.sort(rng.choice(t.n_rows, size=3_000, replace=False)).astype(np.int64)
    vals = rng.integers(0, 40, len(rows)).astype(np.int64)
    t.set_updates(0, rows, vals, np.full(len(rows), 3, dtype=np.uint64))
    assert t.derived_chain_stats()[0] == 1  # pending records leave the base bits alone
    assert t.merge_updates(0, 5) == len(rows)
    cols[0][rows] = vals.astype(np.int32)
    merged = check("merge_updates")
    assert not np.array_equal(merged, after)
    # column 1 brought to new values
    new_b = cols[1].copy()
    changed = rng.choice(t.n_rows, size=5_000, replace=False)
    new_b[changed] = rng.integers(0, 50, len(changed))
    n_changed, applied = t.sync_column(1, new_b)
    assert applied and 0 < n_changed <= len(changed)
    cols[1] = new_b
    synced = check("sync_column")
    assert not np.array_equal(synced, merged)
    # column 0's index rebuilt on other keys (10 and 20 still among them)
    t.build_index(0, L.INDEX_RANGE, list(range(0, 40, 2)))
    assert np.array_equal(check("index rebuild"), synced)
    # a column declared changed
    t.column_changed(1)
    assert np.array_equal(check("column_changed"), synced)
    t.close()


def test_chain_and_group_evicting_each_other(ctx, data):
    """A budget of one leaf, a chain and a column group in turn, on a column sorted by value: each is kept for a
    while, then makes room for the other, whose bitvector may get the same address. Both plans end as one kept
    leaf, so both take their zone classes and their tile offsets from maps keyed by that address: a map that
    outlived its bitvector would rule out the zones the other lives in, or misplace its tiles' runs."""
    _, b, c, d, e = data
    a = (np.arange(N, dtype=np.int64) * 40 // N).astype(np.int32)
    t = make_table(ctx, data, a=a)
    t.set_derived_budget(LEAF_BYTES)
    chain = (F.TableFilterSet({0: interval(5, 10), 1: F.ConstantFilter("<", 24)}), np.flatnonzero((a >= 5) & (a < 10) & (b < 24)))
    group = (F.TableFilterSet({0: interval(25, 30)}), np.flatnonzero((a >= 25) & (a < 30)))
    assert len(chain[1]) and chain[1].max() < 131072 <= group[1].min() and group[1].max() < 2 * 131072
    kept = {"chain": 0, "group": 0}
    holder, changes = None, 0
    for visit in range(10):
        for name, (fs, ref) in (("chain", chain), ("group", group)):
            for zonemap in (True, False):
                got = t.scan(fs, zonemap=zonemap)
                k, _ = t.last_plan()
                assert np.array_equal(got, ref), (visit, name, zonemap, k)
                if zonemap:
                    assert t.last_zones() == (1, 3), (visit, name)
                leaves, held, _ = t.derived_stats()
                assert leaves <= 1 and held <= LEAF_BYTES
                if k == 1:
                    kept[name] += 1
                    changes += holder != name
                    holder = name
                    assert t.derived_chain_stats()[0] == (name == "chain")
            # the tile directory of the run-order scan, through whatever leaf the plan reads now
            raw = t.scan(fs, ordered=False)
            directory, _ = ctx.last_tiles()
            assert int(directory[:, 1].sum()) == len(ref), (visit, name)
            assert np.array_equal(runs_in_row_order(raw, directory), ref), (visit, name)
            if t.last_plan() == (1, 1):
                assert ctx.last_decode_kernel() == L.DECODE_PREFIXED
    assert kept["chain"] >= 2 and kept["group"] >= 2 and changes >= 3, (kept, changes)
    t.close()


def test_default_cost_admits_no_chain(ctx, data):
    a, b, c, d, e = data
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24), 2: in_list(3, 5, 9)})
    ref = oracle_ids(ocols(data), fs)
    t = make_table(ctx, data, cost=None)
    # the column groups as before chains existed: the union kept by its third request, the interval by its
    # fourth, and 60 requests are far from paying a chain's fixed cost on bitvectors of 131,072 bytes
    assert scan_plans(t, fs, ref, 60) == [(6, 1), (6, 1), (4, 2), (3, 2)] + [(3, 1)] * 56
    assert t.derived_stats() == (2, 2 * LEAF_BYTES, 57 + 56)
    assert t.derived_chain_stats() == (0, 0)
    # "never" refuses at any count, and 0 then admits at once
    t.set_derived_chain_cost(NEVER)
    assert scan_plans(t, fs, ref, 3) == [(3, 1)] * 3
    t.set_derived_chain_cost(0)
    assert scan_plans(t, fs, ref, 2) == [(1, 2), (1, 1)]
    assert t.derived_chain_stats() == (1, 1)
    t.close()
