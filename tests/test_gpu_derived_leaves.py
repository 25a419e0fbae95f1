"""Derived leaves: a combination of one column's index / validity bitvectors that scans keep planning
(a RANGE interval's L(hi) AND NOT L(lo), with or without the validity leaf; the union behind an IN-list
on an EQUALITY index) is materialised once and read as one leaf from then on. That changes how many
bitvectors a scan reads and never what it returns: every scan here is compared with the oracle or
numpy — before admission, on the scan that materialises, after it, after every kind of index
maintenance, under MVCC views that may and may not use the kept leaf, and while a budget of one leaf
makes two intervals evict each other (their bitvectors then share an address, which the zone maps are
keyed by). Tables hold 300,001 rows: three 131,072-row tiles, the last partial and not a multiple of 64."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, padded_words, runs_in_row_order
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 300_001
LEAF_BYTES = None  # one table-owned bitvector of a fresh N-row table (set by the ctx fixture)
TXN = 4611686018427388000
NOT_DELETED = np.uint64(2 ** 64 - 2)


@pytest.fixture(scope="module")
def ctx():
    global LEAF_BYTES
    c = Context(0)
    LEAF_BYTES = padded_words(N) * 8
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """The columns every test builds its table from (never modified: tests copy what they change)."""
    rng = np.random.default_rng(41)
    a = rng.integers(0, 40, N).astype(np.int32)   # the interval's column (RANGE index, every value a key)
    b = rng.integers(0, 50, N).astype(np.int64)   # a second column's leaf (RANGE index)
    c = rng.integers(0, 12, N).astype(np.int64)   # the IN-list's column (EQUALITY index)
    d = rng.integers(-1000, 1000, N).astype(np.int64)  # summed, no index
    valid_a = rng.random(N) >= 0.1
    for x in (a, b, c, d, valid_a):
        x.setflags(write=False)
    return a, b, c, d, valid_a


def make_table(ctx, data, nullable=False, a=None):
    a0, b, c, d, valid_a = data
    a = a0 if a is None else a
    t = CubitTable(ctx, N)
    t.add_column(0, a, validity_from_mask(valid_a) if nullable else None)
    t.add_column(1, b)
    t.add_column(2, c)
    t.add_column(3, d)
    t.build_index(0, L.INDEX_RANGE)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_EQUALITY)
    return t


def interval(lo, hi):
    return F.ConjunctionAndFilter([F.ConstantFilter(">=", lo), F.ConstantFilter("<", hi)])


def oracle_ids(cols, fs, n=N, tx=None):
    return O.table_scan(cols, F.serialize(fs), n, tx=tx)


def scan_plans(t, fs, ref, times, txn=None, what=""):
    """`times` ordered scans of fs, each equal to ref; their (K, passes)."""
    plans = []
    for i in range(times):
        got = t.scan(fs, txn=txn)
        plans.append(t.last_plan())
        assert np.array_equal(got, ref), (what, i, plans)
    return plans


def test_interval_with_a_second_column(ctx, data):
    a, b, c, d, _ = data
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})
    ref = oracle_ids([O.Column(a), O.Column(b)], fs)
    assert np.array_equal(ref, np.flatnonzero((a >= 10) & (a < 20) & (b < 24)))
    t = make_table(ctx, data)
    assert t.derived_stats() == (0, 0, 0)
    # scans 1-3 read L(20), L(10) and the second column's leaf; the fourth materialises the interval
    # (one extra bits-only pass) and it and the later ones read two
    assert scan_plans(t, fs, ref, 3) == [(3, 1)] * 3
    assert t.derived_stats() == (0, 0, 0)
    assert scan_plans(t, fs, ref, 3) == [(2, 2), (2, 1), (2, 1)]
    assert t.derived_stats() == (1, LEAF_BYTES, 2)
    # the literals in the other order are the same combination
    fs_r = F.TableFilterSet({1: F.ConstantFilter("<", 24),
                             0: F.ConjunctionAndFilter([F.ConstantFilter("<", 20), F.ConstantFilter(">=", 10)])})
    assert scan_plans(t, fs_r, ref, 1) == [(2, 1)]
    assert t.derived_stats() == (1, LEAF_BYTES, 3)
    # a budget of 0 frees it and keeps the old plan for good
    t.set_derived_budget(0)
    assert t.derived_stats()[:2] == (0, 0)
    assert scan_plans(t, fs, ref, 6) == [(3, 1)] * 6
    assert t.derived_stats()[:2] == (0, 0)
    # ... and a budget brings it back by the admission rule
    t.set_derived_budget(LEAF_BYTES)
    assert scan_plans(t, fs, ref, 4) == [(3, 1)] * 3 + [(2, 2)]
    assert t.derived_stats()[:2] == (1, LEAF_BYTES)
    t.close()


def test_nullable_interval_and_in_list(ctx, data):
    a, b, c, d, valid_a = data
    vw = validity_from_mask(valid_a)
    t = make_table(ctx, data, nullable=True)
    # NN AND NOT L(10) AND L(20): a group of three, kept from its third request
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})
    ref = oracle_ids([O.Column(a, vw), O.Column(b)], fs)
    assert np.array_equal(ref, np.flatnonzero(valid_a & (a >= 10) & (a < 20) & (b < 24)))
    assert scan_plans(t, fs, ref, 5) == [(4, 1), (4, 1), (2, 2), (2, 1), (2, 1)]
    assert t.derived_stats() == (1, LEAF_BYTES, 2)
    # x IN (3, 5, 9) on the EQUALITY index: a union of three
    in_list = F.ConjunctionOrFilter([F.ConstantFilter("=", v) for v in (3, 5, 9)])
    fs_in = F.TableFilterSet({2: in_list, 1: F.ConstantFilter("<", 24)})
    ref_in = oracle_ids([O.Column(a, vw), O.Column(b), O.Column(c)], fs_in)
    assert np.array_equal(ref_in, np.flatnonzero(np.isin(c, (3, 5, 9)) & (b < 24)))
    assert scan_plans(t, fs_in, ref_in, 5) == [(4, 1), (4, 1), (2, 2), (2, 1), (2, 1)]
    assert t.derived_stats() == (2, 2 * LEAF_BYTES, 4)
    # both kept leaves in one plan
    fs_all = F.TableFilterSet({0: interval(10, 20), 2: in_list})
    ref_all = oracle_ids([O.Column(a, vw), O.Column(b), O.Column(c)], fs_all)
    assert scan_plans(t, fs_all, ref_all, 2) == [(2, 1)] * 2
    assert t.count(fs_all) == len(ref_all)
    t.close()


def test_interval_alone_takes_the_prefixed_decode(ctx, data):
    a, b, c, d, _ = data
    fs = F.TableFilterSet({0: interval(10, 20)})
    mask = (a >= 10) & (a < 20)
    ref = oracle_ids([O.Column(a)], fs)
    assert np.array_equal(ref, np.flatnonzero(mask))
    want_sum = int((d[mask].astype(object) * b[mask].astype(object)).sum())
    t = make_table(ctx, data)
    # count and sum_product plan the same combination: their requests count, and they share the entry
    plans = []
    for k in range(4):
        if k % 2 == 0:
            assert t.count(fs) == len(ref)
        else:
            assert t.sum_product(3, 1, fs) == (want_sum, len(ref))
        plans.append(t.last_plan())
    assert plans == [(2, 1)] * 3 + [(1, 2)]
    assert t.derived_stats() == (1, LEAF_BYTES, 0)
    # the plan is now one table-owned bitvector: the decode takes its offsets from the zone counts
    raw = t.scan(fs, ordered=False)
    assert t.last_plan() == (1, 1) and ctx.last_decode_kernel() == L.DECODE_PREFIXED
    directory, _ = ctx.last_tiles()
    assert int(directory[:, 1].sum()) == len(ref)
    assert np.array_equal(runs_in_row_order(raw, directory), ref)
    assert np.array_equal(t.scan(fs, ordered=True), ref)
    assert ctx.last_decode_kernel() == L.DECODE_PREFIXED
    assert np.array_equal(t.scan(fs, zonemap=False), ref)
    assert t.count(fs) == len(ref) and t.last_plan() == (1, 1)
    assert t.sum_product(3, 1, fs) == (want_sum, len(ref)) and t.last_plan() == (1, 1)
    assert t.derived_stats() == (1, LEAF_BYTES, 5)
    t.close()


def test_maintenance_drops_the_entry(ctx, data):
    a, b, c, d, _ = data
    fs = F.TableFilterSet({0: interval(10, 20)})
    admitted = [(2, 1)] * 3 + [(1, 2)]
    t = make_table(ctx, data)
    cols = [a.copy(), b.copy(), c.copy(), d.copy()]

    def ref():
        got = oracle_ids([O.Column(cols[0])], fs, n=len(cols[0]))
        assert np.array_equal(got, np.flatnonzero((cols[0] >= 10) & (cols[0] < 20)))
        return got

    assert scan_plans(t, fs, ref(), 4, what="fresh") == admitted
    rng = np.random.default_rng(5)
    # an append in place (bitvectors are allocated in steps of 1,048,576 rows), then one that grows them
    for n_new, what in ((50_000, "append in place"), (750_000, "append that grows")):
        words_before = padded_words(t.n_rows)
        add = [rng.integers(0, 40, n_new).astype(np.int32), rng.integers(0, 50, n_new).astype(np.int64),
               rng.integers(0, 12, n_new).astype(np.int64), rng.integers(-9, 9, n_new).astype(np.int64)]
        t.append({i: x for i, x in enumerate(add)})
        assert (padded_words(t.n_rows) > words_before) == (what == "append that grows")
        cols = [np.concatenate([x, y]) for x, y in zip(cols, add)]
        assert t.derived_stats()[:2] == (0, 0), what
        r = ref()
        assert len(r) > int(((a >= 10) & (a < 20)).sum())  # the new rows qualify too
        assert scan_plans(t, fs, r, 4, what=what) == admitted
        assert t.derived_stats()[0] == 1
    # update records merged into the column and its index
    n = t.n_rows
    rows = np.sort(rng.choice(n, size=3_000, replace=False)).astype(np.int64)
    vals = rng.integers(0, 40, len(rows)).astype(np.int64)
    t.set_updates(0, rows, vals, np.full(len(rows), 3, dtype=np.uint64))
    # (pending records leave the base bits alone: a scan without a transaction still reads the kept leaf)
    assert scan_plans(t, fs, ref(), 2, what="records pending, no transaction") == [(1, 1)] * 2
    assert t.derived_stats()[0] == 1
    assert t.merge_updates(0, 5) == len(rows)
    assert t.derived_stats()[:2] == (0, 0)
    before = ref()
    cols[0][rows] = vals.astype(np.int32)
    r = ref()
    assert not np.array_equal(r, before)
    assert scan_plans(t, fs, r, 4, what="merged") == admitted
    # the index rebuilt on other keys (10 and 20 still among them)
    t.build_index(0, L.INDEX_RANGE, list(range(0, 40, 2)))
    assert t.derived_stats()[:2] == (0, 0)
    assert scan_plans(t, fs, r, 4, what="rebuilt") == admitted
    assert t.derived_stats()[0] == 1
    t.close()


def test_mvcc_views(ctx, data):
    a, b, c, d, _ = data
    rng = np.random.default_rng(9)
    t = make_table(ctx, data)
    # column 0 updated at version 7, column 1 at version 3, deletes committed at 4
    rows0 = np.sort(rng.choice(N, size=4_000, replace=False)).astype(np.int64)
    vals0 = rng.integers(0, 40, len(rows0)).astype(np.int64)
    vers0 = np.full(len(rows0), 7, dtype=np.uint64)
    rows1 = np.sort(rng.choice(N, size=4_000, replace=False)).astype(np.int64)
    vals1 = rng.integers(0, 50, len(rows1)).astype(np.int64)
    vers1 = np.full(len(rows1), 3, dtype=np.uint64)
    t.set_updates(0, rows0, vals0, vers0)
    t.set_updates(1, rows1, vals1, vers1)
    del_rows = np.sort(rng.choice(N, size=20_000, replace=False)).astype(np.int64)
    t.set_deletes(del_rows, np.full(len(del_rows), 4, dtype=np.uint64))
    deleted = np.full(N, NOT_DELETED, dtype=np.uint64)
    deleted[del_rows] = 4
    ocols = [O.Column(a, updates=(rows0, vals0, vers0)), O.Column(b, updates=(rows1, vals1, vers1))]
    fs = F.TableFilterSet({0: interval(10, 20), 1: F.ConstantFilter("<", 24)})

    def view(start, tid):
        return L.Txn(start, tid), oracle_ids(ocols, fs, tx=O.Mvcc(start, tid, deleted=deleted))

    # a snapshot before everything: base values, no delete in effect; the interval is kept from its
    # fourth request
    old, ref_old = view(2, TXN + 1)
    assert np.array_equal(ref_old, np.flatnonzero((a >= 10) & (a < 20) & (b < 24)))
    assert scan_plans(t, fs, ref_old, 5, txn=old, what="old") == [(3, 1)] * 3 + [(2, 2), (2, 1)]
    # sees column 1's updates and the deletes, not column 0's: the kept interval, column 1's leaf patched,
    # the visibility leaf
    mid, ref_mid = view(5, TXN + 2)
    assert len(ref_mid) < len(ref_old)
    assert scan_plans(t, fs, ref_mid, 2, txn=mid, what="mid") == [(3, 1)] * 2
    # sees column 0's updates too: its own two leaves, patched
    new, ref_new = view(10, TXN + 3)
    assert not np.array_equal(ref_new, ref_mid)
    assert scan_plans(t, fs, ref_new, 2, txn=new, what="new") == [(4, 1)] * 2
    # the entry is still there for those who may use it
    assert scan_plans(t, fs, ref_old, 1, txn=old, what="old again") == [(2, 1)]
    assert scan_plans(t, fs, ref_mid, 1, txn=mid, what="mid again") == [(3, 1)]
    assert t.derived_stats()[0] == 1
    t.close()


def test_two_intervals_evicting_each_other(ctx, data):
    """A budget of one leaf and two intervals in turn on a column sorted by value: each is kept for a
    while, then makes room for the other, whose bitvector may get the same address. The zone maps are
    keyed by address and informative here (every interval lies in one zone), so a map that outlived its
    bitvector would rule out the zones the other interval lives in."""
    _, b, c, d, _ = data
    a = (np.arange(N, dtype=np.int64) * 40 // N).astype(np.int32)
    t = make_table(ctx, data, a=a)
    t.set_derived_budget(LEAF_BYTES)
    A = (F.TableFilterSet({0: interval(5, 10)}), np.flatnonzero((a >= 5) & (a < 10)))
    B = (F.TableFilterSet({0: interval(25, 30)}), np.flatnonzero((a >= 25) & (a < 30)))
    assert len(A[1]) and len(B[1]) and A[1].max() < 131072 <= B[1].min() and B[1].max() < 2 * 131072
    kept = {"A": 0, "B": 0}
    holder, changes = None, 0
    for visit in range(10):
        for name, (fs, ref) in (("A", A), ("B", B)):
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
    assert kept["A"] >= 2 and kept["B"] >= 2 and changes >= 3, (kept, changes)
    t.close()
