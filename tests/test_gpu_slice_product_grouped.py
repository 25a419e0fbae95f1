"""cubit_table_sum_product_grouped (CubitTable.sum_product_by) against Python integers: per group of one
or two EQUALITY-indexed columns, sum(a * b), the rows where neither operand is NULL and count(*) over a
filter's rows, on all three paths — path=None (the library chooses), "slices" (the fused kernel over
both operands' bit slices, four groups per launch) and "column" (scan + probe + reduce per group). The
reference is a.astype(object) * b.astype(object) (NULL → 0) over the values the oracle fetches at the
oracle's row ids (O.table_scan, O.fetch), grouped in numpy by the group columns' visible values — never
the library's other path."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_gpu_group_aggregate import visible

pytestmark = pytest.mark.gpu

TXN_START = 4611686018427388000
PATHS = [None, "slices", "column"]
A, B, KEY, G3, G2, G9, G17, GN = range(8)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def expected(ocols, by, plan, n, tx=None, col_a=A, col_b=B):
    """{key tuple: (sum, count_valid, count_rows)} over the oracle's rows."""
    ids = O.table_scan(ocols, plan, n, 0, tx)
    if len(ids) == 0:
        return {}
    av, aok = visible(ocols, col_a, ids, tx, None)
    bv, bok = visible(ocols, col_b, ids, tx, None)
    ok = aok & bok
    prod = av.astype(object) * bv.astype(object)
    prod[~ok] = 0
    labels = []
    for g in by:
        gv, gok = visible(ocols, g, ids, tx, None)
        labels += [np.where(gok, gv, 0), (~gok).astype(np.int64)]
    uniq, inv = np.unique(np.stack(labels, axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = {}
    for u, row in enumerate(uniq):
        m = inv == u
        key = tuple(None if row[2 * j + 1] else int(row[2 * j]) for j in range(len(by)))
        out[key] = (int(prod[m].sum()), int(ok[m].sum()), int(m.sum()))
    return out


def check_groups(t, ocols, by, n, fs=None, txn=None, tx=None, paths=PATHS, what=None):
    """Every path equals the expected dict and last_sum_product names the path that ran; returns the
    expected dict and what path=None reported."""
    want = expected(ocols, by, F.serialize(fs), n, tx)
    auto = None
    for path in paths:
        got = t.sum_product_by(A, B, by, fs, txn=txn, path=path)
        assert got == want, (what, by, path, got, want)
        used, launches = t.last_sum_product()
        assert (launches > 0) == used
        if path is None:
            auto = (used, launches)
        elif want:
            assert used == (path == "slices"), (what, by, path)
    return want, auto


def build(ctx, n, seed):
    """a: 24 slices with NULLs; b: 0 … 10, 4 slices; key: 0 … 99 with an exact RANGE index; group columns
    of 3 and 2 values (the combination (2, 1) empty, TPC-H Q1's shape), 9 and 17 values, and a nullable one
    of 3 values — each with an every-value EQUALITY index."""
    rng = np.random.default_rng(seed)
    a = rng.integers(90_000, 90_000 + (1 << 24), n).astype(np.int64)
    b = rng.integers(0, 11, n).astype(np.int64)
    a[:2], b[:2] = [90_000, 90_000 + (1 << 24) - 1][:n], [0, 10][:n]
    av = rng.random(n) >= 0.05
    av[:2] = True
    key = rng.integers(0, 100, n).astype(np.int32)
    g3 = rng.integers(0, 3, n).astype(np.int32)
    g2 = rng.integers(0, 2, n).astype(np.int32)
    g2[g3 == 2] = 0
    g9 = rng.integers(-4, 5, n).astype(np.int64)
    g17 = (rng.integers(0, 17, n) * 1000).astype(np.int32)
    gn = rng.integers(5, 8, n).astype(np.int32)
    gnv = rng.random(n) >= 0.1
    datas = [a, b, key, g3, g2, g9, g17, gn]
    vws = [validity_from_mask(av), None, None, None, None, None, None, validity_from_mask(gnv)]
    t = CubitTable(ctx, n)
    for c, (d, vw) in enumerate(zip(datas, vws)):
        t.add_column(c, d, vw)
    t.build_index(A, L.INDEX_SLICED)
    t.build_index(B, L.INDEX_SLICED)
    t.build_index(KEY, L.INDEX_RANGE)
    for c in (G3, G2, G9, G17, GN):
        t.build_index(c, L.INDEX_EQUALITY)
    return t, [O.Column(d, vw) for d, vw in zip(datas, vws)], datas


@pytest.fixture(scope="module")
def main(ctx):
    n = 262_147  # two whole tiles and a tail of three rows
    t, ocols, datas = build(ctx, n, 61)
    yield t, ocols, datas, n
    t.close()


@pytest.mark.parametrize("n", [1, 65, 131_073])
def test_row_counts_one_and_two_group_columns(ctx, n):
    t, ocols, _ = build(ctx, n, 60 + n)
    for by in ([G3], [GN], [G3, G2], [GN, G3], [G2, GN]):
        for fs in (None, F.TableFilterSet({KEY: F.ConstantFilter("<", 50)})):
            check_groups(t, ocols, by, n, fs, what=n)
    t.close()


@pytest.mark.parametrize("by", [[G3], [GN], [G3, G2], [GN, G3], [G2, GN]], ids=str)
def test_groups_with_a_null_slot(main, by):
    """262,147 rows: one and two group columns, the nullable one on either side (its NULL slot is the
    complemented validity), under no filter, a half-open one and one that keeps 2 %."""
    t, ocols, datas, n = main
    for fs in (None, F.TableFilterSet({KEY: F.ConstantFilter("<", 50)}), F.TableFilterSet({KEY: F.ConstantFilter("<", 2)})):
        want, auto = check_groups(t, ocols, by, n, fs, what=fs)
        if GN in by:
            assert any(None in k for k in want)
    # every row of 24 × 4 slices: the rule takes the slices
    assert check_groups(t, ocols, by, n, None, paths=[None])[1][0] is True


def test_second_and_third_launch_and_an_empty_group(main, ctx):
    """9 groups run as three launches of the fused kernel and 17 as five; 3 × 2 groups as two. The group
    (2, 1) has no row: it is left out, and the call itself writes four zeros for it."""
    t, ocols, datas, n = main
    for by, launches, occupied in (([G9], 3, 9), ([G17], 5, 17), ([G3, G2], 2, 5), ([G9, G2], 5, 18)):
        want, _ = check_groups(t, ocols, by, n, F.TableFilterSet({KEY: F.ConstantFilter(">=", 10)}), what=by)
        assert len(want) == occupied
        t.sum_product_by(A, B, by, path="slices")
        assert t.last_sum_product() == (True, launches), by
    groups = t.aggregate_groups([G3, G2])
    assert (2, 1) in groups and len(groups) == 6
    arr = (C.c_int * 2)(G3, G2)
    out = ctx.alloc(6 * 32)
    for flags in (L.SUM_FROM_SLICES, L.SUM_FROM_COLUMN):
        L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, 6 * 32))
        L.check(t.lib.cubit_table_sum_product_grouped(t.handle, None, 0, None, A, B, arr, 2, flags, C.c_void_p(out.addr), 6))
        ctx.check()
        res = out.download(np.int64, 24).reshape(6, 4)
        assert list(res[groups.index((2, 1))]) == [0, 0, 0, 0] and all(r[3] > 0 for g, r in zip(groups, res) if g != (2, 1))
    # a filter that folds to FALSE: zeros everywhere
    fs = F.TableFilterSet({KEY: F.ConstantFilter(">", 1000)})
    assert t.sum_product_by(A, B, [G3, G2], fs) == {}
    out.free()


def test_refusals(main, ctx):
    t, ocols, datas, n = main
    arr = (C.c_int * 2)(G3, G2)
    out = ctx.alloc(6 * 32)
    call = t.lib.cubit_table_sum_product_grouped
    assert call(t.handle, None, 0, None, A, B, arr, 2, 0, C.c_void_p(out.addr), 5) == L.ERR_CAPACITY  # one short
    assert call(t.handle, None, 0, None, A, B, arr, 2, 0, C.c_void_p(out.addr), 6) == L.OK
    assert call(t.handle, None, 0, None, A, B, arr, 2, L.SUM_FROM_SLICES | L.SUM_FROM_COLUMN, C.c_void_p(out.addr), 6) == L.ERR_INVALID
    assert call(t.handle, None, 0, None, A, B, arr, 2, L.SUM_GATHER_B, C.c_void_p(out.addr), 6) == L.ERR_INVALID
    assert call(t.handle, None, 0, None, A, 99, arr, 2, 0, C.c_void_p(out.addr), 6) == L.ERR_INVALID
    assert call(t.handle, None, 0, None, A, G3, arr, 2, 0, C.c_void_p(out.addr), 6) == L.ERR_UNSUPPORTED  # an INT32 operand
    ctx.check()
    out.free()
    with pytest.raises(L.CubitError) as e:  # KEY has a RANGE index, no every-value EQUALITY index
        t.sum_product_by(A, B, [KEY])
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.CubitError) as e:  # a group column without any index
        t.sum_product_by(A, B, [A])
    assert e.value.code == L.ERR_UNSUPPORTED
    t.use_sliced(False)
    try:
        with pytest.raises(L.CubitError) as e:
            t.sum_product_by(A, B, [G3], path="slices")
        assert e.value.code == L.ERR_INVALID
        assert check_groups(t, ocols, [G3], n, paths=[None, "column"])[1] == (False, 0)
    finally:
        t.use_sliced(True)


def test_a_slot_that_exists_only_through_an_update(ctx):
    """An update record moves three rows of a group column to a value its index has never seen: the slot
    is in the numbering, has rows on the column path only, and closes the fused kernel while the record
    is visible — as does a visible update of an operand."""
    n = 150_001
    t, ocols, datas = build(ctx, n, 62)
    base_ocols = list(ocols)  # the columns without their update records: what a scan with no transaction sees
    rows = np.array([5, 131_072, n - 1], np.int64)
    versions = np.array([3, 3, 3], np.uint64)
    t.set_updates(G3, rows, np.array([7, 7, 7], np.int64), versions)
    ocols[G3] = O.Column(datas[G3], None, (rows, np.array([7, 7, 7], np.int64), versions))
    assert (7,) in t.aggregate_groups([G3])
    txn, tx = L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1)
    with pytest.raises(L.CubitError) as e:
        t.sum_product_by(A, B, [G3], txn=txn, path="slices")
    assert e.value.code == L.ERR_INVALID
    want, auto = check_groups(t, ocols, [G3], n, txn=txn, tx=tx, paths=[None, "column"])
    assert want[(7,)][2] == 3 and auto == (False, 0)
    # not visible without the transaction: the slices answer, and the slot has no row
    want, _ = check_groups(t, base_ocols, [G3], n)
    assert (7,) not in want
    # a visible update of b closes the slices too; the sum is over the updated values
    t.set_updates(B, rows, np.array([1000, -3, 2 ** 40], np.int64), versions)
    ocols[B] = O.Column(datas[B], None, (rows, np.array([1000, -3, 2 ** 40], np.int64), versions))
    with pytest.raises(L.CubitError) as e:
        t.sum_product_by(A, B, [G2], txn=txn, path="slices")
    assert e.value.code == L.ERR_INVALID
    check_groups(t, ocols, [G2], n, txn=txn, tx=tx, paths=[None, "column"])
    t.close()


def test_q1_shape(ctx):
    """TPC-H Q1's sum(l_extendedprice * (1 - l_discount)) per l_returnflag, l_linestatus in hundredths:
    300,007 rows, 24-bit prices, discounts 0 … 10, 3 × 2 groups, a date bound that keeps about 98 %.
    Per group 100 · Σ price - Σ price · disc from aggregate_by + sum_product_by equals the Python integers,
    on every path; the automatic rule reads the slices, in two launches."""
    rng = np.random.default_rng(63)
    n = 300_007
    price = rng.integers(90_000, 90_000 + (1 << 24), n).astype(np.int64)
    price[:2] = [90_000, 90_000 + (1 << 24) - 1]
    disc = rng.integers(0, 11, n).astype(np.int64)
    disc[:2] = [0, 10]
    flag = rng.integers(0, 3, n).astype(np.int32)
    status = rng.integers(0, 2, n).astype(np.int32)
    date = rng.integers(0, 2500, n).astype(np.int32)
    t = CubitTable(ctx, n)
    for c, d in enumerate((price, disc, date, flag, status)):
        t.add_column(c, d)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    t.build_index(2, L.INDEX_RANGE, list(range(50, 2500, 50)))
    t.build_index(3, L.INDEX_EQUALITY)
    t.build_index(4, L.INDEX_EQUALITY)
    fs = F.TableFilterSet({2: F.ConstantFilter("<", 2450)})
    keep = date < 2450
    assert 0.97 < keep.mean() < 0.99
    want = {}
    for f in range(3):
        for s in range(2):
            m = keep & (flag == f) & (status == s)
            p, d = price[m].astype(object), disc[m].astype(object)
            want[(f, s)] = int((p * (100 - d)).sum())
    for path in PATHS:
        sums = t.aggregate_by(0, [3, 4], fs, ops=L.AGG_SUM, path=path)
        prods = t.sum_product_by(0, 1, [3, 4], fs, path=path)
        assert {k: 100 * sums[k].sum - prods[k][0] for k in sums} == want, path
        assert all(prods[k][1] == prods[k][2] == sums[k].count_rows for k in sums)
        if path is None:
            assert t.last_sum_product() == (True, 2)
    t.close()
