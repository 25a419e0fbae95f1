"""cubit_table_aggregate_grouped (CubitTable.aggregate_by) against Python integers: per group of one
or two EQUALITY-indexed columns, sum / min / max / count(col) / count(*) of a column over a filter's
rows, on all three paths — path=None (the library chooses), "slices" (the fused evaluate + aggregate
over the value column's bit slices, a batch of groups per launch) and "column" (scan + probe + reduce
per group). Expected values are reductions over the values the oracle fetches at the oracle's row ids
(O.table_scan, O.fetch), grouped in numpy by the group columns' visible values, so MVCC deletes,
inserts and updates are the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library initialises the GPU (the caller-stream case makes a torch stream)

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Aggregate, Context, CubitTable
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 3 * 131_072 + 37
U64 = (1 << 64) - 1
TXN_START = 4611686018427388000
PATHS = [None, "slices", "column"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def exact_sum(a):
    """The sum of an int64 / uint64 array as a Python int (32-bit halves summed in 64 bits)."""
    if len(a) == 0:
        return 0
    lo = int((a & a.dtype.type(0xFFFFFFFF)).astype(np.uint64).sum())
    hi = int((a >> a.dtype.type(32)).astype(np.int64 if a.dtype == np.int64 else np.uint64).sum())
    return (hi << 32) + lo


def double_keys(bits):
    mag = bits & np.int64(0x7FFFFFFFFFFFFFFF)
    key = np.where(bits < 0, -mag, mag)
    key[mag > np.int64(0x7FF0000000000000)] = 0x7FF8000000000000
    return key


def double_value(key):
    key = int(key)
    if key >= 0:
        return key
    return ((1 << 63) | (-key)) - (1 << 64)


def reduce_values(vals, typ, ops):
    """(sum, min, max, count) of the valid visible values (int64: values, DOUBLE bit patterns, UINT64
    bits, dictionary codes), in the form the library reports."""
    n = len(vals)
    if typ == L.TYPE_UINT64:
        u = vals.view(np.uint64)
        s, lo, hi = exact_sum(u), (int(u.min()) if n else None), (int(u.max()) if n else None)
        mn = None if lo is None else (lo - (1 << 64) if lo >> 63 else lo)
        mx = None if hi is None else (hi - (1 << 64) if hi >> 63 else hi)
    elif typ == L.TYPE_DOUBLE:
        k = double_keys(vals)
        s, mn, mx = 0, (double_value(k.min()) if n else None), (double_value(k.max()) if n else None)
    else:
        s, mn, mx = exact_sum(vals), (int(vals.min()) if n else None), (int(vals.max()) if n else None)
    return (s if ops & L.AGG_SUM else 0, mn if ops & L.AGG_MIN else None, mx if ops & L.AGG_MAX else None, n)


def visible(ocols, c, ids, tx, codes):
    if codes is not None and c in codes:  # a dictionary column: its codes and NULL-ness are known here
        v, ok = codes[c]
        return v[ids].astype(np.int64), ok[ids]
    v, ok = O.fetch(ocols[c], ids, 0, tx, with_valid=True)
    return np.ascontiguousarray(v), ok


def expected(ocols, col, typ, by, plan, n, tx, ops, codes=None, keyfn=None):
    """{key tuple: Aggregate} over the oracle's rows, grouped by the group columns' visible values."""
    ids = O.table_scan(ocols, plan, n, 0, tx)
    vals, vok = visible(ocols, col, ids, tx, codes)
    labels = []
    for g in by:
        gv, gok = visible(ocols, g, ids, tx, codes)
        labels += [np.where(gok, gv, 0), (~gok).astype(np.int64)]
    out = {}
    if len(ids) == 0:
        return out, 0
    uniq, inv = np.unique(np.stack(labels, axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for u, row in enumerate(uniq):
        m = inv == u
        key = tuple(None if row[2 * j + 1] else (keyfn[g](int(row[2 * j])) if keyfn and g in keyfn else int(row[2 * j]))
                    for j, g in enumerate(by))
        s, mn, mx, cv = reduce_values(np.ascontiguousarray(vals[m][vok[m]]), typ, ops)
        out[key] = Aggregate(s, mn, mx, cv, int(m.sum()))
    return out, len(ids)


def check_groups(t, ocols, col, typ, by, n, fs=None, residual=None, txn=None, tx=None, ops=None, zonemap=True,
                 paths=PATHS, codes=None, keyfn=None, what=None, after=None):
    """Every path equals the expected dict, last_grouped names the path that ran, and the groups add up
    to count() and aggregate() of the same filter. Returns (the expected dict, whether path=None read
    the slices). after(path) runs behind each aggregate_by, while the table's last_* counters are still
    that call's."""
    if ops is None:
        ops = L.AGG_ALL if typ not in (L.TYPE_DOUBLE, L.TYPE_VARCHAR) else L.AGG_MIN | L.AGG_MAX
    want, n_ids = expected(ocols, col, typ, by, F.serialize(fs, residual), n, tx, ops, codes, keyfn)
    chose = None
    for path in paths:
        got = t.aggregate_by(col, by, fs, residual, txn=txn, ops=ops, path=path, zonemap=zonemap)
        assert got == want, (what, col, by, path, ops, got, want)
        if after:
            after(path)
        used, n_groups, launches = t.last_grouped()
        assert n_groups == len(t.aggregate_groups(by)) >= len(want)
        assert (launches > 0) == used or not want
        if path is None:
            chose = used
        elif n_ids:  # (a filter that folds to FALSE runs neither path)
            assert used == (path == "slices"), (what, col, path)
        assert sum(a.count_rows for a in got.values()) == n_ids == t.count(fs, residual, txn=txn)
        whole = t.aggregate(col, fs, residual, txn=txn, ops=ops)
        assert sum(a.sum for a in got.values()) == whole.sum
        assert sum(a.count_valid for a in got.values()) == whole.count_valid
    return want, chose


def int_column(rng, n, dtype, lo, hi, null_frac=0.05):
    v = rng.integers(lo, hi, n, endpoint=True).astype(dtype)
    v[:2] = [lo, hi][:n]
    valid = rng.random(n) >= null_frac
    valid[:2] = True
    return v, valid


# ------------------------------------------------------------------ the main table

A, B, C_, D, E, G3, G2, G5, G7 = range(9)


def main_columns(n, seed=51):
    """Values: 12-bit INT32 with NULLs, 24-bit INT64, negative-to-positive INT64 with NULLs, UINT64 with
    0 and 2^64 - 1 (each with a bit-sliced index), a small INT64 with a RANGE index for the filters.
    Groups: 3 values x 2 values with the combination (2, 1) empty (TPC-H Q1's shape), and two nullable
    ones of 4 and 6 values (5 and 7 slots)."""
    rng = np.random.default_rng(seed)
    a, av = int_column(rng, n, np.int32, 1000, 1000 + 4095)
    b, _ = int_column(rng, n, np.int64, 90_000, 90_000 + (1 << 24) - 1, null_frac=0)
    c, cv = int_column(rng, n, np.int64, -5_000_000_000, 5_000_000_123)
    d = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    d[:4] = np.array([0, 1, U64 - 1, U64], dtype=np.uint64)[:n]
    dv = rng.random(n) >= 0.05
    dv[:4] = True
    e = rng.integers(0, 10, n, endpoint=True).astype(np.int64)
    g3 = rng.integers(0, 2, n, endpoint=True).astype(np.int32)
    g2 = rng.integers(0, 1, n, endpoint=True).astype(np.int32)
    g2[g3 == 2] = 0
    g5 = rng.integers(10, 13, n, endpoint=True).astype(np.int64)
    g5v = rng.random(n) >= 0.1
    g7 = (rng.integers(0, 5, n, endpoint=True) * 1000 - 2500).astype(np.int32)
    g7v = rng.random(n) >= 0.1
    av[g5 == 13] = False  # one group whose every value is NULL (grouping column 0 by column G5)
    datas = [a, b, c, d, e, g3, g2, g5, g7]
    vws = [validity_from_mask(av), None, validity_from_mask(cv), validity_from_mask(dv), None, None, None,
           validity_from_mask(g5v), validity_from_mask(g7v)]
    return datas, vws


TYPES = [L.TYPE_INT32, L.TYPE_INT64, L.TYPE_INT64, L.TYPE_UINT64, L.TYPE_INT64, L.TYPE_INT32, L.TYPE_INT32, L.TYPE_INT64,
         L.TYPE_INT32]


def make_main(ctx, n, seed=51):
    datas, vws = main_columns(n, seed)
    t = CubitTable(ctx, n)
    for i, (data, vw) in enumerate(zip(datas, vws)):
        t.add_column(i, data, vw)
        t.build_index(i, L.INDEX_SLICED if i < 4 else (L.INDEX_RANGE if i == 4 else L.INDEX_EQUALITY))
    return t, [O.Column(x, vw) for x, vw in zip(datas, vws)], datas, vws


@pytest.fixture(scope="module")
def main(ctx):
    t, ocols, datas, vws = make_main(ctx, N)
    yield t, ocols
    t.close()


FILTERS = {
    "none": (None, None),
    "q6": (F.TableFilterSet({A: F.ConjunctionAndFilter([F.ConstantFilter(">=", 2000), F.ConstantFilter("<", 3000)]),
                             E: F.ConjunctionAndFilter([F.ConstantFilter(">=", 5), F.ConstantFilter("<=", 7)]),
                             B: F.ConstantFilter("<", 90_000 + (1 << 23))}), None),
    "dnf": (None, F.Or(F.And(F.Cmp(A, "<", 1100), F.Cmp(E, ">", 2)), F.And(F.Cmp(C_, ">", 4_000_000_000), F.Cmp(E, "<", 5)),
                       F.IsNull(C_))),
    "cnf": (None, F.And(F.Or(F.Cmp(A, "<", 3000), F.Cmp(E, ">", 8)), F.Or(F.Cmp(C_, ">", 0), F.Cmp(E, "<", 2)))),
    "on the group column": (F.TableFilterSet({G3: F.ConstantFilter("!=", 1), E: F.ConstantFilter("<", 9)}), None),
    "false": (F.TableFilterSet({A: F.ConstantFilter("<", 990)}), None),
}


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("col", [A, B, C_, D])
def test_value_types_by_two_columns_every_filter(main, col, name):
    """12-bit INT32, 24-bit INT64, INT64 across zero and UINT64 with 0 and 2^64 - 1, grouped 3 x 2 with
    one combination empty, under no filter, a Q6-shaped conjunction, a DNF and a CNF residual, a
    predicate on the group column itself (its value 1 excluded: those groups are absent) and a filter
    that folds to FALSE (no group at all)."""
    t, ocols = main
    fs, residual = FILTERS[name]
    want, _ = check_groups(t, ocols, col, TYPES[col], [G3, G2], N, fs, residual, what=name)
    assert (2, 1) not in want
    if name == "none":
        assert sorted(want) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
        assert t.aggregate_groups([G3, G2]) == [(i, j) for i in range(3) for j in range(2)]
        t.aggregate_by(col, [G3, G2], ops=L.AGG_SUM, path="slices")
        assert t.last_grouped() == (True, 6, 1)  # Q1's shape is one launch
    if name == "on the group column":
        assert sorted(want) == [(0, 0), (0, 1), (2, 0)]
    if name == "false":
        assert want == {} and t.last_zones()[0] == 0


def test_nullable_group_columns_and_an_all_null_group(main):
    """5 x 7 slots of two nullable group columns: the NULL group of each and (NULL, NULL) are present;
    a nullable value column counts fewer valid rows than rows; the group G5 = 13 holds only NULLs of
    column A: count_valid 0, min / max None."""
    t, ocols = main
    want, _ = check_groups(t, ocols, C_, TYPES[C_], [G5, G7], N)
    assert len(want) == 35 and (None, None) in want and (None, -2500) in want and (13, None) in want
    assert all(a.count_valid < a.count_rows for a in want.values())
    want, _ = check_groups(t, ocols, A, TYPES[A], [G5], N, *FILTERS["q6"][:1])
    want, _ = check_groups(t, ocols, A, TYPES[A], [G5], N)
    assert sorted(want, key=str) == sorted([(10,), (11,), (12,), (13,), (None,)], key=str)
    assert want[(13,)].count_valid == 0 < want[(13,)].count_rows
    assert want[(13,)].min is None and want[(13,)].max is None and want[(13,)].sum == 0
    assert t.aggregate_groups([G5])[-1] == (None,)
    for ops in range(8):
        check_groups(t, ocols, C_, TYPES[C_], [G7, G3], N, *FILTERS["dnf"], ops=ops, what=ops)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 9, 17, 33])
def test_group_counts_on_both_sides_of_every_batch_boundary(ctx, k):
    """k slots of one column: a launch takes 8 groups for SUM and the counts, 4 with MIN / MAX."""
    rng = np.random.default_rng(600 + k)
    v, _ = int_column(rng, N, np.int64, 90_000, 90_000 + (1 << 24) - 1, null_frac=0)
    g = (rng.integers(0, k - 1, N, endpoint=True) * 3 - 7).astype(np.int64)
    g[:k] = np.arange(k) * 3 - 7
    e = rng.integers(0, 10, N, endpoint=True).astype(np.int64)
    t = CubitTable(ctx, N)
    for i, (data, enc) in enumerate([(v, L.INDEX_SLICED), (g, L.INDEX_EQUALITY), (e, L.INDEX_RANGE)]):
        t.add_column(i, data)
        t.build_index(i, enc)
    ocols = [O.Column(v), O.Column(g), O.Column(e)]
    fs = F.TableFilterSet({2: F.ConstantFilter("<", 9)})
    for ops, per_launch in [(L.AGG_SUM, 8), (L.AGG_ALL, 4)]:
        want, _ = check_groups(t, ocols, 0, L.TYPE_INT64, [1], N, fs, ops=ops, what=(k, ops))
        assert sorted(want) == [(j * 3 - 7,) for j in range(k)]
        t.aggregate_by(0, 1, fs, ops=ops, path="slices")
        assert t.last_grouped() == (True, k, -(-k // per_launch))
    t.close()


def test_double_and_varchar_values_and_a_varchar_group_column(ctx):
    rng = np.random.default_rng(52)
    pool_d = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 1e300, -1e300, 5e-324], dtype=np.float64)
    x = pool_d[rng.integers(0, len(pool_d), N)]
    xv = rng.random(N) >= 0.05
    pool = sorted({bytes(rng.integers(97, 123, rng.integers(1, 6)).astype(np.uint8)) for _ in range(40)})
    s = [None if rng.random() < 0.05 else pool[i] for i in rng.integers(0, len(pool), N)]
    flags = [b"A", b"N", b"R", b"north-east"]
    gs = [None if rng.random() < 0.03 else flags[i] for i in rng.integers(0, len(flags), N)]
    t = CubitTable(ctx, N)
    t.add_column(0, x, validity_from_mask(xv))
    d1 = t.add_string_column(1, s)
    d2 = t.add_string_column(2, gs)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    t.build_index(2, L.INDEX_EQUALITY)
    ocols = [O.Column(x, validity_from_mask(xv)), O.StringColumn(s), O.StringColumn(gs)]
    codes = {1: d1.encode(s), 2: d2.encode(gs)}
    keyfn = {2: d2.entry}
    for fs in [None, F.TableFilterSet({0: F.ConstantFilter("<", np.float64(np.inf))}),
               F.TableFilterSet({1: F.ConstantFilter(">", pool[17])}), F.TableFilterSet({2: F.ConstantFilter(">", b"A")})]:
        for col, typ in ((0, L.TYPE_DOUBLE), (1, L.TYPE_VARCHAR)):
            want, _ = check_groups(t, ocols, col, typ, [2], N, fs, codes=codes, keyfn=keyfn, what=(fs, col))
    assert sorted(want) == [(b"N",), (b"R",), (b"north-east",)]  # > "A": neither "A" nor the NULL group
    assert t.aggregate_groups([2]) == [(f,) for f in sorted(flags)] + [(None,)]
    for col in (0, 1):
        for path in PATHS:  # the keys are not linear in the value
            with pytest.raises(L.CubitError) as e:
                t.aggregate_by(col, [2], ops=L.AGG_SUM, path=path)
            assert e.value.code == L.ERR_UNSUPPORTED
    t.close()


def test_clustered_column_skips_zones(ctx):
    rng = np.random.default_rng(53)
    a = np.sort(rng.integers(0, 4000, N).astype(np.int32))  # clustered: zones hold ranges
    b, bv = int_column(rng, N, np.int64, -70_000, 70_000)
    g = rng.integers(0, 4, N, endpoint=True).astype(np.int32)
    bw = validity_from_mask(bv)
    t = CubitTable(ctx, N)
    for i, (data, vw, enc) in enumerate([(a, None, L.INDEX_SLICED), (b, bw, L.INDEX_SLICED), (g, None, L.INDEX_EQUALITY)]):
        t.add_column(i, data, vw)
        t.build_index(i, enc)
    ocols = [O.Column(a), O.Column(b, bw), O.Column(g)]
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 100), F.ConstantFilter("<", 300)])})
    check_groups(t, ocols, 1, L.TYPE_INT64, [2], N, fs)
    check_groups(t, ocols, 1, L.TYPE_INT64, [2], N, fs, zonemap=False)
    for path in ("slices", "column"):
        skipped = t.aggregate_by(1, [2], fs, path=path)
        ev, nz = t.last_zones()
        assert 0 < ev < nz == 4, (path, ev, nz)
        assert t.aggregate_by(1, [2], fs, path=path, zonemap=False) == skipped
        assert t.last_zones() == (nz, nz)
    # the three queries answered from the slices plan alike: the same leaves, passes and zones
    plans = []
    for call in (lambda: t.aggregate(1, fs, path="slices"), lambda: t.quantile(1, 0.5, fs, path="slices"),
                 lambda: t.aggregate_by(1, [2], fs, path="slices")):
        call()
        plans.append((t.last_plan(), t.last_zones()))
    assert plans[0] == plans[1] == plans[2] and plans[0][1][0] < plans[0][1][1], plans
    t.close()


# ------------------------------------------------------------------ MVCC


def test_deletes_inserts_and_updates(ctx):
    rng = np.random.default_rng(54)
    b, bv = int_column(rng, N, np.int64, -70_000, 70_000)
    g = rng.integers(0, 4, N, endpoint=True).astype(np.int64)  # keys 0 ... 4, not nullable
    h = rng.integers(0, 2, N, endpoint=True).astype(np.int32)
    bw = validity_from_mask(bv)
    # committed deletes (id 5) and a writer's own uncommitted ones; the last 10,000 rows were
    # inserted by transaction 8
    writer = TXN_START + 9
    dels = np.arange(0, N, 7, dtype=np.int64)
    del_ids = np.where(np.arange(len(dels)) % 3 == 0, writer, 5).astype(np.uint64)
    deleted = np.full(N, np.uint64(2 ** 64 - 2), dtype=np.uint64)
    deleted[dels] = del_ids
    inserted = np.zeros(N, dtype=np.uint64)
    inserted[N - 10_000:] = 8

    def build():
        t = CubitTable(ctx, N)
        for i, (data, vw, enc) in enumerate([(b, bw, L.INDEX_SLICED), (g, None, L.INDEX_EQUALITY), (h, None, L.INDEX_EQUALITY)]):
            t.add_column(i, data, vw)
            t.build_index(i, enc)
        t.set_deletes(dels, del_ids)
        t.set_inserts(np.array([N - 10_000]), np.array([N]), np.array([8], dtype=np.uint64))
        return t

    t = build()
    ocols = [O.Column(b, bw), O.Column(g), O.Column(h)]
    fs = F.TableFilterSet({0: F.ConstantFilter(">", -10_000)})
    counts = {}
    for name, (start, tid) in {"reader": (10, TXN_START + 1), "writer": (10, writer), "early": (3, TXN_START + 2)}.items():
        txn, tx = L.Txn(start, tid), O.Mvcc(start, tid, inserted=inserted, deleted=deleted)
        for by in ([1], [1, 2]):
            want, chose = check_groups(t, ocols, 0, L.TYPE_INT64, by, N, fs, txn=txn, tx=tx, what=name)
            assert chose is True  # the visibility leaf is in the program, the slices stay
        counts[name] = sum(a.count_rows for a in want.values())
    assert counts["writer"] < counts["reader"]  # the writer's own deletes
    assert counts["early"] != counts["reader"]  # it sees neither the deletes nor the inserted rows
    txn, tx = L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, inserted=inserted, deleted=deleted)
    w, wx = L.Txn(10, writer), O.Mvcc(10, writer, inserted=inserted, deleted=deleted)
    early, ex = L.Txn(3, TXN_START + 2), O.Mvcc(3, TXN_START + 2, inserted=inserted, deleted=deleted)

    # a visible update of the value column: the column path runs, and path="slices" raises
    m = 3000
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(-80_000, 1 << 20, m).astype(np.int64)
    ok = rng.random(m) >= 0.15
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    t.set_updates(0, rows, new, vers, ok)
    ocols[0] = O.Column(b, bw, updates=(rows, new, vers, ok))
    for x, xx in ((txn, tx), (w, wx)):
        _, chose = check_groups(t, ocols, 0, L.TYPE_INT64, [1, 2], N, fs, txn=x, tx=xx, paths=[None, "column"])
        assert chose is False
        with pytest.raises(L.CubitError) as e:
            t.aggregate_by(0, [1, 2], fs, txn=x, path="slices")
        assert e.value.code == L.ERR_INVALID and b"update" in t.lib.cubit_last_error()
    _, chose = check_groups(t, ocols, 0, L.TYPE_INT64, [1], N, fs, txn=early, tx=ex)  # invisible: the slices stay
    assert chose is True
    t.close()
    t = build()
    ocols[0] = O.Column(b, bw)

    # a visible update of a group column: to an existing key, to a value in no key (77, the writer's
    # own: a new group for the writer alone) and SET NULL on a column without NULLs
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(0, 4, m, endpoint=True).astype(np.int64)
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    new[vers == writer] = np.where(rng.random(int((vers == writer).sum())) < 0.5, 77, new[vers == writer])
    ok = rng.random(m) >= 0.1
    t.set_updates(1, rows, new, vers, ok)
    ocols[1] = O.Column(g, None, updates=(rows, new, vers, ok))
    assert t.aggregate_groups([1]) == [(0,), (1,), (2,), (3,), (4,), (77,), (None,)]
    for by in ([1], [2, 1]):
        seen, chose = check_groups(t, ocols, 0, L.TYPE_INT64, by, N, fs, txn=w, tx=wx, paths=[None, "column"], what="writer")
        assert chose is False and any(77 in k for k in seen) and any(None in k for k in seen)
        with pytest.raises(L.CubitError) as e:
            t.aggregate_by(0, by, fs, txn=w, path="slices")
        assert e.value.code == L.ERR_INVALID
        seen, chose = check_groups(t, ocols, 0, L.TYPE_INT64, by, N, fs, txn=txn, tx=tx, paths=[None, "column"], what="reader")
        assert chose is False and not any(77 in k for k in seen) and any(None in k for k in seen)
        seen, chose = check_groups(t, ocols, 0, L.TYPE_INT64, by, N, fs, txn=early, tx=ex, what="early")
        assert chose is True and not any(77 in k or None in k for k in seen)
    t.close()


# ------------------------------------------------------------------ maintenance, shapes, errors


def test_append_and_merge_equal_a_fresh_table(ctx):
    n0 = N - 5_003
    datas, vws = main_columns(N, seed=55)
    valids = [None if vw is None else np.unpackbits(vw.view(np.uint8), bitorder="little")[:N].astype(bool) for vw in vws]
    t = CubitTable(ctx, n0)
    for i, (data, valid) in enumerate(zip(datas, valids)):
        t.add_column(i, data[:n0], None if valid is None else validity_from_mask(valid[:n0]))
        t.build_index(i, L.INDEX_SLICED if i < 4 else (L.INDEX_RANGE if i == 4 else L.INDEX_EQUALITY))
    t.append({i: data[n0:] for i, data in enumerate(datas)},
             {i: validity_from_mask(valid[n0:]) for i, valid in enumerate(valids) if valid is not None})
    fresh, ocols, _, _ = make_main(ctx, N, seed=55)
    fs = FILTERS["q6"][0]
    for col, by in ((B, [G3, G2]), (A, [G5]), (C_, [G7, G5])):
        for f in (None, fs):
            check_groups(t, ocols, col, TYPES[col], by, N, f, what="append")
            for path in PATHS:
                assert t.aggregate_by(col, by, f, path=path) == fresh.aggregate_by(col, by, f, path=path)
    # merge_updates on group columns (SET NULL among the records of the nullable one) and on a value column
    rng = np.random.default_rng(56)
    for c, lo, hi in ((G3, 0, 2), (G5, 10, 13), (B, 90_000, 90_000 + (1 << 24) - 1)):
        rows = np.sort(rng.choice(N, N // 100, replace=False)).astype(np.int64)
        new = rng.integers(lo, hi, len(rows), endpoint=True).astype(np.int64)
        ok = rng.random(len(rows)) >= (0.2 if c == G5 else 0.0)
        t.set_updates(c, rows, new, np.full(len(rows), 5, np.uint64), ok)
        assert t.merge_updates(c, 6) > 0
        datas[c] = datas[c].copy()
        datas[c][rows] = np.where(ok, new, 0).astype(datas[c].dtype)
        if not ok.all():
            valids[c] = valids[c].copy()
            valids[c][rows] = ok
    merged = CubitTable(ctx, N)
    mcols = []
    for i, (data, valid) in enumerate(zip(datas, valids)):
        vw = None if valid is None else validity_from_mask(valid)
        merged.add_column(i, data, vw)
        merged.build_index(i, L.INDEX_SLICED if i < 4 else (L.INDEX_RANGE if i == 4 else L.INDEX_EQUALITY))
        mcols.append(O.Column(data, vw))
    for col, by in ((B, [G3, G2]), (C_, [G5, G3])):
        want, _ = check_groups(t, mcols, col, TYPES[col], by, N, fs, what="merge")
        for path in PATHS:
            assert t.aggregate_by(col, by, path=path) == merged.aggregate_by(col, by, path=path)
    for x in (t, fresh, merged):
        x.close()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_tiny_and_empty_tables(ctx, n):
    t, ocols, datas, _ = make_main(ctx, n)
    for col, by in ((C_, [G3]), (B, [G3, G2]), (D, [G5, G7])):
        want, _ = check_groups(t, ocols, col, TYPES[col], by, n, paths=PATHS if n else [None, "column"])
        check_groups(t, ocols, col, TYPES[col], by, n, FILTERS["q6"][0], paths=PATHS if n else [None, "column"])
        assert (want == {}) == (n == 0)
    t.close()


def test_errors(main, ctx):
    t, _ = main
    with pytest.raises(L.CubitError) as e:  # a RANGE index, and a bit-sliced one, are no group columns
        t.aggregate_by(B, [E])
    assert e.value.code == L.ERR_UNSUPPORTED and b"column 4" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:
        t.aggregate_by(B, [G3, A])
    assert e.value.code == L.ERR_UNSUPPORTED and b"column 0" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:
        t.aggregate_by(B, [G3, G2, G5])
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.CubitError) as e:
        t.aggregate_by(B, [])
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.CubitError) as e:
        t.aggregate_by(B, [G3], path="slices", ops=L.AGG_SUM | L.AGG_FROM_COLUMN)
    assert e.value.code == L.ERR_INVALID and b"both" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:
        t.aggregate_by(E, [G3], path="slices")  # no bit-sliced index on the value column
    assert e.value.code == L.ERR_INVALID
    assert t.aggregate_by(E, [G3]) == t.aggregate_by(E, [G3], path="column") and t.last_grouped()[0] is False
    cols = (C.c_int * 2)(G3, G2)
    out = t.ctx.alloc(6 * 48)
    grouped = t.lib.cubit_table_aggregate_grouped
    assert grouped(t.handle, None, 0, None, B, cols, 2, L.AGG_SUM, out.ptr, 5) == L.ERR_CAPACITY
    assert grouped(t.handle, None, 0, None, B, cols, 2, 8, out.ptr, 6) == L.ERR_INVALID
    assert grouped(t.handle, None, 0, None, 99, cols, 2, L.AGG_SUM, out.ptr, 6) == L.ERR_INVALID
    assert grouped(t.handle, None, 0, None, B, cols, 2, L.AGG_SUM, out.ptr, 6) == L.OK
    t.ctx.check()
    # two faults at once: the earlier check answers
    both = L.AGG_SUM | L.AGG_FROM_SLICES | L.AGG_FROM_COLUMN
    assert grouped(t.handle, None, 0, None, 99, cols, 2, both, out.ptr, 6) == L.ERR_INVALID
    assert b"both" in t.lib.cubit_last_error()
    assert grouped(t.handle, None, 0, None, 99, cols, 2, 8, out.ptr, 6) == L.ERR_INVALID
    assert b"ops 8" in t.lib.cubit_last_error()
    unindexed = (C.c_int * 2)(G3, A)  # A has no EQUALITY index, and one slot is no room for the groups
    assert grouped(t.handle, None, 0, None, B, unindexed, 2, L.AGG_SUM, out.ptr, 1) == L.ERR_UNSUPPORTED
    assert b"column 0" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:  # no sliced index, and a filter no row passes: refused, no zeros
        t.aggregate_by(E, [G3], FILTERS["false"][0], FILTERS["false"][1], path="slices")
    assert e.value.code == L.ERR_INVALID and b"column 4" in t.lib.cubit_last_error()
    out.free()
    # more than 256 groups: 17 x 16 slots
    rng = np.random.default_rng(57)
    n = 4_099
    u = CubitTable(ctx, n)
    for i, k in enumerate((1, 17, 16, 257)):
        data = rng.integers(0, k - 1, n, endpoint=True).astype(np.int64)
        data[:k] = np.arange(k)
        u.add_column(i, data)
        u.build_index(i, L.INDEX_SLICED if i == 0 else L.INDEX_EQUALITY)
    for by in ([1, 2], [3]):
        with pytest.raises(L.CubitError) as e:
            u.aggregate_by(0, by)
        assert e.value.code == L.ERR_UNSUPPORTED
    assert len(u.aggregate_by(0, [2, 2])) == 16  # 16 x 16 slots are 256 groups; the diagonal has rows
    assert u.last_grouped()[1] == 256
    u.close()


def test_a_callers_non_blocking_stream_gives_the_same_result(main):
    t, ocols = main
    want = {(col, tuple(by), path): t.aggregate_by(col, by, FILTERS["dnf"][0], FILTERS["dnf"][1], path=path)
            for col, by in ((B, [G3, G2]), (C_, [G5, G7])) for path in PATHS}
    stream = torch.cuda.Stream()  # a pool stream: hipStreamNonBlocking
    c2 = Context(0, stream=stream.cuda_stream)
    try:
        t2, _, _, _ = make_main(c2, N)
        for (col, by, path), w in want.items():
            assert t2.aggregate_by(col, list(by), FILTERS["dnf"][0], FILTERS["dnf"][1], path=path) == w
        t2.close()
    finally:
        c2.close()
