"""cubit_table_aggregate (CubitTable.aggregate) against Python integers: sum / min / max / count(col)
/ count(*) of a column over a filter's rows on all three paths — path=None (the library chooses),
"slices" (the fused evaluate + aggregate over the column's bit-sliced index) and "column" (scan +
probe + reduce). Expected values are reductions over the values the oracle fetches at the oracle's
row ids (O.table_scan, O.fetch), so MVCC deletes, inserts and updates are the reference's."""
import numpy as np
import pytest

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
CMPS = ["=", "!=", "<", "<=", ">", ">="]


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
    """cubit_fp_key of DOUBLE bit patterns (int64): every NaN one key above +inf, -x → -pattern(x)."""
    mag = bits & np.int64(0x7FFFFFFFFFFFFFFF)
    key = np.where(bits < 0, -mag, mag)
    key[mag > np.int64(0x7FF0000000000000)] = 0x7FF8000000000000
    return key


def double_value(key):
    """cubit_fp_value: a DOUBLE key as the bit pattern (an int64) column_statistics hands out."""
    key = int(key)
    if key >= 0:
        return key
    p = (1 << 63) | (-key)
    return p - (1 << 64)


def reduce_values(vals, typ, ops):
    """Aggregate(sum, min, max, count) of the valid visible values `vals` (int64: values, DOUBLE bit
    patterns, UINT64 bits, dictionary codes), in the form the library reports."""
    n = len(vals)
    s = mn = mx = None
    if typ == L.TYPE_UINT64:
        u = vals.view(np.uint64)
        s, lo, hi = exact_sum(u), (int(u.min()) if n else None), (int(u.max()) if n else None)
        mn = None if lo is None else (lo - (1 << 64) if lo >> 63 else lo)  # the bits as an int64
        mx = None if hi is None else (hi - (1 << 64) if hi >> 63 else hi)
    elif typ == L.TYPE_DOUBLE:
        k = double_keys(vals)
        s, mn, mx = 0, (double_value(k.min()) if n else None), (double_value(k.max()) if n else None)
    else:
        s, mn, mx = exact_sum(vals), (int(vals.min()) if n else None), (int(vals.max()) if n else None)
    return (s if ops & L.AGG_SUM else 0, mn if ops & L.AGG_MIN else None, mx if ops & L.AGG_MAX else None, n)


def expected(ocols, col, typ, plan, n, tx, ops, codes=None):
    ids = O.table_scan(ocols, plan, n, 0, tx)
    if codes is not None:  # a dictionary column: its codes and NULL-ness are known here
        c, ok = codes
        vals = c[ids][ok[ids]].astype(np.int64)
    else:
        v, ok = O.fetch(ocols[col], ids, 0, tx, with_valid=True)
        vals = np.ascontiguousarray(v[ok])
    s, mn, mx, cv = reduce_values(vals, typ, ops)
    return Aggregate(s, mn, mx, cv, len(ids))


def check_paths(t, ocols, col, typ, n, fs=None, residual=None, txn=None, tx=None, ops=None, zonemap=True,
                paths=PATHS, codes=None, what=None, after=None):
    """Every path equals the expected reduction; returns whether path=None read the slices. after(path)
    runs behind each call, while the table's last_* counters are still that call's."""
    if ops is None:
        ops = L.AGG_ALL if typ not in (L.TYPE_DOUBLE, L.TYPE_VARCHAR) else L.AGG_MIN | L.AGG_MAX
    want = expected(ocols, col, typ, F.serialize(fs, residual), n, tx, ops, codes)
    chose = None
    for path in paths:
        got = t.aggregate(col, fs, residual, txn=txn, ops=ops, path=path, zonemap=zonemap)
        assert got == want, (what, col, path, ops, got, want)
        if after:
            after(path)
        used = t.last_aggregate_from_slices()
        if path is None:
            chose = used
        elif want.count_rows:  # (a filter that folds to FALSE runs neither path)
            assert used == (path == "slices"), (what, col, path)
    return chose


def int_column(rng, n, dtype, lo, hi, null_frac=0.05):
    v = rng.integers(lo, hi, n, endpoint=True).astype(dtype)
    v[:2] = [lo, hi]
    valid = rng.random(n) >= null_frac
    valid[:2] = True
    return v, valid


# ------------------------------------------------------------------ columns and filters


@pytest.fixture(scope="module")
def typed(ctx):
    """12-bit INT32 with 5 % NULLs, 24-bit INT64, negative-to-positive INT64, UINT64 (each with a
    bit-sliced index), and a small INT64 with a RANGE index for the Q6-shaped conjunction."""
    rng = np.random.default_rng(31)
    a, av = int_column(rng, N, np.int32, 1000, 1000 + 4095)
    b, _ = int_column(rng, N, np.int64, 90_000, 90_000 + (1 << 24) - 1, null_frac=0)
    c, cv = int_column(rng, N, np.int64, -5_000_000_000, 5_000_000_123)
    d = rng.integers(0, U64, N, dtype=np.uint64, endpoint=True)
    d[:4] = [0, 1, U64 - 1, U64]
    dv = rng.random(N) >= 0.05
    dv[:4] = True
    e = rng.integers(0, 10, N, endpoint=True).astype(np.int64)
    vws = [validity_from_mask(av), None, validity_from_mask(cv), validity_from_mask(dv), None]
    t = CubitTable(ctx, N)
    for i, (data, vw) in enumerate(zip([a, b, c, d, e], vws)):
        t.add_column(i, data, vw)
        t.build_index(i, L.INDEX_SLICED if i < 4 else L.INDEX_RANGE)
    ocols = [O.Column(x, vw) for x, vw in zip([a, b, c, d, e], vws)]
    types = [L.TYPE_INT32, L.TYPE_INT64, L.TYPE_INT64, L.TYPE_UINT64, L.TYPE_INT64]
    yield t, ocols, types
    t.close()


FILTERS = {
    "none": (None, None),
    "q6": (F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 2000), F.ConstantFilter("<", 3000)]),
                             4: F.ConjunctionAndFilter([F.ConstantFilter(">=", 5), F.ConstantFilter("<=", 7)]),
                             1: F.ConstantFilter("<", 90_000 + (1 << 23))}), None),
    "or": (None, F.Or(F.Cmp(0, "<", 1100), F.And(F.Cmp(2, ">", 4_000_000_000), F.Cmp(4, "<", 5)), F.IsNull(2))),
    "false": (F.TableFilterSet({0: F.ConstantFilter("<", 990)}), None),
}


@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("col", [0, 1, 2, 3])
def test_integer_columns_every_path(typed, col, name):
    t, ocols, types = typed
    fs, residual = FILTERS[name]
    check_paths(t, ocols, col, types[col], N, fs, residual, what=name)
    if name == "false":
        assert t.aggregate(col, fs, residual) == Aggregate(0, None, None, 0, 0)
        assert t.last_zones()[0] == 0


@pytest.mark.parametrize("col", [0, 2, 3])
def test_is_null_on_the_aggregated_column(typed, col):
    t, ocols, types = typed
    fs = F.TableFilterSet({col: F.IsNullFilter()})
    check_paths(t, ocols, col, types[col], N, fs)
    got = t.aggregate(col, fs, path="slices")
    assert got.count_valid == 0 < got.count_rows and got.min is None and got.max is None and got.sum == 0


def test_every_ops_subset_and_unasked_slots(typed):
    t, ocols, types = typed
    fs, residual = FILTERS["q6"]
    for ops in range(8):
        check_paths(t, ocols, 2, types[2], N, fs, residual, ops=ops, what=ops)
    # the raw slots: those of ops not asked for are 0
    plan = F.serialize(fs, residual)
    arr = F.to_ctypes(plan.nodes)
    out = t.ctx.alloc(48)
    for flag in (L.AGG_FROM_SLICES, L.AGG_FROM_COLUMN):
        L.check(t.lib.cubit_memset_d(t.ctx.handle, out.ptr, 0xFF, 48))
        L.check(t.lib.cubit_table_aggregate(t.handle, arr, len(plan.nodes), None, 2, L.AGG_MAX | flag, out.ptr))
        t.ctx.check()
        slots = out.download(np.int64, 6)
        assert slots[0] == slots[1] == slots[2] == 0 and slots[3] != 0 and 0 < slots[4] <= slots[5]


def test_double_min_max_with_nan_zeros_and_infinities(ctx):
    rng = np.random.default_rng(32)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 1e300, -1e300, 5e-324], dtype=np.float64)
    wide = pool[rng.integers(0, len(pool), N)]
    narrow = 1.0 + rng.random(N)
    valid = rng.random(N) >= 0.05
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, wide, vw)
    t.add_column(1, narrow, vw)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    ocols = [O.Column(wide, vw), O.Column(narrow, vw)]
    nan_bits, ninf_bits = 0x7FF8000000000000, int(np.float64(-np.inf).view(np.int64))
    got = t.aggregate(0, path="slices")
    assert (got.min, got.max) == (ninf_bits, nan_bits)  # NaN above +inf, as DuckDB orders it
    for fs in [None, F.TableFilterSet({0: F.ConstantFilter("=", np.float64(0.0))}),  # ±0: one key, reported as +0.0
               F.TableFilterSet({0: F.ConstantFilter("<", np.float64(np.inf))}),
               F.TableFilterSet({1: F.ConstantFilter(">", np.float64(1.25))})]:
        for col in (0, 1):
            check_paths(t, ocols, col, L.TYPE_DOUBLE, N, fs, what=fs)
    zeros = t.aggregate(0, F.TableFilterSet({0: F.ConstantFilter("=", np.float64(-0.0))}), path="slices")
    assert zeros.min == zeros.max == 0 and zeros.count_valid > 0
    for path in PATHS:  # the keys are not linear in the value
        with pytest.raises(L.CubitError) as e:
            t.aggregate(0, ops=L.AGG_SUM, path=path)
        assert e.value.code == L.ERR_UNSUPPORTED
    t.close()


def test_dictionary_min_max_are_codes(ctx):
    rng = np.random.default_rng(33)
    pool = sorted({bytes(rng.integers(97, 123, rng.integers(1, 6)).astype(np.uint8)) for _ in range(60)})
    vals = [None if rng.random() < 0.05 else pool[i] for i in rng.integers(0, len(pool), N)]
    vals[0], vals[1] = pool[0], pool[-1]
    t = CubitTable(ctx, N)
    d = t.add_string_column(0, vals)
    t.build_index(0, L.INDEX_SLICED)
    codes = d.encode(vals)
    ocols = [O.StringColumn(vals)]
    for fs in [None, F.TableFilterSet({0: F.ConstantFilter(">", pool[17])}),
               F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", pool[3]), F.ConstantFilter("<", pool[9])])})]:
        check_paths(t, ocols, 0, L.TYPE_VARCHAR, N, fs, codes=codes, what=fs)
    assert t.aggregate(0, path="slices")[1:3] == (0, len(d) - 1)
    for path in PATHS:
        with pytest.raises(L.CubitError) as e:
            t.aggregate(0, ops=L.AGG_ALL, path=path)
        assert e.value.code == L.ERR_UNSUPPORTED
    t.close()


def test_refusals(typed):
    t, _, _ = typed
    out = t.ctx.alloc(48)
    agg = t.lib.cubit_table_aggregate
    assert agg(t.handle, None, 0, None, 99, L.AGG_SUM, out.ptr) == L.ERR_INVALID  # unregistered
    assert agg(t.handle, None, 0, None, 0, L.AGG_SUM | L.AGG_FROM_SLICES | L.AGG_FROM_COLUMN, out.ptr) == L.ERR_INVALID
    assert agg(t.handle, None, 0, None, 0, 8, out.ptr) == L.ERR_INVALID
    assert agg(t.handle, None, 0, None, 4, L.AGG_SUM | L.AGG_FROM_SLICES, out.ptr) == L.ERR_INVALID  # no slices
    assert t.aggregate(4) == t.aggregate(4, path="column") and not t.last_aggregate_from_slices()
    # two faults at once: the earlier check answers
    both = L.AGG_SUM | L.AGG_FROM_SLICES | L.AGG_FROM_COLUMN
    assert agg(t.handle, None, 0, None, 99, both, out.ptr) == L.ERR_INVALID and b"both" in t.lib.cubit_last_error()
    assert agg(t.handle, None, 0, None, 99, 8, out.ptr) == L.ERR_INVALID and b"ops 8" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:  # no sliced index, and a filter no row passes: refused, no zeros
        t.aggregate(4, FILTERS["false"][0], path="slices")
    assert e.value.code == L.ERR_INVALID and b"column 4" in t.lib.cubit_last_error()
    out.free()


# ------------------------------------------------------------------ zonemaps


def test_clustered_column_skips_zones(ctx):
    rng = np.random.default_rng(34)
    a = np.sort(rng.integers(0, 4000, N).astype(np.int32))  # clustered: zones hold ranges
    b, bv = int_column(rng, N, np.int64, -70_000, 70_000)
    bw = validity_from_mask(bv)
    t = CubitTable(ctx, N)
    t.add_column(0, a)
    t.add_column(1, b, bw)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    ocols = [O.Column(a), O.Column(b, bw)]
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 100), F.ConstantFilter("<", 300)])})
    for col in (0, 1):
        check_paths(t, ocols, col, [L.TYPE_INT32, L.TYPE_INT64][col], N, fs)
        check_paths(t, ocols, col, [L.TYPE_INT32, L.TYPE_INT64][col], N, fs, zonemap=False)
        for path in ("slices", "column"):
            skipped = t.aggregate(col, fs, path=path)
            ev, nz = t.last_zones()
            assert 0 < ev < nz == 4, (col, path, ev, nz)
            assert t.aggregate(col, fs, path=path, zonemap=False) == skipped
            assert t.last_zones() == (nz, nz)
    t.aggregate(1, fs, path="slices")
    assert t.last_sliced() == 2  # the leaf built from column 0's slices, and the aggregate's own pass
    t.close()


# ------------------------------------------------------------------ MVCC


def test_deletes_inserts_and_updates(ctx):
    rng = np.random.default_rng(35)
    a, av = int_column(rng, N, np.int32, 1000, 3525)
    b, bv = int_column(rng, N, np.int64, -70_000, 70_000)
    aw, bw = validity_from_mask(av), validity_from_mask(bv)
    t = CubitTable(ctx, N)
    t.add_column(0, a, aw)
    t.add_column(1, b, bw)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    dels = np.arange(0, N, 7, dtype=np.int64)
    deleted = np.full(N, np.uint64(2 ** 64 - 2), dtype=np.uint64)
    deleted[dels] = 5
    t.set_deletes(dels, np.full(len(dels), 5, dtype=np.uint64))
    ocols = [O.Column(a, aw), O.Column(b, bw)]
    fs = F.TableFilterSet({1: F.ConstantFilter(">", -10_000)})
    # visible deletes: the visibility leaf is in the program, the slices stay
    txn, tx = L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted)
    for f in (None, fs):
        assert check_paths(t, ocols, 0, L.TYPE_INT32, N, f, txn=txn, tx=tx, what="deletes") is True
    before = t.aggregate(0, fs, txn=L.Txn(3, TXN_START + 2), path="slices")  # a reader that predates them
    assert before.count_rows > t.aggregate(0, fs, txn=txn, path="slices").count_rows
    # update records on both columns: a committed half and a writer's own, SET NULL among them
    writer = TXN_START + 9
    m = 3000
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(-80_000, 1 << 20, m).astype(np.int64)  # also outside the slices' range
    ok = rng.random(m) >= 0.15
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    t.set_updates(1, rows, new, vers, ok)
    ocols = [O.Column(a, aw), O.Column(b, bw, updates=(rows, new, vers, ok))]
    # updates visible on the filter column only: patched into the program, column 0 keeps its slices
    assert check_paths(t, ocols, 0, L.TYPE_INT32, N, fs, txn=txn, tx=tx, what="filter column updated") is True
    # … visible on the aggregated column: the slices hold the base values, so the column path runs
    assert check_paths(t, ocols, 1, L.TYPE_INT64, N, fs, txn=txn, tx=tx, paths=[None, "column"]) is False
    with pytest.raises(L.CubitError) as e:
        t.aggregate(1, fs, txn=txn, path="slices")
    assert e.value.code == L.ERR_INVALID
    w, wx = L.Txn(10, writer), O.Mvcc(10, writer, deleted=deleted)
    assert check_paths(t, ocols, 1, L.TYPE_INT64, N, None, txn=w, tx=wx, paths=[None, "column"]) is False
    # invisible updates (a reader that predates them, no transaction at all) keep the slices
    early, ex = L.Txn(3, TXN_START + 2), O.Mvcc(3, TXN_START + 2, deleted=deleted)
    assert check_paths(t, ocols, 1, L.TYPE_INT64, N, None, txn=early, tx=ex) is True
    assert check_paths(t, [O.Column(a, aw), O.Column(b, bw)], 1, L.TYPE_INT64, N, None) is True
    t.close()


# ------------------------------------------------------------------ maintenance


def test_appends_merge_sync_and_reload(ctx, tmp_path):
    rng = np.random.default_rng(36)
    v, valid = int_column(rng, N, np.int64, 1000, 3525)
    t = CubitTable(ctx, N)
    t.add_column(0, v, validity_from_mask(valid))
    t.build_index(0, L.INDEX_SLICED)

    def check(what):
        n = len(v)
        ocols = [O.Column(v, validity_from_mask(valid))]
        mid = int(np.median(v))
        for fs in (None, F.TableFilterSet({0: F.ConstantFilter(">", mid)}), F.TableFilterSet({0: F.IsNullFilter()})):
            check_paths(t, ocols, 0, L.TYPE_INT64, n, fs, what=what)

    check("built")
    # above the top: slices are added
    e = rng.integers(1000, 100_000, 5_003, endpoint=True).astype(np.int64)
    e[0] = 100_000
    t.append({0: e})
    v, valid = np.concatenate([v, e]), np.concatenate([valid, np.ones(len(e), bool)])
    assert t.index_info(0)[0] == 17
    check("append above the top")
    # below the base: a rebuild
    e = rng.integers(-300, 4000, 4_099, endpoint=True).astype(np.int64)
    e[0] = -300
    ev = rng.random(len(e)) >= 0.2
    ev[0] = True
    t.append({0: e}, {0: validity_from_mask(ev)})
    v, valid = np.concatenate([v, e]), np.concatenate([valid, ev])
    check("append below the base")
    assert t.aggregate(0, path="slices").min == -300
    # merge_updates with SET NULL
    n = len(v)
    rows = np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64)
    new = rng.integers(-9_000, 200_000, len(rows), endpoint=True).astype(np.int64)
    ok = rng.random(len(rows)) >= 0.2
    t.set_updates(0, rows, new, np.full(len(rows), 5, np.uint64), ok)
    assert t.merge_updates(0, 6) > 0
    v, valid = v.copy(), valid.copy()
    v[rows] = np.where(ok, new, 0)
    valid[rows] = ok
    check("merge")
    # sync_column
    v2, valid2 = v.copy(), valid.copy()
    rows = np.sort(rng.choice(n, n // 100, replace=False))
    v2[rows] = rng.integers(-9_000, 200_000, len(rows), endpoint=True)
    valid2[rows] = rng.random(len(rows)) >= 0.2
    n_changed, applied = t.sync_column(0, v2, validity_from_mask(valid2))
    assert applied and n_changed > 0
    v, valid = v2, valid2
    check("sync")
    # save / load round trip
    want = t.aggregate(0, path="slices")
    t.save_index(0, L.INDEX_SLICED, tmp_path / "s.cix")
    twin = CubitTable(ctx, n)
    twin.add_column(0, v, validity_from_mask(valid))
    twin.load_index(0, tmp_path / "s.cix")
    assert twin.aggregate(0, path="slices") == want == twin.aggregate(0, path="column")
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 2000)})
    assert twin.aggregate(0, fs, path="slices") == t.aggregate(0, fs, path="column")
    twin.close()
    t.close()


def test_empty_partition(ctx):
    t = CubitTable(ctx, 0)
    t.add_column(0, np.zeros(0, np.int64))
    t.build_index(0, L.INDEX_SLICED)
    for path in (None, "column"):
        assert t.aggregate(0, path=path) == Aggregate(0, None, None, 0, 0)
        assert t.aggregate(0, F.TableFilterSet({0: F.ConstantFilter(">", 0)}), path=path) == Aggregate(0, None, None, 0, 0)
    t.close()


@pytest.mark.parametrize("value,dtype", [(7, np.int32), (-(1 << 63), np.int64), ((1 << 64) - 1, np.uint64)])
def test_one_distinct_value_has_no_slices(ctx, value, dtype):
    rng = np.random.default_rng(37)
    n = 131_072 + 77
    v = np.full(n, value, dtype=dtype)
    valid = rng.random(n) >= 0.1
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, n)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    assert t.index_info(0)[0] == 0
    typ = L.COLUMN_TYPES[np.dtype(dtype).name]
    ocols = [O.Column(v, vw)]
    check_paths(t, ocols, 0, typ, n)
    check_paths(t, ocols, 0, typ, n, F.TableFilterSet({0: F.IsNotNullFilter()}))
    got = t.aggregate(0, path="slices")
    assert got.sum == int(valid.sum()) * value and got.min == got.max == (value if value < (1 << 63) else -1)
    t.close()


def test_use_sliced_off_takes_the_column_path(typed):
    t, ocols, types = typed
    assert t.aggregate(1) is not None and t.last_aggregate_from_slices()  # every row of a 24-bit column: the slices
    t.use_sliced(False)
    try:
        assert check_paths(t, ocols, 1, types[1], N, paths=[None, "column"]) is False
        with pytest.raises(L.CubitError) as e:
            t.aggregate(1, path="slices")
        assert e.value.code == L.ERR_INVALID
    finally:
        t.use_sliced(True)


# ------------------------------------------------------------------ fuzz


def rand_const_filter(rng, lo, hi, depth=0):
    r = rng.random()
    if depth < 2 and r < 0.3:
        kids = [rand_const_filter(rng, lo, hi, depth + 1) for _ in range(rng.integers(2, 4))]
        return F.ConjunctionAndFilter(kids) if rng.random() < 0.7 else F.ConjunctionOrFilter(kids)
    if r < 0.36:
        return F.IsNullFilter() if rng.random() < 0.5 else F.IsNotNullFilter()
    span = hi - lo
    c = lo - span // 8 - 1 + int(rng.random() * (span + span // 4 + 3))  # reaches past both ends
    return F.ConstantFilter(CMPS[rng.integers(0, 6)], min(max(c, -(1 << 63)), (1 << 63) - 1))


def rand_residual(rng, bounds, depth=0):
    if depth < 2 and rng.random() < 0.5:
        kids = [rand_residual(rng, bounds, depth + 1) for _ in range(rng.integers(2, 4))]
        return F.And(*kids) if rng.random() < 0.5 else F.Or(*kids)
    c = int(rng.integers(0, len(bounds)))
    if rng.random() < 0.1:
        return F.IsNull(c)
    lo, hi = bounds[c]
    return F.Cmp(c, CMPS[rng.integers(0, 6)], min(lo + int(rng.random() * (hi - lo + 1)), (1 << 63) - 1))


@pytest.mark.parametrize("seed", range(25))
def test_fuzz(ctx, seed):
    """20 k rows, two columns of a random span (0 … 62 bits, anywhere in int64) and NULL rate, random
    filter trees and ops, all three paths."""
    rng = np.random.default_rng(9000 + seed)
    n = 20_000 + int(rng.integers(0, 130))
    t = CubitTable(ctx, n)
    ocols, bounds, types = [], [], []
    for c in range(2):
        bits = int(rng.integers(0, 63))
        span = (1 << bits) - 1
        lo = int(rng.integers(-(1 << 62), (1 << 62) - span)) if rng.random() < 0.7 else [0, -(1 << 63), (1 << 63) - 1 - span][seed % 3]
        dtype = np.int32 if bits <= 30 and -(1 << 31) <= lo and lo + span < (1 << 31) else np.int64
        v = (rng.integers(0, span, n, endpoint=True, dtype=np.uint64) + np.uint64(lo & U64)).view(np.int64).astype(dtype)
        valid = rng.random(n) >= [0.0, 0.05, 0.5, 0.99][int(rng.integers(0, 4))]
        vw = validity_from_mask(valid) if not valid.all() else None
        t.add_column(c, v, vw)
        t.build_index(c, L.INDEX_SLICED)
        ocols.append(O.Column(v, vw))
        bounds.append((lo, lo + span))
        types.append(L.TYPE_INT32 if dtype == np.int32 else L.TYPE_INT64)
    for i in range(6):
        filters = {}
        for c in rng.choice(2, size=rng.integers(0, 3), replace=False):
            filters[int(c)] = rand_const_filter(rng, *bounds[int(c)])
        fs = F.TableFilterSet(filters) if filters else None
        residual = rand_residual(rng, bounds) if rng.random() < 0.5 else None
        col = int(rng.integers(0, 2))
        check_paths(t, ocols, col, types[col], n, fs, residual, ops=int(rng.integers(0, 8)), what=(seed, i, fs, residual))
    t.close()
