"""cubit_table_select / cubit_table_top_n (CubitTable.quantile, kth, top_n) against numpy: the six
numbers {value, found, below, equal, count_valid, count_rows} on both paths — "slices" (the radix
select over the column's bit-sliced index) and "column" (scan + probe + array select) — with the
zonemap on and off. Expected values are np.sort / np.lexsort over the values the oracle fetches at the
oracle's row ids (O.table_scan, O.fetch), so MVCC deletes and updates are the reference's; typed
columns (FLOAT, VARCHAR, UBIGINT) are checked over the oracle's row ids into the arrays built here."""
import math

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, Selected
from oracle import oracle as O
from test_gpu_caller_stream import delay, delayed  # noqa: F401  (fixtures: a context behind pending work)

pytestmark = pytest.mark.gpu

ZONE = 131_072
N = 3 * ZONE + 37
U64 = (1 << 64) - 1
TXN_START = 4611686018427388000
PATHS = ["slices", "column"]
QUANTILES = [0.0, 0.1, 0.25, 0.5, 1.0]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def quantile_rank(n, q):
    """quantile_disc's 0-based rank among n values, restated: max(1, n - floor(n - n * q)) - 1."""
    return max(1, n - int(math.floor(n - float(n * q)))) - 1


def want(s, count_rows, desc, rank, to_value=int):
    """Selected from the ascending sort keys s of the qualifying non-NULL rows."""
    m = len(s)
    if rank >= m:
        return Selected(None, False, 0, 0, m, count_rows)
    v = s[m - 1 - rank] if desc else s[rank]
    lo, hi = int(np.searchsorted(s, v, "left")), int(np.searchsorted(s, v, "right"))
    return Selected(to_value(v), True, m - hi if desc else lo, hi - lo, m, count_rows)


def oracle_keys(ocols, col, fs, residual, n, tx=None):
    """(ascending values of the qualifying non-NULL rows, qualifying rows) from the oracle."""
    ids = O.table_scan(ocols, F.serialize(fs, residual), n, 0, tx)
    v, ok = O.fetch(ocols[col], ids, 0, tx, with_valid=True)
    return np.sort(np.ascontiguousarray(v[ok]).astype(np.int64)), len(ids)


def check_select(t, s, count_rows, col, fs=None, residual=None, txn=None, paths=PATHS, zonemaps=(True, False),
                 to_value=int, what=None, ranks=None, quantiles=QUANTILES, after=None):
    """kth at `ranks` (default: both ends, the middle and one past the last) in both directions and
    quantile at `quantiles`, on every path with the zonemap as listed, against the ascending keys s.
    after(path, zonemap) runs behind each call, while the table's last_* counters are still that call's."""
    m = len(s)
    if ranks is None:
        ranks = sorted({0, 1, m // 2, max(m - 2, 0), max(m - 1, 0), m})
    for path in paths:
        for zm in zonemaps:
            for rank in ranks:
                for desc in (False, True):
                    got = t.kth(col, rank, desc, fs, residual, txn=txn, path=path, zonemap=zm)
                    assert got == want(s, count_rows, desc, rank, to_value), (what, path, zm, rank, desc)
                    if after:
                        after(path, zm)
            for q in quantiles:
                got = t.quantile(col, q, fs, residual, txn=txn, path=path, zonemap=zm)
                assert got == want(s, count_rows, False, quantile_rank(m, q) if m else 0, to_value), (what, path, zm, q)
                if after:
                    after(path, zm)
            if path is not None and count_rows:  # (a filter that folds to FALSE runs neither path)
                assert t.last_select()[0] == (path == "slices"), (what, path)


# ------------------------------------------------------------------ the table


@pytest.fixture(scope="module")
def table(ctx):
    """Three zones and a ragged tail: 0 = a nullable 12-bit INT32 with a bit-sliced index, 1 = a small
    INT64 with a RANGE index, 2 = a clustered INT32 (sorted: zones hold ranges) with a bit-sliced index,
    3 = a nullable INT64 of 11 distinct values with a bit-sliced index."""
    rng = np.random.default_rng(51)
    a = rng.integers(1000, 1000 + 4095, N, endpoint=True).astype(np.int32)
    a[:2] = [1000, 1000 + 4095]
    av = rng.random(N) >= 0.05
    av[:2] = True
    b = rng.integers(0, 10, N, endpoint=True).astype(np.int64)
    c = np.sort(rng.integers(0, 4000, N).astype(np.int32))
    d = (rng.integers(0, 10, N, endpoint=True) * 7 - 20).astype(np.int64)
    dv = rng.random(N) >= 0.1
    vws = [validity_from_mask(av), None, None, validity_from_mask(dv)]
    t = CubitTable(ctx, N)
    for i, (data, vw) in enumerate(zip([a, b, c, d], vws)):
        t.add_column(i, data, vw)
        t.build_index(i, L.INDEX_RANGE if i == 1 else L.INDEX_SLICED)
    ocols = [O.Column(x, vw) for x, vw in zip([a, b, c, d], vws)]
    yield t, ocols, (d, dv, b)
    t.close()


FILTERS = {
    "conjunction": (F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 2000), F.ConstantFilter("<", 3000)]),
                                      1: F.ConjunctionAndFilter([F.ConstantFilter(">=", 3), F.ConstantFilter("<=", 7)])}), None),
    "or": (None, F.Or(F.Cmp(0, "<", 1100), F.And(F.Cmp(2, ">", 3000), F.Cmp(1, "<", 5)), F.IsNull(3))),
    "false": (F.TableFilterSet({0: F.ConstantFilter("<", 990)}), None),
    "is_null": (F.TableFilterSet({0: F.IsNullFilter()}), None),
    "none": (None, None),
}


@pytest.mark.parametrize("name", list(FILTERS))
def test_quantile_and_kth_every_filter_both_paths(table, name):
    t, ocols, _ = table
    fs, residual = FILTERS[name]
    s, rows = oracle_keys(ocols, 0, fs, residual, N)
    check_select(t, s, rows, 0, fs, residual, what=name)
    if name == "false":
        assert rows == 0 and t.last_zones()[0] == 0
    if name == "is_null":
        got = t.quantile(0, 0.5, fs, path="slices")
        assert not got.found and got.value is None and got.count_valid == 0 < got.count_rows


def test_clustered_filter_skips_zones_on_both_paths(table):
    t, ocols, _ = table
    fs = F.TableFilterSet({2: F.ConjunctionAndFilter([F.ConstantFilter(">=", 100), F.ConstantFilter("<", 300)])})
    for col in (0, 2, 3):
        s, rows = oracle_keys(ocols, col, fs, None, N)
        check_select(t, s, rows, col, fs, what=("clustered", col))
    for path in PATHS:
        t.quantile(0, 0.5, fs, path=path)
        ev, nz = t.last_zones()
        assert 0 < ev < nz == 4, (path, ev, nz)
        t.quantile(0, 0.5, fs, path=path, zonemap=False)
        assert t.last_zones() == (nz, nz)


def test_unforced_dense_filter_takes_the_slices(table):
    t, ocols, _ = table
    s, rows = oracle_keys(ocols, 0, None, None, N)
    assert t.quantile(0, 0.5) == want(s, rows, False, quantile_rank(len(s), 0.5))
    assert t.last_select() == (True, 3)  # 12 slices, 4 per pass
    fs = F.TableFilterSet({1: F.ConstantFilter(">=", 5)})
    s, rows = oracle_keys(ocols, 0, fs, None, N)
    assert t.kth(0, 7, True, fs) == want(s, rows, True, 7)
    assert t.last_select()[0]
    t.kth(0, 7, False, fs, path="column")
    assert t.last_select() == (False, 8)  # 64 bits, 8 per pass


def test_refusals(table):
    t, _, _ = table
    for call in (lambda: t.quantile(1, 0.5, path="slices"),  # a RANGE index only
                 lambda: t.quantile(0, 1.5), lambda: t.quantile(0, -0.01), lambda: t.quantile(0, float("nan")),
                 lambda: t.kth(99, 0)):  # unregistered
        with pytest.raises(L.CubitError) as e:
            call()
        assert e.value.code == L.ERR_INVALID
    out = t.ctx.alloc(48)
    sel = t.lib.cubit_table_select
    assert sel(t.handle, None, 0, None, 0, 3, 0, 0.0, 0, out.ptr) == L.ERR_INVALID  # mode
    assert sel(t.handle, None, 0, None, 0, 0, 0, 0.0, L.SELECT_FROM_SLICES | L.SELECT_FROM_COLUMN, out.ptr) == L.ERR_INVALID
    assert sel(t.handle, None, 0, None, 0, 0, 0, 0.0, 8, out.ptr) == L.ERR_INVALID  # flags
    # two faults at once: the earlier check answers
    both = L.SELECT_FROM_SLICES | L.SELECT_FROM_COLUMN
    assert sel(t.handle, None, 0, None, 99, 0, 0, 0.0, both, out.ptr) == L.ERR_INVALID and b"both" in t.lib.cubit_last_error()
    assert sel(t.handle, None, 0, None, 99, 0, 0, 0.0, 8, out.ptr) == L.ERR_INVALID and b"flags 8" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:  # no sliced index, and a filter no row passes: refused, no zeros
        t.quantile(1, 0.5, FILTERS["false"][0], path="slices")
    assert e.value.code == L.ERR_INVALID and b"column 1" in t.lib.cubit_last_error()
    # without a sliced index the unforced call and the column path agree
    assert t.quantile(1, 0.5) == t.quantile(1, 0.5, path="column") and not t.last_select()[0]
    t.use_sliced(False)
    try:
        with pytest.raises(L.CubitError) as e:
            t.quantile(0, 0.5, path="slices")
        assert e.value.code == L.ERR_INVALID
        t.quantile(0, 0.5)
        assert not t.last_select()[0]
    finally:
        t.use_sliced(True)


def test_empty_partition(ctx):
    t = CubitTable(ctx, 0)
    t.add_column(0, np.zeros(0, np.int64))
    t.build_index(0, L.INDEX_SLICED)
    for path in (None, "column"):
        assert t.quantile(0, 0.5, path=path) == Selected(None, False, 0, 0, 0, 0)
        assert t.kth(0, 0, path=path) == Selected(None, False, 0, 0, 0, 0)
    ids, vals, sel = t.top_n(0, 5)
    assert len(ids) == 0 and len(vals) == 0 and not sel.found
    t.close()


# ------------------------------------------------------------------ MVCC


def test_deletes_and_updates_of_the_selected_column(ctx):
    rng = np.random.default_rng(52)
    a = rng.integers(1000, 3525, N, endpoint=True).astype(np.int32)
    av = rng.random(N) >= 0.05
    b = rng.integers(-70_000, 70_000, N, endpoint=True).astype(np.int64)
    bv = rng.random(N) >= 0.05
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
    fs = F.TableFilterSet({0: F.ConstantFilter(">", 1500)})
    txn, tx = L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted)
    for f in (None, fs):  # visible deletes: the visibility leaf is in the program, the slices stay
        s, rows = oracle_keys(ocols, 1, f, None, N, tx)
        check_select(t, s, rows, 1, f, txn=txn, zonemaps=(True,), what="deletes")
        t.quantile(1, 0.5, f, txn=txn)
        assert t.last_select()[0]
    # update records of the selected column: a committed half and a writer's own, SET NULL among them
    writer = TXN_START + 9
    m = 3000
    urows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(-80_000, 1 << 20, m).astype(np.int64)  # also outside the slices' range
    ok = rng.random(m) >= 0.15
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    t.set_updates(1, urows, new, vers, ok)
    ocols = [O.Column(a, aw), O.Column(b, bw, updates=(urows, new, vers, ok))]
    # visible: the slices hold the base values, so the column path runs and sees the new ones
    for f, who, whox in ((fs, txn, tx), (None, L.Txn(10, writer), O.Mvcc(10, writer, deleted=deleted))):
        s, rows = oracle_keys(ocols, 1, f, None, N, whox)
        check_select(t, s, rows, 1, f, txn=who, paths=[None, "column"], zonemaps=(True,), what="visible updates")
        assert int(s[-1]) > 70_000  # a new value above the slices' top is the maximum
        t.kth(1, 0, True, f, txn=who)
        assert not t.last_select()[0]
        with pytest.raises(L.CubitError) as e:
            t.quantile(1, 0.5, f, txn=who, path="slices")
        assert e.value.code == L.ERR_INVALID
    # invisible (a reader that predates them): the slices may run, and both paths see the base values
    early, ex = L.Txn(3, TXN_START + 2), O.Mvcc(3, TXN_START + 2, deleted=deleted)
    s, rows = oracle_keys(ocols, 1, fs, None, N, ex)
    check_select(t, s, rows, 1, fs, txn=early, zonemaps=(True,), what="invisible updates")
    t.quantile(1, 0.5, fs, txn=early)
    assert t.last_select()[0]
    # updates on the filter column only: patched into the program, the selected column keeps its slices
    s, rows = oracle_keys(ocols, 0, F.TableFilterSet({1: F.ConstantFilter(">", 0)}), None, N, tx)
    check_select(t, s, rows, 0, F.TableFilterSet({1: F.ConstantFilter(">", 0)}), txn=txn, zonemaps=(True,),
                 what="filter column updated")
    t.close()


# ------------------------------------------------------------------ maintenance


def test_append_and_merge_updates(ctx):
    rng = np.random.default_rng(53)
    v = rng.integers(1000, 3525, N, endpoint=True).astype(np.int64)
    valid = rng.random(N) >= 0.05
    t = CubitTable(ctx, N)
    t.add_column(0, v, validity_from_mask(valid))
    t.build_index(0, L.INDEX_SLICED)

    def check(what):
        mid = int(np.median(v))
        for fs, mask in ((None, np.ones(len(v), bool)), (F.TableFilterSet({0: F.ConstantFilter(">", mid)}), valid & (v > mid))):
            check_select(t, np.sort(v[mask & valid]), int(mask.sum()), 0, fs, zonemaps=(True,), what=what)

    check("built")
    e = rng.integers(1000, 100_000, 5_003, endpoint=True).astype(np.int64)
    e[0] = 100_000  # above the old top: slices are added
    t.append({0: e})
    v, valid = np.concatenate([v, e]), np.concatenate([valid, np.ones(len(e), bool)])
    check("append above the top")
    assert t.kth(0, 0, True, path="slices").value == 100_000 == t.kth(0, 0, True, path="column").value
    n = len(v)
    rows = np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64)
    new = rng.integers(-9_000, 200_000, len(rows), endpoint=True).astype(np.int64)
    new[0] = 200_000  # above the top again
    ok = rng.random(len(rows)) >= 0.2  # SET NULL among them
    ok[0] = True
    t.set_updates(0, rows, new, np.full(len(rows), 5, np.uint64), ok)
    assert t.merge_updates(0, 6) > 0
    v, valid = v.copy(), valid.copy()
    v[rows] = np.where(ok, new, 0)
    valid[rows] = ok
    check("merge")
    assert t.kth(0, 0, True, path="slices").value == 200_000
    t.close()


# ------------------------------------------------------------------ typed columns


def float_keys(pattern):
    """cubit_fp_key of FLOAT bit patterns: every NaN one key above +inf, -x → -pattern(x)."""
    u = pattern.astype(np.int64) & 0xFFFFFFFF
    mag = u & 0x7FFFFFFF
    return np.where(mag > 0x7F800000, 0x7FC00000, np.where(u >> 31 != 0, -mag, mag))


def float_value(key):
    """A FLOAT key as the zero-extended bit pattern column_statistics hands out."""
    key = int(key)
    return key if key >= 0 else (0x80000000 | -key)


def test_float_with_nan_and_negative_zero(ctx, table):
    _, ocols, (_, _, b) = table
    rng = np.random.default_rng(54)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 3e38, -3e38, 1e-45], dtype=np.float32)
    f = np.where(rng.random(N) < 0.5, pool[rng.integers(0, len(pool), N)], rng.normal(0, 100, N).astype(np.float32))
    f = f.astype(np.float32)
    valid = rng.random(N) >= 0.05
    t = CubitTable(ctx, N)
    t.add_column(0, f, validity_from_mask(valid))
    t.add_column(1, b)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_RANGE)
    keys = float_keys(f.view(np.int32))
    for fs, mask in ((None, np.ones(N, bool)), (F.TableFilterSet({1: F.ConstantFilter("<", 4)}), b < 4)):
        check_select(t, np.sort(keys[mask & valid]), int(mask.sum()), 0, fs, zonemaps=(True,), to_value=float_value, what=fs)
    assert t.kth(0, 0, True, path="slices").value == 0x7FC00000  # NaN above +inf
    n_neg = int((keys[valid] < 0).sum())
    zero = t.kth(0, n_neg, path="slices")
    assert zero.value == 0 and zero.equal == int((keys[valid] == 0).sum())  # -0.0 and +0.0: one value, +0.0
    # top-N with the threshold handed back as a pattern: inside the ±0 class, inside the NaN class
    # (col = NaN), and just past it (col > +inf keeps the NaN rows)
    n_nan = int((keys[valid] == 0x7FC00000).sum())
    assert n_nan > 200 and zero.equal > 200
    ids = np.flatnonzero(valid).astype(np.int64)
    for desc, k in ((False, n_neg + 100), (True, 100), (True, n_nan + 50), (False, 1)):
        for path in PATHS:
            got_ids, got_vals, sel = t.top_n(0, k, desc, path=path)
            want_ids, want_keys = top_n_expected(ids, keys[ids], k, desc)
            assert np.array_equal(got_ids, want_ids), (desc, k, path)
            assert np.array_equal(got_vals.astype(np.uint32), f.view(np.uint32)[want_ids]), (desc, k, path)
            assert np.array_equal(float_keys(got_vals), want_keys), (desc, k, path)
            assert sel == want(np.sort(keys[valid]), N, desc, k - 1, float_value), (desc, k, path)
    t.close()


def test_ubigint_and_varchar(ctx):
    rng = np.random.default_rng(55)
    n = ZONE + 4_001
    u = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    u[:4] = [0, 1 << 63, (1 << 63) - 1, U64]
    uv = rng.random(n) >= 0.05
    uv[:4] = True
    pool = sorted({bytes(rng.integers(97, 123, rng.integers(1, 6)).astype(np.uint8)) for _ in range(60)})
    strs = [None if rng.random() < 0.05 else pool[i] for i in rng.integers(0, len(pool), n)]
    t = CubitTable(ctx, n)
    t.add_column(0, u, validity_from_mask(uv))
    d = t.add_string_column(1, strs)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    codes, cv = d.encode(strs)
    ukeys = (u ^ np.uint64(1 << 63)).view(np.int64)

    def bits(key):  # the value's bits as an int64
        return int(np.int64(key) ^ np.int64(-(1 << 63)))

    fs = F.TableFilterSet({1: F.ConstantFilter(">", pool[17])})
    mask = cv & (codes > 17)
    check_select(t, np.sort(ukeys[uv]), n, 0, zonemaps=(True,), to_value=bits, what="ubigint")
    check_select(t, np.sort(ukeys[uv & mask]), int(mask.sum()), 0, fs, zonemaps=(True,), to_value=bits, what="ubigint filtered")
    assert t.kth(0, 0, True, path="slices").value == -1  # 2^64 - 1: unsigned order across 2^63
    # top-N with thresholds on both sides of 2^63 (the filter constant is the value's bits)
    for f_, m_ in ((None, uv), (fs, uv & mask)):
        ids = np.flatnonzero(m_).astype(np.int64)
        for desc, k in ((False, 1), (False, 3), (True, 2), (True, 1000), (False, len(ids) // 2 + 7)):
            for path in PATHS:
                got_ids, got_vals, _ = t.top_n(0, k, desc, f_, path=path)
                want_ids, _ = top_n_expected(ids, ukeys[ids], k, desc)
                assert np.array_equal(got_ids, want_ids), (desc, k, path)
                assert np.array_equal(got_vals.view(np.uint64), u[want_ids]), (desc, k, path)
    check_select(t, np.sort(codes[cv].astype(np.int64)), n, 1, zonemaps=(True,), what="varchar")
    check_select(t, np.sort(codes[mask].astype(np.int64)), int(mask.sum()), 1, fs, zonemaps=(True,), what="varchar filtered")
    with pytest.raises(L.CubitError) as e:  # the threshold is a code: no filter constant
        t.top_n(1, 3)
    assert e.value.code == L.ERR_UNSUPPORTED
    t.close()


# ------------------------------------------------------------------ top-N


def top_n_expected(ids, vals, k, desc):
    order = np.lexsort((ids, ~vals if desc else vals))[:k]  # ~: descending without overflow at INT64_MIN
    return ids[order], vals[order]


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("filtered", [False, True], ids=["all", "filtered"])
def test_top_n_cuts_inside_a_tie_class(table, filtered, desc):
    t, ocols, (d, dv, b) = table
    fs = F.TableFilterSet({1: F.ConstantFilter(">=", 3)}) if filtered else None
    ids = O.table_scan(ocols, F.serialize(fs, None), N, 0, None)
    v, ok = O.fetch(ocols[3], ids, 0, None, with_valid=True)
    ids, vals = ids[ok], np.ascontiguousarray(v[ok]).astype(np.int64)
    count_rows, cv = len(ok), len(ids)
    # the threshold class: 11 distinct values, so one class holds about a tenth of the rows, in every
    # zone; k cuts it inside the second zone
    thr = 15
    before = int((vals > thr).sum() if desc else (vals < thr).sum())
    ties = ids[vals == thr]
    assert (ties < ZONE).any() and (ties >= 2 * ZONE).any()
    k_cut = before + int((ties < ZONE + 50_000).sum())
    assert ZONE <= ties[k_cut - before - 1] < 2 * ZONE and ties[k_cut - before] < 2 * ZONE
    for k in (0, 1, k_cut, cv, cv + 1000):
        for path in PATHS:
            got_ids, got_vals, sel = t.top_n(3, k, desc, fs, path=path)
            want_ids, want_vals = top_n_expected(ids, vals, k, desc)
            assert np.array_equal(got_ids, want_ids) and np.array_equal(got_vals, want_vals), (k, path)
            if k:
                assert sel == want(np.sort(vals), count_rows, desc, k - 1), (k, path)
                assert t.last_select()[0] == (path == "slices")
            raw_ids, _, _ = t.top_n(3, k, desc, fs, path=path, sort=False, capacity=k + 5)
            assert np.array_equal(raw_ids, np.sort(want_ids)), (k, path)  # the ids arrive ascending
    got_ids, _, sel = t.top_n(3, cv + 1000, desc, fs)  # no NULL row is returned
    assert len(got_ids) == cv and not sel.found and sel.count_rows - sel.count_valid == count_rows - cv
    with pytest.raises(L.CubitError) as e:
        t.top_n(3, k_cut, desc, fs, capacity=k_cut - 1)
    assert e.value.code == L.ERR_CAPACITY


# ------------------------------------------------------------------ a caller's stream


def test_on_a_callers_stream_behind_pending_work(delayed):
    """Every call queues behind a spin on the caller's non-blocking stream: uploads, index builds, the
    select's passes and steps and the top-N's scans must all be ordered on that stream."""
    dl = delayed()
    rng = np.random.default_rng(56)
    n = ZONE + 5_003
    a = rng.integers(-500, 3000, n, endpoint=True).astype(np.int64)
    av = rng.random(n) >= 0.1
    b = rng.integers(0, 10, n, endpoint=True).astype(np.int64)
    t = CubitTable(dl.ctx, n)
    t.add_column(0, a, validity_from_mask(av))
    t.add_column(1, b)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_RANGE)
    fs = F.TableFilterSet({1: F.ConstantFilter("<", 6)})
    mask = b < 6
    s = np.sort(a[mask & av])
    for path in PATHS:
        assert t.quantile(0, 0.5, fs, path=path) == want(s, int(mask.sum()), False, quantile_rank(len(s), 0.5))
        assert t.kth(0, 3, True, fs, path=path) == want(s, int(mask.sum()), True, 3)
        ids = np.flatnonzero(mask & av).astype(np.int64)
        got_ids, got_vals, _ = t.top_n(0, 777, False, fs, path=path)
        want_ids, want_vals = top_n_expected(ids, a[ids], 777, False)
        assert np.array_equal(got_ids, want_ids) and np.array_equal(got_vals, want_vals)
    t.close()
