"""cubit_table_select_grouped (CubitTable.quantile_by, kth_by) against numpy: per group of one or two
EQUALITY-indexed columns the six numbers {value, found, below, equal, count_valid, count_rows} of the
select, on all three paths — path=None (the library chooses), "slices" (the grouped radix select over
the value column's bit slices, a batch of groups per launch) and "column" (scan + probe + one array
select for all groups) — with the zonemap on and off. Expected values are np.sort over the values the
oracle fetches at the oracle's row ids (O.table_scan, O.fetch), grouped in numpy by the group columns'
visible values, so MVCC deletes and updates are the reference's; the grouped result also equals the
loop of kth / quantile calls with AND g = key."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, Selected
from oracle import oracle as O
from test_gpu_caller_stream import delay, delayed  # noqa: F401  (fixtures: a context behind pending work)
from test_gpu_table_select import float_keys, float_value, quantile_rank, want

pytestmark = pytest.mark.gpu

ZONE = 131_072
N = 3 * ZONE + 37
U64 = (1 << 64) - 1
TXN_START = 4611686018427388000
PATHS = ["slices", "column", None]
QUANTILES = [0.0, 0.1, 0.5, 1.0]
BATCH = 8  # kGroupBatchSelect (cubit_program.hpp): groups per launch of the slice path
ARRAY_PASSES = 16  # the column path: 64 bits, 4 per pass


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def visible(ocols, c, ids, tx, known):
    """(comparison keys as int64, validity) of column c at the oracle's row ids; `known`: columns whose
    keys and NULL-ness are arrays built by the test (dictionary codes, FLOAT / UBIGINT keys)."""
    if known is not None and c in known:
        v, ok = known[c]
        return v[ids].astype(np.int64), ok[ids]
    v, ok = O.fetch(ocols[c], ids, 0, tx, with_valid=True)
    return np.ascontiguousarray(v).astype(np.int64), ok


def group_rows(ocols, col, by, fs, residual, n, tx=None, known=None, keyfn=None):
    """{key tuple: (ascending keys of the group's qualifying non-NULL rows, the group's qualifying rows)}
    over the oracle's rows, grouped by the group columns' visible values."""
    ids = O.table_scan(ocols, F.serialize(fs, residual), n, 0, tx)
    out = {}
    if len(ids) == 0:
        return out
    vals, vok = visible(ocols, col, ids, tx, known)
    labels = []
    for g in by:
        gv, gok = visible(ocols, g, ids, tx, known)
        labels += [np.where(gok, gv, 0), (~gok).astype(np.int64)]
    uniq, inv = np.unique(np.stack(labels, axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for u, row in enumerate(uniq):
        m = inv == u
        key = tuple(None if row[2 * j + 1] else (keyfn[g](int(row[2 * j])) if keyfn and g in keyfn else int(row[2 * j]))
                    for j, g in enumerate(by))
        out[key] = (np.sort(vals[m][vok[m]]), int(m.sum()))
    return out


def ranks_of_the_largest(groups):
    """{0, 1, the middle, last, one past the last} of the largest group: smaller groups are both found
    and not found within one call."""
    m = max((len(s) for s, _ in groups.values()), default=0)
    return sorted({0, 1, m // 2, max(m - 1, 0), m})


def key_filter(by, key, residual):
    """residual AND g = key for every group column (IS NULL for the NULL slot)."""
    terms = ([residual] if residual is not None else []) + [
        F.IsNull(g) if k is None else F.Cmp(g, "=", k) for g, k in zip(by, key)]
    return terms[0] if len(terms) == 1 else F.And(*terms)


def check_by(t, groups, col, by, fs=None, residual=None, txn=None, paths=PATHS, zonemaps=(True, False), to_value=int,
             what=None, launches=None, passes=None):
    """kth_by at the ranks of the largest group in both directions and quantile_by at QUANTILES on every
    path with the zonemap as listed: all six numbers per group equal numpy's, the result equals the
    loop of kth / quantile calls with AND g = key, and last_select_grouped reports the path, the groups
    and the launches. Returns whether path=None read the slices."""
    calls = [("kth", rank, desc) for rank in ranks_of_the_largest(groups) for desc in (False, True)]
    calls += [("quantile", q, False) for q in QUANTILES]
    all_keys = t.aggregate_groups(by)
    chose = None
    for kind, x, desc in calls:
        if kind == "kth":
            expect = {k: want(s, rows, desc, x, to_value) for k, (s, rows) in groups.items()}
        else:
            expect = {k: want(s, rows, False, quantile_rank(len(s), x) if len(s) else 0, to_value)
                      for k, (s, rows) in groups.items()}
        looped = {}  # the ungrouped call per key, on the path it picks itself
        for key in all_keys:
            f = key_filter(by, key, residual)
            one = t.kth(col, x, desc, fs, f, txn=txn) if kind == "kth" else t.quantile(col, x, fs, f, txn=txn)
            if one.count_rows:
                looped[key] = one
        assert looped == expect, (what, kind, x, desc)
        for path in paths:
            for zm in zonemaps:
                if kind == "kth":
                    got = t.kth_by(col, x, by, desc, fs, residual, txn=txn, path=path, zonemap=zm)
                else:
                    got = t.quantile_by(col, x, by, fs, residual, txn=txn, path=path, zonemap=zm)
                assert got == expect, (what, kind, x, desc, path, zm)
                used, n_groups, n_launches, n_passes = t.last_select_grouped()
                assert n_groups == len(all_keys) >= len(expect)
                if path is None:
                    chose = used
                elif groups:  # (a filter that folds to FALSE runs neither path)
                    assert used == (path == "slices"), (what, path)
                if groups:
                    assert (n_launches > 0) == used
                    if used and launches is not None:
                        assert n_launches == launches, (what, n_launches)
                    if used and passes is not None:
                        assert n_passes == passes, (what, n_passes)
                    if not used:
                        assert n_passes == ARRAY_PASSES
    return chose


# ------------------------------------------------------------------ the table

A, T, ONE, FIVE, E, CL, G1, G2, G3, G4 = range(10)


def main_columns(n, seed=61):
    """Values, each with a bit-sliced index: 0 = a nullable 12-bit INT32, 1 = a nullable INT64 of 11
    distinct values (heavy ties), 2 = one distinct value (no slice), 3 = a 5-bit INT32 (5 mod 4 != 0).
    4 = a small INT64 with a RANGE index for the filters, 5 = a clustered INT32 (sorted: zones hold
    ranges). Groups, each with an every-value EQUALITY index: 6 = 3 values, 7 = 2 values, nullable (the
    pair (2, 1) has no row), 8 = BATCH + 1 values (two launches, one with a single group), 9 = 25."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1000, 1000 + 4095, n, endpoint=True).astype(np.int32)
    a[:2] = [1000, 1000 + 4095][:n]
    av = rng.random(n) >= 0.05
    av[:2] = True
    tie = (rng.integers(0, 10, n, endpoint=True) * 7 - 20).astype(np.int64)
    tv = rng.random(n) >= 0.1
    one = np.full(n, 4242, dtype=np.int64)
    five = rng.integers(-3, 28, n, endpoint=True).astype(np.int32)
    five[:2] = [-3, 28][:n]
    e = rng.integers(0, 10, n, endpoint=True).astype(np.int64)
    cl = np.sort(rng.integers(0, 4000, n).astype(np.int32))
    g1 = rng.choice(np.array([0, 1, 2], dtype=np.int32), n, p=[0.6, 0.3, 0.1])  # skewed: one largest group
    g2 = rng.integers(0, 1, n, endpoint=True).astype(np.int32)
    g2[g1 == 2] = 0
    g2v = rng.random(n) >= 0.1
    g3 = (rng.integers(0, BATCH, n, endpoint=True) * 3 - 7).astype(np.int64)
    g3[rng.random(n) < 0.3] = -7  # the largest group
    g3[:BATCH + 1] = (np.arange(BATCH + 1) * 3 - 7)[:n]
    g4 = rng.integers(100, 124, n, endpoint=True).astype(np.int32)
    g4[rng.random(n) < 0.2] = 100
    g4[:25] = np.arange(100, 125)[:n]
    datas = [a, tie, one, five, e, cl, g1, g2, g3, g4]
    vws = [validity_from_mask(av), validity_from_mask(tv), None, None, None, None, None, validity_from_mask(g2v), None, None]
    return datas, vws


ENCODINGS = [L.INDEX_SLICED] * 4 + [L.INDEX_RANGE, L.INDEX_SLICED] + [L.INDEX_EQUALITY] * 4


def make_main(ctx, n, seed=61):
    datas, vws = main_columns(n, seed)
    t = CubitTable(ctx, n)
    for i, (data, vw) in enumerate(zip(datas, vws)):
        t.add_column(i, data, vw)
        t.build_index(i, ENCODINGS[i])
    return t, [O.Column(x, vw) for x, vw in zip(datas, vws)], datas, vws


@pytest.fixture(scope="module")
def main(ctx):
    t, ocols, datas, vws = make_main(ctx, N)
    yield t, ocols
    t.close()


FILTERS = {
    "conjunction": (F.TableFilterSet({A: F.ConjunctionAndFilter([F.ConstantFilter(">=", 2000), F.ConstantFilter("<", 3000)]),
                                      E: F.ConjunctionAndFilter([F.ConstantFilter(">=", 3), F.ConstantFilter("<=", 7)])}), None),
    "or": (None, F.Or(F.Cmp(A, "<", 1100), F.And(F.Cmp(CL, ">", 3000), F.Cmp(E, "<", 5)), F.IsNull(T))),
    "false": (F.TableFilterSet({A: F.ConstantFilter("<", 990)}), None),
    "is_null": (F.TableFilterSet({A: F.IsNullFilter()}), None),
    "none": (None, None),
}
# group layout → (the launches of the slice path, the groups)
LAYOUTS = {"g1": ([G1], 1, 3), "g1 x g2": ([G1, G2], 2, 9), "g3": ([G3], 2, BATCH + 1), "g4": ([G4], 4, 25)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(FILTERS))
def test_every_filter_every_layout_every_path(main, name, layout):
    t, ocols = main
    fs, residual = FILTERS[name]
    by, launches, n_groups = LAYOUTS[layout]
    groups = group_rows(ocols, A, by, fs, residual, N)
    check_by(t, groups, A, by, fs, residual, what=(name, layout), launches=launches, passes=3)
    assert len(t.aggregate_groups(by)) == n_groups
    if name == "false":
        assert groups == {} and t.last_zones()[0] == 0
    if name == "is_null":  # every group: found = 0 with count_rows > 0
        got = t.quantile_by(A, 0.5, by, fs, path="slices")
        assert got and all(not s.found and s.value is None and s.count_valid == 0 < s.count_rows for s in got.values())
    if name == "none":
        assert len(groups) == (n_groups if layout != "g1 x g2" else 8)  # (2, 1) has no row
        if layout == "g1 x g2":
            assert (2, 1) not in groups and (0, None) in groups and t.aggregate_groups(by)[2] == (0, None)
        sizes = sorted(len(s) for s, _ in groups.values())
        assert sizes[0] < sizes[-1]  # so one rank is found in some groups and past the end in others


@pytest.mark.parametrize("col,passes", [(T, 2), (ONE, 1), (FIVE, 2)], ids=["ties", "one value", "five bits"])
def test_value_columns_of_other_widths(main, col, passes):
    """11 distinct values with NULLs (7 slices: chunks of 3 and 4), one distinct value (no slice, one
    pass) and 5 slices (chunks of 1 and 4), by the column with two launches."""
    t, ocols = main
    for name in ("none", "conjunction"):
        fs, residual = FILTERS[name]
        groups = group_rows(ocols, col, [G3], fs, residual, N)
        check_by(t, groups, col, [G3], fs, residual, what=(col, name), launches=2, passes=passes)
    if col == ONE:
        got = t.kth_by(ONE, 5, [G3], path="slices")
        assert all(s.value == 4242 and s.below == 0 and s.equal == s.count_valid for s in got.values())


def test_clustered_filter_skips_zones_on_both_paths(main):
    t, ocols = main
    fs = F.TableFilterSet({CL: F.ConjunctionAndFilter([F.ConstantFilter(">=", 100), F.ConstantFilter("<", 300)])})
    for col, by in ((A, [G1, G2]), (T, [G3])):
        check_by(t, group_rows(ocols, col, by, fs, None, N), col, by, fs, what=("clustered", col))
    for path in ("slices", "column"):
        skipped = t.quantile_by(A, 0.5, [G3], fs, path=path)
        ev, nz = t.last_zones()
        assert 0 < ev < nz == 4, (path, ev, nz)
        assert t.quantile_by(A, 0.5, [G3], fs, path=path, zonemap=False) == skipped
        assert t.last_zones() == (nz, nz)


def test_a_filter_that_empties_one_whole_group(main):
    t, ocols = main
    fs = F.TableFilterSet({G1: F.ConstantFilter("!=", 1), E: F.ConstantFilter("<", 9)})
    for by in ([G1], [G1, G2]):
        groups = group_rows(ocols, A, by, fs, None, N)
        assert groups and not any(k[0] == 1 for k in groups)
        check_by(t, groups, A, by, fs, what="g1 != 1")


def test_unforced_dense_filter_takes_the_slices_and_counts_a_sliced_leaf(main):
    t, ocols = main
    t.quantile_by(A, 0.5, [G4])
    assert t.last_select_grouped() == (True, 25, 4, 3)  # 25 groups in batches of 8; 12 slices, 4 per pass
    before = t.last_select()
    t.kth_by(A, 3, [G3], True, FILTERS["conjunction"][0], path="column")
    assert t.last_select_grouped() == (False, BATCH + 1, 0, ARRAY_PASSES)
    assert t.last_select() == before  # the ungrouped call's counters stay its own
    t.count(FILTERS["conjunction"][0])
    t.quantile_by(A, 0.5, [G3], FILTERS["conjunction"][0], path="column")
    column_sliced = t.last_sliced()
    t.quantile_by(A, 0.5, [G3], FILTERS["conjunction"][0], path="slices")
    assert t.last_sliced() == column_sliced + 1  # the slice path is one more sliced leaf


# ------------------------------------------------------------------ typed columns


def test_float_with_nan_and_negative_zero(ctx):
    rng = np.random.default_rng(64)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 3e38, -3e38, 1e-45], dtype=np.float32)
    f = np.where(rng.random(N) < 0.5, pool[rng.integers(0, len(pool), N)], rng.normal(0, 100, N).astype(np.float32))
    f = f.astype(np.float32)
    valid = rng.random(N) >= 0.05
    g = rng.integers(0, 4, N, endpoint=True).astype(np.int32)
    e = rng.integers(0, 10, N, endpoint=True).astype(np.int64)
    t = CubitTable(ctx, N)
    for i, (data, vw, enc) in enumerate([(f, validity_from_mask(valid), L.INDEX_SLICED), (g, None, L.INDEX_EQUALITY),
                                         (e, None, L.INDEX_RANGE)]):
        t.add_column(i, data, vw)
        t.build_index(i, enc)
    ocols = [O.Column(f, validity_from_mask(valid)), O.Column(g), O.Column(e)]
    known = {0: (float_keys(f.view(np.int32)), valid)}
    for fs in (None, F.TableFilterSet({2: F.ConstantFilter("<", 4)})):
        groups = group_rows(ocols, 0, [1], fs, None, N, known=known)
        check_by(t, groups, 0, [1], fs, zonemaps=(True,), to_value=float_value, what=("float", fs))
    top = t.kth_by(0, 0, [1], True, path="slices")
    assert all(s.value == 0x7FC00000 for s in top.values())  # NaN above +inf in every group
    t.close()


def test_ubigint_and_varchar_values_and_a_varchar_group_column(ctx):
    rng = np.random.default_rng(65)
    n = ZONE + 4_001
    u = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    u[:4] = [0, 1 << 63, (1 << 63) - 1, U64]
    uv = rng.random(n) >= 0.05
    uv[:4] = True
    pool = sorted({bytes(rng.integers(97, 123, rng.integers(1, 6)).astype(np.uint8)) for _ in range(60)})
    strs = [None if rng.random() < 0.05 else pool[i] for i in rng.integers(0, len(pool), n)]
    flags = [b"A", b"N", b"R", b"north-east"]
    gs = [None if rng.random() < 0.03 else flags[i] for i in rng.integers(0, len(flags), n)]
    t = CubitTable(ctx, n)
    t.add_column(0, u, validity_from_mask(uv))
    d1 = t.add_string_column(1, strs)
    d2 = t.add_string_column(2, gs)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    t.build_index(2, L.INDEX_EQUALITY)
    ocols = [O.Column(u, validity_from_mask(uv)), O.StringColumn(strs), O.StringColumn(gs)]
    codes1, codes2 = d1.encode(strs), d2.encode(gs)
    known = {0: ((u ^ np.uint64(1 << 63)).view(np.int64), uv), 1: codes1, 2: codes2}
    keyfn = {2: d2.entry}

    def bits(key):  # the value's bits as an int64
        return int(np.int64(key) ^ np.int64(-(1 << 63)))

    for fs in (None, F.TableFilterSet({1: F.ConstantFilter(">", pool[17])})):
        groups = group_rows(ocols, 0, [2], fs, None, n, known=known, keyfn=keyfn)
        check_by(t, groups, 0, [2], fs, zonemaps=(True,), to_value=bits, what="ubigint")
        groups = group_rows(ocols, 1, [2], fs, None, n, known=known, keyfn=keyfn)
        check_by(t, groups, 1, [2], fs, zonemaps=(True,), what="varchar")  # the values are codes
    assert t.aggregate_groups([2]) == [(f,) for f in sorted(flags)] + [(None,)]
    top = t.kth_by(0, 0, [2], True, path="slices")
    assert (None,) in top and max(bits(np.int64(s.value) ^ np.int64(-(1 << 63))) for s in top.values()) <= 0
    assert any(s.value == -1 for s in top.values())  # 2^64 - 1: unsigned order across 2^63
    t.close()


# ------------------------------------------------------------------ MVCC


def test_deletes_and_updates_of_the_value_and_a_group_column(ctx):
    rng = np.random.default_rng(66)
    b = rng.integers(-70_000, 70_000, N, endpoint=True).astype(np.int64)
    bv = rng.random(N) >= 0.05
    g = rng.integers(0, 4, N, endpoint=True).astype(np.int64)  # keys 0 ... 4, not nullable
    h = rng.integers(0, 2, N, endpoint=True).astype(np.int32)
    bw = validity_from_mask(bv)
    dels = np.arange(0, N, 7, dtype=np.int64)
    deleted = np.full(N, np.uint64(2 ** 64 - 2), dtype=np.uint64)
    deleted[dels] = 5

    def build():
        t = CubitTable(ctx, N)
        for i, (data, vw, enc) in enumerate([(b, bw, L.INDEX_SLICED), (g, None, L.INDEX_EQUALITY), (h, None, L.INDEX_EQUALITY)]):
            t.add_column(i, data, vw)
            t.build_index(i, enc)
        t.set_deletes(dels, np.full(len(dels), 5, dtype=np.uint64))
        return t

    t = build()
    ocols = [O.Column(b, bw), O.Column(g), O.Column(h)]
    fs = F.TableFilterSet({0: F.ConstantFilter(">", -10_000)})
    writer = TXN_START + 9
    txn, tx = L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted)
    w, wx = L.Txn(10, writer), O.Mvcc(10, writer, deleted=deleted)
    early, ex = L.Txn(3, TXN_START + 2), O.Mvcc(3, TXN_START + 2, deleted=deleted)
    # visible deletes: the visibility leaf is in the program, the slices stay
    for by in ([1], [1, 2]):
        chose = check_by(t, group_rows(ocols, 0, by, fs, None, N, tx), 0, by, fs, txn=txn, zonemaps=(True,), what="deletes")
        assert chose is True
    assert sum(s.count_rows for s in t.quantile_by(0, 0.5, [1], txn=txn).values()) < \
        sum(s.count_rows for s in t.quantile_by(0, 0.5, [1], txn=early).values())

    # a visible update of the value column (SET NULL among the records, values outside the slices' range)
    m = 3000
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(-80_000, 1 << 20, m).astype(np.int64)
    ok = rng.random(m) >= 0.15
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    t.set_updates(0, rows, new, vers, ok)
    ocols[0] = O.Column(b, bw, updates=(rows, new, vers, ok))
    for x, xx in ((txn, tx), (w, wx)):
        groups = group_rows(ocols, 0, [1, 2], fs, None, N, xx)
        assert max(int(s[-1]) for s, _ in groups.values()) > 70_000  # a new value above the slices' top
        chose = check_by(t, groups, 0, [1, 2], fs, txn=x, paths=[None, "column"], zonemaps=(True,), what="value updated")
        assert chose is False
        with pytest.raises(L.CubitError) as e:
            t.quantile_by(0, 0.5, [1, 2], fs, txn=x, path="slices")
        assert e.value.code == L.ERR_INVALID and b"update" in t.lib.cubit_last_error()
    chose = check_by(t, group_rows(ocols, 0, [1], fs, None, N, ex), 0, [1], fs, txn=early, zonemaps=(True,), what="invisible")
    assert chose is True  # invisible to a reader that predates them: the slices stay
    t.close()  # (after merge_updates the slice path works again: test_merge_updates_and_a_ragged_append)

    # a visible update of a group column: to an existing key, to a value the index has never seen (77,
    # the writer's own) and SET NULL on a column without NULLs
    t = build()
    ocols[0] = O.Column(b, bw)
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.integers(0, 4, m, endpoint=True).astype(np.int64)
    vers = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    new[vers == writer] = np.where(rng.random(int((vers == writer).sum())) < 0.5, 77, new[vers == writer])
    ok = rng.random(m) >= 0.1
    t.set_updates(1, rows, new, vers, ok)
    ocols[1] = O.Column(g, None, updates=(rows, new, vers, ok))
    assert t.aggregate_groups([1]) == [(0,), (1,), (2,), (3,), (4,), (77,), (None,)]
    for by in ([1], [2, 1]):
        groups = group_rows(ocols, 0, by, fs, None, N, wx)
        assert any(77 in k for k in groups) and any(None in k for k in groups)
        chose = check_by(t, groups, 0, by, fs, txn=w, paths=[None, "column"], zonemaps=(True,), what="writer")
        assert chose is False
        with pytest.raises(L.CubitError) as e:
            t.kth_by(0, 0, by, False, fs, txn=w, path="slices")
        assert e.value.code == L.ERR_INVALID
        groups = group_rows(ocols, 0, by, fs, None, N, tx)
        assert not any(77 in k for k in groups) and any(None in k for k in groups)
        chose = check_by(t, groups, 0, by, fs, txn=txn, paths=[None, "column"], zonemaps=(True,), what="reader")
        assert chose is False
        groups = group_rows(ocols, 0, by, fs, None, N, ex)
        assert not any(77 in k or None in k for k in groups)
        chose = check_by(t, groups, 0, by, fs, txn=early, zonemaps=(True,), what="early")
        assert chose is True
    t.close()


# ------------------------------------------------------------------ maintenance


def test_merge_updates_and_a_ragged_append(ctx):
    rng = np.random.default_rng(67)
    v = rng.integers(1000, 3525, N, endpoint=True).astype(np.int64)
    valid = rng.random(N) >= 0.05
    g = (rng.integers(0, BATCH, N, endpoint=True) * 3 - 7).astype(np.int64)
    t = CubitTable(ctx, N)
    t.add_column(0, v, validity_from_mask(valid))
    t.add_column(1, g)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_EQUALITY)

    def check(what):
        mid = int(np.median(v))
        ocols = [O.Column(v, validity_from_mask(valid)), O.Column(g)]
        for fs in (None, F.TableFilterSet({0: F.ConstantFilter(">", mid)})):
            check_by(t, group_rows(ocols, 0, [1], fs, None, len(v)), 0, [1], fs, zonemaps=(True,), what=what)

    check("built")
    # update records of the value column and of the group column, merged: the slice path works and agrees
    for c in (0, 1):
        rows = np.sort(rng.choice(N, N // 100, replace=False)).astype(np.int64)
        if c == 0:
            new = rng.integers(-9_000, 200_000, len(rows), endpoint=True).astype(np.int64)
            new[0] = 200_000  # above the top: slices are added
            ok = rng.random(len(rows)) >= 0.2  # SET NULL among them
            ok[0] = True
        else:
            new = (rng.integers(0, BATCH, len(rows), endpoint=True) * 3 - 7).astype(np.int64)
            ok = np.ones(len(rows), bool)
        t.set_updates(c, rows, new, np.full(len(rows), 5, np.uint64), ok)
        reader = L.Txn(10, TXN_START + 1)
        with pytest.raises(L.CubitError) as e:
            t.quantile_by(0, 0.5, [1], txn=reader, path="slices")
        assert e.value.code == L.ERR_INVALID
        t.quantile_by(0, 0.5, [1], txn=reader)
        assert not t.last_select_grouped()[0]
        assert t.merge_updates(c, 6) > 0
        assert t.quantile_by(0, 0.5, [1], txn=reader, path="slices") == t.quantile_by(0, 0.5, [1], txn=reader, path="column")
        if c == 0:
            v, valid = v.copy(), valid.copy()
            v[rows] = np.where(ok, new, 0)
            valid[rows] = ok
        else:
            g = g.copy()
            g[rows] = new
        check(("merge", c))
    assert max(s.value for s in t.kth_by(0, 0, [1], True, path="slices").values()) == 200_000
    # a ragged batch appended: the numbers follow
    n_new = 5_003
    ev = rng.integers(1000, 300_000, n_new, endpoint=True).astype(np.int64)
    ev[0] = 300_000
    eg = (rng.integers(0, BATCH, n_new, endpoint=True) * 3 - 7).astype(np.int64)
    t.append({0: ev, 1: eg})
    v, valid, g = np.concatenate([v, ev]), np.concatenate([valid, np.ones(n_new, bool)]), np.concatenate([g, eg])
    check("append")
    assert max(s.value for s in t.kth_by(0, 0, [1], True, path="slices").values()) == 300_000
    t.close()


# ------------------------------------------------------------------ refusals, shapes, a caller's stream


def test_refusals(main, ctx):
    t, _ = main
    with pytest.raises(L.CubitError) as e:  # a RANGE index, and a bit-sliced one, are no group columns
        t.quantile_by(A, 0.5, [E])
    assert e.value.code == L.ERR_UNSUPPORTED and b"column 4" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:
        t.kth_by(A, 0, [G1, T])
    assert e.value.code == L.ERR_UNSUPPORTED and b"column 1" in t.lib.cubit_last_error()
    with pytest.raises(L.CubitError) as e:
        t.quantile_by(A, 0.5, [G1, G2, G3])
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.CubitError) as e:  # the ungrouped call exists for that
        t.quantile_by(A, 0.5, [])
    assert e.value.code == L.ERR_INVALID
    for q in (float("nan"), 1.5, -0.01):
        with pytest.raises(L.CubitError) as e:
            t.quantile_by(A, q, [G1])
        assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.CubitError) as e:  # no bit-sliced index on the value column
        t.quantile_by(E, 0.5, [G1], path="slices")
    assert e.value.code == L.ERR_INVALID and b"column 4" in t.lib.cubit_last_error()
    assert t.quantile_by(E, 0.5, [G1]) == t.quantile_by(E, 0.5, [G1], path="column") and not t.last_select_grouped()[0]
    t.use_sliced(False)
    try:
        with pytest.raises(L.CubitError) as e:
            t.quantile_by(A, 0.5, [G1], path="slices")
        assert e.value.code == L.ERR_INVALID
        t.quantile_by(A, 0.5, [G1])
        assert not t.last_select_grouped()[0]
    finally:
        t.use_sliced(True)
    cols = (C.c_int * 2)(G1, G2)
    out = t.ctx.alloc(9 * 48)
    grouped = t.lib.cubit_table_select_grouped
    both = L.SELECT_FROM_SLICES | L.SELECT_FROM_COLUMN
    assert grouped(t.handle, None, 0, None, A, cols, 2, L.SELECT_RANK, 0, 0.0, 0, out.ptr, 8) == L.ERR_CAPACITY
    assert grouped(t.handle, None, 0, None, A, cols, 2, L.SELECT_RANK, 0, 0.0, both, out.ptr, 9) == L.ERR_INVALID
    assert b"both" in t.lib.cubit_last_error()
    assert grouped(t.handle, None, 0, None, A, cols, 2, L.SELECT_RANK, 0, 0.0, 8, out.ptr, 9) == L.ERR_INVALID  # flags
    assert b"flags 8" in t.lib.cubit_last_error()
    assert grouped(t.handle, None, 0, None, A, cols, 2, 3, 0, 0.0, 0, out.ptr, 9) == L.ERR_INVALID  # mode
    assert grouped(t.handle, None, 0, None, 99, cols, 2, L.SELECT_RANK, 0, 0.0, 0, out.ptr, 9) == L.ERR_INVALID
    assert grouped(t.handle, None, 0, None, A, cols, 0, L.SELECT_RANK, 0, 0.0, 0, out.ptr, 9) == L.ERR_INVALID
    assert grouped(t.handle, None, 0, None, A, None, 1, L.SELECT_RANK, 0, 0.0, 0, out.ptr, 9) == L.ERR_INVALID
    assert b"null" in t.lib.cubit_last_error()
    assert grouped(t.handle, None, 0, None, A, cols, 2, L.SELECT_RANK, 0, 0.0, 0, out.ptr, 9) == L.OK
    t.ctx.check()
    out.free()
    # more than 256 groups: 17 x 16 slots, and 257 values of one column
    rng = np.random.default_rng(68)
    n = 4_099
    u = CubitTable(ctx, n)
    for i, k in enumerate((1, 17, 16, 257)):
        data = rng.integers(0, k - 1, n, endpoint=True).astype(np.int64)
        data[:k] = np.arange(k)
        u.add_column(i, data)
        u.build_index(i, L.INDEX_SLICED if i == 0 else L.INDEX_EQUALITY)
    for by in ([1, 2], [3]):
        with pytest.raises(L.CubitError) as e:
            u.quantile_by(0, 0.5, by)
        assert e.value.code == L.ERR_UNSUPPORTED
    for path in PATHS:  # 16 x 16 slots are 256 groups; the diagonal has rows
        assert len(u.quantile_by(0, 0.5, [2, 2], path=path)) == 16
    assert u.last_select_grouped()[1] == 256
    u.close()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_tiny_and_empty_tables(ctx, n):
    t, ocols, _, _ = make_main(ctx, n)
    for col, by in ((A, [G1]), (T, [G1, G2]), (FIVE, [G3])):
        groups = group_rows(ocols, col, by, None, None, n)
        check_by(t, groups, col, by, paths=PATHS if n else [None, "column"], zonemaps=(True,), what=n)
        assert (groups == {}) == (n == 0)
    t.close()


def test_on_a_callers_stream_behind_pending_work(delayed):
    """Every call queues behind a spin on the caller's non-blocking stream: uploads, index builds and
    each batch's passes and steps must all be ordered on that stream."""
    dl = delayed()
    rng = np.random.default_rng(69)
    n = ZONE + 5_003
    a = rng.integers(-500, 3000, n, endpoint=True).astype(np.int64)
    av = rng.random(n) >= 0.1
    b = rng.integers(0, 10, n, endpoint=True).astype(np.int64)
    g = rng.integers(0, BATCH, n, endpoint=True).astype(np.int32)
    t = CubitTable(dl.ctx, n)
    t.add_column(0, a, validity_from_mask(av))
    t.add_column(1, b)
    t.add_column(2, g)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_EQUALITY)
    fs = F.TableFilterSet({1: F.ConstantFilter("<", 6)})
    mask = b < 6
    groups = {(k,): (np.sort(a[mask & av & (g == k)]), int((mask & (g == k)).sum())) for k in range(BATCH + 1)}
    for path in PATHS:
        assert t.quantile_by(0, 0.5, [2], fs, path=path) == {
            k: want(s, rows, False, quantile_rank(len(s), 0.5)) for k, (s, rows) in groups.items()}
        assert t.kth_by(0, 3, [2], True, fs, path=path) == {k: want(s, rows, True, 3) for k, (s, rows) in groups.items()}
    t.close()
