"""The bit-sliced index (CUBIT_INDEX_SLICED) at table level against the oracle: every column type,
constants at and around both ends of the slices' range, one-leaf intervals, narrowing, zonemaps, MVCC
updates, appends (inside the range, above the top, below the base), merges and syncs, persistence,
an empty partition, the table function and the fused sum. Every scan is also run with the slices
switched off (use_sliced(False)): the two must agree, as both must with the oracle."""
import struct

import numpy as np
import pytest

from conftest import revenue_from_answer
from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.scan_function import ROW_ID, CubitScanFunction
from cubit_amd.table import Context, CubitTable, Dictionary
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 3 * 131_072 + 37
CMPS = ["=", "!=", "<", "<=", ">", ">="]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TXN_START = 4611686018427388000
HEADER = struct.Struct("<8sIIQQIIqqQQ")  # magic, version, encoding, n_rows, nwp, exact_all, empty, vmin, vmax, n_keys, n_bv
TAIL_BYTES = 16


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def bit_length(span):
    return int(span).bit_length()


def makes_a_leaf(cmp, c, base, bits):
    """Does `v cmp c` neither miss nor cover the slices' range [base, base + 2^bits - 1]? (Then it is
    one launch over the slices; otherwise it folds to FALSE / the valid rows.)"""
    top = base + (1 << bits) - 1
    lo, hi = {"=": (c, c), "!=": (c, c), "<": (I64_MIN, c - 1), "<=": (I64_MIN, c), ">": (c + 1, I64_MAX),
              ">=": (c, I64_MAX)}[cmp]
    lo, hi = max(lo, base), min(hi, top)
    return lo <= hi and not (lo == base and hi == top)


def scan_both(t, fs, cols, n, txn=None, tx=None, zonemap=True, what=None):
    """The scan with the slices on and off, both equal to the oracle; returns last_sliced() of the first."""
    want = O.table_scan(cols, F.serialize(fs), n, 0, tx)
    t.use_sliced(True)
    got = t.scan(fs, txn=txn, zonemap=zonemap)
    k = t.last_sliced()
    assert np.array_equal(got, want), ("sliced", what)
    t.use_sliced(False)
    off = t.scan(fs, txn=txn, zonemap=zonemap)
    assert t.last_sliced() == 0
    t.use_sliced(True)
    assert np.array_equal(off, want), ("plain", what)
    return k


def int_column(rng, n, dtype, lo, hi, absent, null_frac=0.05):
    v = rng.integers(lo, hi, n, endpoint=True).astype(dtype)
    v[v == absent] = absent + 1
    v[:2] = [lo, hi]
    valid = rng.random(n) >= null_frac
    valid[:2] = True
    return v, valid


def read_index(path):
    raw = path.read_bytes()
    h = HEADER.unpack_from(raw)
    assert h[9] == 0  # no keys
    nwp, n_bv = h[4], h[10]
    words = np.frombuffer(raw, dtype=np.uint64, offset=HEADER.size + TAIL_BYTES).reshape(n_bv, nwp)
    return {"vmin": h[7], "vmax": h[8], "empty": h[6], "n_bv": n_bv, "slices": words}


def device_slices(ctx, keys, valid, base, bits):
    """cubit_bitslice_build over a column of keys uploaded here."""
    import ctypes as C

    n = len(keys)
    pw = int(ctx.lib.cubit_padded_words(n))
    d_col = ctx.upload(np.ascontiguousarray(keys))
    d_val = ctx.upload(validity_from_mask(valid))
    buf = ctx.alloc(max(bits, 1) * pw * 8)
    ptrs = (C.c_void_p * max(bits, 1))(*[buf.addr + s * pw * 8 for s in range(max(bits, 1))])
    typ = L.TYPE_INT32 if keys.dtype == np.int32 else L.TYPE_INT64
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, typ, d_val.ptr, n, base, bits, ptrs))
    ctx.check()
    return buf.download(np.uint64, max(bits, 1) * pw).reshape(-1, pw)[:bits]


# ------------------------------------------------------------------ types and constants


@pytest.mark.parametrize("dtype,lo,hi", [(np.int32, 1000, 3525), (np.int64, -5_000_000_000, 5_000_000_123)],
                         ids=["int32", "int64"])
def test_integer_columns_every_comparison_at_the_ends(ctx, dtype, lo, hi):
    rng = np.random.default_rng(7)
    absent = lo + (hi - lo) // 3
    v, valid = int_column(rng, N, dtype, lo, hi, absent)
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    bits = bit_length(hi - lo)
    n_bv, n_bytes = t.index_info(0)
    assert n_bv == bits and n_bytes >= bits * (N // 8)  # b * n_rows / 8 bytes (and the padding)
    cols = [O.Column(v, vw)]
    interior = int(v[5])
    for c in [lo - 1, lo, interior, absent, hi, hi + 1, lo + (1 << bits) - 1, lo + (1 << bits), I64_MIN, I64_MAX]:
        for cmp in CMPS:
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            scan_both(t, fs, cols, N, what=(cmp, c))
            # without the zonemaps (they skip a filter the column's min / max prove false before any
            # leaf is built) the launches are exactly the comparisons that cut the slices' range
            k = scan_both(t, fs, cols, N, zonemap=False, what=(cmp, c))
            assert k == (1 if makes_a_leaf(cmp, c, lo, bits) else 0), (cmp, c, k)
    t.close()


def test_double_columns(ctx):
    """NaN / ±inf / -0.0: the keys span all 64 bits, where the slices would move more bytes than the
    column (the byte rule leaves such a column to K0: no leaf from slices, same rows). Doubles in
    [1, 2) span 52 bits of key and are answered from the slices."""
    rng = np.random.default_rng(8)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5, 1e300, -1e300, 5e-324], dtype=np.float64)
    wide = pool[rng.integers(0, len(pool), N)]
    narrow = 1.0 + rng.random(N)
    narrow[:2] = [1.0, np.nextafter(2.0, 1.0)]
    valid = rng.random(N) >= 0.05
    valid[:2] = True
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, wide, vw)
    t.add_column(1, narrow, vw)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    assert t.index_info(0)[0] == 64 and t.index_info(1)[0] == 52
    cols = [O.Column(wide, vw), O.Column(narrow, vw)]
    for c in [np.float64(x) for x in (0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, 3.25, -1e300)]:
        for cmp in CMPS:
            assert scan_both(t, F.TableFilterSet({0: F.ConstantFilter(cmp, c)}), cols, N, what=(cmp, c)) == 0
    seen = 0
    for c in [np.float64(x) for x in (0.5, 1.0, narrow[7], 1.25, np.nextafter(2.0, 1.0), 2.0, np.nan, -np.inf, -0.0)]:
        for cmp in CMPS:
            seen += scan_both(t, F.TableFilterSet({1: F.ConstantFilter(cmp, c)}), cols, N, what=(cmp, c))
    assert seen >= 12  # the constants inside [1, 2) are launches over the slices
    t.close()


def test_ubigint_full_range_and_narrow(ctx):
    rng = np.random.default_rng(9)
    full = rng.integers(0, (1 << 64) - 1, N, dtype=np.uint64, endpoint=True)
    full[:4] = [0, 1, (1 << 64) - 2, (1 << 64) - 1]
    near = (np.uint64((1 << 63) - 500) + rng.integers(0, 1000, N).astype(np.uint64))  # straddles 2^63
    near[:2] = [(1 << 63) - 500, (1 << 63) + 499]
    valid = rng.random(N) >= 0.05
    valid[:4] = True
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, full, vw)
    t.add_column(1, near, vw)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    assert t.index_info(0)[0] == 64 and t.index_info(1)[0] == 10
    cols = [O.Column(full, vw), O.Column(near, vw)]
    for c in [0, 1, 1 << 63, (1 << 64) - 1, int(full[9]), 12345]:
        for cmp in CMPS:
            assert scan_both(t, F.TableFilterSet({0: F.ConstantFilter(cmp, c)}), cols, N, what=(cmp, c)) == 0
    seen = 0
    for c in [0, (1 << 63) - 501, (1 << 63) - 500, (1 << 63) - 1, 1 << 63, (1 << 63) + 499, (1 << 63) + 500, (1 << 64) - 1]:
        for cmp in CMPS:
            seen += scan_both(t, F.TableFilterSet({1: F.ConstantFilter(cmp, c)}), cols, N, what=(cmp, c))
    assert seen >= 12
    t.close()


def test_dictionary_column(ctx):
    rng = np.random.default_rng(10)
    pool = sorted({bytes(rng.integers(97, 123, rng.integers(1, 6)).astype(np.uint8)) for _ in range(60)})
    vals = [None if rng.random() < 0.05 else pool[i] for i in rng.integers(0, len(pool), N)]
    vals[0], vals[1] = pool[0], pool[-1]
    t = CubitTable(ctx, N)
    t.add_string_column(0, vals)
    t.build_index(0, L.INDEX_SLICED)
    assert t.index_info(0)[0] == bit_length(len(pool) - 1)
    cols = [O.StringColumn(vals)]
    seen = 0
    for c in [b"", pool[0], pool[17], pool[17] + b"\x01", pool[-1], pool[-1] + b"z", b"zzzzzzz"]:
        for cmp in CMPS:
            seen += scan_both(t, F.TableFilterSet({0: F.ConstantFilter(cmp, c)}), cols, N, what=(cmp, c))
    assert seen >= 10
    t.close()


# ------------------------------------------------------------------ intervals and interactions


def test_two_sided_range_is_one_leaf_and_range_keys_keep_their_index_leaves(ctx):
    rng = np.random.default_rng(11)
    v, valid = int_column(rng, N, np.int32, 1000, 3525, 2000)
    vw = validity_from_mask(valid)
    cols = [O.Column(v, vw)]
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    for lo, hi in [(1500, 2500), (1000, 3525), (999, 1001), (3525, 4000), (2000, 2001), (2500, 1500)]:
        fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", lo), F.ConstantFilter("<", hi)])})
        k = scan_both(t, fs, cols, N, what=(lo, hi))
        t.scan(fs)
        covers = lo <= 1000 and hi > 1000 + (1 << 12) - 1
        if lo < hi and hi > 1000 and lo <= 1000 + (1 << 12) - 1 and not covers:
            assert k == 1 and t.last_plan()[0] == 1, (lo, hi, k, t.last_plan())  # one pass over the slices, not two
        else:
            assert k == 0, (lo, hi, k)
    # three bounds and a != on the same column: the bounds fold, the != stays its own leaf
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">", 1200), F.ConstantFilter("<=", 3000),
                                                      F.ConstantFilter(">=", 1100), F.ConstantFilter("!=", 2222)])})
    assert scan_both(t, fs, cols, N) == 2
    t.close()
    # with a RANGE index on the column, key constants still take index leaves
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_RANGE, [1500, 2000, 2500, 3000])
    t.build_index(0, L.INDEX_SLICED)
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 1500), F.ConstantFilter("<", 2500)])})
    assert scan_both(t, fs, cols, N) == 0
    assert scan_both(t, F.TableFilterSet({0: F.ConstantFilter("<", 3000)}), cols, N) == 0
    t.close()


def test_narrowing_zonemaps_and_or_trees(ctx):
    rng = np.random.default_rng(12)
    a = np.sort(rng.integers(0, 4000, N).astype(np.int32))  # clustered: zones hold ranges
    b, bvalid = int_column(rng, N, np.int64, -70_000, 70_000, 11)
    c = rng.integers(0, 1000, N).astype(np.int32)
    bw = validity_from_mask(bvalid)
    t = CubitTable(ctx, N)
    t.add_column(0, a)
    t.add_column(1, b, bw)
    t.add_column(2, c)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    t.build_index(2, L.INDEX_RANGE)
    cols = [O.Column(a), O.Column(b, bw), O.Column(c)]
    sets = [
        F.TableFilterSet({0: F.ConstantFilter("<", 777), 1: F.ConstantFilter(">=", 12_345)}),
        F.TableFilterSet({2: F.ConjunctionAndFilter([F.ConstantFilter(">=", 10), F.ConstantFilter("<", 12)]),
                          1: F.ConstantFilter(">", 0), 0: F.ConstantFilter("!=", 5)}),
        F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 1000), F.ConstantFilter("<", 1100)]),
                          1: F.ConjunctionAndFilter([F.ConstantFilter(">", -100), F.ConstantFilter("<=", 100)]),
                          2: F.ConstantFilter("=", 3)}),
        F.TableFilterSet({0: F.ConjunctionOrFilter([F.ConstantFilter("<", 50), F.ConstantFilter("=", 3999),
                                                    F.ConjunctionAndFilter([F.ConstantFilter(">", 2000),
                                                                            F.ConstantFilter("<=", 2003)])]),
                          1: F.ConjunctionOrFilter([F.ConstantFilter("<", -69_000), F.IsNullFilter()])}),
    ]
    residual = F.Or(F.Cmp(0, "<", 100), F.And(F.Cmp(1, ">", 69_000), F.Cmp(2, "<", 500), F.Cmp(0, ">=", 3000)),
                    F.IsNull(1))  # a cross-column OR tree
    for i, fs in enumerate(sets):
        for narrowing in (True, False):
            t.use_narrowing(narrowing)
            for zonemap in (True, False):
                k = scan_both(t, fs, cols, N, zonemap=zonemap, what=(i, narrowing, zonemap))
                if not narrowing:
                    assert k >= 1, (i, k)
        t.use_narrowing(True)
    want = O.table_scan(cols, F.serialize(None, residual), N)
    assert np.array_equal(t.scan(None, residual), want)
    assert t.last_sliced() == 3
    t.use_sliced(False)
    assert np.array_equal(t.scan(None, residual), want)
    t.use_sliced(True)
    # clustered values: the leaf from slices keeps K0's zone statistics, so zones are still skipped
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 100), F.ConstantFilter("<", 300)])})
    assert scan_both(t, fs, cols, N) == 1
    t.scan(fs)
    ev, nz = t.last_zones()
    assert ev < nz
    t.close()


# ------------------------------------------------------------------ MVCC


def test_visible_updates_inside_and_outside_the_range(ctx):
    rng = np.random.default_rng(13)
    v, valid = int_column(rng, N, np.int32, 1000, 3525, 2000)
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    m = 3000
    rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
    new = rng.choice(np.array([1000, 2000, 2222, 3525, 999, -5, 3526, 9000, 1 << 20], dtype=np.int64), m)
    upd_valid = rng.random(m) >= 0.15  # SET NULL among them
    writer = TXN_START + 9
    versions = np.where(rng.random(m) < 0.6, 5, writer).astype(np.uint64)
    t.set_updates(0, rows, new, versions, upd_valid)
    cols = [O.Column(v, vw, updates=(rows, new, versions, upd_valid))]
    readers = [(L.Txn(3, TXN_START + 1), O.Mvcc(3, TXN_START + 1)),  # before the update: the base
               (L.Txn(10, TXN_START + 2), O.Mvcc(10, TXN_START + 2)),  # after the committed records
               (L.Txn(10, writer), O.Mvcc(10, writer))]  # the writer sees its own too
    for txn, tx in readers:
        for c in [-5, 998, 999, 1000, 2000, 2222, 3525, 3526, 5095, 5096, 9000, 1 << 20, (1 << 20) + 1]:
            for cmp in CMPS:
                scan_both(t, F.TableFilterSet({0: F.ConstantFilter(cmp, c)}), cols, N, txn=txn, tx=tx, what=(cmp, c))
        fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 900), F.ConstantFilter("<", 2223)])})
        scan_both(t, fs, cols, N, txn=txn, tx=tx)
        scan_both(t, F.TableFilterSet({0: F.IsNullFilter()}), cols, N, txn=txn, tx=tx)
    t.close()


# ------------------------------------------------------------------ append


def check_scans(t, cols, n, consts):
    for c in consts:
        for cmp in CMPS:
            scan_both(t, F.TableFilterSet({0: F.ConstantFilter(cmp, c)}), cols, n, what=(cmp, c))
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">", consts[1]), F.ConstantFilter("<", consts[-2])])})
    scan_both(t, fs, cols, n)


def test_appends_inside_above_and_below(ctx, tmp_path):
    rng = np.random.default_rng(14)
    v, valid = int_column(rng, N, np.int32, 1000, 3525, 2000)
    t = CubitTable(ctx, N)
    t.add_column(0, v, validity_from_mask(valid))
    t.build_index(0, L.INDEX_SLICED)
    # inside the range: byte-identical to a fresh build on a twin
    e1, ev1 = int_column(rng, 70_001, np.int32, 1000, 3525, 2000, null_frac=0.1)
    t.append({0: e1}, {0: validity_from_mask(ev1)})
    v, valid = np.concatenate([v, e1]), np.concatenate([valid, ev1])
    twin = CubitTable(ctx, len(v))
    twin.add_column(0, v, validity_from_mask(valid))
    twin.build_index(0, L.INDEX_SLICED)
    t.save_index(0, L.INDEX_SLICED, tmp_path / "a.cix")
    twin.save_index(0, L.INDEX_SLICED, tmp_path / "b.cix")
    assert (tmp_path / "a.cix").read_bytes() == (tmp_path / "b.cix").read_bytes()
    twin.close()
    check_scans(t, [O.Column(v, validity_from_mask(valid))], len(v), [999, 1000, 2000, 2777, 3525, 3526])
    # above the top: slices are added (12 → 17 bits)
    e2 = rng.integers(1000, 100_000, 5_003, endpoint=True).astype(np.int32)
    e2[0] = 100_000
    t.append({0: e2})
    v, valid = np.concatenate([v, e2]), np.concatenate([valid, np.ones(len(e2), bool)])
    assert t.index_info(0)[0] == bit_length(100_000 - 1000) == 17
    check_scans(t, [O.Column(v, validity_from_mask(valid))], len(v), [999, 1000, 3526, 5095, 5096, 99_999, 100_000, 100_001])
    # below the base: one rebuild
    e3 = rng.integers(-300, 4000, 4_099, endpoint=True).astype(np.int32)
    e3[0] = -300
    ev3 = rng.random(len(e3)) >= 0.2
    ev3[0] = True
    t.append({0: e3}, {0: validity_from_mask(ev3)})
    v, valid = np.concatenate([v, e3]), np.concatenate([valid, ev3])
    assert t.index_info(0)[0] == bit_length(100_000 + 300) == 17
    t.save_index(0, L.INDEX_SLICED, tmp_path / "c.cix")
    ix = read_index(tmp_path / "c.cix")
    assert (ix["vmin"], ix["vmax"]) == (-300, 100_000)
    assert np.array_equal(ix["slices"], device_slices(ctx, v, valid, -300, 17))
    check_scans(t, [O.Column(v, validity_from_mask(valid))], len(v), [-301, -300, 0, 1000, 99_999, 100_000, 100_001])
    # NULL rows only: nothing to slice, the padding they replace is already 0
    t.append({0: np.zeros(100, np.int32)}, {0: np.zeros(2, np.uint64)})
    v, valid = np.concatenate([v, np.zeros(100, np.int32)]), np.concatenate([valid, np.zeros(100, bool)])
    check_scans(t, [O.Column(v, validity_from_mask(valid))], len(v), [-301, -300, 0, 1000, 100_000, 100_001])
    t.close()


def test_empty_partition_build_append_scan(ctx):
    t = CubitTable(ctx, 0)
    t.add_column(0, np.zeros(0, np.int64))
    t.build_index(0, L.INDEX_SLICED)
    assert t.index_info(0)[0] == 0
    assert len(t.scan(F.TableFilterSet({0: F.ConstantFilter(">", 0)}))) == 0
    rng = np.random.default_rng(15)
    v = rng.integers(-40, 40, 200_003, endpoint=True).astype(np.int64)
    t.append({0: v})
    assert t.index_info(0)[0] == 7
    cols = [O.Column(v)]
    for c in [-41, -40, 0, 40, 41]:
        for cmp in CMPS:
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            scan_both(t, fs, cols, len(v), what=(cmp, c))
            k = scan_both(t, fs, cols, len(v), zonemap=False, what=(cmp, c))
            assert k == (1 if makes_a_leaf(cmp, c, -40, 7) else 0), (cmp, c, k)
    t.close()


# ------------------------------------------------------------------ merge and sync


@pytest.mark.parametrize("how", ["merge", "sync"])
def test_merge_and_sync_reslice(ctx, how, tmp_path):
    rng = np.random.default_rng(16 if how == "merge" else 17)
    v, valid = int_column(rng, N, np.int64, 1000, 3525, 2000, null_frac=0.05)
    t = CubitTable(ctx, N)
    t.add_column(0, v, validity_from_mask(valid))
    t.build_index(0, L.INDEX_SLICED)
    steps = [(1000, 3525), (1000, 70_000), (-9_000, 70_000)]  # inside; past the top; past both ends
    for step, (lo, hi) in enumerate(steps):
        m = N // 100
        rows = np.sort(rng.choice(N, m, replace=False)).astype(np.int64)
        new = rng.integers(lo, hi, m, endpoint=True).astype(np.int64)
        new[:2] = [lo, hi]
        ok = rng.random(m) >= 0.2  # value → NULL, and NULL → value where the row was NULL
        ok[:2] = True
        rows_null = np.flatnonzero(~valid)[:50]  # NULL → value for sure
        if how == "merge":
            rows = np.unique(np.concatenate([rows, rows_null]))
            new = rng.integers(lo, hi, len(rows), endpoint=True).astype(np.int64)
            ok = rng.random(len(rows)) >= 0.2
            new[:2], ok[:2] = [lo, hi], True
            ok[np.isin(rows, rows_null)] = True
            t.set_updates(0, rows, new, np.full(len(rows), 5, np.uint64), ok)
            assert t.merge_updates(0, 6) > 0
            v[rows] = np.where(ok, new, 0)
            valid[rows] = ok
        else:
            v2, valid2 = v.copy(), valid.copy()
            v2[rows_null], valid2[rows_null] = lo + 1, True
            v2[rows], valid2[rows] = new, ok
            n_changed, applied = t.sync_column(0, v2, validity_from_mask(valid2))
            assert applied and n_changed > 0
            v, valid = v2, valid2
        t.save_index(0, L.INDEX_SLICED, tmp_path / f"{how}{step}.cix")
        ix = read_index(tmp_path / f"{how}{step}.cix")
        bits = ix["n_bv"]
        assert ix["vmin"] == min(lo, 1000) and ix["vmax"] == hi and bits == bit_length(ix["vmax"] - ix["vmin"])
        assert np.array_equal(ix["slices"], device_slices(ctx, v, valid, ix["vmin"], bits)), (how, step)
        cols = [O.Column(v, validity_from_mask(valid))]
        check_scans(t, cols, N, [lo - 1, lo, 2000, 3525, 3526, hi, hi + 1])
    t.close()


# ------------------------------------------------------------------ persistence


def test_save_load_and_refusals(ctx, tmp_path):
    rng = np.random.default_rng(18)
    v, valid = int_column(rng, N, np.int32, 1000, 3525, 2000)
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    path = tmp_path / "s.cix"
    t.save_index(0, L.INDEX_SLICED, path)
    ix = read_index(path)
    assert (ix["vmin"], ix["vmax"], ix["n_bv"]) == (1000, 3525, 12)
    twin = CubitTable(ctx, N)
    twin.add_column(0, v, vw)
    twin.load_index(0, path)
    assert twin.index_info(0) == t.index_info(0)
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 1234), F.ConstantFilter("<", 2345)])})
    assert scan_both(twin, fs, [O.Column(v, vw)], N) == 1
    twin.save_index(0, L.INDEX_SLICED, tmp_path / "t.cix")
    assert (tmp_path / "t.cix").read_bytes() == path.read_bytes()
    # re-registering the column drops the index
    twin.add_column(0, v, vw)
    assert twin.index_info(0) == (0, 0)
    with pytest.raises(L.CubitError):
        twin.save_index(0, L.INDEX_SLICED, tmp_path / "none.cix")
    size = CubitTable(ctx, N - 1)
    size.add_column(0, v[:-1])
    typ = CubitTable(ctx, N)
    typ.add_column(0, v.astype(np.int64))
    for other in (size, typ):
        with pytest.raises(L.CubitError):
            other.load_index(0, path)
    # a hand-truncated n_bv: the count no longer is the bit length of vmax - vmin
    raw = bytearray(path.read_bytes())
    h = list(HEADER.unpack_from(raw))
    h[10] -= 1
    HEADER.pack_into(raw, 0, *h)
    (tmp_path / "short.cix").write_bytes(bytes(raw))
    with pytest.raises(L.CubitError):
        t.load_index(0, tmp_path / "short.cix")
    # n = 0 only, and the quantile form keeps refusing it
    with pytest.raises(L.CubitError):
        t.build_index(0, L.INDEX_SLICED, [1, 2])
    with pytest.raises(L.CubitError):
        t.build_index_quantiles(0, 8, L.INDEX_SLICED)
    # a dictionary column's file names its dictionary
    pool = [b"a", b"b", b"c", b"d", b"e"]
    vals = [pool[i] for i in rng.integers(0, 5, 1000)]
    vals[0], vals[1] = pool[0], pool[4]
    d = Dictionary(pool)
    s1 = CubitTable(ctx, 1000)
    s1.add_string_column(0, vals, d)
    s1.build_index(0, L.INDEX_SLICED)
    s1.save_index(0, L.INDEX_SLICED, tmp_path / "d.cix")
    s2 = CubitTable(ctx, 1000)
    s2.add_string_column(0, vals, Dictionary(pool + [b"f"]))
    with pytest.raises(L.CubitError):
        s2.load_index(0, tmp_path / "d.cix")
    s3 = CubitTable(ctx, 1000)
    s3.add_string_column(0, vals, d)
    s3.load_index(0, tmp_path / "d.cix")
    assert s3.index_info(0)[0] == 3
    for x in (t, twin, size, typ, s1, s2, s3):
        x.close()


# ------------------------------------------------------------------ table function and fused sum


def test_table_function_over_a_sliced_column(ctx):
    from test_gpu_scan_function import drain, ordered

    rng = np.random.default_rng(19)
    v, valid = int_column(rng, N, np.int32, 1000, 3525, 2000)
    vw = validity_from_mask(valid)
    t = CubitTable(ctx, N)
    t.add_column(0, v, vw)
    t.build_index(0, L.INDEX_SLICED)
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 1500), F.ConstantFilter("<", 1600)])})
    fn = CubitScanFunction(t, [ROW_ID, 0], [0, 1], fs)
    chunks = drain(fn, 4)
    fn.close()
    keep = O.table_scan([O.Column(v, vw)], F.serialize(fs), N)
    assert np.array_equal(ordered(chunks, 0), keep)
    assert np.array_equal(ordered(chunks, 1), v[keep])
    t.close()


def test_q6_fused_sum_with_shipdate_sliced_only(ctx, li001, golden):
    li = li001
    t = CubitTable(ctx, li.n_rows)
    t.add_column(0, li.l_shipdate)
    t.add_column(1, li.l_discount)
    t.add_column(2, li.l_quantity)
    t.add_column(3, li.l_extendedprice)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE)
    rev, n = t.sum_product(3, 1, F.q6_filter_set())
    assert t.last_sliced() >= 1
    assert rev == revenue_from_answer(golden["tpch"]["q6_revenue"]["0.01"]["revenue"])
    assert n == 1191
    t.close()
