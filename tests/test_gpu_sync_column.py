"""cubit_table_sync_column: a column brought to new contents given whole (what a host engine holds
after committed UPDATEs — the values, no list of changed rows). The changed rows are found on the
GPU (column_diff_kernel), decoded into ascending row ids and merged through the update merge's
second half, so after every sync the table must stand as after cubit_table_merge_updates of one
record per changed row:

* n_changed equals numpy's count (NULL-ness differs, or valid on both sides and the stored bits
  differ; a NULL row whose slot differs but stays NULL does not count);
* the downloaded column and validity equal the new arrays (a row that became NULL holds 0, an
  unchanged NULL row keeps its old slot);
* every index leaf equals its predicate over the new column (check_index_bits, as
  test_gpu_merge_scale.py), scans equal the oracle, statistics contain the new values.

Explicit-key indexes are also compared with a second table built fresh from the new column: the
key list and every bitvector, read through save_index / read_index. Whole index files are not
compared, because a maintained index legitimately differs from a fresh one: it keeps the wider
vmin / vmax it has seen, and an every-distinct-value index keeps keys no row holds any more.
"""
import math

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, Dictionary
from oracle import oracle as O
from test_gpu_maintenance import check_index_bits, rand_filter, read_index

pytestmark = pytest.mark.gpu

N = 3 * 131_072 + 37  # more than one decode tile, a ragged last word


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def words(mask):
    return validity_from_mask(mask)


def raw_bits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def changed_rows(old, ook, new, nok):
    """The rows a sync must count: NULL-ness differs, or valid on both sides with different bits."""
    return (ook != nok) | (ook & nok & (raw_bits(old) != raw_bits(new)))


def expected_column(old, new, nok, ch):
    want = old.copy()
    want[ch] = np.where(nok[ch], new[ch], np.zeros(1, dtype=old.dtype))
    return want


def mutate(rng, old, ook, frac, lo, hi, nulls=True):
    """New contents: about `frac` of the rows given a random value of [lo, hi) (outside the old
    keys and statistics at both ends), value → NULL and NULL → value (nulls=True), NULL rows whose
    slot changes while they stay NULL, and changes in row 0, in the last row and in all 64 rows of
    one word."""
    n = len(old)
    new, nok = old.copy(), ook.copy()
    pick = rng.random(n) < frac
    new[pick] = rng.integers(lo, hi, int(pick.sum())).astype(old.dtype)
    if nulls:
        to_null = rng.random(n) < frac / 4
        nok[to_null] = False
        to_value = ~ook & (rng.random(n) < 0.3)
        nok[to_value] = True
        new[to_value] = rng.integers(lo, hi, int(to_value.sum())).astype(old.dtype)
    stay_null = ~ook & ~nok
    new[stay_null] = rng.integers(lo, hi, int(stay_null.sum())).astype(old.dtype)  # must not count
    w = 64 * 777
    for r in [0, n - 1] + list(range(w, w + 64)):
        if not ook[r]:
            nok[r] = True  # NULL -> value
        elif nok[r]:
            new[r] = old[r] + 1
    return new, nok


def column_validity(t, col):
    ids = np.arange(t.n_rows, dtype=np.int64) + t.row_base
    return t.fetch(col, ids)[1]


def check_state(t, col, want, wok, encs, tmp_path):
    """The column, its validity, every index leaf and the statistics against the expected arrays."""
    assert np.array_equal(raw_bits(t.download_column(col)), raw_bits(want)), col
    assert np.array_equal(column_validity(t, col), wok), col
    for enc in encs:
        check_index_bits(t, col, enc, want, wok, tmp_path)
    if want.dtype.kind == "i" and wok.any():
        lo, hi, has_null, _ = t.column_statistics(col)
        assert lo <= int(want[wok].min()) and hi >= int(want[wok].max()), (col, lo, hi)
        assert has_null or wok.all()


def check_scans(rng, t, cols, oks, n_random=6):
    """A range, an equality, an off-key constant, IS NULL and a conjunction over every column, then
    random filter sets, against the oracle over the expected columns."""
    ocols = [O.Column(c, words(ok) if not ok.all() else None) for c, ok in zip(cols, oks)]
    sets = [F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 10), F.ConstantFilter("<", 31)])}),
            F.TableFilterSet({0: F.ConstantFilter("=", 20)}),
            F.TableFilterSet({0: F.ConstantFilter("<", 54)}),  # no key of any index here
            F.TableFilterSet({0: F.ConstantFilter("=", -3)}),
            F.TableFilterSet({0: F.IsNullFilter()})]
    if len(cols) > 1:
        sets.append(F.TableFilterSet({0: F.ConstantFilter("<", 25), 1: F.ConstantFilter(">=", 15)}))
        sets.append(F.TableFilterSet({c: F.ConstantFilter(">", 52) for c in range(len(cols))}))
        sets.append(F.TableFilterSet({len(cols) - 1: F.IsNullFilter(), 0: F.IsNotNullFilter()}))
    for _ in range(n_random):
        sets.append(F.TableFilterSet({int(c): rand_filter(rng) for c in
                                      rng.choice(len(cols), size=rng.integers(1, len(cols) + 1), replace=False)}))
    for fs in sets:
        ref = O.table_scan(ocols, F.serialize(fs), t.n_rows, row_base=t.row_base)
        assert np.array_equal(t.scan(fs), ref), fs
        assert t.count(fs) == len(ref), fs


def same_as_fresh_build(ctx, t, col, want, wok, enc, keys, tmp_path):
    """An explicit-key index after syncs: the key list and every bitvector of a fresh build."""
    u = CubitTable(ctx, len(want), row_base=t.row_base)
    u.add_column(col, want, words(wok) if not wok.all() else None)
    u.build_index(col, enc, keys)
    a, b = tmp_path / "synced.bin", tmp_path / "fresh.bin"
    t.save_index(col, enc, a)
    u.save_index(col, enc, b)
    ia, ib = read_index(a), read_index(b)
    assert np.array_equal(ia["keys"], ib["keys"]) and np.array_equal(ia["bvs"], ib["bvs"]), (col, enc)
    u.close()


# (dtype, registered with validity, [(encoding, keys)])
FORMS = [(np.int32, True, [(L.INDEX_RANGE, None)]),
         (np.int64, True, [(L.INDEX_RANGE, [10, 20, 30, 40]), (L.INDEX_BINS, [0, 10, 20, 30, 40, 50])]),
         (np.int64, False, [(L.INDEX_EQUALITY, None)])]


def build_forms(ctx, rng, n, row_base=0):
    t = CubitTable(ctx, n, row_base=row_base)
    cols, oks = [], []
    for c, (dt, with_valid, defs) in enumerate(FORMS):
        v = rng.integers(0, 50, n).astype(dt)
        ok = rng.random(n) > 0.08 if with_valid else np.ones(n, dtype=bool)
        t.add_column(c, v, words(ok) if with_valid else None)
        for enc, keys in defs:
            t.build_index(c, enc, keys)
        cols.append(v)
        oks.append(ok)
    return t, cols, oks


@pytest.mark.parametrize("frac,row_base", [(0.01, 0), (0.10, 11)])
def test_sync_random_changes_every_form(ctx, tmp_path, frac, row_base):
    """INT32 / INT64 with NULLs and a column registered without validity, under every-value RANGE,
    explicit-key RANGE + BINS and EQUALITY indexes. At 10 % the column without validity gets its
    first NULLs (a validity is created); at 1 % it is synced with validity = None."""
    rng = np.random.default_rng(int(frac * 1000) + row_base)
    t, cols, oks = build_forms(ctx, rng, N, row_base)
    for c, (dt, with_valid, defs) in enumerate(FORMS):
        nulls = with_valid or frac > 0.05
        new, nok = mutate(rng, cols[c], oks[c], frac, -4, 56, nulls=nulls)
        ch = changed_rows(cols[c], oks[c], new, nok)
        assert ch[0] and ch[-1] and ch[64 * 777:64 * 778].all()
        got = t.sync_column(c, new, words(nok) if nulls else None)
        assert got == (int(ch.sum()), True), (c, got, int(ch.sum()))
        cols[c], oks[c] = expected_column(cols[c], new, nok, ch), nok
        check_state(t, c, cols[c], oks[c], [e for e, _ in defs], tmp_path)
        for enc, keys in defs:
            if keys is not None:
                same_as_fresh_build(ctx, t, c, cols[c], oks[c], enc, keys, tmp_path)
    check_scans(rng, t, cols, oks)
    t.close()


def test_sync_several_workgroups_and_tile_runs(ctx, tmp_path):
    """2,100,011 rows: more than one workgroup stride of the diff's words and 17 decode tiles."""
    rng = np.random.default_rng(77)
    n = 2_100_011
    old = rng.integers(0, 50, n).astype(np.int64)
    ook = rng.random(n) > 0.05
    t = CubitTable(ctx, n)
    t.add_column(0, old, words(ook))
    t.build_index(0, L.INDEX_RANGE)
    new, nok = mutate(rng, old, ook, 0.01, -4, 56)
    ch = changed_rows(old, ook, new, nok)
    assert t.sync_column(0, new, words(nok)) == (int(ch.sum()), True)
    want = expected_column(old, new, nok, ch)
    check_state(t, 0, want, nok, [L.INDEX_RANGE], tmp_path)
    check_scans(rng, t, [want], [nok], n_random=2)
    t.close()


def test_no_change_keeps_everything(ctx, tmp_path):
    """The same contents again (NULL slots differing): (0, True), the same results, and the zone
    skip of a clustered range still prunes as before: nothing was invalidated."""
    rng = np.random.default_rng(3)
    v = np.sort(rng.integers(0, 50, N)).astype(np.int64)  # clustered: zones prune
    ok = rng.random(N) > 0.05
    t = CubitTable(ctx, N)
    t.add_column(0, v, words(ok))
    t.build_index(0, L.INDEX_RANGE)
    fs = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 10), F.ConstantFilter("<", 13)])})
    before = t.scan(fs)
    live, nz = t.last_zones()
    assert live < nz
    same = v.copy()
    same[~ok] = 99  # NULL slots differ: still no change
    assert t.sync_column(0, same, words(ok)) == (0, True)
    assert t.sync_column(0, same, words(ok), max_changed=0) == (0, True)
    assert np.array_equal(t.scan(fs), before)
    assert t.last_zones() == (live, nz)
    check_state(t, 0, v, ok, [L.INDEX_RANGE], tmp_path)
    t.close()


def test_max_changed_decides(ctx, tmp_path):
    """max_changed = n_changed - 1: applied False and the table, its indexes and scans are those
    from before the call; max_changed = n_changed applies."""
    rng = np.random.default_rng(4)
    t, cols, oks = build_forms(ctx, rng, N)
    new, nok = mutate(rng, cols[1], oks[1], 0.01, -4, 56)
    ch = changed_rows(cols[1], oks[1], new, nok)
    m = int(ch.sum())
    assert t.sync_column(1, new, words(nok), max_changed=m - 1) == (m, False)
    encs = [e for e, _ in FORMS[1][2]]
    check_state(t, 1, cols[1], oks[1], encs, tmp_path)
    check_scans(rng, t, cols, oks, n_random=2)
    assert t.sync_column(1, new, words(nok), max_changed=m) == (m, True)
    cols[1], oks[1] = expected_column(cols[1], new, nok, ch), nok
    check_state(t, 1, cols[1], oks[1], encs, tmp_path)
    check_scans(rng, t, cols, oks, n_random=2)
    t.close()


def test_two_syncs_then_append_then_sync(ctx, tmp_path):
    """Two syncs in a row, then an append (capacity padding beyond n_rows) and a third sync."""
    rng = np.random.default_rng(5)
    t, cols, oks = build_forms(ctx, rng, N)
    encs = [[e for e, _ in defs] for _, _, defs in FORMS]
    for _ in range(2):
        new, nok = mutate(rng, cols[0], oks[0], 0.02, -4, 56)
        ch = changed_rows(cols[0], oks[0], new, nok)
        assert t.sync_column(0, new, words(nok)) == (int(ch.sum()), True)
        cols[0], oks[0] = expected_column(cols[0], new, nok, ch), nok
        check_state(t, 0, cols[0], oks[0], encs[0], tmp_path)
    nb = 70_001
    extra = [rng.integers(-2, 52, nb).astype(FORMS[c][0]) for c in range(3)]
    t.append({c: extra[c] for c in range(3)})
    for c in range(3):
        cols[c] = np.concatenate([cols[c], extra[c]])
        oks[c] = np.concatenate([oks[c], np.ones(nb, dtype=bool)])
    for c in (1, 2):
        new, nok = mutate(rng, cols[c], oks[c], 0.01, -6, 58, nulls=c == 1)
        ch = changed_rows(cols[c], oks[c], new, nok)
        assert ch[-1]
        assert t.sync_column(c, new, words(nok) if c == 1 else None) == (int(ch.sum()), True)
        cols[c], oks[c] = expected_column(cols[c], new, nok, ch), nok
        check_state(t, c, cols[c], oks[c], encs[c], tmp_path)
    same_as_fresh_build(ctx, t, 1, cols[1], oks[1], L.INDEX_RANGE, [10, 20, 30, 40], tmp_path)
    check_scans(rng, t, cols, oks)
    t.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("index", [None, L.INDEX_RANGE])
def test_float_patterns(ctx, dt, index):
    """FLOAT / DOUBLE compare as bit patterns: -0.0 <-> +0.0 counts and is probed back exactly,
    NaN -> value and value -> NaN; comparisons order through the key (NaN largest, -0.0 = +0.0)."""
    rng = np.random.default_rng(6)
    pool = np.array([0.0, -0.0, 1.5, -2.25, math.inf, -math.inf, math.nan, 3.0, 1e-30, 7.0], dtype=dt)
    old = pool[rng.integers(0, len(pool), N)]
    ook = rng.random(N) > 0.05
    old[:4] = np.array([0.0, -0.0, 2.0, math.nan], dtype=dt)
    ook[:4] = True
    t = CubitTable(ctx, N)
    t.add_column(0, old, words(ook))
    if index is not None:
        t.build_index(0, index)
    new, nok = old.copy(), ook.copy()
    pick = rng.random(N) < 0.02
    new[pick] = np.concatenate([pool, np.array([12345.5, -8.0], dtype=dt)])[rng.integers(0, len(pool) + 2, int(pick.sum()))]
    nok[rng.random(N) < 0.005] = False
    new[:4] = np.array([-0.0, 0.0, math.nan, 4.0], dtype=dt)
    nok[:4] = True
    ch = changed_rows(old, ook, new, nok)
    assert ch[:4].all()
    assert t.sync_column(0, new, words(nok)) == (int(ch.sum()), True)
    want = expected_column(old, new, nok, ch)
    assert t.download_column(0).view(np.uint8).tobytes() == want.view(np.uint8).tobytes()
    assert np.array_equal(column_validity(t, 0), nok)
    got, ok = t.fetch(0, np.arange(4, dtype=np.int64))
    assert ok.all() and np.array_equal(got, raw_bits(new[:4]).astype(np.int64))  # -0.0 / +0.0 / NaN as given
    ocol = O.Column(want, words(nok))
    for c in [dt(0.0), dt(math.nan), dt(12345.5), dt(-8.0), dt(math.inf), dt(1.5), dt(4.0)]:
        for cmp in ("=", "<", ">=", "!="):
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            assert np.array_equal(t.scan(fs), O.table_scan([ocol], F.serialize(fs), N)), (cmp, c)
    fs = F.TableFilterSet({0: F.IsNullFilter()})
    assert np.array_equal(t.scan(fs), np.flatnonzero(~nok))
    lo, hi, _, _ = t.column_statistics(0)
    as_float = lambda x: np.array([x], dtype=np.int64).astype(raw_bits(want).dtype).view(dt)[0]  # noqa: E731
    assert as_float(lo) == -math.inf and math.isnan(as_float(hi))
    t.close()


@pytest.mark.parametrize("index", [L.INDEX_RANGE, L.INDEX_EQUALITY])
def test_uint64_above_2_63(ctx, index):
    rng = np.random.default_rng(8)
    pool = np.array([0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 7, 2 ** 64 - 1, 12345, 2 ** 62], dtype=np.uint64)
    old = pool[rng.integers(0, len(pool), N)]
    ook = rng.random(N) > 0.05
    t = CubitTable(ctx, N)
    t.add_column(0, old, words(ook))
    t.build_index(0, index)
    new, nok = old.copy(), ook.copy()
    pick = rng.random(N) < 0.02
    new[pick] = np.concatenate([pool, np.array([2 ** 63 + 99, 5], dtype=np.uint64)])[
        rng.integers(0, len(pool) + 2, int(pick.sum()))]
    nok[rng.random(N) < 0.005] = False
    ch = changed_rows(old, ook, new, nok)
    assert t.sync_column(0, new, words(nok)) == (int(ch.sum()), True)
    want = expected_column(old, new, nok, ch)
    assert np.array_equal(t.download_column(0), want)
    assert np.array_equal(column_validity(t, 0), nok)
    ocol = O.Column(want, words(nok))
    for c in [0, 2 ** 63, 2 ** 63 + 99, 2 ** 64 - 1, 5, 2 ** 62]:
        for cmp in ("=", "<", ">=", "!="):
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            assert np.array_equal(t.scan(fs), O.table_scan([ocol], F.serialize(fs), N, 0)), (cmp, c)
    t.close()


@pytest.mark.parametrize("index", [None, L.INDEX_EQUALITY])
def test_varchar_by_codes(ctx, index):
    """A VARCHAR column synced by codes of its dictionary (Dictionary.encode); a code outside the
    dictionary is refused and leaves the table as it was."""
    rng = np.random.default_rng(9)
    pool = [b"apple", b"banana", b"cherry", b"damson", b"elder", b"fig", b"grape", b"unused"]
    n = 70_003
    vals = [pool[i] if rng.random() > 0.05 else None for i in rng.integers(0, 7, n)]
    d = Dictionary(pool)
    t = CubitTable(ctx, n)
    t.add_string_column(0, vals, d)
    if index is not None:
        t.build_index(0, index)
    new = list(vals)
    for r in rng.choice(n, 1500, replace=False):
        new[r] = pool[int(rng.integers(0, 8))] if rng.random() > 0.1 else None  # "unused" comes in
    new[0] = b"unused" if vals[0] != b"unused" else b"fig"
    codes, valid = d.encode(new)
    old_codes, old_valid = d.encode(vals)
    ch = changed_rows(old_codes, old_valid, codes, valid)
    bad = codes.copy()
    bad[0] = len(pool)
    with pytest.raises(L.CubitError):
        t.sync_column(0, bad, words(valid))
    col = O.StringColumn(vals)
    fs = F.TableFilterSet({0: F.ConstantFilter("=", b"cherry")})
    assert np.array_equal(t.scan(fs), O.table_scan([col], F.serialize(fs), n))  # untouched by the refusal
    assert np.array_equal(t.download_column(0), old_codes)
    assert t.sync_column(0, codes, words(valid)) == (int(ch.sum()), True)
    assert np.array_equal(column_validity(t, 0), valid)
    assert np.array_equal(t.download_column(0)[valid], codes[valid])
    col = O.StringColumn(new)
    for c in [b"cherry", b"unused", b"apple", b"zzz", b"b"]:
        for cmp in ("=", "<", ">=", "!="):
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            assert np.array_equal(t.scan(fs), O.table_scan([col], F.serialize(fs), n)), (cmp, c)
    assert np.array_equal(t.scan(F.TableFilterSet({0: F.IsNullFilter()})), np.flatnonzero(~valid))
    t.close()


def test_on_device_input_gives_the_same(ctx, tmp_path):
    """The new contents read in place from device memory (a DeviceBuffer, or an address with
    on_device=True) against the same sync from host arrays on a twin table."""
    rng = np.random.default_rng(10)
    old = rng.integers(0, 50, N).astype(np.int32)
    ook = rng.random(N) > 0.05
    new, nok = mutate(rng, old, ook, 0.03, -4, 56)
    ch = changed_rows(old, ook, new, nok)
    want = expected_column(old, new, nok, ch)
    results = []
    for form in ("host", "buffer", "address"):
        t = CubitTable(ctx, N)
        t.add_column(0, old, words(ook))
        t.build_index(0, L.INDEX_RANGE)
        if form == "host":
            got = t.sync_column(0, new, words(nok))
        else:
            d_new, d_ok = ctx.upload(new), ctx.upload(words(nok)[:(N + 63) // 64])
            got = (t.sync_column(0, d_new, d_ok) if form == "buffer"
                   else t.sync_column(0, d_new.addr, d_ok.addr, on_device=True))
        assert got == (int(ch.sum()), True), form
        ix = check_index_bits(t, 0, L.INDEX_RANGE, want, nok, tmp_path)
        results.append((t.download_column(0), column_validity(t, 0), ix["keys"].copy(), ix["bvs"].copy()))
        t.close()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a, b)
    assert np.array_equal(results[0][0], want) and np.array_equal(results[0][1], nok)


def test_refusals(ctx):
    """Outstanding update records, an unregistered column, a wrong dtype or length: refused, and
    the column is as it was."""
    n = 1000
    v = np.arange(n, dtype=np.int64)
    t = CubitTable(ctx, n)
    t.add_column(0, v)
    t.build_index(0, L.INDEX_RANGE, [100, 500])
    with pytest.raises(L.CubitError) as e:
        t.sync_column(7, v)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(ValueError):
        t.sync_column(0, v.astype(np.int32))
    with pytest.raises(ValueError):
        t.sync_column(0, v[:-1])
    t.set_updates(0, np.array([5], dtype=np.int64), np.array([77], dtype=np.int64), np.array([1], dtype=np.uint64))
    with pytest.raises(L.CubitError) as e:
        t.sync_column(0, v + 1)
    assert e.value.code == L.ERR_INVALID
    assert np.array_equal(t.download_column(0), v)
    assert t.merge_updates(0, 2) == 1  # merged: the sync may run again
    v[5] = 77
    assert t.sync_column(0, v) == (0, True)
    assert t.sync_column(0, v + 1) == (n, True)
    assert np.array_equal(t.download_column(0), v + 1)
    t.close()
