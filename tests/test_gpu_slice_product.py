"""SELECT sum(a * b), count(*) WHERE <filter> from the bit slices of both columns, against exact integers.

eval_slice_sum_product through its low-level entry point (cubit_bitslice_sum_product, on slices built by
cubit_bitslice_build) and through cubit_table_sum_product with CUBIT_SUM_FROM_SLICES / _FROM_COLUMN / no
flag. The reference everywhere is a.astype(object) * b.astype(object) (NULL → 0) summed over the rows
O.table_scan returns (or a row mask made here), as tests/test_gpu_sum_product.py does it — never the
library's other path, which is checked against the same reference. The sum is the exact two's-complement
128-bit one, so both sides are compared modulo 2^128 where the operands can leave int128.
"""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_gpu_bitslice_aggregate import offsets, pack, slices_on_device
from test_gpu_planner_fuzz import TXN_START, rand_const_filter, rand_residual
from test_gpu_sum_product import (N_C, TILE, extremes_input, force_low_word, in_int128, negative_zero_low_input,
                                  products, sparse_key, total)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
M64, M128 = 2 ** 64, 2 ** 128
U64 = M64 - 1
N_ROWS = [1, 63, 64, 65, 131_071, 131_072, 131_073]
# (n_a, n_b) over {0, 1, 7, 8, 9, 17, 64} × {0, 1, 8, 9, 64}, each pair also swapped
PAIRS = sorted({p for x in (0, 1, 7, 8, 9, 17, 64) for y in (0, 1, 8, 9, 64) for p in ((x, y), (y, x))})
assert len(PAIRS) == 45


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ A. the kernel on a caller's slices


def base_for(rng, bits):
    """A base whose range [base, base + 2^bits - 1] stays inside int64: the ends of int64, around zero."""
    top = (1 << bits) - 1
    if bits == 64:
        return I64_MIN
    return [I64_MIN, I64_MAX - top, -(1 << (bits - 1)) if bits else 7, -1][int(rng.integers(0, 4))]


class Operand:
    def __init__(self, ctx, rng, n, bits, pw):
        self.bits, self.base = bits, base_for(rng, bits)
        self.keys = (offsets(rng, n, bits) + np.uint64(self.base & U64)).view(np.int64)
        self.valid = rng.random(n) >= 0.1
        self.d_valid = ctx.upload(pack(self.valid, (n + 63) // 64))  # ceil(n / 64) words only
        d_col = ctx.upload(self.keys)
        # the slices hold the offsets of every row: a NULL row's bits must not count (V masks them)
        self.buf, self.ptrs = slices_on_device(ctx, bits, pw)
        L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, L.TYPE_INT64, None, n, self.base, bits, self.ptrs))
        ctx.check()
        d_col.free()

    def free(self):
        self.buf.free()
        self.d_valid.free()


def run_bitslice(ctx, a, b, use_va, use_vb, d_f, n, out):
    L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, 32))  # every slot must be written
    L.check(ctx.lib.cubit_bitslice_sum_product(ctx.handle, a.ptrs, a.bits, a.d_valid.ptr if use_va else None, a.base,
                                               b.ptrs, b.bits, b.d_valid.ptr if use_vb else None, b.base,
                                               d_f.ptr if d_f else None, n, out.ptr))
    ctx.check()
    lo, hi, cv, cr = (int(x) for x in out.download(np.int64, 4))
    return ((hi << 64) + (lo & U64)) % M128, cv, cr


@pytest.mark.parametrize("n", N_ROWS)
def test_bitslice_sum_product_matches_python_integers(ctx, n):
    """Every slice-count pair (0 slices, one chunk less one, a whole chunk, one more, several inner
    groups, 64 × 64) at one row, around one word and around one tile; validity on neither, one or both
    sides; the filter NULL (the zero-leaf program) or given with every bit past n_rows set."""
    rng = np.random.default_rng(5000 + n)
    pw = int(ctx.lib.cubit_padded_words(n))
    out = ctx.alloc(32)
    mask = rng.random(n) < 0.6
    mask[0] = mask[n - 1] = True
    d_mask = ctx.upload(pack(mask, pw, pad_ones=True))
    every = np.ones(n, dtype=bool)
    for n_a, n_b in PAIRS:
        a, b = Operand(ctx, rng, n, n_a, pw), Operand(ctx, rng, n, n_b, pw)
        prod = a.keys.astype(object) * b.keys.astype(object)
        for use_va in (False, True):
            for use_vb in (False, True):
                ok = (a.valid if use_va else every) & (b.valid if use_vb else every)
                for d_f, rows in ((None, every), (d_mask, mask)):
                    got = run_bitslice(ctx, a, b, use_va, use_vb, d_f, n, out)
                    sel = rows & ok
                    want = (int(prod[sel].sum()) % M128 if sel.any() else 0, int(sel.sum()), int(rows.sum()))
                    assert got == want, (n, n_a, n_b, a.base, b.base, use_va, use_vb, d_f is not None)
        a.free()
        b.free()
    d_mask.free()
    out.free()


def test_bitslice_argument_checks(ctx):
    lib, h = ctx.lib, ctx.handle
    pw = int(lib.cubit_padded_words(64))
    buf, ptrs = slices_on_device(ctx, 2, pw)
    L.check(lib.cubit_memset_d(h, buf.ptr, 0, 2 * pw * 8))
    out = ctx.alloc(32)
    odd = C.c_void_p(buf.addr + 8)
    assert lib.cubit_bitslice_sum_product(h, ptrs, 65, None, 0, ptrs, 2, None, 0, None, 64, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_sum_product(h, ptrs, 2, None, 0, ptrs, 65, None, 0, None, 64, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_sum_product(h, ptrs, 2, odd, 0, ptrs, 2, None, 0, None, 64, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_sum_product(h, ptrs, 2, None, 0, ptrs, 2, None, 0, odd, 64, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_sum_product(h, None, 2, None, 0, ptrs, 2, None, 0, None, 64, out.ptr) == L.ERR_INVALID
    # no rows: four zeros; no slices on either side: count · base_a · base_b
    L.check(lib.cubit_memset_d(h, out.ptr, 0xFF, 32))
    assert lib.cubit_bitslice_sum_product(h, ptrs, 2, None, 5, ptrs, 2, None, 7, None, 0, out.ptr) == L.OK
    ctx.check()
    assert list(out.download(np.int64, 4)) == [0, 0, 0, 0]
    assert lib.cubit_bitslice_sum_product(h, None, 0, None, -5, None, 0, None, 7, None, 64, out.ptr) == L.OK
    ctx.check()
    assert list(out.download(np.int64, 4)) == [-35 * 64, -1, 64, 64]
    buf.free()
    out.free()


# ------------------------------------------------------------------ B. the table call, tile edges and 128-bit extremes


def sliced_table(ctx, n, a, b, va=None, vb=None, key=None, row_base=7):
    """a (column 0) and b (column 1) with bit-sliced indexes, key (column 2) with an exact RANGE index."""
    t = CubitTable(ctx, n, row_base=row_base)
    vwa = validity_from_mask(va) if va is not None else None
    vwb = validity_from_mask(vb) if vb is not None else None
    t.add_column(0, a, vwa)
    t.add_column(1, b, vwb)
    t.build_index(0, L.INDEX_SLICED)
    t.build_index(1, L.INDEX_SLICED)
    ocols = [O.Column(a, vwa), O.Column(b, vwb)]
    if key is not None:
        t.add_column(2, key)
        t.build_index(2, L.INDEX_RANGE)
        ocols.append(O.Column(key))
    return t, ocols


def check_table_paths(t, ocols, n, prod, fs, row_base, paths=("slices", "column", None), what=None):
    """Every path against the exact sum over the oracle's rows; returns whether auto took the slices."""
    rows = O.table_scan(ocols, F.serialize(fs), n, row_base=row_base) - row_base
    want = (total(prod, rows) % M128, len(rows))
    auto = None
    for path in paths:
        s, c = t.sum_product(0, 1, fs, path=path)
        assert (s % M128, c) == want, (what, path)
        if not len(rows):
            continue  # (a filter folded to FALSE launches nothing)
        from_slices, launches = t.last_sum_product()
        if path == "slices":
            assert from_slices and launches == 1 and t.last_sliced() >= 2, what
        elif path == "column":
            assert not from_slices and launches == 0, what
        else:
            auto = from_slices
    return auto


@pytest.mark.parametrize("n", [1, 63, 64, 65, 131_071, 131_072, 131_073, 262_147])
def test_table_tile_edge_row_counts(ctx, n):
    """41 × 8 slices (one pass) with NULLs on both sides over a row base: the whole table, a filter
    that keeps the first and the last row, and one that keeps nothing."""
    rng = np.random.default_rng(6000 + n)
    a = rng.integers(-(2 ** 40), 2 ** 40, n).astype(np.int64)
    b = rng.integers(-100, 156, n).astype(np.int64)
    a[0], b[0] = -(2 ** 40), -100  # both bases occur: the slice counts do not depend on the draw
    va, vb = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    va[0] = vb[0] = True
    key = rng.integers(0, 4, n).astype(np.int32)
    key[0] = key[n - 1] = 0
    t, ocols = sliced_table(ctx, n, a, b, va, vb, key, row_base=2 ** 33)
    prod = products(a, b, va, vb)
    for fs in (F.TableFilterSet(), F.TableFilterSet({2: F.ConstantFilter("=", 0)}), F.TableFilterSet({2: F.ConstantFilter(">", 9)})):
        check_table_paths(t, ocols, n, prod, fs, 2 ** 33, what=(n, fs.filters))
    t.close()


def test_empty_partition(ctx):
    t, _ = sliced_table(ctx, 0, np.zeros(0, np.int64), np.zeros(0, np.int64))
    for path in (None, "column"):
        assert t.sum_product(0, 1, path=path) == (0, 0)
        assert t.last_sum_product() == (False, 0)
    t.close()


def run_slices_and_column(ctx, a, b, key, what):
    """sparse (key = 0) and dense (every row) row sets through path="slices", "column" and auto."""
    n = len(a)
    t, ocols = sliced_table(ctx, n, a, b, key=key)
    prod = products(a, b)
    for fs in (F.TableFilterSet({2: F.ConstantFilter("=", 0)}), F.TableFilterSet({2: F.ConstantFilter(">=", 0)})):
        check_table_paths(t, ocols, n, prod, fs, 7, what=(what, fs.filters))
    t.close()


def test_int128_extremes_from_slices(ctx):
    """tests/test_gpu_sum_product.py's extremes: one INT64_MIN · INT64_MIN (2^126) and the pair that
    nearly cancels it; a has 64 slices and b 32, so the forced slice path takes four inner groups."""
    rng = np.random.default_rng(128)
    a, b, at = extremes_input(rng)
    prod = products(a, b)
    assert sum(1 for p in prod if p == 2 ** 126) == 1 and sum(1 for p in prod if p == I64_MIN * I64_MAX) == 1
    run_slices_and_column(ctx, a, b, sparse_key(rng, N_C, at), "extremes")


def test_negative_total_with_zero_low_word_from_slices(ctx):
    rng = np.random.default_rng(129)
    a, b, at = negative_zero_low_input(rng)
    key = sparse_key(rng, N_C, at)
    s_rows, others = np.nonzero(key == 0)[0], np.nonzero(key != 0)[0]
    s_free = s_rows[~np.isin(s_rows, at)]
    force_low_word(a, b, [np.concatenate([s_rows[np.isin(s_rows, at)], s_free])], 0)
    force_low_word(a, b, [np.concatenate([s_rows, others])], 0)
    prod = products(a, b)
    for rows in (s_rows, np.arange(N_C)):
        w = total(prod, rows)
        assert w < 0 and w % M64 == 0 and in_int128(w), hex(w)
    run_slices_and_column(ctx, a, b, key, "negative, zero low word")


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_every_tile_sum_carries_from_slices(ctx, dense):
    """The kept rows of every tile add up to -1 (mod 2^64): on the column path every workgroup's partial
    has the low word 2^64 - 1, on the slice path the same total comes out of the three partial sums."""
    rng = np.random.default_rng(130 + dense)
    a = rng.integers(I64_MIN + 1, I64_MAX, N_C, dtype=np.int64, endpoint=True)
    b = rng.integers(-(2 ** 31) + 1, 2 ** 31, N_C).astype(np.int64)
    key = np.zeros(N_C, np.int32) if dense else sparse_key(rng, N_C, np.arange(N_C - 3, N_C))
    kept = np.nonzero(key == 0)[0]
    tiles = [kept[kept // TILE == k] for k in range(3)]
    force_low_word(a, b, tiles, M64 - 1)
    prod = products(a, b)
    assert all(total(prod, g) % M64 == M64 - 1 for g in tiles) and in_int128(total(prod, kept))
    t, ocols = sliced_table(ctx, N_C, a, b, key=key)
    check_table_paths(t, ocols, N_C, prod, F.TableFilterSet({2: F.ConstantFilter("=", 0)}), 7, what=dense)
    t.close()


# ------------------------------------------------------------------ C. differential fuzz over the planner fuzz's filters

def zero_leaf_sum(ctx, a, va, bits_a, b, vb, bits_b):
    """(sum, count_valid, count_rows) of two host columns through the kernel's zero-leaf form."""
    n = len(a)
    pw = int(ctx.lib.cubit_padded_words(n))
    out = ctx.alloc(32)
    sides = []
    for col, valid, bits in ((a, va, bits_a), (b, vb, bits_b)):
        d_col, d_valid = ctx.upload(col), ctx.upload(pack(valid, (n + 63) // 64))
        buf, ptrs = slices_on_device(ctx, bits, pw)
        base = int(col.min())
        assert int(col.max()) - base < (1 << bits)
        L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, L.TYPE_INT64, None, n, base, bits, ptrs))
        sides.append((d_col, d_valid, buf, ptrs, bits, base))
    (_, va_d, _, pa, na, ba), (_, vb_d, _, pb, nb, bb) = sides
    L.check(ctx.lib.cubit_bitslice_sum_product(ctx.handle, pa, na, va_d.ptr, ba, pb, nb, vb_d.ptr, bb, None, n, out.ptr))
    ctx.check()
    lo, hi, cv, cr = (int(x) for x in out.download(np.int64, 4))
    for d_col, d_valid, buf, *_ in sides:
        d_col.free()
        d_valid.free()
        buf.free()
    out.free()
    return (hi << 64) + (lo & U64), cv, cr


FORMS = {L.FORM_CONJ: "conj", L.FORM_DNF: "dnf", L.FORM_CNF: "cnf", L.FORM_POSTFIX: "postfix"}


def slice_product_fuzz(ctx, seed, iters):
    rng = np.random.default_rng(seed)
    n, base = 400_003, 11  # three whole tiles and a tail
    t = CubitTable(ctx, n, row_base=base)
    ocols = []
    for c in range(4):  # the planner fuzz's filter columns and index sets
        data = rng.integers(0, 50, n).astype(np.int32 if c % 2 == 0 else np.int64)
        valid = rng.random(n) > (0.15 if c != 1 else 0.0)
        vw = validity_from_mask(valid) if c != 1 else None
        t.add_column(c, data, vw)
        ocols.append(O.Column(data, vw))
    t.build_index(0, L.INDEX_RANGE)
    t.build_index(1, L.INDEX_EQUALITY)
    t.build_index(2, L.INDEX_RANGE, [10, 20, 30, 40])
    t.build_index(2, L.INDEX_BINS, [0, 10, 20, 30, 40, 50])
    # a: 41 slices from a negative base; b: 0 … 200, 8 slices (one pass: auto may take the slices), with
    # an exact RANGE index beside them so that a filter on b is decoded on the column path
    a = rng.integers(-(2 ** 40), 2 ** 40, n).astype(np.int64)
    b = rng.integers(0, 201, n).astype(np.int64)
    a[0], b[0], b[1] = -(2 ** 40), 0, 200
    va, vb = rng.random(n) > 0.15, rng.random(n) > 0.10
    for c, (d, v) in ((4, (a, va)), (5, (b, vb))):
        vw = validity_from_mask(v)
        t.add_column(c, d, vw)
        t.build_index(c, L.INDEX_SLICED)
        ocols.append(O.Column(d, vw))
    t.build_index(5, L.INDEX_RANGE)
    prod = products(a, b, va, vb)
    dels = np.arange(0, n, 7, dtype=np.int64)
    deleted = np.full(n, np.uint64(2 ** 64 - 2), dtype=np.uint64)
    deleted[dels] = 5
    tally = {"leaves": set(), "forms": set(), "auto_slices": 0, "auto_column": 0, "multipass": 0, "empty": 0, "txn": 0,
             "b_filter": 0, "skipped_zones": 0}

    def check(i, fs, residual, txn, tx):
        plan = F.serialize(fs, residual)
        rows = O.table_scan(ocols, plan, n, row_base=base, tx=tx)
        want = (total(prod, rows - base), len(rows))
        tally["empty"] += len(rows) == 0
        for path in (None, "slices", "column"):
            for z in (False, True):
                got = t.sum_product(4, 5, fs, residual, txn=txn, zonemap=z, path=path)
                assert got == want, (seed, i, "txn" if txn else "", path, z, fs.filters, plan.nodes)
                if not len(rows):
                    continue  # (a filter folded to FALSE launches nothing and reports nothing new)
                from_slices, launches = t.last_sum_product()
                assert from_slices == (launches == 1)
                if path is not None:
                    assert from_slices == (path == "slices")
                else:
                    tally["auto_slices" if from_slices else "auto_column"] += 1
                if from_slices:
                    k, passes = t.last_plan()
                    tally["leaves"].add(k)
                    tally["forms"].add(FORMS[t.last_form()] if k else "conj")
                    tally["multipass"] += passes > 1
                    ev, nz = t.last_zones()
                    tally["skipped_zones"] += ev < nz

    # K = 0: the table call's smallest program is one leaf (every row: a bitvector of ones), so the
    # zero-leaf instantiation runs on the same two columns through cubit_bitslice_sum_product, no filter
    assert zero_leaf_sum(ctx, a, va, 41, b, vb, 8) == (total(prod, np.arange(n)), int((va & vb).sum()), n)
    tally["leaves"].add(0)
    tally["forms"].add("conj")
    t.set_deletes(dels, np.full(len(dels), 5, dtype=np.uint64))
    check(-2, F.TableFilterSet(), None, None, None)  # the whole table
    check(-1, F.TableFilterSet({0: F.ConstantFilter(">", 1000)}), None, None, None)
    assert tally["empty"] == 1
    for i in range(iters):
        filters = {}
        for c in rng.choice(4, size=rng.integers(0, 4), replace=False):
            filters[int(c)] = rand_const_filter(rng)
        fs = F.TableFilterSet(filters)
        if rng.random() < 0.3:
            lo = int(rng.integers(0, 199))
            fs.push_filter(5, F.ConjunctionAndFilter([F.ConstantFilter(">=", lo),
                                                      F.ConstantFilter("<=", lo + int(rng.integers(0, 3)))]))
            tally["b_filter"] += 1
        residual = rand_residual(rng, 4) if rng.random() < 0.5 else None
        check(i, fs, residual, None, None)
        if i % 4 == 0:
            tally["txn"] += 1
            check(i, fs, residual, L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted))
    t.close()
    return tally


FUZZ_SEED, FUZZ_ITERS = 2031, 100


def test_slice_product_fuzz_matches_exact_integers(ctx):
    """Seed 2031, 100 plans (+ the whole table and a FALSE fold; 25 of them again under a transaction
    that sees deletes), each through path None / "slices" / "column" with the zonemap skip on and off.
    The tallies are asserted so that the test cannot pass vacuously: every leaf count 0 … 8 and all four
    program forms ran on the slice path, and the automatic rule took each path at least once. (The
    table call's smallest program has one leaf; K = 0 runs on the same columns through the low-level
    entry point.) Measured with this seed: leaf counts {0 … 8}, forms conj / dnf / cnf / postfix, 74
    automatic calls from the slices and 90 from the column, 87 slice-path runs of more than one pass,
    39 plans with a filter on b, 45 checks with no row."""
    tally = slice_product_fuzz(ctx, FUZZ_SEED, FUZZ_ITERS)
    print("slice product fuzz tallies:", tally)
    assert set(range(0, 9)) <= tally["leaves"], tally
    assert tally["forms"] == {"conj", "dnf", "cnf", "postfix"}, tally
    assert tally["auto_slices"] >= 5 and tally["auto_column"] >= 5, tally


# ------------------------------------------------------------------ D. what closes the slice path


def small_table(ctx, rng, n=200_003):
    a = rng.integers(-(2 ** 23), 2 ** 23, n).astype(np.int64)
    b = rng.integers(0, 11, n).astype(np.int64)
    va = rng.random(n) >= 0.05
    va[[3, 131_072, n - 1]] = True  # the rows the update tests write
    key = np.sort(rng.integers(0, 100, n)).astype(np.int32)  # clustered: a bound on it skips zones
    t, ocols = sliced_table(ctx, n, a, b, va, None, key, row_base=0)
    return t, ocols, a, b, va, key, n


@pytest.mark.parametrize("col", [0, 1], ids=["update_on_a", "update_on_b"])
def test_visible_update_closes_the_slices(ctx, col):
    rng = np.random.default_rng(77 + col)
    t, ocols, a, b, va, key, n = small_table(ctx, rng)
    rows = np.array([3, 131_072, n - 1], np.int64)
    vals = np.array([12_345, -7, 2 ** 40], np.int64)
    t.set_updates(col, rows, vals, np.array([3, 3, 3], np.uint64))
    seen = [a.copy(), b.copy()]
    seen[col][rows] = vals
    txn = L.Txn(10, TXN_START + 1)
    fs = F.TableFilterSet({2: F.ConstantFilter(">=", 0)})
    with pytest.raises(L.CubitError) as e:
        t.sum_product(0, 1, fs, txn=txn, path="slices")
    assert e.value.code == L.ERR_INVALID
    want = int(products(seen[0], seen[1], va).sum())
    for path in (None, "column"):
        assert t.sum_product(0, 1, fs, txn=txn, path=path) == (want, n), path
        assert t.last_sum_product() == (False, 0)
    # without the transaction the record is not visible: the slices answer, over the base values
    assert t.sum_product(0, 1, fs, path="slices") == (int(products(a, b, va).sum()), n)
    t.close()


def test_use_sliced_off_and_missing_index(ctx):
    rng = np.random.default_rng(79)
    t, ocols, a, b, va, key, n = small_table(ctx, rng)
    prod = products(a, b, va)
    fs = F.TableFilterSet({2: F.ConstantFilter(">=", 0)})
    assert check_table_paths(t, ocols, n, prod, fs, 0) is True  # every row of 24 × 4 slices: auto takes the slices
    t.use_sliced(False)
    try:
        assert check_table_paths(t, ocols, n, prod, fs, 0, paths=(None, "column")) is False
        with pytest.raises(L.CubitError) as e:
            t.sum_product(0, 1, fs, path="slices")
        assert e.value.code == L.ERR_INVALID
    finally:
        t.use_sliced(True)
    # both force flags together
    out = ctx.alloc(32)
    rc = t.lib.cubit_table_sum_product(t.handle, None, 0, None, 0, 1, C.c_void_p(out.addr), None,
                                       L.SUM_FROM_SLICES | L.SUM_FROM_COLUMN)
    assert rc == L.ERR_INVALID
    out.free()
    t.close()
    # a column without a sliced index: every observable of the call is today's
    t2 = CubitTable(ctx, n)
    t2.add_column(0, a, validity_from_mask(va))
    t2.add_column(1, b)
    t2.add_column(2, key)
    t2.build_index(2, L.INDEX_RANGE)
    t2.build_index(0, L.INDEX_SLICED)  # a alone is not enough
    with pytest.raises(L.CubitError) as e:
        t2.sum_product(0, 1, fs, path="slices")
    assert e.value.code == L.ERR_INVALID
    assert t2.sum_product(0, 1, fs) == (int(prod.sum()), n)
    assert t2.last_sum_product() == (False, 0) and t2.last_sliced() == 0 and t2.last_sum_decode() == 0
    t2.close()


def test_zonemap_skip_reports_fewer_zones_and_the_same_sum(ctx):
    rng = np.random.default_rng(80)
    t, ocols, a, b, va, key, n = small_table(ctx, rng)
    prod = products(a, b, va)
    fs = F.TableFilterSet({2: F.ConstantFilter("<", 20)})  # the clustered key: the second zone holds none
    rows = O.table_scan(ocols, F.serialize(fs), n)
    want = (total(prod, rows), len(rows))
    assert 0 < len(rows) < 131_072
    assert t.sum_product(0, 1, fs, path="slices") == want
    assert t.last_zones() == (1, 2) and t.last_sum_product() == (True, 1)
    assert t.sum_product(0, 1, fs, path="slices", zonemap=False) == want
    assert t.last_zones() == (2, 2)
    t.close()
