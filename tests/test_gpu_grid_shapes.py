"""The tile-walking kernels with several tiles per workgroup and with more than 64 workgroups.

Every slice-answered kernel, the fused filter+SUM, the quantile histogram and the decode kernels walk
their tiles with a persistent grid sized by the device's compute units. On a 256-CU device a table of a
few tiles gives every workgroup one tile, so the accumulators carried across the tile loop, tile_at()
over a live-tile list, the uneven shares of tiles % grid != 0 and the finishing kernels' strided folds
over more than 64 partials never run in the other test modules. cubit_ctx_set_compute_units lowers the
count the launchers see, and cubit_ctx_last_grid reports the workgroups and tiles a launch used, so each
test here proves the regime it ran in:

  A  5 * 131,072 + 37 rows (six tiles, the last of 37 rows) with the count at 1, 2 and 3: six, three and
     two tiles per workgroup for the one-workgroup-per-CU kernels (the grouped ones), and three each, then
     shares of 2 / 2 / 1 / 1, then one each for the two-per-CU kernels.
  B  70 * 131,072 + 37 rows (71 tiles) with the override off (71 workgroups: the finishing lanes 0 … 6 fold
     two partials) and at 33 (33 workgroups of two or three tiles, or 66 workgroups, five with two).
  C  the fused sum, the quantile histogram and the decode kernels at A's shape; the decode at 8 tiles
     through the capped, pair and one-per-tile regimes of its grid rule.
  D  the setting itself.

Expected values are the exact references of the modules whose checkers run here — O.table_scan / O.fetch
for the rows, Python integers for the sums, np.sort for the ranks — and every call runs with the override
off as well, against the same reference. A kernel counts as seen in a regime only on a forced "slices"
call that launched, from what last_grid() reports; top_n's last launch is the decode of its rows, so its
select is not counted. The last test asserts that every kernel was seen in both regimes.

The caps kAggMaxGrid (1,024 workgroups) and kProductMaxGrid (731) stay unreached: a 256-CU device launches
512 workgroups at most and the override only lowers, so the static_asserts on the workspaces remain the
only guard of those two."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, runs_in_row_order
from oracle import oracle as O
import test_gpu_bitslice_aggregate as raw_aggregate
import test_gpu_bitslice_select as raw_select
import test_gpu_bitslice_select_grouped as raw_select_grouped
import test_gpu_row_lists as row_lists
from test_gpu_caller_stream import scan_tiles
from test_gpu_group_aggregate import check_groups
from test_gpu_index_quantiles import expected_keys
from test_gpu_slice_product import Operand, check_table_paths, run_bitslice
from test_gpu_slice_product_grouped import check_groups as check_product_groups
from test_gpu_slice_product_grouped import expected as product_expected
from test_gpu_sum_product import packed_pieces, products, total
from test_gpu_table_aggregate import check_paths
from test_gpu_table_select import check_select, oracle_keys, top_n_expected, want
from test_gpu_table_select_grouped import check_by, group_rows

pytestmark = pytest.mark.gpu

ZONE = 131_072
N_A = 5 * ZONE + 37
N_B = 70 * ZONE + 37
M128 = 2 ** 128
TXN_START = 4611686018427388000
V, W, Z = 0, 1, 2          # the 40-bit value column, the 20-bit second operand, the one-valued column
F0 = 3                     # f0 … f7: the filter columns
G9, GN, POS = 11, 12, 13   # the group columns (9 values; 3 values, nullable) and the row's tile
N_COLS = 14
CUS_A = [1, 2, 3]
CU_B = 33
# workgroups per CU of each kernel's launcher (slice_grid's wpc)
WPC = {"aggregate": 2, "select": 2, "sum_product": 2, "aggregate_by": 1, "select_by": 1, "sum_product_by": 1,
       "raw_aggregate": 2, "raw_select": 2, "raw_sum_product": 2, "raw_select_grouped": 1}
METHODS = {"aggregate": "aggregate", "kth": "select", "quantile": "select", "aggregate_by": "aggregate_by",
           "kth_by": "select_by", "quantile_by": "select_by", "sum_product": "sum_product",
           "sum_product_by": "sum_product_by"}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_compute_units(0)
    c.set_decode_kernel(L.DECODE_AUTO)
    c.close()


@pytest.fixture(autouse=True)
def device_settings(ctx):
    """Every test starts and ends with the device's own count and the automatic decode policy."""
    ctx.set_compute_units(0)
    ctx.set_decode_kernel(L.DECODE_AUTO)
    yield
    ctx.set_compute_units(0)
    ctx.set_decode_kernel(L.DECODE_AUTO)


@pytest.fixture(scope="module")
def tally():
    """kernel -> the regimes ("A": tiles > workgroups, "B": workgroups > 64) its launches were seen in."""
    return {k: set() for k in WPC}


def regimes(wg, tiles):
    return ({"A"} if tiles > wg else set()) | ({"B"} if wg > 64 else set())


def qualifying(result):
    """The qualifying rows a table call reported: 0 means it may have launched nothing."""
    if isinstance(result, dict):
        return sum(r.count_rows if hasattr(r, "count_rows") else r[2] for r in result.values())
    return result.count_rows if hasattr(result, "count_rows") else result[1]


class Watched:
    """A CubitTable whose slice-answered calls are followed by a look at the launch: on a forced "slices"
    call that found rows, last_grid() must name the live tiles and min(tiles, wpc * compute units)
    workgroups, and the regime goes to the tally and to `seen` (this table's own)."""

    def __init__(self, t, ctx, tally):
        self._t, self._ctx, self._tally = t, ctx, tally
        self.seen = {k: set() for k in WPC}
        self.slices_calls = 0

    def __getattr__(self, name):
        attr = getattr(self._t, name)
        kernel = METHODS.get(name)
        if kernel is None:
            return attr

        def call(*args, **kwargs):
            result = attr(*args, **kwargs)
            if kwargs.get("path") == "slices" and qualifying(result):
                wg, tiles = self._ctx.last_grid()
                live, zones = self._t.last_zones()
                cu = self._ctx.compute_units()[1]
                assert tiles == live <= zones, (name, wg, tiles, live, zones)
                assert wg == min(tiles, WPC[kernel] * cu), (name, wg, tiles, cu)
                self.slices_calls += 1
                self.seen[kernel] |= regimes(wg, tiles)
                self._tally[kernel] |= regimes(wg, tiles)
            return result

        return call


def note_raw(ctx, tally, kernel, n):
    """After a raw cubit_bitslice_* call over n rows: every tile, min(tiles, wpc * compute units) workgroups."""
    wg, tiles = ctx.last_grid()
    assert tiles == (n + ZONE - 1) // ZONE, (kernel, wg, tiles)
    assert wg == min(tiles, WPC[kernel] * ctx.compute_units()[1]), (kernel, wg, tiles)
    tally[kernel] |= regimes(wg, tiles)
    return regimes(wg, tiles)


# ------------------------------------------------------------------ the tables


def spread(rng, n, dtype, lo, hi, null_frac):
    """Values strictly inside (lo, hi): a test places the extremes itself."""
    v = rng.integers(lo + 1000, hi - 1000, n).astype(dtype)
    return v, rng.random(n) >= null_frac


class Data:
    """The host arrays of a table and the oracle's columns over them.

    late=False (part A): f0 … f7 over 0 … 9 with every-value indexes (RANGE on the even ones, EQUALITY on
    the odd ones), the tiles 1 and 3 of f0 holding 7 … 9 only (f0 <= 6 is dead there: a live-tile list of
    four, {0, 2, 4, 5}); the value column's extremes in its first two rows.
    late=True (part B): f0 over 0 … 9 and f1 over 0 … 999 with a RANGE key at 1 (f1 < 1: one row in a
    thousand); the value column's minimum in tile 65 and its maximum in tile 69, group 8 of g9 in tiles 65 and
    67 only — all of them on rows both filters keep."""

    def __init__(self, n, seed, late):
        rng = np.random.default_rng(seed)
        self.n, self.late = n, late
        lo, hi = -(2 ** 39), 2 ** 39 + 123
        v, vv = spread(rng, n, np.int64, lo, hi, 0.10)
        w, wv = spread(rng, n, np.int64, -300_000, 700_000, 0.05)  # (sum_product takes INT64 operands)
        g9 = rng.integers(0, 8 if late else 9, n).astype(np.int32)
        gn = rng.integers(5, 8, n).astype(np.int32)
        gnv = rng.random(n) >= 0.1
        fs = [rng.integers(0, 10, n).astype(np.int32) for _ in range(2 if late else 8)]
        if late:
            fs[1] = rng.integers(0, 1000, n).astype(np.int32)
            self.at_min, self.at_max = 65 * ZONE + 5, 69 * ZONE + 77
            self.only8 = np.concatenate([65 * ZONE + 100 + 7 * np.arange(300), 67 * ZONE + 11 * np.arange(300)])
            special = np.concatenate([[self.at_min, self.at_max], self.only8])
            g9[self.only8] = 8
            fs[0][special] = 0
            fs[1][special] = 0
        else:
            self.at_min, self.at_max = 0, 1
            special = np.array([0, 1])
            for tile in (1, 3):
                fs[0][tile * ZONE:(tile + 1) * ZONE] = rng.integers(7, 10, ZONE)
            for i, f in enumerate(fs):
                f[:10] = np.roll(np.arange(10), i)  # every value in every column: no literal folds away
        v[self.at_min], v[self.at_max] = lo, hi
        vv[special] = True
        wv[special] = True
        self.v, self.vv, self.w, self.wv, self.g9 = v, vv, w, wv, g9
        z, zv = np.full(n, 42, dtype=np.int64), rng.random(n) >= 0.05
        pos = (np.arange(n) // ZONE).astype(np.int32)
        self.cols = {V: (v, validity_from_mask(vv), L.INDEX_SLICED, None),
                     W: (w, validity_from_mask(wv), L.INDEX_SLICED, None),
                     G9: (g9, None, L.INDEX_EQUALITY, None),
                     GN: (gn, validity_from_mask(gnv), L.INDEX_EQUALITY, None)}
        if late:
            self.cols[F0] = (fs[0], None, L.INDEX_RANGE, None)
            self.cols[F0 + 1] = (fs[1], None, L.INDEX_RANGE, [1])
        else:
            self.cols[Z] = (z, validity_from_mask(zv), L.INDEX_SLICED, None)
            self.cols[POS] = (pos, None, L.INDEX_EQUALITY, None)
            for i, f in enumerate(fs):
                self.cols[F0 + i] = (f, None, L.INDEX_RANGE if i % 2 == 0 else L.INDEX_EQUALITY, None)
        self.ocols = [O.Column(np.zeros(1, np.int32))] * N_COLS  # (unregistered ids: never read)
        for c, (data, vw, _, _) in self.cols.items():
            self.ocols[c] = O.Column(data, vw)
        self.dels = np.arange(0, n, 7, dtype=np.int64)  # every 7th row, deleted at version 5
        self.deleted = np.full(n, np.uint64(2 ** 64 - 2), dtype=np.uint64)
        self.deleted[self.dels] = 5

    def reader(self):
        return L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=self.deleted)

    def ids(self, fs, residual, tx=None):
        return O.table_scan(self.ocols, F.serialize(fs, residual), self.n, 0, tx)

    def upload(self, ctx, row_base=0):
        t = CubitTable(ctx, self.n, row_base=row_base)
        for c, (data, vw, enc, keys) in self.cols.items():
            t.add_column(c, data, vw)
            t.build_index(c, enc, keys)
        t.set_derived_budget(0)
        t.set_derived_chain_cost(2 ** 64 - 1)  # a repeated filter stays its leaves
        if not self.late:  # seen by a transaction only
            t.set_deletes(self.dels, np.full(len(self.dels), 5, dtype=np.uint64))
        return t


class LazyProducts:
    """products(v, w) at the rows asked for: total(prod, rows) of a 9 M-row table without 9 M Python ints."""

    def __init__(self, d):
        self.d = d

    def __getitem__(self, idx):
        d = self.d
        return products(d.v[idx], d.w[idx], d.vv[idx], d.wv[idx])


@pytest.fixture(scope="module")
def small():
    return Data(N_A, 91, late=False)


@pytest.fixture(scope="module")
def table_a(ctx, small):
    t = small.upload(ctx)
    yield t
    t.close()


@pytest.fixture(scope="module")
def table_a_based(ctx, small):
    t = small.upload(ctx, row_base=2 ** 33 + 5)
    yield t
    t.close()


@pytest.fixture(scope="module")
def big(ctx):
    """Part B's table, built once: 9.2 M rows."""
    if ctx.compute_units()[0] < 71:
        pytest.skip(f"a device of {ctx.compute_units()[0]} compute units launches no 71 workgroups")
    d = Data(N_B, 92, late=True)
    t = d.upload(ctx)
    yield d, t
    t.close()


# ------------------------------------------------------------------ part A's filters


def lit(kind, i):
    """D_i ("dense"): f_i <= 6 on an even column, f_i != 3 on an odd one; S_i ("sparse"): f_i <= 1 / f_i = 3."""
    op, c = {("D", 0): ("<=", 6), ("D", 1): ("!=", 3), ("S", 0): ("<=", 1), ("S", 1): ("=", 3)}[(kind, i & 1)]
    return F.Cmp(F0 + i, op, c)


def pairs(*ij):
    return F.Or(*[F.And(lit("D", i), lit("S", j)) for i, j in ij])


ONE = F.TableFilterSet({F0 + 2: F.ConstantFilter("<=", 6)})
# name -> (pushed filters, residual, under the reader that sees the delete list, live tiles with the zonemap on)
FILTERS_A = {
    "none": (None, None, False, 6),                                    # the zero-leaf program
    "one_leaf": (ONE, None, False, 6),
    "six_leaves": (None, pairs((2, 3), (4, 5), (6, 7)), False, 6),     # an OR of three ANDs
    "two_passes": (None, pairs((0, 1), (2, 3), (4, 5), (6, 7), (2, 5)), False, 6),  # ten leaves: a part is kept first
    "dead_zone": (F.TableFilterSet({F0: F.ConstantFilter("<=", 6)}), None, False, 4),
    "last_tile": (F.TableFilterSet({POS: F.ConstantFilter("=", 5)}), None, False, 1),
    "mvcc": (ONE, None, True, 6),
}
PUSHED_A = [k for k, f in FILTERS_A.items() if f[1] is None]  # (the product checkers take pushed filters only)


def case_a(small, name):
    fs, residual, mvcc, live = FILTERS_A[name]
    txn, tx = small.reader() if mvcc else (None, None)
    return fs, residual, txn, tx, live


def test_part_a_filters_are_what_they_claim(small):
    """On the reference alone: the dead-zone filter has rows in the tiles 0, 2, 4 and 5 only, the last-tile
    filter in the 37-row tail only, every other one in all six; the reader sees fewer rows."""
    for name in FILTERS_A:
        fs, residual, txn, tx, live = case_a(small, name)
        ids = small.ids(fs, residual, tx)
        tiles = sorted(set((ids // ZONE).tolist()))
        assert tiles == {6: [0, 1, 2, 3, 4, 5], 4: [0, 2, 4, 5], 1: [5]}[live], (name, tiles)
        assert len(ids) == 37 if name == "last_tile" else len(ids) > 1000 * live, name
    assert len(small.ids(ONE, None, small.reader()[1])) < len(small.ids(ONE, None))
    assert not (small.ids(ONE, None, small.reader()[1]) % 7 == 0).any()


def reached(w, kernel, cu):
    """Whether a part A test saw `kernel` with several tiles per workgroup: it has to, except where the
    override leaves the two-per-CU kernels a workgroup per tile (3 compute units, six tiles)."""
    if cu * WPC[kernel] >= 6:
        assert "A" not in w.seen[kernel]
    else:
        assert "A" in w.seen[kernel], (kernel, cu, w.seen)


def both_settings(ctx, cu):
    """The override off, then on: every checker compares both with the same exact reference."""
    for units in (0, cu):
        ctx.set_compute_units(units)
        yield units
    ctx.set_compute_units(0)


# ------------------------------------------------------------------ A. several tiles per workgroup


@pytest.mark.parametrize("cu", CUS_A)
def test_a_aggregate(ctx, tally, small, table_a, cu):
    w = Watched(table_a, ctx, tally)
    for _ in both_settings(ctx, cu):
        for name in FILTERS_A:
            fs, residual, txn, tx, live = case_a(small, name)

            def after(path):
                if path == "slices" and name == "two_passes":
                    assert table_a.last_plan()[1] >= 2, table_a.last_plan()

            for zm in (True, False):
                for ops in (L.AGG_SUM, L.AGG_MIN | L.AGG_MAX, L.AGG_ALL):
                    check_paths(w, small.ocols, V, L.TYPE_INT64, N_A, fs, residual, txn=txn, tx=tx, ops=ops, zonemap=zm,
                                paths=["slices"], what=(name, cu, zm), after=after)
                    assert table_a.last_zones() == (live if zm else 6, 6), (name, zm)
                check_paths(w, small.ocols, V, L.TYPE_INT64, N_A, fs, residual, txn=txn, tx=tx, zonemap=zm, paths=[None],
                            what=(name, cu, zm))
            if name in ("none", "dead_zone"):  # no slice at all: sum = count * base
                check_paths(w, small.ocols, Z, L.TYPE_INT64, N_A, fs, residual, paths=["slices", None], what=(name, cu, "z"))
    reached(w, "aggregate", cu)


@pytest.mark.parametrize("cu", CUS_A)
@pytest.mark.parametrize("name", list(FILTERS_A))
def test_a_aggregate_by(ctx, tally, small, table_a, cu, name):
    """One group column (nine groups: two launches of the SUM kernel, 8 a batch, three of the MIN / MAX
    one, 4 a batch) and two, one of them nullable (36 slots), with the zonemap off."""
    w = Watched(table_a, ctx, tally)
    fs, residual, txn, tx, live = case_a(small, name)
    for _ in both_settings(ctx, cu):
        for ops in (L.AGG_SUM, L.AGG_ALL):
            check_groups(w, small.ocols, V, L.TYPE_INT64, [G9], N_A, fs, residual, txn=txn, tx=tx, ops=ops,
                         paths=["slices"], what=(name, cu))
            assert table_a.last_grouped()[2] >= 2 or name == "last_tile"
        check_groups(w, small.ocols, V, L.TYPE_INT64, [G9, GN], N_A, fs, residual, txn=txn, tx=tx, zonemap=False,
                     paths=["slices", None], what=(name, cu, "two columns, no zonemap"))
    reached(w, "aggregate_by", cu)


@pytest.mark.parametrize("cu", CUS_A)
def test_a_select_and_top_n(ctx, tally, small, table_a, table_a_based, cu):
    """quantile and kth over 41 slices (eleven passes), and top_n on a table whose row ids start past 2^33."""
    w = Watched(table_a, ctx, tally)
    base = table_a_based.row_base
    for _ in both_settings(ctx, cu):
        for name in FILTERS_A:
            fs, residual, txn, tx, live = case_a(small, name)
            s, rows = oracle_keys(small.ocols, V, fs, residual, N_A, tx)
            m = len(s)
            def after(path, zm):
                if path == "slices":
                    assert table_a.last_select() == (True, 11), table_a.last_select()
                    assert table_a.last_zones() == (live if zm else 6, 6), (name, zm)

            check_select(w, s, rows, V, fs, residual, txn=txn, paths=["slices", None], ranks=sorted({0, m // 2, m - 1, m}),
                         quantiles=[0.0, 0.5], what=(name, cu), after=after)
            if name in ("none", "dead_zone"):
                sz, rz = oracle_keys(small.ocols, Z, fs, residual, N_A, tx)
                check_select(w, sz, rz, Z, fs, residual, paths=["slices"], zonemaps=(True,), ranks=[0, len(sz)],
                             quantiles=[0.5], what=(name, cu, "z"))
            # top-N rows: the select, then the decode of the rows up to the value, over a row base
            ids = O.table_scan(small.ocols, F.serialize(fs, residual), N_A, base, tx)
            vals, ok = O.fetch(small.ocols[V], ids, base, tx, with_valid=True)
            for desc in (False, True) if txn is None else ():  # (the delete list is the other table's)
                want_ids, want_vals = top_n_expected(ids[ok], np.ascontiguousarray(vals[ok]).astype(np.int64), 1500, desc)
                for path in ("slices", None):
                    got_ids, got_vals, sel = table_a_based.top_n(V, 1500, desc, fs, residual, txn=txn, path=path)
                    assert np.array_equal(got_ids, want_ids), (name, cu, desc, path)
                    assert np.array_equal(got_vals, want_vals), (name, cu, desc, path)
                    assert sel == want(s, rows, desc, 1499), (name, cu, desc, path)
    reached(w, "select", cu)


@pytest.mark.parametrize("cu", CUS_A)
@pytest.mark.parametrize("name", ["none", "six_leaves", "two_passes", "dead_zone", "last_tile", "mvcc"])
def test_a_select_by(ctx, tally, small, table_a, cu, name):
    """quantile_by and kth_by: nine groups are two launches of eight; two group columns with the zonemap on."""
    w = Watched(table_a, ctx, tally)
    fs, residual, txn, tx, live = case_a(small, name)
    for _ in both_settings(ctx, cu):
        groups = group_rows(small.ocols, V, [G9], fs, residual, N_A, tx)
        check_by(w, groups, V, [G9], fs, residual, txn=txn, paths=["slices", None], what=(name, cu),
                 launches=2 if live > 1 else None, passes=11)
        if name in ("none", "dead_zone"):
            groups = group_rows(small.ocols, V, [G9, GN], fs, residual, N_A, tx)
            check_by(w, groups, V, [G9, GN], fs, residual, paths=["slices"], zonemaps=(True,), what=(name, cu, "two"))
    if live > 1:
        reached(w, "select_by", cu)


@pytest.mark.parametrize("cu", CUS_A)
def test_a_sum_product(ctx, tally, small, table_a, table_a_based, cu):
    """sum(v * w) from both columns' slices: pushed filters through check_table_paths (on the table with a
    row base too), the residual trees, the reader and the zonemap-off runs directly."""
    w, wb = Watched(table_a, ctx, tally), Watched(table_a_based, ctx, tally)
    prod = products(small.v, small.w, small.vv, small.wv)
    for _ in both_settings(ctx, cu):
        for name in PUSHED_A:
            fs = FILTERS_A[name][0] or F.TableFilterSet()
            if not FILTERS_A[name][2]:
                check_table_paths(w, small.ocols, N_A, prod, fs, 0, paths=("slices", None), what=(name, cu))
                check_table_paths(wb, small.ocols, N_A, prod, fs, table_a_based.row_base, paths=("slices",), what=(name, cu))
        for name in FILTERS_A:
            fs, residual, txn, tx, live = case_a(small, name)
            ids = small.ids(fs, residual, tx)
            for zm in (True, False):
                got = w.sum_product(V, W, fs, residual, txn=txn, zonemap=zm, path="slices")
                assert (got[0] % M128, got[1]) == (total(prod, ids) % M128, len(ids)), (name, cu, zm)
                assert table_a.last_sum_product() == (True, 1) and table_a.last_zones() == (live if zm else 6, 6)
    reached(w, "sum_product", cu)
    reached(wb, "sum_product", cu)


@pytest.mark.parametrize("cu", CUS_A)
def test_a_sum_product_by(ctx, tally, small, table_a, cu):
    """sum_product_by: nine groups are three launches of four; two group columns under no filter and the
    dead-zone one; the reader."""
    w = Watched(table_a, ctx, tally)
    for _ in both_settings(ctx, cu):
        for name in PUSHED_A:
            fs, _, txn, tx, live = case_a(small, name)
            for by in ([G9], [G9, GN]) if name in ("none", "dead_zone") else ([G9],):
                check_product_groups(w, small.ocols, by, N_A, fs, txn=txn, tx=tx, paths=["slices", None], what=(name, cu))
        for name in ("six_leaves", "two_passes"):  # (the checker takes no residual)
            residual = FILTERS_A[name][1]
            for zm in (True, False):
                got = w.sum_product_by(V, W, [G9], None, residual, path="slices", zonemap=zm)
                assert got == product_expected(small.ocols, [G9], F.serialize(None, residual), N_A), (name, cu, zm)
                assert table_a.last_sum_product() == (True, 3), (name, table_a.last_sum_product())
    reached(w, "sum_product_by", cu)


@pytest.mark.parametrize("cu", CUS_A)
def test_a_raw_bitslice_calls(ctx, tally, cu):
    """cubit_bitslice_aggregate, _select, _select_grouped and _sum_product on a caller's slices, through the
    checkers of their own modules (Python integers, np.sort): they size their grids from the context too."""
    rng = np.random.default_rng(9300 + cu)
    seen = {k: set() for k in WPC if k.startswith("raw")}
    for _ in both_settings(ctx, cu):
        for bits, dtype in ((0, np.int64), (13, np.int32), (40, np.int64)):
            raw_aggregate.check_span(ctx, rng, N_A, bits, True, dtype)
            seen["raw_aggregate"] |= note_raw(ctx, tally, "raw_aggregate", N_A)
            raw_select.check_span(ctx, rng, N_A, bits, True, dtype, "random")
            seen["raw_select"] |= note_raw(ctx, tally, "raw_select", N_A)
        for bits, n_groups, shape in ((13, 9, "spread"), (40, 17, "spread"), (5, 8, "one holds all")):
            raw_select_grouped.check_case(ctx, rng, N_A, bits, n_groups, True, True, shape)
            seen["raw_select_grouped"] |= note_raw(ctx, tally, "raw_select_grouped", N_A)
        seen["raw_sum_product"] |= raw_sum_product(ctx, tally, rng, N_A, ((40, 20), (9, 17), (0, 8)))
    for kernel, got in seen.items():
        assert ("A" in got) == (cu * WPC[kernel] < 6), (kernel, cu, got)


def offset_product_sum(a, b, sel):
    """The exact sum of a.keys * b.keys over sel for operands of few slices (n_a + n_b <= 36, below 2^27
    rows): the offsets' products fit 64 bits, the bases (anywhere in int64) enter as Python integers."""
    ao = (a.keys[sel].view(np.uint64) - np.uint64(a.base & (2 ** 64 - 1)))
    bo = (b.keys[sel].view(np.uint64) - np.uint64(b.base & (2 ** 64 - 1)))
    assert int(ao.max(initial=0)) < 2 ** a.bits and int(bo.max(initial=0)) < 2 ** b.bits and len(ao) < 2 ** 27
    return int((ao * bo).sum()) + b.base * int(ao.sum()) + a.base * int(bo.sum()) + len(ao) * a.base * b.base


def raw_sum_product(ctx, tally, rng, n, slice_pairs):
    """test_bitslice_sum_product_matches_python_integers' body at one row count."""
    pw = int(ctx.lib.cubit_padded_words(n))
    out = ctx.alloc(32)
    mask = rng.random(n) < 0.6
    mask[0] = mask[n - 1] = True
    d_mask = ctx.upload(raw_aggregate.pack(mask, pw, pad_ones=True))
    every = np.ones(n, dtype=bool)
    seen = set()
    for n_a, n_b in slice_pairs:
        a, b = Operand(ctx, rng, n, n_a, pw), Operand(ctx, rng, n, n_b, pw)
        prod = None if n_a + n_b <= 36 else a.keys.astype(object) * b.keys.astype(object)
        for use_va, use_vb in ((False, False), (True, True)):
            ok = (a.valid if use_va else every) & (b.valid if use_vb else every)
            for d_f, rows in ((None, every), (d_mask, mask)):
                got = run_bitslice(ctx, a, b, use_va, use_vb, d_f, n, out)
                seen |= note_raw(ctx, tally, "raw_sum_product", n)
                sel = rows & ok
                exact = offset_product_sum(a, b, sel) if prod is None else (int(prod[sel].sum()) if sel.any() else 0)
                assert got == (exact % M128, int(sel.sum()), int(rows.sum())), (n, n_a, n_b, use_va, d_f is not None)
        a.free()
        b.free()
    d_mask.free()
    out.free()
    return seen


# ------------------------------------------------------------------ B. more than 64 workgroups

DENSE = F.TableFilterSet({F0: F.ConstantFilter("<", 1)})       # one row in ten: every tile above the LDS stages
SPARSE = F.TableFilterSet({F0 + 1: F.ConstantFilter("<", 1)})  # one in a thousand
FILTERS_B = {"dense": DENSE, "sparse": SPARSE}
SETTINGS_B = [0, CU_B]


def test_part_b_reference_needs_the_late_tiles(big):
    """On the reference alone: without the tiles 64 … 70 — the second partial of the finishing lanes 0 … 6
    at 71 workgroups, the workgroups 64 and 65 and the second tiles of the workgroups 0 … 4 at 66 — the
    minimum, the maximum, the sum, the counts and the set of groups all differ, under either filter."""
    d, _ = big
    for name, fs in FILTERS_B.items():
        ids = d.ids(fs, None)
        early = ids[ids < 64 * ZONE]
        assert 0 < len(early) < len(ids), name
        full, cut = d.v[ids][d.vv[ids]], d.v[early][d.vv[early]]
        assert full.min() < cut.min() and full.max() > cut.max(), name
        assert raw_aggregate.exact_sum(full) != raw_aggregate.exact_sum(cut), name
        assert set(d.g9[ids].tolist()) == set(range(9)) and set(d.g9[early].tolist()) == set(range(8)), name
        assert int(np.argmin(d.v)) // ZONE == 65 and int(np.argmax(d.v)) // ZONE == 69


def expect_b(w, kernel, units):
    """71 workgroups with the override off; at 33 the one-per-CU kernels walk two or three tiles each and
    the two-per-CU ones launch 66 workgroups, five of them with two tiles."""
    want_seen = {"B"} if units == 0 else ({"A"} if WPC[kernel] == 1 else {"A", "B"})
    assert w.seen[kernel] == want_seen, (kernel, units, w.seen[kernel])


@pytest.mark.parametrize("units", SETTINGS_B)
def test_b_aggregate_and_aggregate_by(ctx, tally, big, units):
    d, t = big
    w = Watched(t, ctx, tally)
    ctx.set_compute_units(units)
    try:
        for name, fs in FILTERS_B.items():
            check_paths(w, d.ocols, V, L.TYPE_INT64, N_B, fs, ops=L.AGG_ALL, paths=["slices"], what=(name, units))
            check_groups(w, d.ocols, V, L.TYPE_INT64, [G9], N_B, fs, ops=L.AGG_ALL, paths=["slices"], what=(name, units))
        check_groups(w, d.ocols, V, L.TYPE_INT64, [G9, GN], N_B, SPARSE, ops=L.AGG_SUM, paths=["slices", None],
                     what=("two", units))
    finally:
        ctx.set_compute_units(0)
    expect_b(w, "aggregate", units)
    expect_b(w, "aggregate_by", units)


@pytest.mark.parametrize("units", SETTINGS_B)
def test_b_select_and_select_by(ctx, tally, big, units):
    d, t = big
    w = Watched(t, ctx, tally)
    ctx.set_compute_units(units)
    try:
        for name, fs in FILTERS_B.items():
            s, rows = oracle_keys(d.ocols, V, fs, None, N_B)
            m = len(s)
            check_select(w, s, rows, V, fs, paths=["slices"], zonemaps=(True,), ranks=[0, m - 1], quantiles=[0.5],
                         what=(name, units))
        groups = group_rows(d.ocols, V, [G9], SPARSE, None, N_B)
        assert len(groups[(8,)][0]) > 0
        check_by(w, groups, V, [G9], SPARSE, paths=["slices"], zonemaps=(True,), what=units, launches=2, passes=11)
    finally:
        ctx.set_compute_units(0)
    expect_b(w, "select", units)
    expect_b(w, "select_by", units)


@pytest.mark.parametrize("units", SETTINGS_B)
def test_b_sum_product_and_sum_product_by(ctx, tally, big, units):
    d, t = big
    w = Watched(t, ctx, tally)
    ctx.set_compute_units(units)
    try:
        for name, fs in FILTERS_B.items():
            check_table_paths(w, d.ocols, N_B, LazyProducts(d), fs, 0, paths=("slices",), what=(name, units))
        check_product_groups(w, d.ocols, [G9], N_B, SPARSE, paths=["slices"], what=units)
        check_product_groups(w, d.ocols, [G9], N_B, DENSE, paths=["slices"], what=units)
    finally:
        ctx.set_compute_units(0)
    expect_b(w, "sum_product", units)
    expect_b(w, "sum_product_by", units)


@pytest.mark.parametrize("units", SETTINGS_B)
def test_b_raw_bitslice_calls(ctx, tally, big, units):
    rng = np.random.default_rng(9400 + units)
    ctx.set_compute_units(units)
    try:
        raw_aggregate.check_span(ctx, rng, N_B, 13, True, np.int32)
        seen = {"raw_aggregate": note_raw(ctx, tally, "raw_aggregate", N_B)}
        raw_select.check_span(ctx, rng, N_B, 13, True, np.int32, "two")
        seen["raw_select"] = note_raw(ctx, tally, "raw_select", N_B)
        raw_select_grouped.check_case(ctx, rng, N_B, 5, 9, True, True, "spread")
        seen["raw_select_grouped"] = note_raw(ctx, tally, "raw_select_grouped", N_B)
        seen["raw_sum_product"] = raw_sum_product(ctx, tally, rng, N_B, ((13, 9),))
    finally:
        ctx.set_compute_units(0)
    for kernel, got in seen.items():
        assert got == ({"B"} if units == 0 else ({"A"} if WPC[kernel] == 1 else {"A", "B"})), (kernel, units, got)


# ------------------------------------------------------------------ C. the fused sum, the quantile histogram, the decode


@pytest.mark.parametrize("cu", [1, 2])
@pytest.mark.parametrize("packed", [False, True], ids=["plain_a", "packed_a"])
def test_c_fused_sum_walks_several_tiles(ctx, small, cu, packed):
    """eval_sum_product over six tiles in one or two … four workgroups: its LDS stage is reused between the
    tiles of one workgroup. b decoded from a three-value range of its RANGE index (nullable) and gathered,
    a plain and read from its BITPACKING segments, staged tiles (1 % of the rows) and direct ones; the
    forced "column" path is the same kernel. Against exact Python integers."""
    rng = np.random.default_rng(9500)
    n = N_A
    vals = np.array([-(2 ** 41), -3, 8, 2 ** 32 + 1, 2 ** 36, 2 ** 43 - 7], dtype=np.int64)
    a = rng.integers(-(2 ** 39), 2 ** 39, n).astype(np.int64)
    b = vals[rng.integers(0, 6, n)]
    va, vb = rng.random(n) > 0.15, rng.random(n) > 0.2
    key = rng.integers(0, 100, n).astype(np.int32)
    key[n - 1], va[n - 1], vb[n - 1], b[n - 1] = 0, True, True, vals[2]  # the last row of the 37-row tile counts
    t = CubitTable(ctx, n, row_base=7)
    if packed:
        t.add_bitpacked_column(0, *packed_pieces(a, va, [(0, n)]), np.int64, validity=validity_from_mask(va))
    else:
        t.add_column(0, a, validity_from_mask(va))
    t.add_column(1, b, validity_from_mask(vb))
    t.add_column(2, key)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE)
    ocols = [O.Column(a, validity_from_mask(va)), O.Column(b, validity_from_mask(vb)), O.Column(key)]
    prod = products(a, b, va, vb)
    three = F.ConjunctionAndFilter([F.ConstantFilter(">=", int(vals[1])), F.ConstantFilter("<=", int(vals[3]))])
    cases = [("sparse", F.TableFilterSet({2: F.ConstantFilter("<", 1)}), 0),
             ("dense", F.TableFilterSet({2: F.ConstantFilter(">=", 0)}), 0),
             ("b in three values", F.TableFilterSet({1: three, 2: F.ConstantFilter("<", 50)}), 3)]
    try:
        for units in both_settings(ctx, cu):
            for name, fs, decoded in cases:
                rows = O.table_scan(ocols, F.serialize(fs), n, row_base=7) - 7
                assert rows[-1] == n - 1 or name != "dense"
                expect = (total(prod, rows), len(rows))
                for path in (None, "column"):
                    for gather in (False, True):
                        assert t.sum_product(0, 1, fs, gather_b=gather, path=path) == expect, (name, units, path, gather)
                        assert t.last_sum_product() == (False, 0) and t.last_sum_packed() == packed
                        if decoded:
                            assert t.last_sum_decode() == (0 if gather else decoded), (name, gather)
                        # (without a live-tile list the kernel walks the padded partition's eight tiles)
                        wg, tiles = ctx.last_grid()
                        assert tiles in (6, 8) and wg == min(tiles, 2 * ctx.compute_units()[1]), (name, units, wg, tiles)
                        assert units == 0 or tiles > wg
    finally:
        t.close()


def test_c_quantile_histogram_on_one_compute_unit(ctx):
    """build_index_quantiles with the histogram's workgroups striding over many tiles (four, then two
    workgroups for 80 or 160 tiles of 8,192 / 4,096 rows): the keys equal numpy's and the override-off ones."""
    rng = np.random.default_rng(9600)
    v = rng.integers(10 ** 6, 10 ** 6 + 2 ** 40, N_A).astype(np.int64)
    ok = rng.random(N_A) >= 0.08
    v[~ok] = np.where(rng.random(N_A) < 0.5, -(2 ** 62), 2 ** 62)[~ok]  # NULL slots far outside: they move no edge
    narrow = rng.integers(8035, 8035 + 2526, N_A).astype(np.int32)
    every = np.ones(N_A, dtype=bool)
    for data, valid, bins in ((v, ok, 64), (v, ok, 1024), (narrow, every, 64)):
        keys = {}
        for units in both_settings(ctx, 1):
            t = CubitTable(ctx, N_A)
            t.add_column(0, data, None if valid.all() else validity_from_mask(valid))
            keys[units] = [t.build_index_quantiles(0, bins, enc).tolist() for enc in (L.INDEX_RANGE, L.INDEX_BINS)]
            t.close()
        expect = [expected_keys(data.astype(np.int64), valid, bins, enc, data.dtype.type)
                  for enc in (L.INDEX_RANGE, L.INDEX_BINS)]
        assert keys[1] == keys[0] == expect, (data.dtype, bins)


def decode_grid(work, cu):
    """eval_decode_impl's grid rule: (workgroups, regime)."""
    if work <= 2 * cu:
        return work, "one per tile"
    if work <= 4 * cu:
        return (work + 1) // 2, "pairs"
    return 2 * cu, "capped"


def decode_kernel(forced, ordered, live, work, grid, cu):
    """decode_kernel_for as include/cubit_gpu.h and cubit_internal.hpp document it, for a program of several
    leaves (no prefixed decode): the look-back kernel when forced, for an ordered scan under AUTO, and under
    AUTO while the tiles fit three workgroups per compute unit; a live-tile list takes the run kernel;
    else the forced one; else the run kernel from three tiles per workgroup, the pair kernel below."""
    if forced == L.DECODE_LOOKBACK or (forced == L.DECODE_AUTO and (ordered or work <= 3 * cu)):
        return L.DECODE_LOOKBACK
    if live:
        return L.DECODE_RUNS
    if forced != L.DECODE_AUTO:
        return forced
    return L.DECODE_RUNS if work > 2 * grid else L.DECODE_PAIRS


def test_c_decode_grid_rule_regimes(ctx):
    """scan_tiles over 1,000,003 rows (8 tiles) with 1 … 4 compute units: the capped (2 workgroups of four
    tiles), pair (4 of two) and one-per-tile regimes of the decode grid, under AUTO and every forced
    kernel, ordered and in tile runs, over every tile and over a live-tile list of six (the tiles 2 and 5
    of the first column are dead). Rows and directory equal the oracle's; last_grid() and
    last_decode_kernel() what the grid rule and decode_kernel_for give for the lowered count."""
    n, base = 1_000_003, 9
    rng = np.random.default_rng(9700)
    ship = rng.integers(8000, 10_600, n).astype(np.int32)
    for tile in (2, 5):
        ship[tile * ZONE:(tile + 1) * ZONE] = rng.integers(9300, 10_600, ZONE)
    disc = rng.integers(0, 11, n).astype(np.int64)
    qty = rng.integers(100, 5100, n).astype(np.int64)
    t = CubitTable(ctx, n, row_base=base)
    for c, a in enumerate((ship, disc, qty)):
        t.add_column(c, a)
    t.build_index(0, L.INDEX_RANGE, list(range(8000, 10_601, 100)))
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE, [2400])
    t.set_derived_budget(0)
    t.set_derived_chain_cost(2 ** 64 - 1)
    q6 = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 8800), F.ConstantFilter("<", 9200)]),
                           1: F.ConjunctionAndFilter([F.ConstantFilter(">=", 5), F.ConstantFilter("<=", 7)]),
                           2: F.ConstantFilter("<", 2400)})
    ref = O.table_scan([O.Column(ship), O.Column(disc), O.Column(qty)], F.serialize(q6), n, row_base=base)
    counts = np.bincount((ref - base) // ZONE, minlength=8)
    assert [i for i in range(8) if counts[i] == 0] == [2, 5] and counts[7] > 0
    seen = set()
    try:
        for cu in (0, 1, 2, 3, 4):
            ctx.set_compute_units(cu)
            units = ctx.compute_units()[1]
            for kernel in (L.DECODE_AUTO, L.DECODE_PAIRS, L.DECODE_RUNS, L.DECODE_LOOKBACK):
                ctx.set_decode_kernel(kernel)
                for ordered in (False, True):
                    for zonemap in (False, True):
                        where = (cu, kernel, ordered, zonemap)
                        got, k, directory, bufs = scan_tiles(ctx, t, q6, n, ordered=ordered, zonemap=zonemap)
                        for b in bufs:
                            b.free()
                        assert k == len(ref) and directory[:, 1].tolist() == counts.tolist(), where
                        rows = got if ordered else runs_in_row_order(got, directory)
                        assert np.array_equal(rows, ref), where
                        work = 6 if zonemap else 8
                        assert t.last_zones() == (work, 8), where
                        grid, regime = decode_grid(work, units)
                        ran = decode_kernel(kernel, ordered, zonemap, work, grid, units)
                        assert ctx.last_decode_kernel() == ran, (where, ctx.last_decode_kernel(), ran)
                        assert ctx.last_grid() == ((work if ran == L.DECODE_LOOKBACK else grid), work), (where, ctx.last_grid())
                        if cu and ran != L.DECODE_LOOKBACK:
                            seen.add(regime)
    finally:
        ctx.set_compute_units(0)
        ctx.set_decode_kernel(L.DECODE_AUTO)
        t.close()
    assert seen == {"capped", "pairs", "one per tile"}, seen


def test_c_kept_row_list_on_one_compute_unit(ctx, row_list_data):
    """test_third_scan_reads_the_list's sequence (the dense rounds' leaf, row ids past 2^32) with the override
    at 1: the prefixed decode and the row-list kernel launch a workgroup per tile whatever the count."""
    v, row_base = 2, row_lists.BASES[1]
    ref = row_list_data[2][v] + row_base
    ctx.set_compute_units(1)
    t = row_lists.make_table(ctx, row_list_data, row_base)
    try:
        flags = [row_lists.check_scan(ctx, t, row_lists.eq(v), ref, row_base, what=(v, i)) for i in range(4)]
        assert flags == [False, False, True, True]
        assert ctx.last_grid() == (row_lists.TILES, row_lists.TILES)
        assert t.row_list_stats() == (1, row_lists.list_bytes(len(ref)), 2)
        t.use_row_lists(False)
        assert row_lists.check_scan(ctx, t, row_lists.eq(v), ref, row_base, what=(v, "off")) is False
        t.use_row_lists(True)
        assert row_lists.check_scan(ctx, t, row_lists.eq(v), ref, row_base, ordered=True, what=(v, "ordered")) is True
        assert t.row_list_stats()[2] == 3
    finally:
        ctx.set_compute_units(0)
        t.close()


row_list_data = row_lists.data  # (the fixture, under a name of this module's)


# ------------------------------------------------------------------ D. the setting itself


def test_d_setting_refusals_restore_and_stream(ctx, table_a):
    lib = ctx.lib
    device, in_use = ctx.compute_units()
    assert 1 <= device == in_use
    for bad in (-1, device + 1, 2 ** 31 - 1, -(2 ** 31)):
        assert lib.cubit_ctx_set_compute_units(ctx.handle, bad) == L.ERR_INVALID, bad
        assert str(device).encode() in lib.cubit_last_error()
        assert ctx.compute_units() == (device, device)
    dev, use, wg, tiles = C.c_int(), C.c_int(), C.c_uint32(), C.c_uint32()
    assert lib.cubit_ctx_set_compute_units(None, 1) == L.ERR_INVALID
    assert lib.cubit_ctx_compute_units(None, C.byref(dev), C.byref(use)) == L.ERR_INVALID
    assert lib.cubit_ctx_compute_units(ctx.handle, None, C.byref(use)) == L.ERR_INVALID
    assert lib.cubit_ctx_last_grid(None, C.byref(wg), C.byref(tiles)) == L.ERR_INVALID
    assert lib.cubit_ctx_last_grid(ctx.handle, C.byref(wg), None) == L.ERR_INVALID
    for n in (1, device, max(device // 2, 1)):
        ctx.set_compute_units(n)
        assert ctx.compute_units() == (device, n)
    # the setting survives set_stream; 0 restores the device's count
    stream = C.c_void_p()
    L.check(lib.cubit_copy_stream_create(ctx.handle, C.byref(stream)))  # (a non-blocking stream of the library's)
    try:
        ctx.set_compute_units(1)
        ctx.set_stream(stream.value)
        assert ctx.compute_units() == (device, 1)
        got = table_a.aggregate(V, path="slices")
        assert ctx.last_grid() == (2, 6) and got.count_rows == N_A
        ctx.set_stream(None)
        assert ctx.compute_units() == (device, 1)
        assert table_a.aggregate(V, path="slices") == got and ctx.last_grid() == (2, 6)
    finally:
        ctx.set_stream(None)
        ctx.set_compute_units(0)
        L.check(lib.cubit_copy_stream_destroy(ctx.handle, stream))
    assert table_a.aggregate(V, path="slices") == got and ctx.last_grid() == (6, 6)
    assert ctx.compute_units() == (device, device)
    # a fresh context starts at the device's count with no launch reported
    other = Context(0)
    try:
        assert other.compute_units() == (device, device) and other.last_grid() == (0, 0)
    finally:
        other.close()


# ------------------------------------------------------------------ the tally


def test_every_kernel_ran_in_both_regimes(ctx, tally):
    """Run with the whole module: the tally is its tests'. Every kernel was seen with more tiles than
    workgroups and with more than 64 workgroups, from what its launcher reported."""
    print("regimes seen:", {k: sorted(v) for k, v in tally.items()})
    if ctx.compute_units()[0] < 71:
        assert all("A" in v for v in tally.values()), tally
        pytest.skip(f"a device of {ctx.compute_units()[0]} compute units launches no 71 workgroups")
    assert all(v == {"A", "B"} for v in tally.values()), tally
