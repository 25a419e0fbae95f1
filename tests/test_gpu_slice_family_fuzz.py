"""Random filter trees through the slice-answered selects and GROUP BY aggregates: CubitTable.kth,
quantile, top_n and aggregate_by on both forced paths and on the library's own choice, against numpy
over the rows the oracle returns (O.table_scan, O.fetch). aggregate() has test_fuzz
(test_gpu_table_aggregate.py); this is the same for the other two kernels of the family, over trees
wide enough to reach every program form, six and more leaves and plans of more than one pass — the last
test checks that they did.

Per seed: one tile and a ragged tail of 1 … 130 rows; four literal columns over 0 … 49 — no index, a
RANGE index over every value, a RANGE index over [10, 20, 30, 40], an every-value EQUALITY index — two
of them with 10 % NULLs; two value columns of a random span (0 … 62 bits, anywhere in int64) and NULL
rate with a bit-sliced index; one or two EQUALITY-indexed group columns of 2 … 9 values, one nullable.
Eight trees each: a pushed filter set and, half the time, a residual of depth <= 2, their constants
reaching past both ends of the values; on every other seed each tree also runs under a reader that sees
a delete list. Fixed seeds."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_gpu_group_aggregate import check_groups
from test_gpu_sliced_fuzz import rand_const_filter, rand_residual
from test_gpu_table_select import check_select, top_n_expected, want

pytestmark = pytest.mark.gpu

ZONE = 131_072
U64 = (1 << 64) - 1
TXN_START = 4611686018427388000
PATHS = [None, "slices", "column"]
SEEDS = range(24)
TREES = 8
N_LITERAL = 4
RANGE_KEYS = [10, 20, 30, 40]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


class Tally:
    """What the slices-path calls planned: the (form, leaves) cells and the passes, the trees that ran no kernel."""

    def __init__(self):
        self.seeds, self.cells, self.passes, self.folded = set(), set(), set(), 0


@pytest.fixture(scope="module")
def tally():
    return Tally()


def value_column(rng, n, seed):
    """As test_fuzz draws them: a span of 0 … 62 bits anywhere in int64, INT32 where it fits."""
    bits = int(rng.integers(0, 63))
    span = (1 << bits) - 1
    lo = int(rng.integers(-(1 << 62), (1 << 62) - span)) if rng.random() < 0.7 else [0, -(1 << 63), (1 << 63) - 1 - span][seed % 3]
    dtype = np.int32 if bits <= 30 and -(1 << 31) <= lo and lo + span < (1 << 31) else np.int64
    v = (rng.integers(0, span, n, endpoint=True, dtype=np.uint64) + np.uint64(lo & U64)).view(np.int64).astype(dtype)
    valid = rng.random(n) >= [0.0, 0.05, 0.5, 0.99][int(rng.integers(0, 4))]
    return v, (validity_from_mask(valid) if not valid.all() else None), (L.TYPE_INT32 if dtype == np.int32 else L.TYPE_INT64)


def make_columns(rng, n, seed):
    """[(data, validity words or None, index encoding or None, index keys or None)], the value columns'
    ids and types, the group columns' ids."""
    cols = []
    nullable = set(int(c) for c in rng.choice(N_LITERAL, size=2, replace=False))
    kinds = [(None, None), (L.INDEX_RANGE, None), (L.INDEX_RANGE, RANGE_KEYS), (L.INDEX_EQUALITY, None)]
    for c in range(N_LITERAL):
        d = rng.integers(0, 49, n, endpoint=True).astype(np.int32 if c % 2 == 0 else np.int64)
        vw = validity_from_mask(rng.random(n) >= 0.1) if c in nullable else None
        cols.append((d, vw, *kinds[c]))
    values, types = [], {}
    for _ in range(2):
        v, vw, typ = value_column(rng, n, seed)
        values.append(len(cols))
        types[len(cols)] = typ
        cols.append((v, vw, L.INDEX_SLICED, None))
    groups = []
    n_groups = int(rng.integers(1, 3))
    null_one = int(rng.integers(0, n_groups))
    for j in range(n_groups):
        k = int(rng.integers(2, 10))
        g = (rng.integers(0, k, n) * 3 - 7).astype(np.int32 if j == 0 else np.int64)
        g[:k] = np.arange(k) * 3 - 7
        vw = validity_from_mask(rng.random(n) >= 0.1) if j == null_one else None
        groups.append(len(cols))
        cols.append((g, vw, L.INDEX_EQUALITY, None))
    return cols, values, types, groups


def make_trees(rng):
    trees = []
    for _ in range(TREES):
        filters = {}
        for c in rng.choice(N_LITERAL, size=rng.integers(0, N_LITERAL + 1), replace=False):
            filters[int(c)] = rand_const_filter(rng)
        fs = F.TableFilterSet(filters) if filters else None
        residual = rand_residual(rng, N_LITERAL) if rng.random() < 0.5 else None
        trees.append((fs, residual))
    return trees


@pytest.mark.parametrize("seed", SEEDS)
def test_random_trees_select_top_n_and_group_by(ctx, tally, seed):
    rng = np.random.default_rng(7100 + seed)
    n = ZONE + int(rng.integers(1, 131))
    cols, values, types, groups = make_columns(rng, n, seed)
    t = CubitTable(ctx, n)
    for c, (data, vw, enc, keys) in enumerate(cols):
        t.add_column(c, data, vw)
        if enc is not None:
            t.build_index(c, enc, keys)
    ocols = [O.Column(data, vw) for data, vw, _, _ in cols]
    views = [(None, None)]
    if seed % 2:  # a reader that sees a delete list
        dels = np.sort(rng.choice(n, n // 10, replace=False)).astype(np.int64)
        deleted = np.full(n, np.uint64(2 ** 64 - 2), dtype=np.uint64)
        deleted[dels] = 5
        t.set_deletes(dels, np.full(len(dels), 5, dtype=np.uint64))
        views.append((L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted)))

    def after(path, zm=True):
        if path != "slices":
            return
        leaves, passes = t.last_plan()
        if leaves == 0:  # folded to FALSE, or the zonemaps rule out every zone: no kernel
            assert rows == 0, (what, t.last_plan())
            tally.folded += 1
            return
        tally.cells.add((t.last_form(), leaves))
        tally.passes.add(passes)

    try:
        for i, (fs, residual) in enumerate(make_trees(rng)):
            for txn, tx in views:
                col = values[int(rng.integers(0, 2))]
                what = (seed, i, txn is not None, col, fs, residual)
                ids = O.table_scan(ocols, F.serialize(fs, residual), n, 0, tx)
                v, ok = O.fetch(ocols[col], ids, 0, tx, with_valid=True)
                vids, vals = ids[ok], np.ascontiguousarray(v[ok]).astype(np.int64)
                s, rows = np.sort(vals), len(ids)
                m = len(s)
                # kth at a random rank and its mirror, quantile at a random q and both ends
                r = int(rng.integers(0, m + 1))
                check_select(t, s, rows, col, fs, residual, txn=txn, paths=PATHS, zonemaps=(True,),
                             ranks=sorted({r, max(m - 1 - r, 0)}), quantiles=[float(rng.random()), 0.0, 1.0],
                             what=what, after=after)
                # top-N rows in both directions
                k = int(rng.integers(1, min(m, 3000) + 3))
                for desc in (False, True):
                    want_ids, want_vals = top_n_expected(vids, vals, k, desc)
                    for path in PATHS:
                        got_ids, got_vals, sel = t.top_n(col, k, desc, fs, residual, txn=txn, path=path)
                        assert np.array_equal(got_ids, want_ids), (what, k, desc, path)
                        assert np.array_equal(got_vals, want_vals), (what, k, desc, path)
                        assert sel == want(s, rows, desc, k - 1), (what, k, desc, path)
                        if path is not None and rows:
                            assert t.last_select()[0] == (path == "slices"), (what, path)
                # GROUP BY one or two columns, a random subset of the aggregates
                check_groups(t, ocols, col, types[col], groups, n, fs, residual, txn=txn, tx=tx,
                             ops=int(rng.integers(0, 8)), what=what, after=after)
        tally.seeds.add(seed)
    finally:
        t.close()


def test_the_trees_reached_every_form_many_leaves_and_more_than_one_pass(tally):
    """The generator's reach, measured on the plans the slices path ran (last_plan, last_form)."""
    assert tally.seeds == set(SEEDS), "run with the seeds of this module: the tally is theirs"
    print(f"(form, leaves) cells {sorted(tally.cells)} passes {sorted(tally.passes)} folded {tally.folded}")
    assert {f for f, _ in tally.cells} == {L.FORM_POSTFIX, L.FORM_CONJ, L.FORM_DNF, L.FORM_CNF}, tally.cells
    assert max(k for _, k in tally.cells) >= 6, tally.cells
    assert max(tally.passes) >= 2, tally.passes
    assert tally.folded >= 1
