"""Planner fuzz over bit-sliced columns: 200 random pushed filter sets with random cross-column
residual trees over three columns — one with a bit-sliced index only, one with a bit-sliced index
beside a RANGE index on a few keys, one plain (K0) — with NULLs and update records whose values
also lie outside the slices' range. Fixed seeds; every tree, for a reader that predates the
updates, one that sees the committed half and the writer, must return exactly the oracle's rows,
with the slices on and off."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TXN_START = 4611686018427388000
CMPS = ["=", "!=", "<", "<=", ">", ">="]
LO, HI = 0, 49  # base values; constants and updates reach past both ends


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def rand_const_filter(rng, depth=0):
    r = rng.random()
    if depth < 2 and r < 0.3:
        kids = [rand_const_filter(rng, depth + 1) for _ in range(rng.integers(2, 4))]
        return F.ConjunctionAndFilter(kids) if rng.random() < 0.7 else F.ConjunctionOrFilter(kids)
    if r < 0.36:
        return F.IsNullFilter() if rng.random() < 0.5 else F.IsNotNullFilter()
    return F.ConstantFilter(CMPS[rng.integers(0, 6)], int(rng.integers(LO - 8, HI + 20)))


def rand_residual(rng, n_cols, depth=0):
    if depth < 2 and rng.random() < 0.5:
        kids = [rand_residual(rng, n_cols, depth + 1) for _ in range(rng.integers(2, 4))]
        return F.And(*kids) if rng.random() < 0.5 else F.Or(*kids)
    c = int(rng.integers(0, n_cols))
    if rng.random() < 0.1:
        return F.IsNull(c)
    return F.Cmp(c, CMPS[rng.integers(0, 6)], int(rng.integers(LO - 8, HI + 20)))


def test_random_trees_over_sliced_columns(ctx):
    rng = np.random.default_rng(4242)
    n = 400_003
    writer = TXN_START + 5
    t = CubitTable(ctx, n)
    data = []
    for c in range(3):
        d = rng.integers(LO, HI, n, endpoint=True).astype(np.int32 if c == 0 else np.int64)
        vw = validity_from_mask(rng.random(n) > 0.1)
        t.add_column(c, d, vw)
        data.append((d, vw))
    t.build_index(0, L.INDEX_SLICED)                    # sliced only: bounds fold into one leaf
    t.build_index(1, L.INDEX_RANGE, [10, 20, 30, 40])   # keys on the index, the rest from the slices
    t.build_index(1, L.INDEX_SLICED)
    # column 2: plain
    upd = {}
    for c in range(3):
        rows = np.sort(rng.choice(n, size=3000, replace=False)).astype(np.int64)
        vals = rng.integers(LO - 6, HI + 15, len(rows)).astype(np.int64)  # also outside the slices' range
        ok = rng.random(len(rows)) >= 0.1  # SET NULL among them
        vers = np.where(rng.random(len(rows)) < 0.5, np.uint64(3), np.uint64(writer)).astype(np.uint64)
        t.set_updates(c, rows, vals, vers, ok)
        upd[c] = (rows, vals, vers, ok)
    ocols = [O.Column(d, vw, updates=upd[c]) for c, (d, vw) in enumerate(data)]
    views = [(2, TXN_START + 6), (10, TXN_START + 7), (2, writer)]
    from_slices = 0
    for i in range(200):
        filters = {}
        for c in rng.choice(3, size=rng.integers(1, 4), replace=False):
            filters[int(c)] = rand_const_filter(rng)
        fs = F.TableFilterSet(filters)
        residual = rand_residual(rng, 3) if rng.random() < 0.5 else None
        plan = F.serialize(fs, residual)
        start, tid = views[i % 3]
        ref = O.table_scan(ocols, plan, n, tx=O.Mvcc(start, tid))
        got = t.scan(fs, residual, txn=L.Txn(start, tid))
        from_slices += t.last_sliced()
        assert np.array_equal(got, ref), (i, start, tid, fs, residual)
        if i % 4 == 0:
            t.use_sliced(False)
            off = t.scan(fs, residual, txn=L.Txn(start, tid))
            t.use_sliced(True)
            assert np.array_equal(off, ref), ("plain", i, start, tid, fs, residual)
    assert from_slices >= 100  # the trees did go through the slices
    t.close()
