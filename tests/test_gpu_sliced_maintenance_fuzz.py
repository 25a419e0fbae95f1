"""The bit-sliced index and the queries answered from it, through sequences of table maintenance.

Every other test of the slice-answered queries (aggregate, aggregate_by, kth / quantile / top_n, sum_product,
sum_product_by) runs on slices built once; every other test of the slices' upkeep checks one step from a fresh
table. Here a table of four literal columns, five value columns with bit-sliced indexes (two INT64 operands,
an INT32, a UINT64 that reaches 0 and 2^64 - 1, a finite DOUBLE) and one or two group columns goes through a
random sequence of appends (inside the slices' range, above the top by a slice or more, below the base,
NULL-only, the first valid rows of an all-NULL column; in every third seed the first one crosses the table's
capacity, and an append, a merge and a sync follow on the reallocated bitvectors), update lists, merges
at random horizons, syncs (host and on-device, one in four refused by max_changed; some of both nothing but
SET NULL) and delete lists — the
generator and its model are tests/sliced_maintenance_model.py — and after every write

1. the slices are read back (save_index / read_index) and compared word for word, padding included, with
   numpy over the downloaded column: bit r of slice k = valid[r] & ((key[r] - vmin) mod 2^64 >> k & 1); vmin /
   vmax contain the valid keys, the slice count is the bit length of vmax - vmin, `empty` means no valid row;
2. two filter trees of the seed's pool (one of them with a leaf on a sliced value column) run under no transaction, two readers and the writer, each on a value
   column drawn at random, through every slice-answered query on path None, "slices" and "column": exact
   against Python integers over the oracle's rows (O.table_scan, O.fetch). A forced slice path must be refused
   exactly when the model says an update record of a column it reads is visible to the transaction (or the
   index is empty: bind_slices' other condition), and answered from the slices otherwise — also while update
   records of the filter's columns are visible.

The last test asserts what the generator reached, from the model's tally."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.table import Aggregate, Context, padded_words
from oracle import oracle as O
from sliced_maintenance_model import (A, B, I64_MIN, PLAN, Tally, as_bits, bit_length, keys_of, order_keys,
                                      product_sums, reference_slices, run_plan)
from test_gpu_sliced_index import read_index
from test_gpu_table_aggregate import double_value, reduce_values
from test_gpu_table_select import check_select, top_n_expected, want

pytestmark = pytest.mark.gpu

PATHS = [None, "slices", "column"]
M128 = 1 << 128
TO_VALUE = {L.TYPE_UINT64: lambda key: int(np.int64(key) ^ np.int64(I64_MIN)), L.TYPE_DOUBLE: double_value}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tally():
    return Tally()


@pytest.fixture(scope="module")
def kept():
    """What the library kept across the seeds' repeated trees: [leaf groups replaced by a kept combination, row-list
    decodes, writes after which fewer combinations were kept than before them]."""
    return [0, 0, 0]


def group_by(ocols, ids, tx, by, bits, ok, typ, ops):
    """The rows `ids` grouped by the visible values of the group columns: a dense label per row, the key tuple of
    each label (None: the NULL group) and {key tuple: Aggregate} of the value column's bit patterns `bits` (valid
    where `ok`) over the groups that hold a row."""
    rows = len(ids)
    labels = np.zeros(rows, dtype=np.int64)
    group_keys = [()]
    for g in by:
        gv, gok = O.fetch(ocols[g], ids, 0, tx, with_valid=True)
        u, inv = np.unique(np.where(gok, 2 * gv.astype(np.int64) + 1, 0), return_inverse=True)
        labels = labels * len(u) + inv.reshape(-1)
        group_keys = [gk + (None if x == 0 else int(x - 1) // 2,) for gk in group_keys for x in u]
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.r_[True, labels[order][1:] != labels[order][:-1], True]) if rows else []
    grouped = {}
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        at = order[lo:hi]
        grouped[group_keys[labels[at[0]]]] = Aggregate(*reduce_values(np.ascontiguousarray(bits[at][ok[at]]), typ, ops), int(hi - lo))
    return labels, group_keys, grouped


class Checks:
    def __init__(self, tmp_path, kept):
        self.tmp, self.kept, self.kept_before = tmp_path, kept, 0

    def slices(self, t, m, cols, what):
        n = m.n
        self.kept[2] += t.derived_stats()[0] < self.kept_before  # the write dropped what the queries had admitted
        assert t.n_rows == n, what
        nwp = padded_words(n)
        for c in cols:
            col = m.cols[c]
            path = self.tmp / f"col{c}.cix"
            t.save_index(c, L.INDEX_SLICED, path)
            ix = read_index(path)
            data = t.download_column(c)
            valid = col.valid
            assert np.array_equal(as_bits(data)[valid], as_bits(col.data)[valid]), (what, c, "the column")
            keys = keys_of(col.typ, data)
            vk = keys[valid]
            assert bool(ix["empty"]) == (len(vk) == 0), (what, c, ix["empty"])
            n_bv = ix["n_bv"]
            if len(vk):
                assert ix["vmin"] <= int(vk.min()) and ix["vmax"] >= int(vk.max()), (what, c, ix["vmin"], ix["vmax"])
                assert n_bv == bit_length(ix["vmax"] - ix["vmin"]), (what, c, n_bv, ix["vmin"], ix["vmax"])
            else:
                assert n_bv == 0, (what, c, n_bv)
            # the model's statistics are the classes' yardstick: they must be the library's
            assert (bool(ix["empty"]), n_bv) == (col.empty, col.n_bv()), (what, c, ix["vmin"], ix["vmax"], col.vmin, col.vmax)
            assert ix["slices"].shape == (n_bv, nwp), (what, c, ix["slices"].shape, nwp)
            ref = reference_slices(keys, valid, ix["vmin"], n_bv, nwp)
            if not np.array_equal(ix["slices"], ref):
                k, w = (int(x[0]) for x in np.nonzero(ix["slices"] != ref))
                raise AssertionError((what, c, "slice", k, "word", w, "of", (n + 63) // 64, hex(int(ix["slices"][k, w])),
                                      hex(int(ref[k, w]))))

    def queries(self, t, m, ocols, fs, residual, view, col, refuse, d, what):
        n, typ, by = m.n, m.cols[col].typ, m.groups
        txn = tx = None
        ocols = ocols[view is None]  # no transaction: every row, the base values (no MVCC delta applied)
        if view is not None:
            txn, tx = L.Txn(*view), O.Mvcc(view[0], view[1], inserted=m.inserted, deleted=m.deleted)
        to_value = TO_VALUE.get(typ, int)

        def paths(kind):
            return [None, "column"] if refuse[kind] else PATHS

        def refused(kind, call):
            if refuse[kind]:
                with pytest.raises(L.CubitError):
                    call()

        ids = O.table_scan(ocols, F.serialize(fs, residual), n, 0, tx)
        rows = len(ids)
        v, ok = O.fetch(ocols[col], ids, 0, tx, with_valid=True)
        vids, keys = ids[ok] + t.row_base, order_keys(typ, np.ascontiguousarray(v[ok]))
        s = np.sort(keys)
        cv = len(s)

        # aggregate: every op the type has
        bits = np.ascontiguousarray(v)
        every = L.AGG_MIN | L.AGG_MAX if typ == L.TYPE_DOUBLE else L.AGG_ALL
        whole = Aggregate(*reduce_values(np.ascontiguousarray(bits[ok]), typ, every), rows)
        for path in paths("single"):
            got = t.aggregate(col, fs, residual, txn=txn, path=path)
            assert got == whole, (what, "aggregate", path, got, whole)
            if path is not None and rows:
                assert t.last_aggregate_from_slices() == (path == "slices"), (what, path)
        refused("single", lambda: t.aggregate(col, fs, residual, txn=txn, path="slices"))

        # kth at a random rank and its mirror, quantile at a random q and both ends
        r = int(d["rank"] * (cv + 1))
        check_select(t, s, rows, col, fs, residual, txn=txn, paths=paths("single"), zonemaps=(True,), to_value=to_value,
                     ranks=sorted({r, max(cv - 1 - r, 0)}), quantiles=[d["q"], 0.0, 1.0], what=what)
        refused("single", lambda: t.kth(col, r, False, fs, residual, txn=txn, path="slices"))

        # top-N rows in both directions
        k = 1 + int(d["k"] * (min(cv, 3000) + 2))
        for desc in (False, True):
            want_ids, want_keys = top_n_expected(vids, keys, k, desc)
            for path in paths("single"):
                got_ids, got_vals, sel = t.top_n(col, k, desc, fs, residual, txn=txn, path=path)
                assert np.array_equal(got_ids, want_ids), (what, k, desc, path)
                assert np.array_equal(order_keys(typ, got_vals), want_keys), (what, k, desc, path)
                assert sel == want(s, rows, desc, k - 1, to_value), (what, k, desc, path)
                if path is not None and rows:
                    assert t.last_select()[0] == (path == "slices"), (what, path)
        refused("single", lambda: t.top_n(col, k, False, fs, residual, txn=txn, path="slices"))

        # GROUP BY the group columns, a random subset of the aggregates
        ops = d["ops"] & every
        labels, group_keys, grouped = group_by(ocols, ids, tx, by, bits, ok, typ, ops)
        for path in paths("grouped"):
            got = t.aggregate_by(col, by, fs, residual, txn=txn, ops=ops, path=path)
            assert got == grouped, (what, "aggregate_by", path, ops, got, grouped)
            if path is not None and rows:
                assert t.last_grouped()[0] == (path == "slices"), (what, path)
        refused("grouped", lambda: t.aggregate_by(col, by, fs, residual, txn=txn, ops=ops, path="slices"))

        # sum(A * B), plain and grouped: 128-bit two's complement, so equal modulo 2^128
        av, aok = O.fetch(ocols[A], ids, 0, tx, with_valid=True)
        bv, bok = O.fetch(ocols[B], ids, 0, tx, with_valid=True)
        both = aok & bok
        total = product_sums(av, bv, both, np.zeros(rows, dtype=np.int64), 1 if rows else 0)
        for path in paths("product"):
            got, cnt = t.sum_product(A, B, fs, residual, txn=txn, path=path)
            assert cnt == rows and (got - (total[0] if rows else 0)) % M128 == 0, (what, path, got, total, cnt, rows)
            if path is not None and rows:
                assert t.last_sum_product()[0] == (path == "slices"), (what, path)
        refused("product", lambda: t.sum_product(A, B, fs, residual, txn=txn, path="slices"))

        sums = product_sums(av, bv, both, labels, len(group_keys))
        valid_rows = np.bincount(labels, weights=None, minlength=len(group_keys))
        valid_both = np.bincount(labels[both], minlength=len(group_keys))
        wanted = {gk: (sums[i] % M128, int(valid_both[i]), int(valid_rows[i]))
                  for i, gk in enumerate(group_keys) if valid_rows[i]}
        for path in paths("product_by"):
            got = t.sum_product_by(A, B, by, fs, residual, txn=txn, path=path)
            assert {gk: (x[0] % M128, x[1], x[2]) for gk, x in got.items()} == wanted, (what, path, got, wanted)
            if path is not None and wanted:
                assert t.last_sum_product()[0] == (path == "slices"), (what, path)
        refused("product_by", lambda: t.sum_product_by(A, B, by, fs, residual, txn=txn, path="slices"))

        self.kept_before = t.derived_stats()[0]

    def finish(self, t):
        self.kept[0] += t.derived_stats()[2]
        self.kept[1] += t.row_list_stats()[2]


@pytest.mark.parametrize("seed", list(PLAN))
def test_slices_and_their_queries_through_random_maintenance(ctx, tally, kept, tmp_path, seed):
    run_plan(ctx, seed, tally, Checks(tmp_path, kept))


def test_the_generator_reached_every_maintenance_class_and_an_answer_behind_it(tally, kept):
    """Every class of sliced_maintenance_model.REQUIRED occurred and was followed by an answered forced-slices
    call on its column before that column's next write, and at least a third of the forced calls were answered:
    counted from the model (the same tally tests/test_sliced_maintenance_model.py asserts without a GPU). The
    repeated trees must also have been kept as derived leaves and used between the writes, and writes must have
    dropped what was kept (the library's own counters: derived_stats before and after each write)."""
    print(f"ops {dict(tally.ops)} forced {tally.forced} answered {tally.answered} (empty index: {tally.refused_empty}) "
          f"confirmed {dict(tally.confirmed)} derived replacements {kept[0]} row-list decodes {kept[1]} dropped by a write {kept[2]}")
    tally.check(PLAN)
    assert kept[0] > 0 and kept[2] > 0, kept
