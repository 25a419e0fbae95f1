"""tests/test_gpu_sliced_maintenance_fuzz.py without a GPU: the generator driven against a stub table that only
records its calls, so that the reach of the fixed seeds — every maintenance class followed by an answered
forced-slices call on its column, a third of the forced calls answered — is asserted from the model alone and a
change of the generator cannot silently lose a class. The references the GPU module compares the library with
(the numpy slices, the exact product sums, the merge of an update list, the key maps) are held here against
slower restatements."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from sliced_maintenance_model import (DBL, PLAN, REQUIRED, UBIG, VALUE_COLS, WRITER, Model, Stub, Tally, bits_of_keys,
                                      keys_of, order_keys, product_sums, reference_slices, run_plan, values_of_bits)


@pytest.fixture(scope="module")
def dry():
    tally, calls = Tally(), {}
    for seed in PLAN:
        tables = []

        def make(ctx, n, row_base=0):
            tables.append(Stub(ctx, n, row_base))
            return tables[-1]

        run_plan(None, seed, tally, None, make)
        calls[seed] = tables[0]
    return tally, calls


def test_the_fixed_seeds_reach_every_class_and_an_answer_behind_it(dry):
    tally, _ = dry
    print({c: (tally.occurred[c], tally.confirmed[c]) for c in REQUIRED}, tally.forced, tally.answered)
    tally.check(PLAN)


def test_the_stub_saw_the_operations_the_tally_counted(dry):
    tally, calls = dry
    seen = {name: sum(t.calls[name] for t in calls.values()) for name in ("append", "merge_updates", "sync_column", "set_deletes")}
    assert seen["append"] == tally.ops["append"] and seen["set_deletes"] == tally.ops["deletes"]
    assert seen["sync_column"] == tally.ops["sync"] and seen["merge_updates"] >= tally.ops["merge"]
    for seed, t in calls.items():
        grows = PLAN[seed][1] is not None
        assert (t.n_rows > 1_048_576) == grows, (seed, t.n_rows)  # the capacity is crossed where planned, only there
        assert t.n_rows < (1_250_000 if grows else 500_000), (seed, t.n_rows)
        assert t.calls["close"] == 1


def test_reference_slices_bit_by_bit():
    rng = np.random.default_rng(1)
    n, nwp = 200, 8
    keys = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)
    valid = rng.random(n) > 0.2
    vmin = int(keys.min())
    got = reference_slices(keys, valid, vmin, 64, nwp)
    assert got.shape == (64, nwp)
    for k in (0, 1, 31, 32, 63):
        for r in range(n):
            bit = (int(got[k, r >> 6]) >> (r & 63)) & 1
            assert bit == (int(valid[r]) & (((int(keys[r]) - vmin) % (1 << 64)) >> k) & 1), (k, r)
        assert int(got[k, n >> 6]) >> (n & 63) == 0 and not got[k, (n >> 6) + 1:].any()  # zero past the last row
    assert reference_slices(keys, valid, vmin, 0, nwp).shape == (0, nwp)


def test_product_sums_equal_python_integers():
    rng = np.random.default_rng(2)
    n = 5000
    a = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)
    b = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)
    a[:4], b[:4] = [-(1 << 63), -(1 << 63), (1 << 63) - 1, 0], [-(1 << 63), (1 << 63) - 1, (1 << 63) - 1, 5]
    ok = rng.random(n) > 0.1
    ok[:4] = True
    labels = rng.integers(0, 7, n)
    labels[labels == 3] = 2  # label 3 stays empty
    got = product_sums(a, b, ok, labels, 7)
    for g in range(7):
        m = ok & (labels == g)
        assert got[g] == sum(int(x) * int(y) for x, y in zip(a[m], b[m])), g
    assert got[3] == 0 and product_sums(a[:0], b[:0], ok[:0], labels[:0], 0) == []


def test_key_maps_invert_and_keep_the_order():
    rng = np.random.default_rng(3)
    for typ in (L.TYPE_INT64, L.TYPE_INT32, L.TYPE_UINT64, L.TYPE_DOUBLE):
        lo, hi = (-(1 << 31), (1 << 31) - 1) if typ == L.TYPE_INT32 else (-0x7FEFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF)
        keys = np.sort(rng.integers(lo, hi, 1000, dtype=np.int64, endpoint=True))
        keys[:3] = [lo, 0, hi]
        keys = np.sort(keys)
        vals = values_of_bits(typ, bits_of_keys(typ, keys))
        assert np.array_equal(keys_of(typ, vals), keys), typ
        assert (np.diff(vals.astype(object) if typ != L.TYPE_DOUBLE else vals) >= 0).all(), typ  # ascending with the keys
        if typ == L.TYPE_DOUBLE:
            assert np.isfinite(vals).all()
    assert values_of_bits(L.TYPE_UINT64, bits_of_keys(L.TYPE_UINT64, np.array([-(1 << 63), (1 << 63) - 1])))[1] == 2 ** 64 - 1
    assert order_keys(L.TYPE_UINT64, np.array([0], dtype=np.int64))[0] == -(1 << 63)


def test_merged_records_are_each_rows_prefix_below_the_horizon():
    rng = np.random.default_rng(4)
    m = Model(rng, 3000, 0)
    for horizon in (0, 3, 6, 9, 50):
        rows, vers = [], []
        for r in np.sort(rng.choice(3000, 400, replace=False)):
            vs = sorted(set(rng.integers(1, 10, rng.integers(1, 4)).tolist())) + ([WRITER] if rng.random() < 0.3 else [])
            rows += [int(r)] * len(vs)
            vers += vs
        vals = np.arange(len(rows), dtype=np.int64)
        ok = rng.random(len(rows)) > 0.2
        m.cols[0].upd = (np.array(rows, dtype=np.int64), vals, np.array(vers, dtype=np.uint64), ok)
        got_rows, got_vals, got_ok, keep = m.merged_records(0, horizon)
        exp, kept = {}, []
        i = 0
        while i < len(rows):  # tests/test_gpu_maintenance_fuzz.py's Model.merge
            j = i
            while j < len(rows) and rows[j] == rows[i]:
                j += 1
            p = i
            while p < j and vers[p] < horizon:
                p += 1
            if p > i:
                exp[rows[i]] = (int(vals[p - 1]), bool(ok[p - 1]))
            kept += list(range(p, j))
            i = j
        assert {int(r): (int(v), bool(o)) for r, v, o in zip(got_rows, got_vals, got_ok)} == exp, horizon
        assert np.flatnonzero(keep).tolist() == kept, horizon


def test_the_models_columns_are_what_the_issue_asks_for():
    for seed in (0, 1, 2):
        m = Model(np.random.default_rng(seed), 131_072 + 77, seed)
        assert [m.cols[c].typ for c in VALUE_COLS] == [L.TYPE_INT64, L.TYPE_INT64, L.TYPE_INT32, L.TYPE_UINT64, L.TYPE_DOUBLE]
        assert sum(m.cols[c].nullable for c in range(4)) == 2 and 1 <= len(m.groups) <= 2
        assert np.isfinite(m.cols[DBL].data).all() and m.cols[UBIG].data.dtype == np.uint64
        assert all(m.cols[c].enc == L.INDEX_SLICED for c in VALUE_COLS)
