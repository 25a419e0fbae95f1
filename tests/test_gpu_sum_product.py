"""SELECT sum(a * b), count(*) WHERE <filter> against exact integers.

cubit_table_sum_product evaluates, compacts, gathers and reduces with code of its own
(eval_sum_product: tile evaluation and tail mask, the 4,096-entry stage and the dense-tile
bypass, the packed-a reader and its staged group records, b decoded from its range index, the
128-bit wave / block reduce), next to gather_sum_product_kernel, sum_product_arrays_kernel (the
MVCC fallback) and the host logic that chooses among them. Every result here is compared with
`==` against Python integers over the oracle's rows: the rows come from O.table_scan, the sum
from a.astype(object) * b.astype(object) over those rows where a and b are both valid, the count
is the number of rows.
"""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_gpu_planner_fuzz import TXN_START, rand_const_filter, rand_residual

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
M64 = 2 ** 64
TILE = 131_072   # rows per tile of the fused kernel
STAGE = 4096     # rows of a tile the kernel stages in LDS; a tile that keeps more is summed directly


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def products(a, b, va=None, vb=None):
    """a[i] * b[i] as Python ints (0 where a or b is NULL: such a row adds nothing to a SUM)."""
    p = a.astype(object) * b.astype(object)
    if va is not None:
        p[~va] = 0
    if vb is not None:
        p[~vb] = 0
    return p


def total(prod, idx):
    return int(prod[idx].sum()) if len(idx) else 0


def in_int128(x):
    return -(2 ** 127) <= x < 2 ** 127


def gather_sum(ctx, d_a, d_b, d_ids, d_cnt, max_n, row_base):
    out = ctx.alloc(16)
    L.check(ctx.lib.cubit_gather_sum_product(ctx.handle, d_a.ptr, d_b.ptr, d_ids.ptr, d_cnt.ptr, max_n, row_base,
                                             out.ptr))
    ctx.check()
    lo, hi = (int(x) for x in out.download(np.int64, 2))
    out.free()
    return (hi << 64) + (lo & (M64 - 1))


def top_level_or(plan):
    """A child of the plan's root AND is an OR (a pushed column's filter, or the residual tree)."""
    def end(i):
        j = i + 1
        for _ in range(plan.nodes[i][3]):
            j = end(j)
        return j
    j = 1
    for _ in range(plan.nodes[0][3]):
        if plan.nodes[j][0] == L.FILTER_OR:
            return True
        j = end(j)
    return False


# ------------------------------------------------------------------ A. differential fuzz

# 12 values of b, spread widely: negatives, small ones, values past 2^31 and past 2^40
B_VALUES = np.array([-(2 ** 44) - 3, -(2 ** 33) + 1, -70_000, -2, 0, 5, 1000, 2 ** 31 + 7, 2 ** 35, 2 ** 40 + 11,
                     2 ** 42 - 5, 2 ** 44 + 1], dtype=np.int64)


def rand_b_filter(rng):
    """A top-level constant filter on b: equality, a closed range covering 1, 2, 3, 4 or 6 of its
    values (bounds on the values or just outside them), or an open range."""
    r = rng.random()
    if r < 0.2:
        return F.ConstantFilter("=", int(B_VALUES[rng.integers(0, len(B_VALUES))]))
    if r < 0.85:
        k = int(rng.choice([1, 2, 3, 4, 6]))
        i = int(rng.integers(0, len(B_VALUES) - k + 1))
        lo, hi = int(B_VALUES[i]), int(B_VALUES[i + k - 1])
        lo_f = F.ConstantFilter(">=", lo) if rng.random() < 0.5 else F.ConstantFilter(">", lo - 1)
        hi_f = F.ConstantFilter("<=", hi) if rng.random() < 0.5 else F.ConstantFilter("<", hi + 1)
        return F.ConjunctionAndFilter([lo_f, hi_f])
    return F.ConstantFilter(["<", "<=", ">", ">="][rng.integers(0, 4)], int(B_VALUES[rng.integers(0, len(B_VALUES))]))


def fused_sum_fuzz(ctx, seed, iters):
    """Random filter sets (with residual trees, with a filter on b, under a transaction that sees
    deletes) through the fused sum with b decoded / gathered and the zonemap skip on / off; every
    result equals the exact one. Returns the coverage tallies."""
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
    # a: small values and full-range ones below 2^62; b: 12 values, exact range index.
    # |sum| < 400,003 * 2^62 * (2^44 + 3) < 2^125
    a = np.where(rng.random(n) < 0.5, rng.integers(-10_000, 10_000, n), rng.integers(-(2 ** 62) + 1, 2 ** 62, n))
    a = a.astype(np.int64)
    va = rng.random(n) > 0.15
    b = B_VALUES[rng.integers(0, len(B_VALUES), n)]
    vb = rng.random(n) > 0.10
    for c, (d, v) in ((4, (a, va)), (5, (b, vb))):
        vw = validity_from_mask(v)
        t.add_column(c, d, vw)
        ocols.append(O.Column(d, vw))
    t.build_index(5, L.INDEX_RANGE)
    prod = products(a, b, va, vb)
    dels = np.arange(0, n, 7, dtype=np.int64)
    deleted = np.full(n, np.uint64(2 ** 64 - 2), dtype=np.uint64)
    deleted[dels] = 5
    t.set_deletes(dels, np.full(len(dels), 5, dtype=np.uint64))

    tally = {"leaves": set(), "multipass": 0, "decode": set(), "or": 0, "residual": 0, "dense": 0, "sparse": 0,
             "b_filter": 0, "txn": 0, "empty": 0}

    def check(i, fs, residual, txn, tx):
        plan = F.serialize(fs, residual)
        rows = O.table_scan(ocols, plan, n, row_base=base, tx=tx)
        want = (total(prod, rows - base), len(rows))
        per_tile = np.bincount((rows - base) // TILE, minlength=4)
        tally["dense"] += bool(per_tile.max() > STAGE)
        tally["sparse"] += bool(len(rows) and per_tile.max() < STAGE)
        tally["empty"] += len(rows) == 0
        for g in (False, True):
            for z in (False, True):
                got = t.sum_product(4, 5, fs, residual, txn=txn, gather_b=g, zonemap=z)
                assert got == want, (seed, i, "txn" if txn else "", g, z, fs.filters, plan.nodes)
                if len(rows):  # (a filter folded to FALSE launches nothing and reports nothing new)
                    k, passes = t.last_plan()
                    tally["leaves"].add(k)
                    tally["multipass"] += passes > 1
                    if g:
                        assert t.last_sum_decode() == 0
                    else:
                        tally["decode"].add(t.last_sum_decode())

    # the whole table, and a filter that folds to FALSE (column 0's exact index ends at 49)
    check(-2, F.TableFilterSet(), None, None, None)
    check(-1, F.TableFilterSet({0: F.ConstantFilter(">", 1000)}), None, None, None)
    assert tally["empty"] == 1
    for i in range(iters):
        filters = {}
        for c in rng.choice(4, size=rng.integers(0, 4), replace=False):
            filters[int(c)] = rand_const_filter(rng)
        fs = F.TableFilterSet(filters)
        if rng.random() < 0.5:
            fs.push_filter(5, rand_b_filter(rng))
            tally["b_filter"] += 1
        residual = rand_residual(rng, 4) if rng.random() < 0.5 else None
        tally["residual"] += residual is not None
        tally["or"] += top_level_or(F.serialize(fs, residual))
        check(i, fs, residual, None, None)
        if i % 4 == 0:
            tally["txn"] += 1
            check(i, fs, residual, L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=deleted))
    t.close()
    return tally


FUZZ_SEED, FUZZ_ITERS = 2025, 120


def test_fused_sum_fuzz_matches_exact_integers(ctx):
    """Seed 2025, 120 plans (+ the whole table and a FALSE fold; 30 of them again under the
    transaction): the tallies are asserted below so that the test cannot pass vacuously.
    Measured with this seed: leaf counts {1..8}, 128 runs of more than one pass, decode {0, 1, 2,
    3, 4}, 28 plans with a top-level OR, 63 with a residual, 52 with a filter on b, 79 checks with
    a tile above 4,096 rows and 21 with every tile below, 52 with no row (seeds 2026 and 2027 meet
    every condition too)."""
    tally = fused_sum_fuzz(ctx, FUZZ_SEED, FUZZ_ITERS)
    print("fused sum fuzz tallies:", tally)
    assert set(range(1, 9)) <= tally["leaves"], tally      # every leaf count 1..8 …
    assert tally["multipass"] >= 1, tally                  # … and a plan of more than one pass
    assert {0, 1, 2, 3, 4} <= tally["decode"], tally       # b gathered and decoded from 1, 2, 3, 4 values
    assert tally["or"] >= 10 and tally["residual"] >= 10, tally
    assert tally["dense"] >= 1 and tally["sparse"] >= 1, tally  # the direct and the staged path


# ------------------------------------------------------------------ B. b pinned to one or two values

def test_b_pinned_to_one_or_two_values(ctx):
    """A filter that leaves b one value decodes it from no leaf at all: the kernel multiplies by
    that value (last_sum_decode() == 1). One, two and no value, on sparse (staged) and dense
    (direct) tiles, decoded and gathered."""
    rng = np.random.default_rng(31)
    n = 300_007
    vals = np.array([-(2 ** 40) + 11, -5, 3, 2 ** 33 - 3, 2 ** 33 + 17, 2 ** 45], dtype=np.int64)
    b = vals[rng.integers(0, len(vals), n)]
    vb = rng.random(n) > 0.05
    a = rng.integers(-(10 ** 12), 10 ** 12, n).astype(np.int64)
    va = rng.random(n) > 0.1
    # c: sparse tiles (2 % pass) in the first half, every row passes in the second (dense tiles)
    c = rng.integers(0, 1000, n).astype(np.int32)
    c[n // 2:] = 0
    t = CubitTable(ctx, n)
    t.add_column(0, a, validity_from_mask(va))
    t.add_column(1, b, validity_from_mask(vb))
    t.add_column(2, c)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE)
    ocols = [O.Column(a, validity_from_mask(va)), O.Column(b, validity_from_mask(vb)), O.Column(c)]
    prod = products(a, b, va, vb)

    def eq(v):
        return F.ConstantFilter("=", int(v))

    def rng_f(lo, hi):
        return F.ConjunctionAndFilter([F.ConstantFilter(">=", int(lo)), F.ConstantFilter("<=", int(hi))])

    cases = [("= vmin", eq(vals[0]), 1), ("= middle", eq(vals[3]), 1), ("= vmax", eq(vals[5]), 1),
             (">= k AND <= k", rng_f(vals[2], vals[2]), 1), ("one key inside", rng_f(vals[1] + 1, vals[3] - 1), 1),
             ("two keys", rng_f(vals[3], vals[4]), 2), ("vmin and a key", rng_f(vals[0] - 9, vals[1]), 2),
             ("absent, inside", eq(4), None), ("absent, below vmin", eq(vals[0] - 1), None)]
    for name, bf, decoded in cases:
        for cf in (F.ConstantFilter("<", 20), None):  # with the sparse / dense column, and b's filter alone
            fs = F.TableFilterSet({1: bf} if cf is None else {1: bf, 2: cf})
            rows = O.table_scan(ocols, F.serialize(fs), n)
            want = (total(prod, rows), len(rows))
            if decoded is None:
                assert want == (0, 0)
            else:
                assert len(rows) > STAGE  # the second half's tiles are summed directly
            for gather in (False, True):
                assert t.sum_product(0, 1, fs, gather_b=gather) == want, (name, cf, gather)
                if decoded is not None:
                    assert t.last_sum_decode() == (0 if gather else decoded), (name, cf, gather)
    t.close()


# ------------------------------------------------------------------ C. 128-bit extremes, four reduce paths

N_C = 262_147  # two whole tiles and a tail of three rows


def force_low_word(a, b, groups, low):
    """Rewrite the last three rows of every group so that the group's exact sum of products is
    low (mod 2^64): a = 1 and three values of b that add up to the missing amount."""
    for g in groups:
        assert len(g) >= 3
        fix, rest = g[-3:], g[:-3]
        r = (low - int(products(a[rest], b[rest]).sum())) % M64
        a[fix] = 1
        b[fix] = [r // 3, r // 3, r - 2 * (r // 3)]  # each below 2^63
    return a, b


def extremes_input(rng):
    """Bulk rows |a| < 2^63, |b| < 2^31 of mixed signs, and in front of them a fixed set with
    operands from {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX}: exactly one INT64_MIN * INT64_MIN
    (2^126) and one INT64_MIN * INT64_MAX, which nearly cancel."""
    a = rng.integers(I64_MIN + 1, I64_MAX, N_C, dtype=np.int64, endpoint=True)
    b = rng.integers(-(2 ** 31) + 1, 2 ** 31, N_C).astype(np.int64)
    fixed = [(I64_MIN, I64_MIN), (I64_MIN, I64_MAX), (I64_MIN + 1, I64_MAX), (I64_MAX, I64_MAX), (I64_MAX, -1),
             (-1, I64_MIN + 1), (I64_MIN, 0), (0, I64_MIN), (I64_MIN, 1), (1, I64_MAX), (-1, -1), (I64_MIN + 1, -1)]
    # spread over the tiles: the first rows, rows around the tile edge, the three-row tail
    at = list(range(6)) + [TILE - 1, TILE, TILE + 1, N_C - 3, N_C - 2, N_C - 1]
    for r, (x, y) in zip(at, fixed):
        a[r], b[r] = x, y
    return a, b, np.array(at)


def negative_zero_low_input(rng):
    """A negative total whose low word is zero: every carry of the low words has to reach the
    high word for the result to come out."""
    a, b, at = extremes_input(rng)
    a[0], b[0] = I64_MIN, 2 ** 62   # -2^125 in place of the 2^126: the total is about -2^126 - 2^125
    return a, b, at


def run_reduce_paths(ctx, a, b, key, upd_row, upd_value):
    """The same a, b and row sets through the four reduce paths. key = 0 on the sparse set S
    (≤ 4,096 rows of a tile: staged), key >= 0 on every row (direct). The fallback runs under a
    transaction that sees b[upd_row] = upd_value."""
    n = len(a)
    t = CubitTable(ctx, n, row_base=7)
    t.add_column(0, a)
    t.add_column(1, b)
    t.add_column(2, key)
    t.build_index(2, L.INDEX_RANGE)
    ocols = [O.Column(a), O.Column(b), O.Column(key)]
    sparse, dense = F.TableFilterSet({2: F.ConstantFilter("=", 0)}), F.TableFilterSet({2: F.ConstantFilter(">=", 0)})
    s_rows = O.table_scan(ocols, F.serialize(sparse), n, row_base=7) - 7
    all_rows = O.table_scan(ocols, F.serialize(dense), n, row_base=7) - 7
    assert np.array_equal(s_rows, np.nonzero(key == 0)[0]) and np.array_equal(all_rows, np.arange(n))
    assert np.bincount(s_rows // TILE).max() <= STAGE and n // 2 > STAGE
    prod = products(a, b)
    b_seen = b.copy()
    b_seen[upd_row] = upd_value
    prod_seen = products(a, b_seen)
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    for name, fs, rows in (("sparse", sparse, s_rows), ("dense", dense, all_rows)):
        want = total(prod, rows)
        assert in_int128(want) and in_int128(total(prod_seen, rows))  # the only precondition: modular below
        # fused: staged (sparse) / direct (dense)
        assert t.sum_product(0, 1, fs) == (want, len(rows)), ("fused", name)
        # cubit_gather_sum_product on the scan's row ids
        ids = t.scan(fs)
        assert np.array_equal(ids, rows + 7)
        d_ids, d_cnt = ctx.upload(ids), ctx.upload(np.array([len(ids)], dtype=np.uint64))
        assert gather_sum(ctx, d_a, d_b, d_ids, d_cnt, len(ids), 7) == want, ("gather", name)
        d_ids.free()
        d_cnt.free()
    # the MVCC fallback (scan + probes + sum_product_arrays_kernel): one visible update on b
    t.set_updates(1, np.array([upd_row], np.int64), np.array([upd_value], np.int64), np.array([3], np.uint64))
    txn = L.Txn(10, TXN_START + 1)
    for name, fs, rows in (("sparse", sparse, s_rows), ("dense", dense, all_rows)):
        assert t.sum_product(0, 1, fs, txn=txn) == (total(prod_seen, rows), len(rows)), ("arrays", name)
        assert t.sum_product(0, 1, fs) == (total(prod, rows), len(rows)), ("fused beside updates", name)
    d_a.free()
    d_b.free()
    t.close()


def sparse_key(rng, n, must):
    """key = 0 on about 2 % of the rows and on `must`, 1..99 elsewhere."""
    key = rng.integers(1, 100, n).astype(np.int32)
    key[rng.random(n) < 0.02] = 0
    key[must] = 0
    return key


def test_int128_extremes_on_every_reduce_path(ctx):
    rng = np.random.default_rng(128)
    a, b, at = extremes_input(rng)
    prod = products(a, b)
    assert sum(1 for p in prod if p == 2 ** 126) == 1 and sum(1 for p in prod if p == I64_MIN * I64_MAX) == 1
    # row 4 (INT64_MAX, -1) is the updated one: b becomes 1 under the transaction
    run_reduce_paths(ctx, a, b, sparse_key(rng, N_C, at), 4, 1)


def test_negative_total_with_zero_low_word(ctx):
    rng = np.random.default_rng(129)
    a, b, at = negative_zero_low_input(rng)
    key = sparse_key(rng, N_C, at)
    s_rows, others = np.nonzero(key == 0)[0], np.nonzero(key != 0)[0]
    # the updated row holds a = 0: the fallback sees the same products
    upd = int(others[0])
    a[upd] = 0
    # the sparse set's sum on three of its rows outside the fixed set, then every row's on three
    # rows outside the sparse set
    s_free = s_rows[~np.isin(s_rows, at)]
    force_low_word(a, b, [np.concatenate([s_rows[np.isin(s_rows, at)], s_free])], 0)
    force_low_word(a, b, [np.concatenate([s_rows, others])], 0)
    prod = products(a, b)
    for rows in (s_rows, np.arange(N_C)):
        w = total(prod, rows)
        assert w < 0 and w % M64 == 0, hex(w)
    run_reduce_paths(ctx, a, b, key, upd, 12345)


def test_every_partial_carries(ctx):
    """Per-workgroup partials whose low word is 2^64 - 1 everywhere: each 128-bit add of the
    final reduce carries. The fused kernel's partial is a tile's sum (one tile per workgroup
    here); the gather and arrays kernels' is the sum of 256 consecutive ids."""
    rng = np.random.default_rng(130)
    # fused, staged and direct: the kept rows of every tile add up to -1 (mod 2^64)
    for dense in (False, True):
        a = rng.integers(I64_MIN + 1, I64_MAX, N_C, dtype=np.int64, endpoint=True)
        b = rng.integers(-(2 ** 31) + 1, 2 ** 31, N_C).astype(np.int64)
        key = np.zeros(N_C, np.int32) if dense else sparse_key(rng, N_C, np.arange(N_C - 3, N_C))
        kept = np.nonzero(key == 0)[0]
        tiles = [kept[kept // TILE == k] for k in range(3)]
        force_low_word(a, b, tiles, M64 - 1)
        prod = products(a, b)
        assert all(total(prod, g) % M64 == M64 - 1 for g in tiles)
        t = CubitTable(ctx, N_C, row_base=7)
        t.add_column(0, a)
        t.add_column(1, b)
        t.add_column(2, key)
        t.build_index(2, L.INDEX_RANGE)
        want = total(prod, kept)
        assert in_int128(want)
        assert t.sum_product(0, 1, F.TableFilterSet({2: F.ConstantFilter("=", 0)})) == (want, len(kept)), dense
        t.close()
    # gather and arrays: 1,024 blocks of 256 ids, each adding up to -1 (mod 2^64)
    n = 1024 * 256
    a = rng.integers(I64_MIN + 1, I64_MAX, n, dtype=np.int64, endpoint=True)
    b = rng.integers(-(2 ** 31) + 1, 2 ** 31, n).astype(np.int64)
    a[5] = 0  # the updated row
    force_low_word(a, b, [np.arange(k * 256, k * 256 + 256) for k in range(1024)], M64 - 1)
    prod = products(a, b)
    want = total(prod, np.arange(n))
    assert in_int128(want) and want % M64 == (-1024) % M64
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    d_ids, d_cnt = ctx.upload(np.arange(n, dtype=np.int64) + 7), ctx.upload(np.array([n], dtype=np.uint64))
    assert gather_sum(ctx, d_a, d_b, d_ids, d_cnt, n, 7) == want
    t = CubitTable(ctx, n, row_base=7)
    t.add_column(0, a)
    t.add_column(1, b)
    t.set_updates(1, np.array([5], np.int64), np.array([99], np.int64), np.array([3], np.uint64))
    assert t.sum_product(0, 1, F.TableFilterSet(), txn=L.Txn(10, TXN_START + 1)) == (want, n)
    t.close()


# ------------------------------------------------------------------ D. cubit_gather_sum_product on its own

@pytest.mark.parametrize("row_base", [0, 11, 2 ** 33])
def test_gather_sum_product_counts_and_row_base(ctx, row_base):
    """Unsorted, repeated ids over a row base; the device count below, at and above max_n (only
    max_n ids are summed then) and zero."""
    rng = np.random.default_rng(77)
    n_rows, max_n = 50_000, 100_000
    a = rng.integers(I64_MIN + 1, I64_MAX, n_rows, dtype=np.int64, endpoint=True)
    b = rng.integers(-(2 ** 40), 2 ** 40, n_rows).astype(np.int64)
    idx = rng.integers(0, n_rows, max_n + 1)          # every row about twice, in random order
    idx[:5] = [n_rows - 1, 0, 0, n_rows - 1, 17]
    prefix = np.concatenate([[0], np.cumsum(products(a, b)[idx])])  # exact sums of the first k ids
    assert in_int128(int(min(prefix))) and in_int128(int(max(prefix)))
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    d_ids = ctx.upload(idx.astype(np.int64) + row_base)
    assert prefix[max_n] != prefix[max_n + 1]  # the id past max_n would change the sum
    for count in (0, 1, 99_999, 100_000, 100_001):
        d_cnt = ctx.upload(np.array([count], dtype=np.uint64))
        assert gather_sum(ctx, d_a, d_b, d_ids, d_cnt, max_n, row_base) == int(prefix[min(count, max_n)]), count
        d_cnt.free()
    for buf in (d_a, d_b, d_ids):
        buf.free()


# ------------------------------------------------------------------ E. packed a: many groups, wide groups

def packed_pieces(a, valid, cuts):
    """Each piece [s, e) compressed on its own (FOR groups) and the segments concatenated."""
    parts, offs, counts, pos = [], [], [], 0
    for s, e in cuts:
        c = O.bp_compress(a[s:e], None if valid is None else valid[s:e], "for")
        assert c is not None and set(O.bp_group_modes(c)) <= {"for"}
        data = np.concatenate([c.data, np.zeros((-len(c.data)) % 8, np.uint8)])
        parts.append(data)
        offs.append(c.seg_off + pos)
        counts.append(c.seg_count)
        pos += len(data)
    data = np.concatenate(parts)
    offs, counts = np.concatenate(offs).astype(np.uint64), np.concatenate(counts).astype(np.uint64)
    ok = slice(None) if valid is None else valid
    assert np.array_equal(O.bp_decode(O.BitpackedColumn(data, offs, None, counts, a.dtype))[ok], a[ok])
    return data, offs, counts


def groups_in_tile(seg_count, tile):
    """Groups (2,048 rows of a segment, fewer at its end) that hold rows of the tile."""
    k, row = 0, 0
    for c in (int(x) for x in seg_count):
        for g0 in range(0, c, 2048):
            g1 = min(g0 + 2048, c)
            k += row + g0 < (tile + 1) * TILE and row + g1 > tile * TILE
        row += c
    return k


def short_segments(rng, with_nulls):
    n = 270_011
    a = rng.integers(-(2 ** 39), 2 ** 39, n).astype(np.int64)
    valid = rng.random(n) > 0.15 if with_nulls else None
    cuts = [(s, s + 1000) for s in range(0, 140_000, 1000)] + [(140_000, n)]
    data, offs, counts = packed_pieces(a, valid, cuts)
    # 140 one-group segments, then the rest: tile 0 reads 132 groups, more than the 96 records
    # the kernel stages (the rows past them come from the unpacked column)
    assert len(counts) == 143 and groups_in_tile(counts, 0) == 132 and groups_in_tile(counts, 1) <= 96
    return n, 3, a, valid, data, offs, counts


def wide_groups(rng):
    widths = [33, 40, 0, 47, 57, 63]
    n = 2048 * len(widths) * 11 + 77  # 66 whole groups and a short one: past one tile
    a = np.empty(n, dtype=np.int64)
    for g, s in enumerate(range(0, n, 2048)):
        w = widths[g % len(widths)]
        k = min(2048, n - s)
        lo = -(2 ** 62) + int(rng.integers(0, 1000))
        blk = lo + (rng.integers(0, 2 ** w, k, dtype=np.uint64).astype(np.int64) if w else np.zeros(k, np.int64))
        if w:
            blk[int(rng.integers(0, k))] = lo
            blk[(int(np.argmin(blk)) + 1) % k] = lo + 2 ** w - 1
        assert int(blk.max()) - int(blk.min()) < 2 ** w and (int(blk.max()) - int(blk.min())).bit_length() == w
        a[s:s + k] = blk
    data, offs, counts = packed_pieces(a, None, [(0, n)])
    assert np.all(counts[:-1] % 2048 == 0)  # whole-group segments
    return n, 0, a, None, data, offs, counts


@pytest.mark.parametrize("case", ["short_segments", "wide_groups", "short_segments_nulls"])
def test_packed_a_beyond_staged_records_and_32_bits(ctx, case):
    """a read from its BITPACKING segments where the tile has more groups than the kernel stages
    (ragged one-group segments), where the FOR width passes 32 bits (two- and three-word reads,
    33 … 63 bits, an all-equal group between), and with NULLs: packed == plain == exact, on
    staged and direct tiles."""
    rng = np.random.default_rng({"short_segments": 51, "wide_groups": 52, "short_segments_nulls": 53}[case])
    n, base, a, valid, data, offs, counts = (wide_groups(rng) if case == "wide_groups"
                                             else short_segments(rng, case.endswith("nulls")))
    b = rng.integers(-50, 50, n).astype(np.int64)
    key = rng.integers(0, 100, n).astype(np.int32)
    vw = None if valid is None else validity_from_mask(valid)
    t = CubitTable(ctx, n, row_base=base)
    t.add_bitpacked_column(0, data, offs, counts, np.int64, validity=vw)
    t.add_column(1, b)
    t.add_column(2, key)
    t.build_index(2, L.INDEX_RANGE)
    ok = slice(None) if valid is None else valid
    assert np.array_equal(t.download_column(0)[ok], a[ok])
    ocols = [O.Column(a, vw), O.Column(b), O.Column(key)]
    prod = products(a, b, valid)
    for f in (F.ConstantFilter("<", 2), F.ConstantFilter(">=", 0)):  # 2 % (staged), every row (direct)
        fs = F.TableFilterSet({2: f})
        rows = O.table_scan(ocols, F.serialize(fs), n, row_base=base)
        per_tile = np.bincount((rows - base) // TILE)
        assert per_tile.max() <= STAGE if f.comparison == "<" else per_tile.min() > STAGE
        want = (total(prod, rows - base), len(rows))
        got_packed = t.sum_product(0, 1, fs)
        assert t.last_sum_packed()
        got_plain = t.sum_product(0, 1, fs, packed_a=False)
        assert not t.last_sum_packed()
        assert got_packed == want and got_plain == want, (case, f)
    t.close()


# ------------------------------------------------------------------ F. tile-edge row counts

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 131_071, 131_072, 131_073])
def test_tile_edge_row_counts(ctx, n):
    """Row counts around a word and around a tile (a last tile of one row), nullable a and b, a row
    base: no filter, b decoded from a three-value range, IS NOT NULL on a."""
    rng = np.random.default_rng(1000 + n)
    vals = np.array([-(2 ** 41), -3, 8, 2 ** 32 + 1, 2 ** 36, 2 ** 43 - 7], dtype=np.int64)
    a = rng.integers(-(2 ** 62), 2 ** 62, n).astype(np.int64)
    b = vals[(np.arange(n) * 5 + 2) % 6]  # every value from six rows on
    va, vb = rng.random(n) > 0.2, rng.random(n) > 0.2
    if n:
        va[-1] = vb[-1] = True  # the last row (alone in its tile at 131,073) counts
        b[-1] = vals[2]
    t = CubitTable(ctx, n, row_base=5)
    t.add_column(0, a, validity_from_mask(va))
    t.add_column(1, b, validity_from_mask(vb))
    t.build_index(1, L.INDEX_RANGE)
    ocols = [O.Column(a, validity_from_mask(va)), O.Column(b, validity_from_mask(vb))]
    prod = products(a, b, va, vb)
    three = F.ConjunctionAndFilter([F.ConstantFilter(">=", int(vals[1])), F.ConstantFilter("<=", int(vals[3]))])
    for name, fs in (("none", F.TableFilterSet()), ("b in three values", F.TableFilterSet({1: three})),
                     ("a is not null", F.TableFilterSet({0: F.IsNotNullFilter()}))):
        if n == 0:
            want = (0, 0)
        else:
            rows = O.table_scan(ocols, F.serialize(fs), n, row_base=5)
            want = (total(prod, rows - 5), len(rows))
            if name == "none":
                assert len(rows) == n
        for gather in (False, True):
            assert t.sum_product(0, 1, fs, gather_b=gather) == want, (n, name, gather)
            if name.startswith("b in") and want[1]:
                # decoded from as many values as b takes in the range among its valid rows
                k = len(set(b[vb].tolist()) & {int(v) for v in vals[1:4]})
                assert t.last_sum_decode() == (0 if gather else k), (n, gather)
                assert n < 63 or k == 3
    t.close()
