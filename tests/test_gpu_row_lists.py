"""Row lists and the derived block pool. A sparse table-owned bitvector that scans decode alone is also
kept as 16-bit offsets per 131,072-row tile (cubit_row_list.hpp): its first decode pays nothing, the
second writes the list beside the row ids, later ones read the list in the bitvector's place. That changes
what a scan reads and never what it returns: every scan here is compared with the oracle, row ids, tile
directory and count, and with the same table once its lists are switched off. The table holds
5 * 131,072 + 4,097 rows: six tiles, the last partial. Column 0 carries an EQUALITY index whose leaves
are the shapes under test (one `=` filter is one leaf as it stands):

  1  tile 0 all in the lower half, tile 1 all in the upper half, tile 2 exactly offsets 65,535 and 65,536,
     tile 3 exactly 0 and 131,071, tile 4 empty, tile 5 its first and its last row
  2  9,000 ids in tile 1 (more than the 8,192-entry stage: the dense rounds of the build) and 500 elsewhere
  3  32,757 ids: L = 2 q + 4 tiles = 65,538, two bytes over half the bitvector's 131,072 (no list)
  4  32,756 ids: L = 65,536, exactly half (a list)
  5  no row at all

Column 1 (RANGE index) gives the second column of a kept chain."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.table import Context, CubitTable, padded_words, runs_in_row_order
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 131072
N = 5 * TILE + 4097
TILES = 6
LEAF_BYTES = padded_words(N) * 8
SENTINEL = np.int64(-0x0123456789ABCDEF)
BASES = (0, 2 ** 32 + 9)


def list_bytes(q):
    return 2 * q + 4 * TILES


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_decode_kernel(L.DECODE_AUTO)
    c.close()


@pytest.fixture(scope="module")
def data():
    """Columns (k, b) and, per value of k, the oracle's row ids at row_base 0 (never modified)."""
    rng = np.random.default_rng(131)
    k = np.zeros(N, dtype=np.int32)
    one = np.concatenate([
        np.arange(3, 65536, 37), [65535],                          # tile 0: below the half, its last row included
        TILE + np.concatenate([[65536], np.arange(65540, TILE, 41), [TILE - 1]]),  # tile 1: the upper half only
        2 * TILE + np.array([65535, 65536]),
        3 * TILE + np.array([0, TILE - 1]),
        5 * TILE + np.array([0, 4096]),
    ])
    k[one] = 1
    free = np.flatnonzero(k == 0)
    in_tile1 = free[(free >= TILE) & (free < 2 * TILE)]
    dense = rng.choice(in_tile1, 9000, replace=False)
    k[dense] = 2
    free = np.flatnonzero(k == 0)
    free = rng.permutation(free[(free < TILE) | (free >= 2 * TILE)])
    k[free[:500]] = 2
    k[free[500:500 + 32757]] = 3
    k[free[33257:33257 + 32756]] = 4
    b = rng.integers(0, 50, N).astype(np.int64)
    cols = [O.Column(k), O.Column(b)]
    refs = {v: O.table_scan(cols, F.serialize(eq(v)), N) for v in range(1, 6)}
    assert [len(refs[v]) for v in range(1, 6)] == [len(one), 9500, 32757, 32756, 0]
    for v in range(1, 5):
        assert np.array_equal(refs[v], np.flatnonzero(k == v))
    assert list_bytes(32756) == LEAF_BYTES // 2 and list_bytes(32757) > LEAF_BYTES // 2
    for x in (k, b, *refs.values()):
        x.setflags(write=False)
    return k, b, refs


def eq(v):
    return F.TableFilterSet({0: F.ConstantFilter("=", v)})


def make_table(ctx, data, row_base=0):
    k, b, _ = data
    t = CubitTable(ctx, N, row_base=row_base)
    t.add_column(0, k)
    t.add_column(1, b)
    t.build_index(0, L.INDEX_EQUALITY, [0, 1, 2, 3, 4, 5])
    t.build_index(1, L.INDEX_RANGE)
    return t


def directory_of(ids, row_base=0, n_rows=N):
    """The tile directory the decode owes for these ascending ids: {start, count}, start 0 where count is 0."""
    tiles = (n_rows + TILE - 1) // TILE
    cnt = np.bincount((ids - row_base) // TILE, minlength=tiles).astype(np.uint64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    start[cnt == 0] = 0
    return np.stack([start, cnt], axis=1)


def raw_scan(ctx, t, fs, capacity=None, ordered=False, pad=64):
    """One scan into a sentinel-filled buffer of capacity + pad ids: (the whole buffer, directory, count,
    answered from a list)."""
    cap = t.n_rows if capacity is None else capacity
    out = ctx.upload(np.full(cap + pad, SENTINEL, dtype=np.int64))
    cnt = ctx.alloc(16)
    t.scan_into(F.serialize(fs).nodes, out.addr, cap, cnt.addr, ordered=ordered)
    ctx.check()
    n = int(cnt.download(np.uint64, 1)[0])
    buf = out.download(np.int64, cap + pad)
    directory, rows_per_tile = ctx.last_tiles()
    assert rows_per_tile in (0, TILE)
    from_list = ctx.last_decode_from_list()
    out.free()
    cnt.free()
    return buf, directory, n, from_list


def check_scan(ctx, t, fs, ref, row_base=0, ordered=False, what=""):
    """One scan equal to ref in row ids, directory and count, nothing written past them; its list flag."""
    buf, directory, n, from_list = raw_scan(ctx, t, fs, ordered=ordered)
    assert n == len(ref), (what, n, len(ref))
    assert np.all(buf[n:] == SENTINEL), what
    if len(ref) or len(directory):
        assert np.array_equal(directory, directory_of(ref, row_base, t.n_rows)), what
    # runs land in tile order under the prefixed decode and the list alike
    assert np.array_equal(buf[:n], ref), what
    if len(ref):
        assert np.array_equal(runs_in_row_order(buf, directory), ref), what
        assert ctx.last_decode_kernel() == L.DECODE_PREFIXED and t.last_plan() == (1, 1), what
    return from_list


@pytest.mark.parametrize("row_base", BASES)
@pytest.mark.parametrize("v", [1, 2, 4])
def test_third_scan_reads_the_list(ctx, data, v, row_base):
    """Halves and edges of a tile (1), the dense rounds of the build (2) and a leaf exactly at the byte rule
    (4), at row_base 0 and past 2^32: scans one and two read the bitvector, three and four the list, and
    the table with its lists switched off reads the bitvector again; all equal the oracle."""
    k, b, refs = data
    ref = refs[v] + row_base
    if row_base:
        assert np.array_equal(ref, O.table_scan([O.Column(k), O.Column(b)], F.serialize(eq(v)), N, row_base))
    t = make_table(ctx, data, row_base)
    assert t.row_list_stats() == (0, 0, 0)
    flags = [check_scan(ctx, t, eq(v), ref, row_base, what=(v, i)) for i in range(4)]
    assert flags == [False, False, True, True]
    assert t.row_list_stats() == (1, list_bytes(len(ref)), 2)
    assert t.derived_stats() == (0, 0, 0)  # a list is no derived leaf
    t.use_row_lists(False)
    assert check_scan(ctx, t, eq(v), ref, row_base, what=(v, "off")) is False
    assert t.row_list_stats() == (1, list_bytes(len(ref)), 2)
    t.use_row_lists(True)
    assert check_scan(ctx, t, eq(v), ref, row_base, ordered=True, what=(v, "ordered")) is True
    assert t.row_list_stats()[2] == 3
    t.close()


def test_empty_leaf(ctx, data):
    """A leaf without rows: the zone maps answer the scan without a launch, so nothing decodes alone and no
    list is built; count 0, nothing written."""
    t = make_table(ctx, data)
    for i in range(4):
        buf, directory, n, from_list = raw_scan(ctx, t, eq(5))
        assert n == 0 and not from_list and np.all(buf == SENTINEL) and len(directory) == 0
    assert t.row_list_stats() == (0, 0, 0)
    t.close()


def test_leaf_just_over_the_rule_keeps_no_list(ctx, data):
    refs = data[2]
    t = make_table(ctx, data)
    flags = [check_scan(ctx, t, eq(3), refs[3], what=i) for i in range(4)]
    assert flags == [False] * 4 and t.row_list_stats() == (0, 0, 0)
    t.close()


@pytest.mark.parametrize("row_base", BASES)
def test_capacity_below_q(ctx, data, row_base):
    """A capacity below the qualifying rows, on the building scan and on list scans: the first `capacity`
    ids are written, the sentinels past them stay, the count is exact. The list the clamped scan built
    holds every row: a later scan with room returns them all."""
    ref = data[2][2] + row_base
    t = make_table(ctx, data, row_base)
    for i, cap in enumerate((len(ref), 9001, 4097, 1, 9100, 0)):
        buf, directory, n, from_list = raw_scan(ctx, t, eq(2), capacity=cap)
        assert n == len(ref) and from_list == (i >= 2), (i, cap)
        assert np.array_equal(buf[:cap], ref[:cap]) and np.all(buf[cap:] == SENTINEL), (i, cap)
        assert np.array_equal(directory, directory_of(ref, row_base)), (i, cap)
    assert check_scan(ctx, t, eq(2), ref, row_base) is True
    t.close()


def test_forced_kernels(ctx, data):
    """Forced PAIRS and RUNS decodes never read a list (and count nothing towards one); LOOKBACK does."""
    refs = data[2]
    t = make_table(ctx, data)
    try:
        for kernel in (L.DECODE_PAIRS, L.DECODE_RUNS):
            ctx.set_decode_kernel(kernel)
            for i in range(3):
                got = t.scan(eq(1))
                assert np.array_equal(got, refs[1]) and not ctx.last_decode_from_list()
                # (RUNS either way: the leaf's empty tile makes a live-tile list, which PAIRS cannot walk)
                assert ctx.last_decode_kernel() in (L.DECODE_PAIRS, L.DECODE_RUNS)
        assert t.row_list_stats() == (0, 0, 0)
        ctx.set_decode_kernel(L.DECODE_LOOKBACK)
        assert [check_scan(ctx, t, eq(1), refs[1], what=i) for i in range(3)] == [False, False, True]
        for kernel in (L.DECODE_PAIRS, L.DECODE_RUNS):
            ctx.set_decode_kernel(kernel)
            raw = t.scan(eq(1), ordered=False)
            directory, _ = ctx.last_tiles()
            assert np.array_equal(runs_in_row_order(raw, directory), refs[1])
            assert not ctx.last_decode_from_list() and ctx.last_decode_kernel() in (L.DECODE_PAIRS, L.DECODE_RUNS)
        assert t.row_list_stats() == (1, list_bytes(len(refs[1])), 1)
        ctx.set_decode_kernel(L.DECODE_AUTO)
        assert check_scan(ctx, t, eq(1), refs[1]) is True
    finally:
        ctx.set_decode_kernel(L.DECODE_AUTO)
        t.close()


def chain_filter():
    return F.TableFilterSet({0: F.ConstantFilter("=", 2), 1: F.ConstantFilter("<", 24)})


def test_kept_chain_decodes_from_its_list(ctx, data):
    """A chain over two columns kept as one bitvector (cost 0: its fourth request) decodes alone from then
    on: its list is written by its second such decode and read after; derived_stats keeps counting the
    bitvector only."""
    k, b, _ = data
    fs = chain_filter()
    ref = O.table_scan([O.Column(k), O.Column(b)], F.serialize(fs), N)
    assert np.array_equal(ref, np.flatnonzero((k == 2) & (b < 24))) and len(ref) > 4000
    t = make_table(ctx, data)
    t.set_derived_chain_cost(0)
    flags = []
    for i in range(8):
        buf, directory, n, from_list = raw_scan(ctx, t, fs)
        assert n == len(ref) and np.array_equal(buf[:n], ref) and np.all(buf[n:] == SENTINEL), i
        assert np.array_equal(directory, directory_of(ref)), i
        flags.append(from_list)
    # requests 1-3 read two leaves; the fourth keeps the chain and is its first decode alone, so the fifth
    # is the earliest that can build and the sixth the earliest that can read
    assert not any(flags[:5]) and flags[5:] == [True] * 3
    assert ctx.last_decode_kernel() == L.DECODE_PREFIXED and t.last_plan() == (1, 1)
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.derived_chain_stats()[0] == 1
    assert t.row_list_stats() == (1, list_bytes(len(ref)), 3)
    t.close()


def test_budget(ctx, data):
    """Budget 0: no list. A budget one byte short of the list: none either, and the scans stay right. The
    list's own bytes: built. A kept bitvector that then needs the room sheds the list first."""
    k, b, refs = data
    need = list_bytes(len(refs[1]))
    for budget, built in ((0, False), (need - 1, False), (need, True)):
        t = make_table(ctx, data)
        t.set_derived_budget(budget)
        flags = [check_scan(ctx, t, eq(1), refs[1], what=(budget, i)) for i in range(4)]
        assert flags == [False, False, built, built], budget
        assert t.row_list_stats() == ((1, need, 2) if built else (0, 0, 0)), budget
        if built:
            t.set_derived_budget(0)  # the budget goes: so does the list
            assert t.row_list_stats() == (0, 0, 2)
            assert check_scan(ctx, t, eq(1), refs[1]) is False
        t.close()
    # one bitvector and the list fit; the chain takes the bitvector's room, a second column group would not fit
    t = make_table(ctx, data)
    t.set_derived_chain_cost(0)
    t.set_derived_budget(LEAF_BYTES + need)
    assert [check_scan(ctx, t, eq(1), refs[1], what=i) for i in range(3)] == [False, False, True]
    assert t.row_list_stats()[:2] == (1, need)
    fs = chain_filter()
    ref = O.table_scan([O.Column(k), O.Column(b)], F.serialize(fs), N)
    for i in range(4):
        assert np.array_equal(t.scan(fs), ref)
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.row_list_stats()[:2] == (1, need)  # both fit
    t.set_derived_budget(LEAF_BYTES + need - 1)  # no longer: the list goes, the bitvector stays
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.row_list_stats()[:2] == (0, 0)
    assert check_scan(ctx, t, eq(1), refs[1]) is False
    t.close()


def test_lists_go_with_every_write(ctx, data):
    """After an append and after a merged update the list is gone, and the scans follow the new rows (the
    list is built again by the second of them)."""
    k, b, refs = data
    rng = np.random.default_rng(7)
    t = make_table(ctx, data)
    assert [check_scan(ctx, t, eq(1), refs[1], what=i) for i in range(3)] == [False, False, True]
    n_new = 3000
    add_k = rng.integers(0, 3, n_new).astype(np.int32)
    add_b = rng.integers(0, 50, n_new).astype(np.int64)
    t.append({0: add_k, 1: add_b})
    assert t.row_list_stats()[:2] == (0, 0)
    k2, b2 = np.concatenate([k, add_k]), np.concatenate([b, add_b])
    ref = O.table_scan([O.Column(k2), O.Column(b2)], F.serialize(eq(1)), len(k2))
    assert len(ref) > len(refs[1]) + 500 and ref[-1] >= N
    assert [check_scan(ctx, t, eq(1), ref, what=("append", i)) for i in range(3)] == [False, False, True]
    rows = np.sort(rng.choice(len(k2), size=2000, replace=False)).astype(np.int64)
    vals = rng.integers(0, 3, len(rows)).astype(np.int64)
    t.set_updates(0, rows, vals, np.full(len(rows), 3, dtype=np.uint64))
    assert t.merge_updates(0, 5) == len(rows)
    assert t.row_list_stats()[:2] == (0, 0)
    k2[rows] = vals.astype(np.int32)
    ref2 = O.table_scan([O.Column(k2), O.Column(b2)], F.serialize(eq(1)), len(k2))
    assert not np.array_equal(ref2, ref)
    assert [check_scan(ctx, t, eq(1), ref2, what=("merge", i)) for i in range(3)] == [False, False, True]
    assert t.row_list_stats()[:2] == (1, 2 * len(ref2) + 4 * TILES)
    t.close()


def test_pool_readmits_without_allocating(ctx, data):
    """A chain is admitted (the table's first admission allocates its blocks), an append drops it, the same
    scans admit it again: no device allocation the second time, one free block fewer while it is kept, and
    the results equal the oracle throughout. Budget 0 empties the pool."""
    k, b, _ = data
    fs = chain_filter()
    rng = np.random.default_rng(9)
    t = make_table(ctx, data)
    t.set_derived_chain_cost(0)
    assert t.derived_pool_stats() == (0, 0)
    ref = O.table_scan([O.Column(k), O.Column(b)], F.serialize(fs), N)
    for i in range(4):
        assert np.array_equal(t.scan(fs), ref), i
    assert t.derived_stats()[:2] == (1, LEAF_BYTES)
    free0, allocs0 = t.derived_pool_stats()
    assert allocs0 >= 1 and free0 == allocs0 - 1
    add_k = rng.integers(0, 3, 1000).astype(np.int32)
    add_b = rng.integers(0, 50, 1000).astype(np.int64)
    t.append({0: add_k, 1: add_b})  # in place: the block size stays
    assert t.derived_stats()[:2] == (0, 0)
    assert t.derived_pool_stats() == (free0 + 1, allocs0)
    k2, b2 = np.concatenate([k, add_k]), np.concatenate([b, add_b])
    ref2 = O.table_scan([O.Column(k2), O.Column(b2)], F.serialize(fs), len(k2))
    assert len(ref2) > len(ref)
    for i in range(6):
        assert np.array_equal(t.scan(fs), ref2), i
    assert t.derived_stats()[:2] == (1, LEAF_BYTES) and t.last_plan() == (1, 1)
    assert t.derived_pool_stats() == (free0, allocs0)
    t.set_derived_budget(0)
    assert t.derived_pool_stats() == (0, allocs0) and t.derived_stats()[:2] == (0, 0)
    assert np.array_equal(t.scan(fs), ref2)
    t.close()
