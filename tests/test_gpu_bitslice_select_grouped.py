"""The grouped slice select's kernels through their low-level entry point (cubit_bitslice_select_grouped)
against np.sort per group: {value, found, count_below, count_equal, count_valid, count_rows} at
d_out + 6 * g over the rows of group g, from slices built by cubit_bitslice_build and hand-built,
pairwise disjoint group bitvectors. Axes: slice counts 0 … 64 on both sides of the chunk width (64: base
INT64_MIN, top INT64_MAX), group counts on both sides of the batch of 8, row counts around one 64-row
word and one 131,072-row tile, validity NULL and given (exactly ceil(n / 64) words), filter NULL and
given (the padding past the rows set), rows in no group, and one group holding every row with the rest
empty. Each row count takes a seeded sample of the other axes that holds every value of every axis."""
import ctypes as C
import itertools

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd.table import Context
from test_gpu_bitslice_select import expected, offsets, pack, quantile_rank, slices_on_device

pytestmark = pytest.mark.gpu

BATCH = 8  # kGroupBatchSelect (cubit_program.hpp)
SLICES = [0, 1, 3, 4, 5, 8, 12, 13, 64]
GROUPS = [1, BATCH, BATCH + 1, 2 * BATCH + 1]
N_ROWS = [1, 63, 64, 65, 131_072, 131_073, 2 * 131_072 + 37]
VALIDITY = [False, True]
FILTER = [False, True]
SHAPES = ["spread", "one holds all"]  # spread: rows in every group and a tenth of the rows in none
AXES = [SLICES, GROUPS, VALIDITY, FILTER, SHAPES]
SAMPLE = 14
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def sample_for(n):
    """A seeded sample of the other axes' combinations in which every value of every axis occurs: each
    axis is walked through a shuffled copy, so SAMPLE >= its length covers it."""
    rng = np.random.default_rng(9000 + n)
    walks = [[axis[i] for i in rng.permutation(len(axis))] for axis in AXES]
    return [tuple(w[i % len(w)] for w in walks) for i in range(SAMPLE)]


def check_case(ctx, rng, n, bits, n_groups, with_validity, with_filter, shape):
    pw = int(ctx.lib.cubit_padded_words(n))
    nw = (n + 63) // 64
    base = -(1 << (bits - 1)) if bits else 7
    u = offsets(rng, n, bits, "random")
    if rng.random() < 0.3:  # heavy ties
        u = u[rng.integers(0, min(n, 3), n)]
    keys = (u + np.uint64(base & U64)).view(np.int64)  # wraps as the unsigned sum does
    valid = rng.random(n) >= 0.1 if with_validity else np.ones(n, dtype=bool)
    rows = rng.random(n) < 0.6 if with_filter else np.ones(n, dtype=bool)
    if shape == "spread":
        grp = rng.integers(0, n_groups, n)
        grp = np.minimum(grp, rng.integers(0, n_groups, n))  # skewed: group 0 the largest
        grp[rng.random(n) < 0.1] = -1  # in no group
    else:
        grp = np.full(n, int(rng.integers(0, n_groups)))
    d_col = ctx.upload(keys)
    d_val = ctx.upload(pack(valid, nw)) if with_validity else None  # ceil(n / 64) words only
    vp = d_val.ptr if d_val else None
    d_f = ctx.upload(pack(rows, pw, pad_ones=True)) if with_filter else None
    fp = d_f.ptr if d_f else None
    masks = np.concatenate([pack(grp == g, pw) for g in range(n_groups)])
    d_g = ctx.upload(masks)
    gptrs = (C.c_void_p * n_groups)(*[d_g.addr + g * pw * 8 for g in range(n_groups)])
    buf, ptrs = slices_on_device(ctx, bits, pw)
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, L.TYPE_INT64, vp, n, base, bits, ptrs))
    out = ctx.alloc(n_groups * 48)
    sorted_keys = [np.sort(keys[rows & valid & (grp == g)]) for g in range(n_groups)]
    count_rows = [int((rows & (grp == g)).sum()) for g in range(n_groups)]
    largest = max(len(s) for s in sorted_keys)
    where = (n, bits, n_groups, with_validity, with_filter, shape)

    def run(mode, k, q):
        L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, n_groups * 48))  # every slot must be written
        L.check(ctx.lib.cubit_bitslice_select_grouped(ctx.handle, ptrs, bits, vp, fp, gptrs, n_groups, n, L.TYPE_INT64,
                                                      base, mode, k, q, out.ptr))
        ctx.check()
        return [tuple(int(x) for x in row) for row in out.download(np.int64, n_groups * 6).reshape(n_groups, 6)]

    for rank in sorted({0, 1, largest // 2, max(largest - 1, 0), largest}):
        for desc in (False, True):
            got = run(L.SELECT_RANK_DESC if desc else L.SELECT_RANK, rank, 0.0)
            want = [expected(s, int, cr, desc, rank) for s, cr in zip(sorted_keys, count_rows)]
            assert got == want, (where, "rank", rank, desc)
    for q in (0.0, 0.1, 0.5, 1.0):
        got = run(L.SELECT_QUANTILE, 12345, q)
        want = [expected(s, int, cr, False, quantile_rank(len(s), q) if len(s) else 0) for s, cr in zip(sorted_keys, count_rows)]
        assert got == want, (where, "q", q)
    if n_groups == 1 and shape == "one holds all":  # one group of every row: the ungrouped call's numbers
        one = ctx.alloc(48)
        L.check(ctx.lib.cubit_bitslice_select(ctx.handle, ptrs, bits, vp, fp, n, L.TYPE_INT64, base, L.SELECT_QUANTILE, 0, 0.5,
                                              one.ptr))
        ctx.check()
        assert tuple(int(x) for x in one.download(np.int64, 6)) == run(L.SELECT_QUANTILE, 0, 0.5)[0]
        one.free()
    for b in (d_col, d_val, d_f, d_g, buf, out):
        if b:
            b.free()


def test_each_sample_holds_every_value_of_every_axis():
    """A condition on the sample, not on the library."""
    assert SAMPLE >= max(len(axis) for axis in AXES)
    for n in N_ROWS:
        cases = sample_for(n)
        for i, axis in enumerate(AXES):
            assert {c[i] for c in cases} == set(axis), (n, i)
    assert len(list(itertools.product(*AXES))) > SAMPLE  # (the whole product is not cheap: hence the sample)


@pytest.mark.parametrize("n", N_ROWS)
def test_grouped_select_matches_sorted_keys_per_group(ctx, n):
    rng = np.random.default_rng(5000 + n)
    cases = sample_for(n)
    for i, axis in enumerate(AXES):
        assert {c[i] for c in cases} == set(axis), (n, i)
    for bits, n_groups, with_validity, with_filter, shape in cases:
        check_case(ctx, rng, n, bits, n_groups, with_validity, with_filter, shape)


def test_bad_arguments_are_refused(ctx):
    pw = int(ctx.lib.cubit_padded_words(64))
    buf, ptrs = slices_on_device(ctx, 2, pw)
    buf.zero()
    grp = ctx.alloc(2 * pw * 8)
    grp.zero()
    gptrs = (C.c_void_p * 2)(grp.addr, grp.addr + pw * 8)
    out = ctx.alloc(2 * 48)
    lib, h = ctx.lib, ctx.handle
    R, T = L.SELECT_RANK, L.TYPE_INT64
    sel = lib.cubit_bitslice_select_grouped
    assert sel(h, ptrs, 65, None, None, gptrs, 2, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, None, gptrs, 2, 64, T, 0, 3, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, None, gptrs, 0, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, None, gptrs, 257, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, None, None, 2, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    odd = C.c_void_p(grp.addr + 8)  # not 16-byte aligned
    assert sel(h, ptrs, 2, odd, None, gptrs, 2, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, odd, gptrs, 2, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    bad = (C.c_void_p * 2)(grp.addr, grp.addr + 8)
    assert sel(h, ptrs, 2, None, None, bad, 2, 64, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    for q in (1.5, -0.1, float("nan")):
        assert sel(h, ptrs, 2, None, None, gptrs, 2, 64, T, 0, L.SELECT_QUANTILE, 0, q, out.ptr) == L.ERR_INVALID
    assert sel(h, ptrs, 2, None, None, gptrs, 2, 1 << 47, T, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    ctx.check()
    # no rows: six zeros per group, nothing launched; rows in no group: six zeros per group
    for n in (0, 64):
        L.check(lib.cubit_memset_d(h, out.ptr, 0xFF, 2 * 48))
        assert sel(h, ptrs, 2, None, None, gptrs, 2, n, T, 0, R, 0, 0.0, out.ptr) == L.OK
        ctx.check()
        assert not out.download(np.int64, 12).any()
    for b in (buf, grp, out):
        b.free()
