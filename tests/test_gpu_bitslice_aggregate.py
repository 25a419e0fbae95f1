"""The fused evaluate + aggregate kernel through its low-level entry point (cubit_bitslice_aggregate)
against Python integers: {sum_lo, sum_hi, min, max, count_valid, count_rows} over the filter's rows
from slices built by cubit_bitslice_build. Sizes: one row, around one 64-row word, around one
131,072-row tile and three tiles and a tail. Spans: 0 bits (no slice: sum = count * base), 1, 12,
around 32 and 63 / 64 bits (base INT64_MIN, top INT64_MAX). With and without a validity mask of
exactly ceil(n / 64) words; filters: none, all zero, one row (first, last), about 1 % and 50 % of the
rows at random (the padding past the rows set, which must be ignored), and one whose rows are all NULL;
every ops subset of {SUM, MIN, MAX, all}, d_out pre-filled with 0xFF."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd.table import Context

pytestmark = pytest.mark.gpu

N_ROWS = [1, 63, 64, 65, 131_071, 131_072, 131_073, 3 * 131_072 + 37]
BITS = [0, 1, 12, 31, 32, 33, 63, 64]
OPS = [L.AGG_SUM, L.AGG_MIN, L.AGG_MAX, L.AGG_ALL]
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def pack(mask, words, pad_ones=False):
    """A bool row mask as LSB-first 64-bit words, padded to `words` words with zeros (or ones)."""
    out = np.full(words, U64 if pad_ones else 0, dtype=np.uint64)
    n = len(mask)
    full = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    full[:n] = mask
    if pad_ones:
        full[n:] = True
    b = np.packbits(full, bitorder="little")
    out.view(np.uint8)[: len(b)] = b
    return out


def offsets(rng, n, bits):
    """n offsets below 2^bits, a fifth of them at the edges (0, 1, the middle, the top)."""
    top = (1 << bits) - 1
    u = rng.integers(0, top, n, dtype=np.uint64, endpoint=True) if bits else np.zeros(n, dtype=np.uint64)
    edges = np.array([0, min(1, top), top // 2, min(top // 2 + 1, top), max(top - 1, 0), top], dtype=np.uint64)
    pick = rng.random(n) < 0.2
    u[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return u


def exact_sum(a):
    """The sum of an int64 / uint64 array as a Python int (32-bit halves summed in 64 bits: exact
    below 2^31 elements)."""
    if len(a) == 0:
        return 0
    lo = int((a & a.dtype.type(0xFFFFFFFF)).astype(np.uint64).sum())
    hi = int((a >> a.dtype.type(32)).astype(np.int64 if a.dtype == np.int64 else np.uint64).sum())
    return (hi << 32) + lo


def slices_on_device(ctx, n_slices, pw):
    buf = ctx.alloc(max(n_slices, 1) * pw * 8)
    ptrs = (C.c_void_p * max(n_slices, 1))(*[buf.addr + s * pw * 8 for s in range(max(n_slices, 1))])
    return buf, ptrs


def filters_for(rng, n, valid, with_validity):
    """(name, bool mask or None) — None is the NULL filter (every row)."""
    one_first = np.zeros(n, dtype=bool)
    one_first[0] = True
    one_last = np.zeros(n, dtype=bool)
    one_last[n - 1] = True
    out = [("null", None), ("zero", np.zeros(n, dtype=bool)), ("first", one_first), ("last", one_last),
           ("1%", rng.random(n) < 0.01), ("50%", rng.random(n) < 0.5)]
    if with_validity:
        out.append(("all_null_rows", ~valid & (rng.random(n) < 0.7)))
    return out


def run(ctx, ptrs, bits, vp, fp, n, typ, base, ops, out):
    L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, 48))  # every slot must be written
    L.check(ctx.lib.cubit_bitslice_aggregate(ctx.handle, ptrs, bits, vp, fp, n, typ, base, ops, out.ptr))
    ctx.check()
    lo, hi, mn, mx, cv, cr = (int(x) for x in out.download(np.int64, 6))
    return (hi << 64) + (lo & U64), mn, mx, cv, cr


def check_span(ctx, rng, n, bits, with_validity, dtype):
    pw = int(ctx.lib.cubit_padded_words(n))
    nw = (n + 63) // 64
    base = -(1 << (bits - 1)) if bits else 7
    u = offsets(rng, n, bits)
    keys = (u + np.uint64(base & U64)).view(np.int64)  # wraps as the unsigned sum does
    if dtype == np.int32:
        assert keys.min() >= -(1 << 31) and keys.max() < (1 << 31)
    valid = rng.random(n) >= 0.1 if with_validity else np.ones(n, dtype=bool)
    d_col = ctx.upload(keys.astype(dtype))
    # the caller's mask holds ceil(n / 64) words only: the kernel must not read past them
    d_val = ctx.upload(pack(valid, nw)) if with_validity else None
    vp = d_val.ptr if d_val else None
    typ = L.TYPE_INT32 if dtype == np.int32 else L.TYPE_INT64
    buf, ptrs = slices_on_device(ctx, bits, pw)
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, typ, vp, n, base, bits, ptrs))
    out = ctx.alloc(48)
    for name, mask in filters_for(rng, n, valid, with_validity):
        d_f = None if mask is None else ctx.upload(pack(mask, pw, pad_ones=name == "50%"))
        rows = np.ones(n, dtype=bool) if mask is None else mask
        sel = keys[rows & valid]
        want_sum = exact_sum(sel)
        for ops in OPS:
            s, mn, mx, cv, cr = run(ctx, ptrs, bits, vp, d_f.ptr if d_f else None, n, typ, base, ops, out)
            where = (n, bits, dtype.__name__, with_validity, name, ops)
            assert (cv, cr) == (len(sel), int(rows.sum())), where
            assert s == (want_sum if ops & L.AGG_SUM else 0), where
            if len(sel):
                assert mn == (int(sel.min()) if ops & L.AGG_MIN else 0), where
                assert mx == (int(sel.max()) if ops & L.AGG_MAX else 0), where
            else:  # min / max are unspecified without a valid row; a slot not asked for is still 0
                assert ops & L.AGG_MIN or mn == 0, where
                assert ops & L.AGG_MAX or mx == 0, where
        if d_f:
            d_f.free()
    for b in (d_col, d_val, buf, out):
        if b:
            b.free()


@pytest.mark.parametrize("with_validity", [False, True], ids=["all_valid", "nulls"])
@pytest.mark.parametrize("n", N_ROWS)
def test_aggregates_match_python_integers(ctx, n, with_validity):
    rng = np.random.default_rng(2000 + n)
    for bits in BITS:
        check_span(ctx, rng, n, bits, with_validity, np.int64)
        if bits <= 32:
            check_span(ctx, rng, n, bits, with_validity, np.int32)


def test_ubigint_full_range_through_its_key(ctx):
    """A UINT64 column's slices are those of key - base with key = v ^ 2^63: the sum adds the values
    unsigned (past 2^64 here), min / max come back as the values' bits."""
    rng = np.random.default_rng(6)
    n = 131_073
    raw = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    raw[:4] = [0, 1, U64 - 1, U64]
    pw = int(ctx.lib.cubit_padded_words(n))
    d_col = ctx.upload(raw)
    buf, ptrs = slices_on_device(ctx, 64, pw)
    base_key = -(1 << 63)  # the key of value 0
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, L.TYPE_UINT64, None, n, base_key, 64, ptrs))
    out = ctx.alloc(48)
    for mask in (None, rng.random(n) < 0.3, np.arange(n) == 3):
        d_f = None if mask is None else ctx.upload(pack(mask, pw))
        sel = raw if mask is None else raw[mask]
        s, mn, mx, cv, cr = run(ctx, ptrs, 64, None, d_f.ptr if d_f else None, n, L.TYPE_UINT64, base_key, L.AGG_ALL, out)
        assert exact_sum(sel[:1000]) == sum(int(x) for x in sel[:1000])
        assert s & ((1 << 128) - 1) == exact_sum(sel)
        assert (mn & U64, mx & U64, cv, cr) == (int(sel.min()), int(sel.max()), len(sel), len(sel))
    # every value 2^64 - 1: one distinct value, no slice at all
    s, mn, mx, cv, cr = run(ctx, ptrs, 0, None, None, n, L.TYPE_UINT64, (1 << 63) - 1, L.AGG_ALL, out)
    assert (s & ((1 << 128) - 1), mn & U64, mx & U64, cv, cr) == (n * U64, U64, U64, n, n)


def test_bad_arguments_are_refused(ctx):
    pw = int(ctx.lib.cubit_padded_words(64))
    buf, ptrs = slices_on_device(ctx, 2, pw)
    out = ctx.alloc(64)
    lib, h = ctx.lib, ctx.handle
    assert lib.cubit_bitslice_aggregate(h, ptrs, 65, None, None, 64, L.TYPE_INT64, 0, L.AGG_SUM, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_aggregate(h, ptrs, 2, None, None, 64, L.TYPE_INT64, 0, 8, out.ptr) == L.ERR_INVALID
    odd = C.c_void_p(buf.addr + 8)  # not 16-byte aligned
    assert lib.cubit_bitslice_aggregate(h, ptrs, 2, odd, None, 64, L.TYPE_INT64, 0, L.AGG_SUM, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_aggregate(h, ptrs, 2, None, odd, 64, L.TYPE_INT64, 0, L.AGG_SUM, out.ptr) == L.ERR_INVALID
    # SUM of keys that are not linear in the value; MIN / MAX of them work
    for typ in (L.TYPE_FLOAT, L.TYPE_DOUBLE, L.TYPE_VARCHAR):
        assert lib.cubit_bitslice_aggregate(h, ptrs, 0, None, None, 64, typ, 0, L.AGG_SUM, out.ptr) == L.ERR_UNSUPPORTED
        assert lib.cubit_bitslice_aggregate(h, ptrs, 0, None, None, 64, typ, 5, L.AGG_MIN | L.AGG_MAX, out.ptr) == L.OK
    ctx.check()
    # no rows: zero counts, nothing launched
    L.check(lib.cubit_memset_d(h, out.ptr, 0xFF, 48))
    assert lib.cubit_bitslice_aggregate(h, ptrs, 2, None, None, 0, L.TYPE_INT64, 0, L.AGG_ALL, out.ptr) == L.OK
    ctx.check()
    assert not out.download(np.int64, 6).any()
