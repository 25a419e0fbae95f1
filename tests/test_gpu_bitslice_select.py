"""The slice select's kernels through their low-level entry point (cubit_bitslice_select) against
np.sort: {value, found, count_below, count_equal, count_valid, count_rows} over the filter's rows from
slices built by cubit_bitslice_build. Sizes: one row, around one 64-row word, around one 131,072-row
tile and three tiles and a tail. Slice counts: 0, 1, one below / at / above the chunk width 4, 2 * 4 + 1,
12, around 32 and 63 / 64 (base INT64_MIN, top INT64_MAX). With and without a validity mask of exactly
ceil(n / 64) words; filters: none, all zero, one row (first, last), about 1 % and 50 % of the rows (the
padding past the rows set, which must be ignored) and one whose rows are all NULL; random values with
a fifth at the edges, all equal, two values only; ranks 0, 1, the middle, m - 2, m - 1 and m (not
found) in both directions and quantiles 0, 0.1, 0.25, 0.5 and 1; d_out pre-filled with 0xFF."""
import ctypes as C
import math

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd.table import Context

pytestmark = pytest.mark.gpu

N_ROWS = [1, 63, 64, 65, 131_071, 131_072, 131_073, 3 * 131_072 + 37]
CHUNK = 4
BITS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 12, 31, 32, 33, 63, 64]
QUANTILES = [0.0, 0.1, 0.25, 0.5, 1.0]
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


def offsets(rng, n, bits, dist):
    """n offsets below 2^bits: random with a fifth at the edges (0, 1, the middle, the top), all
    equal, or two values only."""
    top = (1 << bits) - 1
    if dist == "equal":
        return np.full(n, top // 3, dtype=np.uint64)
    if dist == "two":
        return np.where(rng.random(n) < 0.5, np.uint64(top // 2), np.uint64(top)).astype(np.uint64)
    u = rng.integers(0, top, n, dtype=np.uint64, endpoint=True) if bits else np.zeros(n, dtype=np.uint64)
    edges = np.array([0, min(1, top), top // 2, min(top // 2 + 1, top), max(top - 1, 0), top], dtype=np.uint64)
    pick = rng.random(n) < 0.2
    u[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return u


def quantile_rank(n, q):
    """quantile_disc's 0-based rank among n values, restated: max(1, n - floor(n - n * q)) - 1."""
    floored = int(math.floor(n - float(n * q)))
    return max(1, n - floored) - 1


def slices_on_device(ctx, n_slices, pw):
    buf = ctx.alloc(max(n_slices, 1) * pw * 8)
    ptrs = (C.c_void_p * max(n_slices, 1))(*[buf.addr + s * pw * 8 for s in range(max(n_slices, 1))])
    return buf, ptrs


def filters_for(rng, n, valid, with_validity, every):
    """(name, bool mask or None) — None is the NULL filter (every row)."""
    out = [("null", None), ("50%", rng.random(n) < 0.5)]
    if not every:
        return out
    one_first = np.zeros(n, dtype=bool)
    one_first[0] = True
    one_last = np.zeros(n, dtype=bool)
    one_last[n - 1] = True
    out += [("zero", np.zeros(n, dtype=bool)), ("first", one_first), ("last", one_last), ("1%", rng.random(n) < 0.01)]
    if with_validity:
        out.append(("all_null_rows", ~valid & (rng.random(n) < 0.7)))
    return out


def run(ctx, ptrs, bits, vp, fp, n, typ, base, mode, k, q, out):
    L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, 48))  # every slot must be written
    L.check(ctx.lib.cubit_bitslice_select(ctx.handle, ptrs, bits, vp, fp, n, typ, base, mode, k, q, out.ptr))
    ctx.check()
    return tuple(int(x) for x in out.download(np.int64, 6))


def expected(s, to_value, count_rows, desc, rank):
    """The six slots from the ascending array s of the qualifying non-NULL rows' sort keys; to_value
    maps a key to the value's reported form."""
    m = len(s)
    if rank >= m:
        return (0, 0, 0, 0, m, count_rows)
    v = s[m - 1 - rank] if desc else s[rank]
    lo, hi = int(np.searchsorted(s, v, "left")), int(np.searchsorted(s, v, "right"))
    return (to_value(v), 1, m - hi if desc else lo, hi - lo, m, count_rows)


def check_all_modes(ctx, ptrs, bits, vp, fp, n, typ, base, out, s, to_value, count_rows, where):
    m = len(s)
    for rank in sorted({0, 1, m // 2, max(m - 2, 0), max(m - 1, 0), m}):
        for desc in (False, True):
            got = run(ctx, ptrs, bits, vp, fp, n, typ, base, L.SELECT_RANK_DESC if desc else L.SELECT_RANK, rank, 0.0, out)
            assert got == expected(s, to_value, count_rows, desc, rank), (where, "rank", rank, desc)
    for q in QUANTILES:
        got = run(ctx, ptrs, bits, vp, fp, n, typ, base, L.SELECT_QUANTILE, 12345, q, out)
        assert got == expected(s, to_value, count_rows, False, quantile_rank(m, q) if m else 0), (where, "q", q)


def check_span(ctx, rng, n, bits, with_validity, dtype, dist):
    pw = int(ctx.lib.cubit_padded_words(n))
    nw = (n + 63) // 64
    base = -(1 << (bits - 1)) if bits else 7
    u = offsets(rng, n, bits, dist)
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
    order = np.argsort(keys, kind="stable")  # sorted once; a filter keeps a subsequence
    keys_sorted = keys[order]
    for name, mask in filters_for(rng, n, valid, with_validity, every=dist == "random"):
        d_f = None if mask is None else ctx.upload(pack(mask, pw, pad_ones=name == "50%"))
        rows = np.ones(n, dtype=bool) if mask is None else mask
        s = keys_sorted[(rows & valid)[order]]
        check_all_modes(ctx, ptrs, bits, vp, d_f.ptr if d_f else None, n, typ, base, out, s, int, int(rows.sum()),
                        (n, bits, dtype.__name__, with_validity, dist, name))
        if d_f:
            d_f.free()
    for b in (d_col, d_val, buf, out):
        if b:
            b.free()


@pytest.mark.parametrize("with_validity", [False, True], ids=["all_valid", "nulls"])
@pytest.mark.parametrize("n", N_ROWS)
def test_select_matches_sorted_keys(ctx, n, with_validity):
    rng = np.random.default_rng(4000 + n)
    for i, bits in enumerate(BITS):
        for dist in ("random", "equal", "two"):
            dtype = np.int32 if bits <= 32 and i % 2 else np.int64
            check_span(ctx, rng, n, bits, with_validity, dtype, dist)


def typed_case(ctx, rng, typ, raw, keys, to_value, with_validity=True):
    """Slices of keys - min(key) built from the raw column by cubit_bitslice_build; every mode under no
    filter and a 30 % filter."""
    n = len(raw)
    pw, nw = int(ctx.lib.cubit_padded_words(n)), (n + 63) // 64
    valid = rng.random(n) >= 0.1 if with_validity else np.ones(n, dtype=bool)
    base = int(keys[valid].min())
    span = int(keys[valid].max()) - base
    bits = span.bit_length()
    d_col = ctx.upload(raw)
    d_val = ctx.upload(pack(valid, nw))
    buf, ptrs = slices_on_device(ctx, bits, pw)
    # (a dictionary column's codes are sliced as the INT32 values they are)
    build_typ = L.TYPE_INT32 if typ == L.TYPE_VARCHAR else typ
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, build_typ, d_val.ptr, n, base, bits, ptrs))
    out = ctx.alloc(48)
    for mask in (None, rng.random(n) < 0.3):
        d_f = None if mask is None else ctx.upload(pack(mask, pw))
        rows = np.ones(n, dtype=bool) if mask is None else mask
        s = np.sort(keys[rows & valid])
        check_all_modes(ctx, ptrs, bits, d_val.ptr, d_f.ptr if d_f else None, n, typ, base, out, s, to_value,
                        int(rows.sum()), (typ, bits, mask is None))
    return bits


def test_ubigint_orders_unsigned_across_2_63(ctx):
    rng = np.random.default_rng(7)
    n = 131_073
    raw = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    raw[:6] = [0, 1, (1 << 63) - 1, 1 << 63, U64 - 1, U64]
    keys = (raw ^ np.uint64(1 << 63)).view(np.int64)

    def to_value(key):  # the value's bits as int64
        return int(np.int64(key) ^ np.int64(-(1 << 63)))

    assert typed_case(ctx, rng, L.TYPE_UINT64, raw, keys, to_value, with_validity=False) == 64


def test_double_keys_nan_greatest_and_zeros_equal(ctx):
    rng = np.random.default_rng(8)
    n = 70_001
    f = rng.normal(0, 1e3, n)
    special = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5])
    pick = rng.random(n) < 0.3
    f[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    raw = f.view(np.int64).copy()
    mag = raw & np.int64(0x7FFFFFFFFFFFFFFF)
    keys = np.where(mag > 0x7FF0000000000000, np.int64(0x7FF8000000000000), np.where(raw < 0, -mag, mag))

    def to_value(key):  # the key's bit pattern: -x as sign | magnitude, -0.0 as +0.0, one NaN
        key = int(key)
        return key if key >= 0 else ((1 << 63) | -key) - (1 << 64)

    typed_case(ctx, rng, L.TYPE_DOUBLE, raw, keys, to_value)


def test_dictionary_codes(ctx):
    rng = np.random.default_rng(9)
    n = 65_537
    codes = rng.integers(0, 11, n, dtype=np.int32)
    assert typed_case(ctx, rng, L.TYPE_VARCHAR, codes, codes.astype(np.int64), int) == 4


def test_bad_arguments_are_refused(ctx):
    pw = int(ctx.lib.cubit_padded_words(64))
    buf, ptrs = slices_on_device(ctx, 2, pw)
    buf.zero()
    out = ctx.alloc(64)
    lib, h = ctx.lib, ctx.handle
    R = L.SELECT_RANK
    assert lib.cubit_bitslice_select(h, ptrs, 65, None, None, 64, L.TYPE_INT64, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_select(h, ptrs, 2, None, None, 64, L.TYPE_INT64, 0, 3, 0, 0.0, out.ptr) == L.ERR_INVALID
    odd = C.c_void_p(buf.addr + 8)  # not 16-byte aligned
    assert lib.cubit_bitslice_select(h, ptrs, 2, odd, None, 64, L.TYPE_INT64, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_select(h, ptrs, 2, None, odd, 64, L.TYPE_INT64, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    for q in (1.5, -0.1, float("nan")):
        assert lib.cubit_bitslice_select(h, ptrs, 2, None, None, 64, L.TYPE_INT64, 0, L.SELECT_QUANTILE, 0, q,
                                         out.ptr) == L.ERR_INVALID
    assert lib.cubit_bitslice_select(h, ptrs, 2, None, None, 1 << 47, L.TYPE_INT64, 0, R, 0, 0.0, out.ptr) == L.ERR_INVALID
    ctx.check()
    # no rows: six zeros, nothing launched
    L.check(lib.cubit_memset_d(h, out.ptr, 0xFF, 48))
    assert lib.cubit_bitslice_select(h, ptrs, 2, None, None, 0, L.TYPE_INT64, 0, R, 0, 0.0, out.ptr) == L.OK
    ctx.check()
    assert not out.download(np.int64, 6).any()
    # a rank past 2^32 is not found, not truncated
    assert lib.cubit_bitslice_select(h, ptrs, 2, None, None, 64, L.TYPE_INT64, 5, R, 1 << 32, 0.0, out.ptr) == L.OK
    ctx.check()
    assert list(out.download(np.int64, 6)) == [0, 0, 0, 0, 64, 64]
