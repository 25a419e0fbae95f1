"""The bit-sliced index's two kernels through their low-level entry points (cubit_bitslice_build,
cubit_bitslice_compare) against numpy on the keys: the slices word for word, padding included, and
out = valid AND (lo <= key - base <= hi) for bounds at every edge, both `negate` values, with and
without a validity mask. Sizes: one row, around one 64-row word, around one 131,072-row zone (a
wave of the build kernel takes 64 words, a thread of the compare two) and three zones and a tail.
Spans: 0 bits (no slice at all), 1, 12, around 32 and 63 / 64 bits (base INT64_MIN, top INT64_MAX)."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd.table import Context

pytestmark = pytest.mark.gpu

N_ROWS = [1, 63, 64, 65, 131_071, 131_072, 131_073, 3 * 131_072 + 37]
BITS = [0, 1, 12, 31, 32, 33, 63, 64]
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def pack(mask, words):
    """A bool row mask as LSB-first 64-bit words, zero-padded to `words` words."""
    out = np.zeros(words, dtype=np.uint64)
    b = np.packbits(mask, bitorder="little")
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


def bounds(bits):
    top = (1 << bits) - 1
    mid = top // 2
    b = {(0, top), (0, 0), (min(1, top), top), (0, mid), (mid, top), (mid, mid), (top, top),
         (min(1, top), max(top - 1, 0)), (mid + 1, mid), (3, 1), (0, U64)}
    if bits < 64:
        b |= {(top + 1, min(top + 5, U64)), (mid, U64)}
    return sorted(b)


def slices_on_device(ctx, n_slices, pw):
    buf = ctx.alloc(max(n_slices, 1) * pw * 8)
    ptrs = (C.c_void_p * max(n_slices, 1))(*[buf.addr + s * pw * 8 for s in range(max(n_slices, 1))])
    return buf, ptrs


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
    # the caller's mask holds ceil(n / 64) words only: the kernels must not read past them
    d_val = ctx.upload(pack(valid, nw)) if with_validity else None
    vp = d_val.ptr if d_val else None
    typ = L.TYPE_INT32 if dtype == np.int32 else L.TYPE_INT64
    buf, ptrs = slices_on_device(ctx, bits, pw)
    L.check(ctx.lib.cubit_memset_d(ctx.handle, buf.ptr, 0xFF, buf.nbytes))  # every word must be written
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, typ, vp, n, base, bits, ptrs))
    ctx.check()
    got = buf.download(np.uint64, max(bits, 1) * pw).reshape(-1, pw)
    for s in range(bits):
        want = pack(((u >> np.uint64(s)) & np.uint64(1)).astype(bool) & valid, pw)
        assert np.array_equal(got[s], want), (n, bits, s, dtype)
    out = ctx.alloc(pw * 8)
    for lo, hi in bounds(bits):
        inside = (u >= np.uint64(lo)) & (u <= np.uint64(hi))
        for negate in (0, 1):
            L.check(ctx.lib.cubit_memset_d(ctx.handle, out.ptr, 0xFF, pw * 8))
            L.check(ctx.lib.cubit_bitslice_compare(ctx.handle, ptrs, bits, vp, n, lo, hi, negate, out.ptr))
            ctx.check()
            want = pack(valid & (~inside if negate else inside), pw)
            assert np.array_equal(out.download(np.uint64, pw), want), (n, bits, lo, hi, negate, dtype)
    for b in (d_col, d_val, buf, out):
        if b:
            b.free()


@pytest.mark.parametrize("with_validity", [False, True], ids=["all_valid", "nulls"])
@pytest.mark.parametrize("n", N_ROWS)
def test_build_and_compare_match_numpy(ctx, n, with_validity):
    rng = np.random.default_rng(1000 + n)
    for bits in BITS:
        check_span(ctx, rng, n, bits, with_validity, np.int64)
        if bits <= 32:
            check_span(ctx, rng, n, bits, with_validity, np.int32)


def test_ubigint_column_is_sliced_through_its_key(ctx):
    """A UINT64 column holds the values' bits and is compared through the key v ^ 2^63: the base is
    given as a key, the slices are those of the unsigned difference."""
    rng = np.random.default_rng(5)
    n = 131_073
    raw = rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)
    raw[:4] = [0, 1, U64 - 1, U64]
    pw = int(ctx.lib.cubit_padded_words(n))
    d_col = ctx.upload(raw)
    buf, ptrs = slices_on_device(ctx, 64, pw)
    base_key = -(1 << 63)  # the key of value 0
    L.check(ctx.lib.cubit_bitslice_build(ctx.handle, d_col.ptr, L.TYPE_UINT64, None, n, base_key, 64, ptrs))
    ctx.check()
    got = buf.download(np.uint64, 64 * pw).reshape(64, pw)
    for s in range(64):
        assert np.array_equal(got[s], pack(((raw >> np.uint64(s)) & np.uint64(1)).astype(bool), pw)), s
    out = ctx.alloc(pw * 8)
    lo, hi = 1 << 62, (1 << 63) + 12345
    L.check(ctx.lib.cubit_bitslice_compare(ctx.handle, ptrs, 64, None, n, lo, hi, 0, out.ptr))
    ctx.check()
    assert np.array_equal(out.download(np.uint64, pw), pack((raw >= np.uint64(lo)) & (raw <= np.uint64(hi)), pw))


def test_bad_arguments_are_refused(ctx):
    pw = int(ctx.lib.cubit_padded_words(64))
    buf, ptrs = slices_on_device(ctx, 2, pw)
    out = ctx.alloc(pw * 8)
    assert ctx.lib.cubit_bitslice_build(ctx.handle, buf.ptr, L.TYPE_INT64, None, 64, 0, 65, ptrs) == L.ERR_INVALID
    assert ctx.lib.cubit_bitslice_compare(ctx.handle, ptrs, 65, None, 64, 0, 1, 0, out.ptr) == L.ERR_INVALID
    odd = C.c_void_p(out.addr + 8)  # not 16-byte aligned
    assert ctx.lib.cubit_bitslice_compare(ctx.handle, ptrs, 2, None, 64, 0, 1, 0, odd) == L.ERR_INVALID
