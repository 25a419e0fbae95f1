"""cubit_table_build_index_quantiles: a RANGE / BINS index whose edges are the column's equi-depth
quantiles, chosen on the GPU by a multi-target radix select (quantile_hist_kernel).

The expected keys come from numpy, never from the library: with k the comparison keys of the valid
rows in ascending order and m their number, q_j = k[(j * m) // n_bins]; RANGE keeps the distinct
q_j above k[0], BINS the distinct values of {k[0]} | {q_j} | {k[m-1] + 1}. Where k[m-1] + 1 is not
a key the column's type can hand back (past INT64_MAX; past a FLOAT / DOUBLE NaN) the edge is
k[m-1] itself, and one past +inf is the NaN key: the header states both. Per case: the returned
keys, every leaf against its predicate, the saved index byte for byte against build_index with the
returned keys on a twin table, and scans against the oracle. build_index has no form for an empty
explicit key list (n = 0 asks for every distinct value), so a RANGE result without keys is compared
with the twin only where the column has at most one distinct value, where the two agree."""
import math

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable, Dictionary
from oracle import oracle as O
from test_gpu_maintenance import check_index_bits

pytestmark = pytest.mark.gpu

N = 3 * 131_072 + 37  # several workgroups, a ragged last word
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def words(mask):
    return validity_from_mask(mask)


# ---------------------------------------------------------------- keys, as numpy sees them

def keys_of(v):
    """The comparison key (cubit_fp_key) of every value, as int64."""
    if v.dtype == np.uint64:
        return (v ^ np.uint64(2 ** 63)).view(np.int64)
    if v.dtype.kind == "f":
        wide = v.dtype == np.float64
        u = v.view(np.uint64 if wide else np.uint32).astype(np.uint64)
        sign = (u >> np.uint64(63 if wide else 31)).astype(bool)
        mag = (u & np.uint64(2 ** (63 if wide else 31) - 1)).astype(np.int64)
        inf, nan = (0x7FF0000000000000, 0x7FF8000000000000) if wide else (0x7F800000, 0x7FC00000)
        return np.where(mag > inf, nan, np.where(sign, -mag, mag)).astype(np.int64)
    return v.astype(np.int64)


def abi_value(key, dtype):
    """A key as the C call hands it back (cubit_fp_value), as a Python int of int64."""
    key = int(key)
    if dtype == np.uint64:  # the value's bits
        u = key + 2 ** 63
        return u if u <= I64_MAX else u - 2 ** 64
    if dtype == np.float64 and key < 0:
        return (-key | 2 ** 63) - 2 ** 64
    if dtype == np.float32 and key < 0:
        return -key | 2 ** 31
    return key


def top_edge(kmax, dtype):
    """The BINS edge above the maximum key."""
    if kmax == I64_MAX:
        return kmax
    if np.dtype(dtype).kind == "f":
        inf, nan = (0x7FF0000000000000, 0x7FF8000000000000) if dtype == np.float64 else (0x7F800000, 0x7FC00000)
        return nan if kmax + 1 > inf else kmax + 1
    return kmax + 1


def expected_keys(k, ok, n_bins, enc, dtype):
    ks = np.sort(k[ok])
    m = len(ks)
    q = [int(ks[(j * m) // n_bins]) for j in range(1, n_bins)]
    if enc == L.INDEX_RANGE:
        return sorted(set(q) - {int(ks[0])})
    return sorted({int(ks[0])} | set(q) | {top_edge(int(ks[-1]), dtype)})


def constant_of(key, dtype):
    """A key as the filter constant that has it."""
    if dtype == np.uint64:
        return int(key) + 2 ** 63
    if np.dtype(dtype).kind == "f":
        pat = abi_value(key, dtype)
        return np.array([pat], dtype=np.int64).astype(np.uint64 if dtype == np.float64 else np.uint32).view(dtype)[0]
    return int(key)


def scan_constants(keys, kmin, kmax, dtype):
    """Keys for constants on an index key, strictly inside a bin, below the minimum and above the maximum."""
    out = []
    inf = 0x7FF0000000000000 if dtype == np.float64 else 0x7F800000
    if keys:
        out.append(keys[len(keys) // 2])
    edges = [kmin] + list(keys) + [kmax]
    gaps = [(a, b) for a, b in zip(edges, edges[1:]) if b - a >= 2]
    for a, b in gaps[:1] + gaps[-1:]:
        mid = a + (b - a) // 2
        if np.dtype(dtype).kind != "f" or mid <= inf:  # between +inf and NaN no key is a value
            out.append(mid)
    if kmin > I64_MIN and (np.dtype(dtype).kind != "f" or kmin > -inf):
        out.append(kmin - 1)
    if kmax < I64_MAX and (np.dtype(dtype).kind != "f" or kmax < inf):
        out.append(kmax + 1)
    return out


def check_scans(t, ocols, consts, n):
    sets = [F.TableFilterSet({0: F.ConstantFilter(cmp, c)}) for c in consts for cmp in ("<", "=", ">=")]
    sets.append(F.TableFilterSet({0: F.IsNullFilter()}))
    if len(ocols) > 1 and consts:
        sets.append(F.TableFilterSet({0: F.ConstantFilter("<", consts[0]), 1: F.ConstantFilter(">=", 3)}))
    for fs in sets:
        ref = O.table_scan(ocols, F.serialize(fs), n, row_base=t.row_base)
        assert np.array_equal(t.scan(fs), ref), fs
        assert t.count(fs) == len(ref), fs


def same_file(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def run_case(ctx, tmp_path, v, ok, n_bins, encs=(L.INDEX_RANGE, L.INDEX_BINS)):
    """Build, and check everything a case checks, for each encoding on one table."""
    n, dtype = len(v), v.dtype.type
    valid = None if ok.all() else words(ok)
    side = (np.arange(n) % 7).astype(np.int32)
    t = CubitTable(ctx, n)
    t.add_column(0, v, valid)
    t.add_column(1, side)
    t.build_index(1, L.INDEX_RANGE)
    k = keys_of(v)
    kmin, kmax = int(k[ok].min()), int(k[ok].max())
    ocols = [O.Column(v, valid), O.Column(side)]
    for enc in encs:
        want = expected_keys(k, ok, n_bins, enc, dtype)
        got = t.build_index_quantiles(0, n_bins, enc)
        assert got.dtype == np.int64 and got.tolist() == [abi_value(x, dtype) for x in want], (enc, n_bins)
        ix = check_index_bits(t, 0, enc, k, ok, tmp_path)
        assert ix["keys"].tolist() == want and ix["bvs"].shape[0] == len(want) - (enc == L.INDEX_BINS)
        if want or kmin == kmax:  # (an empty list over several values: see the module's text)
            u = CubitTable(ctx, n)
            u.add_column(0, v, valid)
            u.build_index(0, enc, got.view(np.uint64) if dtype == np.uint64 else got)
            a, b = tmp_path / "quantile.bin", tmp_path / "explicit.bin"
            t.save_index(0, enc, a)
            u.save_index(0, enc, b)
            assert same_file(a, b), (enc, n_bins)
            u.close()
        else:
            assert not ix["exact"]
        consts = [constant_of(x, dtype) for x in scan_constants(want, kmin, kmax, dtype)]
        check_scans(t, ocols, consts, n)
    t.close()


def with_nulls(rng, v, frac, lo, hi):
    """`frac` of the rows NULL, their slots holding values outside the valid range."""
    ok = rng.random(len(v)) >= frac
    v = v.copy()
    outside = np.where(rng.random(len(v)) < 0.5, lo, hi).astype(v.dtype)
    v[~ok] = outside[~ok]
    return v, ok


# ---------------------------------------------------------------- spans

def test_span_12_bits_one_pass(ctx, tmp_path):
    rng = np.random.default_rng(1)
    v = rng.integers(8035, 8035 + 2526, N).astype(np.int32)
    run_case(ctx, tmp_path, v, np.ones(N, dtype=bool), 64)


def test_span_2_24_many_bins(ctx, tmp_path):
    rng = np.random.default_rng(2)
    v = rng.integers(-5, 2 ** 24 - 5, N).astype(np.int64)
    v[:2] = [-5, 2 ** 24 - 6]
    run_case(ctx, tmp_path, v, np.ones(N, dtype=bool), 1024, encs=(L.INDEX_RANGE,))
    run_case(ctx, tmp_path, v.astype(np.int32), np.ones(N, dtype=bool), 64)


def test_span_2_40_nulls_outside_the_range(ctx, tmp_path):
    """8 % NULL; the NULL slots hold values far outside the valid range and must not move an edge."""
    rng = np.random.default_rng(3)
    v = rng.integers(10 ** 6, 10 ** 6 + 2 ** 40, N).astype(np.int64)
    v, ok = with_nulls(rng, v, 0.08, I64_MIN + 3, I64_MAX - 3)
    run_case(ctx, tmp_path, v, ok, 64)
    run_case(ctx, tmp_path, v, ok, 3)


def test_span_of_all_int64(ctx, tmp_path):
    """INT64_MIN and INT64_MAX both present: vmax - vmin is 2^64 - 1, and no edge follows the maximum."""
    rng = np.random.default_rng(4)
    v = rng.integers(I64_MIN, I64_MAX, N, dtype=np.int64, endpoint=True)
    v[5], v[N - 5] = I64_MIN, I64_MAX
    run_case(ctx, tmp_path, v, np.ones(N, dtype=bool), 64)
    run_case(ctx, tmp_path, v, np.ones(N, dtype=bool), 2)


def test_negative_values_only(ctx, tmp_path):
    rng = np.random.default_rng(5)
    v = rng.integers(-900_000, -17, N).astype(np.int32)
    v, ok = with_nulls(rng, v, 0.08, 5, 2 ** 31 - 1)
    run_case(ctx, tmp_path, v, ok, 3)
    run_case(ctx, tmp_path, v, ok, 64)


# ---------------------------------------------------------------- skew

@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_every_row_equal(ctx, tmp_path, dt):
    """One LDS counter takes every row. RANGE: no bitvector, as the n = 0 form; BINS: [v, v + 1)."""
    v = np.full(N, 4242, dtype=dt)
    run_case(ctx, tmp_path, v, np.ones(N, dtype=bool), 64)
    t = CubitTable(ctx, N)
    t.add_column(0, v)
    assert t.build_index_quantiles(0, 64).tolist() == [] and t.index_info(0)[0] == 0
    assert t.build_index_quantiles(0, 2, L.INDEX_BINS).tolist() == [4242, 4243]
    t.close()


def test_two_values_99_to_1(ctx, tmp_path):
    rng = np.random.default_rng(6)
    v = np.where(rng.random(N) < 0.99, 7, 2 ** 33).astype(np.int64)
    ok = np.ones(N, dtype=bool)
    run_case(ctx, tmp_path, v, ok, 2)     # every quantile is the minimum: a RANGE index without keys
    run_case(ctx, tmp_path, v, ok, 1024)  # the last ranks reach the rare value


def test_zipf_like_heavy_value(ctx, tmp_path):
    """One value holds more than half the rows; the rest thin out over a span of more than 2^24."""
    rng = np.random.default_rng(7)
    v = np.minimum(rng.zipf(2.0, N), 2 ** 24).astype(np.int64) * 97
    assert (v == 97).mean() > 0.5 and v.max() > 2 ** 24
    v, ok = with_nulls(rng, v, 0.08, -50, 2 ** 40)
    run_case(ctx, tmp_path, v, ok, 64)
    run_case(ctx, tmp_path, v, ok, 3)


# ---------------------------------------------------------------- NULLs, small tables

def test_all_null(ctx):
    v = np.arange(N, dtype=np.int64)
    t = CubitTable(ctx, N)
    t.add_column(0, v, words(np.zeros(N, dtype=bool)))
    assert t.build_index_quantiles(0, 64).tolist() == []
    assert t.index_info(0)[0] == 0
    assert len(t.scan(F.TableFilterSet({0: F.ConstantFilter("<", 10)}))) == 0
    assert len(t.scan(F.TableFilterSet({0: F.IsNullFilter()}))) == N
    with pytest.raises(L.CubitError) as e:
        t.build_index_quantiles(0, 64, L.INDEX_BINS)
    assert e.value.code == L.ERR_INVALID
    t.close()


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("n_bins", [2, 3, 64, 1024])
def test_small_tables(ctx, tmp_path, n, n_bins):
    """Fewer rows than a vector load, than a word, one row more than a word; n_bins > m."""
    rng = np.random.default_rng(100 * n + n_bins)
    v = rng.integers(-2 ** 20, 2 ** 20, n).astype(np.int64)
    ok = np.ones(n, dtype=bool)
    if n > 1:
        ok[rng.integers(0, n)] = False
        v[~ok] = 2 ** 50
    run_case(ctx, tmp_path, v, ok, n_bins)
    run_case(ctx, tmp_path, v.astype(np.int32), np.ones(n, dtype=bool), n_bins)


def test_column_not_on_a_16_byte_boundary(ctx, tmp_path):
    """A caller-owned device column that starts 4 bytes into an allocation: no 16-byte loads."""
    rng = np.random.default_rng(8)
    v = rng.integers(0, 2 ** 20, N + 1).astype(np.int32)
    buf = ctx.upload(v)
    t = CubitTable(ctx, N)
    t.add_device_column(0, buf.addr + 4, L.TYPE_INT32)
    got = t.build_index_quantiles(0, 64)
    k, ok = v[1:].astype(np.int64), np.ones(N, dtype=bool)
    assert got.tolist() == expected_keys(k, ok, 64, L.INDEX_RANGE, np.int32)
    check_index_bits(t, 0, L.INDEX_RANGE, k, ok, tmp_path)
    t.close()
    buf.free()


# ---------------------------------------------------------------- types

def test_uint64_above_2_63(ctx, tmp_path):
    rng = np.random.default_rng(9)
    v = rng.integers(0, 2 ** 64, N, dtype=np.uint64)
    v[:3] = np.array([0, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    v, ok = with_nulls(rng, v, 0.08, 0, 0)
    ok[:3] = True
    v[:3] = np.array([0, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    run_case(ctx, tmp_path, v, ok, 64)
    w = (v >> np.uint64(30)) + np.uint64(2 ** 63 - 2 ** 20)  # straddles 2^63, the maximum below 2^64 - 1
    run_case(ctx, tmp_path, w, ok, 3)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_float_keys_come_back_as_patterns(ctx, tmp_path, dt):
    """Edges follow cubit_fp_key's order (negatives reversed, -0.0 = +0.0, NaN above +inf)."""
    rng = np.random.default_rng(10)
    v = (rng.standard_normal(N) * 1e3).astype(dt)
    special = np.array([math.nan, math.inf, -math.inf, 0.0, -0.0, 1e-30, -1e-30], dtype=dt)
    pick = rng.random(N) < 0.2
    v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    v, ok = with_nulls(rng, v, 0.08, 12345.0, -0.0)
    run_case(ctx, tmp_path, v, ok, 64)  # the maximum is NaN: the last bin ends at the NaN key
    finite = np.where(np.isnan(v) | np.isinf(v), dt(2.5), v)
    finite[0] = math.inf  # the maximum is +inf: the edge after it is the NaN key
    ok[0] = True
    run_case(ctx, tmp_path, finite, ok, 3)
    finite[0] = dt(1.0)
    run_case(ctx, tmp_path, finite, ok, 64, encs=(L.INDEX_BINS,))


def test_varchar_by_its_codes(ctx, tmp_path):
    rng = np.random.default_rng(11)
    pool = [b"w%05d" % i for i in range(3000)]
    n = 70_003
    vals = [pool[i] if rng.random() > 0.08 else None for i in np.minimum(rng.zipf(1.5, n), 3000) - 1]
    d = Dictionary(pool)
    t = CubitTable(ctx, n)
    t.add_string_column(0, vals, d)
    codes, ok = d.encode(vals)
    got = t.build_index_quantiles(0, 64)
    want = expected_keys(codes.astype(np.int64), ok, 64, L.INDEX_RANGE, np.int32)
    assert got.tolist() == want and len(want) > 3
    check_index_bits(t, 0, L.INDEX_RANGE, codes, ok, tmp_path)
    u = CubitTable(ctx, n)  # build_index takes the strings the codes stand for
    u.add_string_column(0, vals, d)
    u.build_index(0, L.INDEX_RANGE, [pool[c] for c in want])
    a, b = tmp_path / "quantile.bin", tmp_path / "explicit.bin"
    t.save_index(0, L.INDEX_RANGE, a)
    u.save_index(0, L.INDEX_RANGE, b)
    assert same_file(a, b)
    u.close()
    col = O.StringColumn(vals)
    for c in [pool[want[1]], pool[want[1]] + b"x", b"a", b"zzz"]:  # a key, inside a bin, below, above
        for cmp in ("<", "=", ">="):
            fs = F.TableFilterSet({0: F.ConstantFilter(cmp, c)})
            assert np.array_equal(t.scan(fs), O.table_scan([col], F.serialize(fs), n)), (cmp, c)
    assert np.array_equal(t.scan(F.TableFilterSet({0: F.IsNullFilter()})), np.flatnonzero(~ok))
    t.close()


# ---------------------------------------------------------------- maintenance

def test_append_merge_and_sync_keep_the_leaves_exact(ctx, tmp_path):
    rng = np.random.default_rng(12)
    v = rng.integers(0, 2 ** 24, N).astype(np.int64)
    v, ok = with_nulls(rng, v, 0.08, -9, 2 ** 30)
    side = (np.arange(N) % 7).astype(np.int32)
    t = CubitTable(ctx, N)
    t.add_column(0, v, words(ok))
    t.add_column(1, side)
    t.build_index(1, L.INDEX_RANGE)
    keys = {enc: t.build_index_quantiles(0, 64, enc).tolist() for enc in (L.INDEX_RANGE, L.INDEX_BINS)}

    def check(v, ok, side):
        for enc in keys:
            ix = check_index_bits(t, 0, enc, v, ok, tmp_path)
            assert ix["keys"].tolist() == keys[enc]  # explicit keys stay as chosen
        mid = keys[L.INDEX_RANGE][20] + 1
        check_scans(t, [O.Column(v, words(ok)), O.Column(side)], [keys[L.INDEX_RANGE][31], mid, -100, 2 ** 31],
                    len(v))

    nb = 70_001  # appended values reach outside the old range at both ends
    extra, extra_ok = rng.integers(-50, 2 ** 24 + 50, nb).astype(np.int64), rng.random(nb) > 0.05
    t.append({0: extra, 1: np.ones(nb, dtype=np.int32)}, validity={0: words(extra_ok)})
    v, ok, side = np.concatenate([v, extra]), np.concatenate([ok, extra_ok]), np.concatenate([side, np.ones(nb, np.int32)])
    check(v, ok, side)
    rows = np.sort(rng.choice(len(v), 4000, replace=False)).astype(np.int64)
    vals = rng.integers(-50, 2 ** 24 + 50, len(rows)).astype(np.int64)
    t.set_updates(0, rows, vals, np.full(len(rows), 2, dtype=np.uint64))
    assert t.merge_updates(0, 5) == len(rows)
    v[rows], ok[rows] = vals, True
    check(v, ok, side)
    new, nok = v.copy(), ok.copy()
    pick = rng.random(len(v)) < 0.02
    new[pick] = rng.integers(-50, 2 ** 24 + 50, int(pick.sum()))
    nok[rng.random(len(v)) < 0.01] = False
    changed = (ok != nok) | (ok & nok & (v != new))
    assert t.sync_column(0, new, words(nok)) == (int(changed.sum()), True)
    v = np.where(changed & nok, new, np.where(changed, 0, v))
    check(v, nok, side)
    t.close()


# ---------------------------------------------------------------- refusals, the plan

def test_refusals(ctx):
    v = np.arange(1000, dtype=np.int64)
    t = CubitTable(ctx, 1000)
    t.add_column(0, v)
    for args in [(0, 64, L.INDEX_EQUALITY), (0, 0), (0, 1), (0, 1025), (3, 64)]:
        with pytest.raises(L.CubitError) as e:
            t.build_index_quantiles(*args)
        assert e.value.code == L.ERR_INVALID, args
    assert t.index_info(0) == (0, 0)  # nothing was built
    # a cap below the key count: the count is still reported, `cap` keys are written
    import ctypes as C
    out = np.full(8, -1, dtype=np.int64)
    nk = C.c_uint32()
    lib = L.gpu_lib()
    assert lib.cubit_table_build_index_quantiles(t.handle, 0, L.INDEX_RANGE, 10, out.ctypes.data, 4, C.byref(nk)) == 0
    assert nk.value == 9 and out.tolist() == [100, 200, 300, 400, -1, -1, -1, -1]
    assert lib.cubit_table_build_index_quantiles(t.handle, 0, L.INDEX_RANGE, 10, None, 0, None) == 0  # all optional
    assert lib.cubit_table_build_index_quantiles(t.handle, 0, L.INDEX_RANGE, 10, None, 4, C.byref(nk)) == L.ERR_INVALID
    assert t.index_info(0)[0] == 9
    t.close()


def test_off_key_constant_is_answered_by_the_index(ctx):
    """With the quantile RANGE index a constant between two edges costs a candidate check of its
    bin; without it, a K0 pass over the column (last_k0_order lists the K0 comparisons built)."""
    rng = np.random.default_rng(13)
    v = rng.integers(0, 2 ** 24, N).astype(np.int64)
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 5_000_001)})
    ref = np.flatnonzero(v < 5_000_001)
    t = CubitTable(ctx, N)
    t.add_column(0, v)
    assert np.array_equal(t.scan(fs), ref) and t.last_k0_order() == [0]
    keys = t.build_index_quantiles(0, 64)
    assert 5_000_001 not in keys.tolist() and len(keys) == 63
    assert np.array_equal(t.scan(fs), ref) and t.last_k0_order() == []
    t.close()
