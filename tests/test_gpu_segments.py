"""Columns whose DuckDB segments mix codecs (cubit_table_add_segment_column): DuckDB's checkpoint
picks a codec per row group (ColumnDataCheckpointer), so one column may hold UNCOMPRESSED,
CONSTANT, RLE and BITPACKING segments side by side. Each row group here is written by the
oracle's restatement of its codec (bp_compress, rle_compress; a CONSTANT group as its value;
UNCOMPRESSED as the values' bytes); the GPU column equals the values at every valid row for every
integer T, and scans over it (unindexed, range, equality) equal the oracle's."""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RG = 122_880
DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def mixed_column(rng, dt, n_groups, tail):
    """Values, validity and segments: row group g written with codec g mod 4 (shuffled)."""
    dt = np.dtype(dt)
    info = np.iinfo(dt)
    n = n_groups * RG + tail
    vals = np.empty(n, dtype=dt)
    ok = rng.random(n) > 0.05
    segs = []
    codecs = rng.permutation(np.resize([L.CODEC_UNCOMPRESSED, L.CODEC_CONSTANT, L.CODEC_RLE, L.CODEC_BITPACKING],
                                       n_groups + (1 if tail else 0)))
    for g, codec in enumerate(codecs.tolist()):
        lo, hi = g * RG, min(n, (g + 1) * RG)
        m = hi - lo
        if codec == L.CODEC_CONSTANT:
            c = dt.type([info.min, info.max, 0, 7][int(rng.integers(0, 4))])
            vals[lo:hi] = c
            ok[lo:hi] = True  # a CONSTANT segment's rows are all valid and equal
            segs.append((codec, int(c), m))
        elif codec == L.CODEC_RLE:
            v = np.repeat(rng.integers(0, 50, m).astype(dt), rng.integers(1, 200, m))[:m]
            vals[lo:hi] = v
            data, offs, rows = O.rle_compress(v, ok[lo:hi], row_group=RG)
            for o, r, nxt in zip(offs.tolist(), rows.tolist(), offs.tolist()[1:] + [len(data)]):
                segs.append((codec, data[o:nxt].tobytes(), r))
        elif codec == L.CODEC_BITPACKING:
            span = min(1000, int(info.max) // 4)  # max - min must fit T (bp_compress refuses otherwise)
            v = (rng.integers(0, span, m) + (int(info.max) // 4 if info.max > 4000 else 0)).astype(dt)
            vals[lo:hi] = v
            bp = O.bp_compress(v, ok[lo:hi].astype(np.uint8), "auto")
            for o, size, r in zip(bp.seg_off.tolist(), bp.seg_size.tolist(), bp.seg_count.tolist()):
                segs.append((codec, bp.data[o:o + size].tobytes(), r))
        else:
            v = rng.integers(0, min(3000, int(info.max)), m).astype(dt)  # few distinct: the equality index takes them
            v[:2] = [info.min, info.max]
            vals[lo:hi] = v
            segs.append((codec, v.tobytes(), m))
    return vals, ok, segs


@pytest.mark.parametrize("dt", DTYPES)
def test_mixed_codecs_every_type(ctx, dt):
    rng = np.random.default_rng(np.dtype(dt).itemsize * 13 + "iu".index(np.dtype(dt).kind))
    vals, ok, segs = mixed_column(rng, dt, 6, 5_001)
    vw = validity_from_mask(ok)
    t = CubitTable(ctx, len(vals))
    t.add_segment_column(0, segs, dt, vw)
    got = t.download_column(0)
    want = vals.astype(np.uint64) if np.dtype(dt) == np.uint64 else vals.astype(np.int64)
    held = got.view(np.uint64) if np.dtype(dt) == np.uint64 else got.astype(np.int64)
    assert np.array_equal(held[ok], want[ok])
    ocol = O.Column(want.astype(np.uint64) if np.dtype(dt) == np.uint64 else
                    want.astype(np.int32 if t.types[0] == L.TYPE_INT32 else np.int64), vw)
    consts = [0, 7, 49, int(np.iinfo(dt).max), int(np.iinfo(dt).min)]
    for enc in (None, L.INDEX_RANGE, L.INDEX_EQUALITY):
        if enc is not None:
            t.build_index(0, enc)
        for c in consts:
            for op in ("=", "<", ">=", "!="):
                fs = F.TableFilterSet({0: F.ConstantFilter(op, c)})
                assert np.array_equal(t.scan(fs), O.table_scan([ocol], F.serialize(fs), len(vals))), (dt, enc, op, c)
    t.close()


def test_single_codec_columns_match_their_own_entry_points(ctx):
    """All-RLE and all-BITPACKING columns through the mixed entry point equal
    cubit_table_add_rle_column's and cubit_table_add_bitpacked_column's; a bad codec is refused."""
    rng = np.random.default_rng(5)
    v = np.repeat(rng.integers(0, 9, 50_000).astype(np.int32), rng.integers(1, 30, 50_000))[:700_000]
    data, offs, rows = O.rle_compress(v)
    a, b = CubitTable(ctx, len(v)), CubitTable(ctx, len(v))
    a.add_rle_column(0, data, offs, rows, np.int32)
    segs = [(L.CODEC_RLE, data[o:nx].tobytes(), r)
            for o, r, nx in zip(offs.tolist(), rows.tolist(), offs.tolist()[1:] + [len(data)])]
    b.add_segment_column(0, segs, np.int32)
    assert np.array_equal(a.download_column(0), b.download_column(0))
    bp = O.bp_compress(v.astype(np.int64), None, "auto")
    a.add_bitpacked_column(1, bp.data, bp.seg_off, bp.seg_count, np.int64)
    b.add_segment_column(1, [(L.CODEC_BITPACKING, bp.data[o:o + s].tobytes(), r)
                             for o, s, r in zip(bp.seg_off.tolist(), bp.seg_size.tolist(), bp.seg_count.tolist())],
                         np.int64)
    assert np.array_equal(a.download_column(1), b.download_column(1))
    with pytest.raises(L.CubitError):
        b.add_segment_column(2, [(9, b"\0" * 8, len(v))], np.int32)
    a.close()
    b.close()


# ------------------------------------------------------------------ the three entry points' shared path
# 4,101 rows: two full 2,048-value groups and a 5-row tail, the smallest column with more than one
# group and a partial one.
N_SMALL = 4_101


def bp_segments(bp):
    return [(L.CODEC_BITPACKING, bp.data[o:o + s].tobytes(), r)
            for o, s, r in zip(bp.seg_off.tolist(), bp.seg_size.tolist(), bp.seg_count.tolist())]


def small_packed(dt, seed):
    """Values, validity (about 5 % NULL) and their BITPACKING segments as the oracle's compressor
    writes them: FOR groups, or for a 2-byte T ascending values in DELTA_FOR groups, whose three
    header fields leave the packed words off the 4-byte alignment."""
    rng = np.random.default_rng(seed)
    v = (np.cumsum(rng.integers(0, 5, N_SMALL)) if np.dtype(dt).itemsize == 2 else rng.integers(0, 100, N_SMALL)).astype(dt)
    ok = rng.random(N_SMALL) > 0.05
    return v, ok, O.bp_compress(v, ok.astype(np.uint8), "auto")


@pytest.mark.parametrize("dt", [np.int8, np.uint16], ids=lambda d: np.dtype(d).name)
def test_moved_runs_through_both_doors(ctx, dt):
    """A 1- or 2-byte T: the packed runs sit off the 4-byte alignment and are moved behind the padded
    bytes. The same segments through cubit_table_add_bitpacked_column and through
    cubit_table_add_segment_column give the values at every valid row and the same column; only the
    first keeps the packed form, so only there a `<` scan reads the segments, with equal results."""
    v, ok, bp = small_packed(dt, 21)
    assert ("delta_for" if np.dtype(dt).itemsize == 2 else "for") in O.bp_group_modes(bp)  # words to move
    vw = validity_from_mask(ok)
    a, b = CubitTable(ctx, N_SMALL), CubitTable(ctx, N_SMALL)
    a.add_bitpacked_column(0, bp.data, bp.seg_off, bp.seg_count, dt, vw)
    b.add_segment_column(0, bp_segments(bp), dt, vw)
    ga, gb = a.download_column(0), b.download_column(0)
    assert ga.dtype == np.int32 and np.array_equal(ga[ok], v[ok].astype(np.int32))
    assert np.array_equal(ga, gb)
    fs = F.TableFilterSet({0: F.ConstantFilter("<", int(np.median(v)))})
    ref = O.table_scan([O.Column(v.astype(np.int32), vw)], F.serialize(fs), N_SMALL)
    assert 0 < len(ref) < N_SMALL
    for t in (a, b):
        t.use_packed_filter(True)
    ra, rb = a.scan(fs), b.scan(fs)
    assert a.last_packed() >= 1 and b.last_packed() == 0
    assert np.array_equal(ra, ref) and np.array_equal(rb, ref)
    a.close()
    b.close()


def test_packed_sum_kept_by_one_door(ctx):
    """An INT64 column as col_a of sum_product: read from its segments after
    cubit_table_add_bitpacked_column, from the plain column after cubit_table_add_segment_column;
    the sums are equal."""
    v, ok, bp = small_packed(np.int64, 22)
    vw = validity_from_mask(ok)
    a, b = CubitTable(ctx, N_SMALL), CubitTable(ctx, N_SMALL)
    a.add_bitpacked_column(0, bp.data, bp.seg_off, bp.seg_count, np.int64, vw)
    b.add_segment_column(0, bp_segments(bp), np.int64, vw)
    w = np.arange(N_SMALL, dtype=np.int64) % 7 + 1
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 50)})
    keep = ok & (v < 50)
    want = (int((v[keep] * w[keep]).sum()), int(keep.sum()))
    for t in (a, b):
        t.add_column(1, w)
    sa = a.sum_product(0, 1, fs, gather_b=True)
    sb = b.sum_product(0, 1, fs, gather_b=True)
    assert a.last_sum_packed() and not b.last_sum_packed()
    assert sa == sb == want
    a.close()
    b.close()


def test_refused_call_changes_nothing(ctx):
    """Segments one row short of the partition through each entry point, and codec 9 through the
    mixed one: each is refused, and the column, its RANGE index and scans are as before."""
    v, ok, _ = small_packed(np.int64, 23)
    t = CubitTable(ctx, N_SMALL)
    t.add_column(0, v)
    t.build_index(0, L.INDEX_RANGE)
    info = t.index_info(0)
    assert info[0] > 0
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 50)})
    before = t.scan(fs)
    assert np.array_equal(before, O.table_scan([O.Column(v)], F.serialize(fs), N_SMALL))
    short = v[:-1] + 1000  # were it installed, the scan would be empty
    bp = O.bp_compress(short, None, "auto")
    data, offs, rows = O.rle_compress(short)
    rle_segs = [(L.CODEC_RLE, data[o:nx].tobytes(), r)
                for o, r, nx in zip(offs.tolist(), rows.tolist(), offs.tolist()[1:] + [len(data)])]
    calls = [lambda: t.add_bitpacked_column(0, bp.data, bp.seg_off, bp.seg_count, np.int64),
             lambda: t.add_rle_column(0, data, offs, rows, np.int64),
             lambda: t.add_segment_column(0, bp_segments(bp), np.int64),
             lambda: t.add_segment_column(0, rle_segs, np.int64),
             lambda: t.add_segment_column(0, [(L.CODEC_UNCOMPRESSED, short.tobytes(), N_SMALL - 1)], np.int64),
             lambda: t.add_segment_column(0, [(9, b"\0" * 8, N_SMALL)], np.int64)]
    for call in calls:
        with pytest.raises(L.CubitError):
            call()
        assert t.index_info(0) == info
        assert np.array_equal(t.scan(fs), before)
        assert np.array_equal(t.download_column(0), v)
    t.close()


def test_timing_covers_every_tail(ctx):
    """With timing on, each entry point leaves one timed span, whichever stage comes last: the run
    expansion, the unpack, or the copy of an UNCOMPRESSED span. One 2,048-row group per segment."""
    rng = np.random.default_rng(24)
    v = rng.integers(0, 100, 2_048).astype(np.int32)
    bp = O.bp_compress(v, None, "for")
    data, offs, rows = O.rle_compress(np.repeat(v[:256], 8))
    const = (L.CODEC_CONSTANT, 7, 2_048)
    rle = (L.CODEC_RLE, data.tobytes(), 2_048)
    packed = bp_segments(bp)[0]
    plain = (L.CODEC_UNCOMPRESSED, v.tobytes(), 2_048)
    t2, t1 = CubitTable(ctx, 4_096), CubitTable(ctx, 2_048)
    cases = [("runs only", lambda: t2.add_segment_column(0, [const, rle], np.int32)),
             ("unpack last", lambda: t2.add_segment_column(1, [const, packed], np.int32)),
             ("span last", lambda: t2.add_segment_column(2, [packed, plain], np.int32)),
             ("rle", lambda: t1.add_rle_column(0, data, offs, rows, np.int32)),
             ("bitpacked", lambda: t1.add_bitpacked_column(1, bp.data, bp.seg_off, bp.seg_count, np.int32))]
    ctx.enable_timing(True)
    try:
        for name, call in cases:
            ctx.timing_reset()
            call()
            assert len(ctx.kernel_times_ms()) == 1, name
            assert ctx.last_kernel_ms() > 0, name
    finally:
        ctx.timing_reset()
        ctx.enable_timing(False)
    assert np.array_equal(t2.download_column(2), np.concatenate([v, v]))
    assert np.array_equal(t2.download_column(1), np.concatenate([np.full(2_048, 7, np.int32), v]))
    assert np.array_equal(t1.download_column(0), np.repeat(v[:256], 8))
    t2.close()
    t1.close()


def test_empty_partition_takes_no_segments(ctx):
    t = CubitTable(ctx, 0)
    none = np.zeros(0, np.uint64)
    t.add_bitpacked_column(0, np.zeros(0, np.uint8), none, none, np.int16)
    t.add_rle_column(1, np.zeros(0, np.uint8), none, none, np.int64)
    assert t.types == {0: L.TYPE_INT32, 1: L.TYPE_INT64}
    for col in (0, 1):
        assert len(t.scan(F.TableFilterSet({col: F.ConstantFilter(">=", 0)}))) == 0
    t.close()
