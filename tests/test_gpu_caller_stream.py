"""The table API on a caller's non-blocking stream, behind work already pending on it.

include/cubit_gpu.h promises that a context issues all its GPU work on its one stream
(cubit_ctx_set_stream). Every other GPU test runs on the legacy null stream, where the runtime
serialises a wrongly ordered operation and it looks correct. Here each context is bound to a torch
pool stream (hipStreamNonBlocking: no implicit ordering with the null stream) and its `lib` is
replaced by a proxy that enqueues a spin (torch.cuda._sleep) on the context's current stream before
every cubit_* call. Work the library issues on the context stream queues behind the spin; work
wrongly issued on the null stream, or read by the host too early, completes first — a misordering
loses every time instead of rarely. The table function (libcubit_scan.so calls the C ABI itself)
gets the same spin before every cubit_scan_* call.

The delay. torch.cuda._sleep takes cycles of a device clock whose rate is measured, not assumed:
once per module one _sleep is timed with two events on a pool stream, and the cycles are scaled so
that one delay lasts at least 20 times the wall time of the canary's host-side copy (a null-stream
copy_ of one 150,001-row bitvector, 18,944 bytes, and its synchronise), and at least 1 ms (a floor
for host jitter; neither figure is taken from what the library's tests do). On an MI355X this
measured 2,378,000 cycles per ms and a copy of 0.016 ms (20 times: 0.33 ms), so the floor decides:
2,972,000 cycles = 1.24 ms per call.

The canary (test_canary_...) proves the harness with no library logic in it: a stream-ordered
memset issued behind the spin lands after a null-stream write that had already completed, 20 times
of 20. If it fails the delay holds nothing back and no other test here means anything.

A misorder must stay a mismatch, never a wild address: output buffers handed to the raw ABI here
are zeroed through the context and synchronised first, and row ids are checked against the oracle
on the host before they go into a probe.

What the harness cannot show: a call that waits for the stream before its later stream work has
drained the delay by then, so for what follows inside that call these tests prove correctness on a
non-blocking stream, not ordering behind pending work. cubit_table_append, cubit_table_merge_updates
and cubit_table_sync_column (before they rewrite index words in place), cubit_table_save_index (it
reads), cubit_ctx_set_stream (the old stream) and cubit_table_destroy synchronise the stream first;
cubit_table_add_column with a validity mask, the index builds, the quantile select and a scan that
computes zone classes or hides rows wait part-way (a host read of a device result), so only their
work up to that wait runs behind the spin.
"""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest
import torch

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.scan_function import ROW_ID, CubitScanFunction
from cubit_amd.table import Context, CubitTable, Dictionary, pack_strings, padded_words, runs_in_row_order
from oracle import oracle as O
from test_gpu_maintenance_fuzz import run as maintenance_run
from test_gpu_segments import mixed_column
from test_gpu_string_filters import random_strings
from test_gpu_sync_column import changed_rows, expected_column, mutate
from test_gpu_typed_fuzz import typed_round
from test_oracle_bitpacking import REF_SEGMENTS, reference_segment
from test_oracle_rle import runs_column

pytestmark = pytest.mark.gpu

N = 150_001        # two tiles of 131,072 rows, a ragged last word
N3 = 300_001       # three tiles
TXN_START = 4611686018427388000
WRITER = TXN_START + 5
MIN_DELAY_MS = 1.0
COPY_MARGIN = 20


# ------------------------------------------------------------------ the harness

def torch_stream(ptr):
    """The torch handle of a hipStream_t (None / 0: the null stream)."""
    return torch.cuda.ExternalStream(int(ptr)) if ptr else torch.cuda.default_stream()


class DelayedLib:
    """libcubitgpu.so with a spin enqueued on the context's current stream before every call."""

    def __init__(self, lib, cycles, stream):
        self._lib, self._cycles, self._stream = lib, cycles, stream

    def spin(self):
        with torch.cuda.stream(self._stream):
            torch.cuda._sleep(self._cycles)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cubit_"):
            return fn

        def call(*args):
            self.spin()
            rc = fn(*args)
            if name == "cubit_ctx_set_stream" and rc == L.OK:  # the delay follows the context's stream
                ptr = args[1].value if isinstance(args[1], C.c_void_p) else args[1]
                self._stream = torch_stream(ptr)
            return rc

        return call


class DelayedScanLib:
    """libcubit_scan.so with the spin on every given context's stream before every call."""

    def __init__(self, lib, delayed_libs):
        self._lib, self._libs = lib, delayed_libs

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cubit_scan_"):
            return fn

        def call(*args):
            for d in self._libs:
                d.spin()
            return fn(*args)

        return call


class DeviceView:
    """A DeviceBuffer as torch sees it (bytes), for writes that bypass the context."""

    def __init__(self, buf):
        self.__cuda_array_interface__ = {"shape": (buf.nbytes,), "typestr": "|u1", "data": (buf.addr, False),
                                         "version": 2}


def timed_sleep_ms(stream, cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def null_stream_copy_ms(view, ones):
    t0 = time.perf_counter()
    view.copy_(ones)
    torch.cuda.default_stream().synchronize()
    return (time.perf_counter() - t0) * 1e3


@pytest.fixture(scope="module")
def delay():
    """{"cycles", "ms", "copy_ms"}: the calibrated spin, see the module docstring."""
    s = torch.cuda.Stream()
    c0 = Context(0)
    buf = c0.alloc(padded_words(N) * 8)
    view = torch.as_tensor(DeviceView(buf), device="cuda")
    ones = torch.full((buf.nbytes,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        null_stream_copy_ms(view, ones)
    copy_ms = float(np.median([null_stream_copy_ms(view, ones) for _ in range(9)]))
    probe = 1_000_000
    timed_sleep_ms(s, probe)
    per_ms = probe / float(np.median([timed_sleep_ms(s, probe) for _ in range(3)]))
    target = max(COPY_MARGIN * copy_ms, MIN_DELAY_MS)
    cycles = int(math.ceil(1.25 * target * per_ms))
    for _ in range(4):  # the scaled spin is measured itself, not trusted to be linear
        ms = min(timed_sleep_ms(s, cycles) for _ in range(3))
        if ms >= target:
            break
        cycles *= 2
    assert ms >= target, (cycles, ms, target)
    buf.free()
    c0.close()
    print(f"caller-stream delay: {cycles} cycles = {ms:.3f} ms per call ({per_ms:.0f} cycles/ms; "
          f"null-stream copy {copy_ms:.4f} ms, target {target:.3f} ms)")
    return {"cycles": cycles, "ms": ms, "copy_ms": copy_ms}


def pool_stream(cycles):
    """A torch pool stream that the null stream does not queue behind. The runtime multiplexes its
    streams over a few hardware queues, and two streams on one queue run in order: a spin on such a
    stream would hold the null stream back too and hide the very misorders it is there to expose.
    Each candidate is tried with the spin itself: a null-stream kernel must finish while it runs."""
    probe = torch.zeros(16, device="cuda")
    for _ in range(32):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
        probe.add_(1)
        torch.cuda.default_stream().synchronize()
        clear = not s.query()
        s.synchronize()
        if clear:
            return s
    pytest.fail("the null stream waited for the spin on every pool stream: the delay cannot separate them")


class Delayed:
    """A context on its own torch pool stream whose every call queues behind a spin."""

    def __init__(self, delay):
        self.stream = pool_stream(delay["cycles"])
        self.ctx = Context(0, stream=self.stream.cuda_stream)
        self.lib = DelayedLib(self.ctx.lib, delay["cycles"], self.stream)
        self.ctx.lib = self.lib

    def close(self):
        self.ctx.close()


@pytest.fixture
def delayed(delay):
    made = []

    def make():
        d = Delayed(delay)
        d.pool_stream = lambda: pool_stream(delay["cycles"])
        made.append(d)
        return d

    yield make
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def null_ctx():
    c = Context(0)
    yield c
    c.close()


def delayed_scan_lib(monkeypatch, *ds):
    """The table function's library with the spin on the given contexts' streams."""
    real = L.scan_lib()
    proxy = DelayedScanLib(real, [d.lib for d in ds])
    monkeypatch.setattr(L, "scan_lib", lambda: proxy)


def scan_tiles(ctx, t, fs, n_rows, txn=None, ordered=True, zonemap=True):
    """cubit_table_scan_tiles into buffers zeroed through the context first (stale data stays an
    in-range value): (ids as written, count, this scan's tile directory)."""
    nodes = F.to_ctypes(F.serialize(fs).nodes)
    tiles = (n_rows + 131_071) // 131_072
    ids, cnt, d_dir = ctx.alloc(n_rows * 8), ctx.alloc(16), ctx.alloc(tiles * 16)
    for b in (ids, cnt, d_dir):
        b.zero()
    ctx.sync()
    nt, rpt = C.c_uint32(), C.c_uint64()
    flags = (L.SCAN_ORDERED if ordered else 0) | (0 if zonemap else L.SCAN_NO_ZONEMAP)
    L.check(ctx.lib.cubit_table_scan_tiles(t.handle, nodes, len(nodes), C.byref(txn) if txn is not None else None,
                                           C.c_void_p(ids.addr), n_rows, C.c_void_p(cnt.addr), flags,
                                           C.c_void_p(d_dir.addr), tiles, C.byref(nt), C.byref(rpt)))
    ctx.check()
    k = int(cnt.download(np.uint64, 1)[0])
    assert k <= n_rows
    got = ids.download(np.int64, k)
    directory = d_dir.download(np.uint64, 2 * nt.value).reshape(-1, 2)
    return got, k, directory, (ids, cnt, d_dir)


# ------------------------------------------------------------------ the canary

def test_canary_stream_write_lands_after_completed_null_stream_write(delay, delayed):
    d = delayed()
    ctx = d.ctx
    nbytes = padded_words(N) * 8
    buf = ctx.alloc(nbytes)
    view = torch.as_tensor(DeviceView(buf), device="cuda")
    ones = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(20):
        # the proxy enqueues the spin on the context's stream, then the stream-ordered memset
        L.check(ctx.lib.cubit_memset_d(ctx.handle, buf.ptr, 0, nbytes))
        view.copy_(ones)  # the null stream: ordered with nothing on a non-blocking stream
        torch.cuda.default_stream().synchronize()
        held_back = not d.stream.query()  # the null-stream write is done, the memset still queued
        ctx.sync()
        got = buf.download(np.uint8, nbytes)
        assert held_back, (i, delay)
        assert not got.any(), (i, int(np.count_nonzero(got)), delay)


# ------------------------------------------------------------------ index files

@pytest.fixture(scope="module")
def index_case(null_ctx, tmp_path_factory):
    """Three columns with a RANGE (every value), an EQUALITY and an edge-keyed RANGE + BINS index,
    built and saved on a null-stream context; the oracle's rows for a few filter sets."""
    rng = np.random.default_rng(41)
    cols = [rng.integers(0, 50, N).astype(dt) for dt in (np.int32, np.int64, np.int32)]
    ok = rng.random(N) > 0.1
    defs = [(0, L.INDEX_RANGE, None), (1, L.INDEX_EQUALITY, None), (2, L.INDEX_RANGE, [10, 20, 30, 40]),
            (2, L.INDEX_BINS, [0, 10, 20, 30, 40, 50])]
    d = tmp_path_factory.mktemp("null_stream_indexes")
    t = CubitTable(null_ctx, N, row_base=5)
    for c, a in enumerate(cols):
        t.add_column(c, a, validity_from_mask(ok) if c == 0 else None)
    files = []
    for c, enc, keys in defs:
        t.build_index(c, enc, keys)
        files.append(d / f"c{c}_{enc}.cubitix")
        t.save_index(c, enc, files[-1])
    t.close()
    ocols = [O.Column(a, validity_from_mask(ok) if c == 0 else None) for c, a in enumerate(cols)]
    sets = [F.TableFilterSet({0: F.ConstantFilter("<", 17)}),
            F.TableFilterSet({1: F.ConstantFilter("=", 23)}),
            F.TableFilterSet({2: F.ConjunctionAndFilter([F.ConstantFilter(">=", 20), F.ConstantFilter("<", 40)])}),
            F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 5), F.ConstantFilter("<", 30)]),
                              1: F.ConstantFilter("=", 7), 2: F.ConstantFilter("<", 30)})]
    refs = [O.table_scan(ocols, F.serialize(fs), N, row_base=5) for fs in sets]
    assert all(len(r) > 0 for r in refs)
    return dict(cols=cols, ok=ok, defs=defs, files=files, sets=sets, refs=refs)


def index_table(ctx, case):
    t = CubitTable(ctx, N, row_base=5)
    for c, a in enumerate(case["cols"]):
        t.add_column(c, a, validity_from_mask(case["ok"]) if c == 0 else None)
    return t


def test_index_load_behind_pending_work(index_case, delayed, tmp_path):
    """cubit_table_load_index zeroes each bitvector on the context stream; its upload must follow
    that memset in stream order. (The upload used to be a null-stream hipMemcpy: behind a busy
    non-blocking stream the memset landed after it and zeroed the loaded index — this test then
    fails on the first scan with fewer rows than the oracle's.)"""
    ctx = delayed().ctx
    t = index_table(ctx, index_case)
    for (c, enc, _), f in zip(index_case["defs"], index_case["files"]):
        t.load_index(c, f)
    for fs, ref in zip(index_case["sets"], index_case["refs"]):
        got = t.scan(fs)
        assert len(got) == len(ref), (fs, len(got), len(ref))
        assert np.array_equal(got, ref), fs
    for (c, enc, _), f in zip(index_case["defs"], index_case["files"]):
        again = tmp_path / f.name
        t.save_index(c, enc, again)
        assert again.read_bytes() == f.read_bytes(), (c, enc)
    t.close()


def test_index_save_behind_pending_builds(index_case, delayed, tmp_path):
    ctx = delayed().ctx
    t = index_table(ctx, index_case)
    for c, enc, keys in index_case["defs"]:
        t.build_index(c, enc, keys)
    for (c, enc, _), f in zip(index_case["defs"], index_case["files"]):  # no wait between build and save
        mine = tmp_path / f.name
        t.save_index(c, enc, mine)
        assert mine.read_bytes() == f.read_bytes(), (c, enc)
    t.close()


# ------------------------------------------------------------------ the shared sequences

@pytest.mark.parametrize("seed,kernel", [(1, L.DECODE_AUTO), (2, L.DECODE_RUNS)])
def test_maintenance_sequence(delayed, seed, kernel):
    """Appends, update lists, merges, delete lists, insert ids and scans at several snapshots
    (test_gpu_maintenance_fuzz.run), every scan against the oracle."""
    ctx = delayed().ctx
    ctx.set_decode_kernel(kernel)
    counts = maintenance_run(ctx, seed, 60, 150_001)
    assert counts["scan"] > 10 and all(counts[op] > 0 for op in ("append", "updates", "merge", "deletes")), counts


def test_typed_round(delayed, monkeypatch):
    """FLOAT, DOUBLE, UBIGINT, VARCHAR and HUGEINT columns with update records, scans and the table
    function with its copy streams and staged pinned windows (test_gpu_typed_fuzz.typed_round)."""
    d = delayed()
    delayed_scan_lib(monkeypatch, d)
    assert typed_round(d.ctx, 7001, 300_007, with_updates=True) == 24


# ------------------------------------------------------------------ every decode kernel

def test_every_decode_kernel(delayed):
    """One Q6-shaped filter over three tiles under each forced kernel, and a one-bitvector filter
    decoded from its tile counts, ordered and in tile runs: count, ids and tile directory."""
    ctx = delayed().ctx
    rng = np.random.default_rng(6)
    ship = rng.integers(8000, 10_600, N3).astype(np.int32)
    disc = rng.integers(0, 11, N3).astype(np.int64)
    qty = rng.integers(100, 5100, N3).astype(np.int64)
    t = CubitTable(ctx, N3, row_base=9)
    for c, a in enumerate((ship, disc, qty)):
        t.add_column(c, a)
    t.build_index(0, L.INDEX_RANGE, list(range(8000, 10_601, 100)))
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE, [2400])
    q6 = F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 8800), F.ConstantFilter("<", 9200)]),
                           1: F.ConjunctionAndFilter([F.ConstantFilter(">=", 5), F.ConstantFilter("<=", 7)]),
                           2: F.ConstantFilter("<", 2400)})
    one = F.TableFilterSet({2: F.ConstantFilter("<", 2400)})
    ocols = [O.Column(ship), O.Column(disc), O.Column(qty)]
    cases = [(k, q6, O.table_scan(ocols, F.serialize(q6), N3, row_base=9), k)
             for k in (L.DECODE_PAIRS, L.DECODE_RUNS, L.DECODE_LOOKBACK)]
    cases.append((L.DECODE_AUTO, one, O.table_scan(ocols, F.serialize(one), N3, row_base=9), L.DECODE_PREFIXED))
    for kernel, fs, ref, reported in cases:
        assert len(ref) > 0
        ctx.set_decode_kernel(kernel)
        for ordered in (False, True):
            # the zonemap skip off: a live-tile list takes the run kernel whatever is forced; on for
            # the one-bitvector filter, whose tile offsets come from the zone map's counts
            got, k, directory, bufs = scan_tiles(ctx, t, fs, N3, ordered=ordered, zonemap=kernel == L.DECODE_AUTO)
            assert ctx.last_decode_kernel() == reported, (kernel, ordered)
            assert k == len(ref), (kernel, ordered, k, len(ref))
            assert directory.shape[0] == 3 and int(directory[:, 1].sum()) == k, (kernel, ordered)
            tile = (ref - 9) // 131_072
            assert directory[:, 1].tolist() == np.bincount(tile, minlength=3).tolist(), (kernel, ordered)
            last, rpt = ctx.last_tiles()
            assert rpt == 131_072 and np.array_equal(last, directory), (kernel, ordered)
            if ordered:
                assert np.array_equal(got, ref), (kernel, ordered)
            else:
                assert np.array_equal(runs_in_row_order(got, directory), ref), (kernel, ordered)
            for b in bufs:
                b.free()
    t.close()


# ------------------------------------------------------------------ ingest paths the sequences miss

def as_held(got, dt):
    return got.view(np.uint64) if np.dtype(dt) == np.uint64 else got.astype(np.int64)


def test_bitpacked_rle_and_mixed_segment_columns(delayed):
    ctx = delayed().ctx
    for s in REF_SEGMENTS:  # BITPACKING bytes as DuckDB stored them
        col, values, valid = reference_segment(s)
        t = CubitTable(ctx, s["count"])
        t.add_bitpacked_column(0, col.data, col.seg_off, col.seg_count, values.dtype, validity_from_mask(valid))
        got = t.download_column(0)
        assert np.array_equal(got, O.bp_decode(col)), s["name"]
        assert np.array_equal(got[valid], values[valid]), s["name"]
        t.close()
    rng = np.random.default_rng(8)
    v = runs_column(rng, np.int32, N3)
    ok = rng.random(N3) > 0.05
    data, offs, rows = O.rle_compress(v, ok)
    t = CubitTable(ctx, N3)
    t.add_rle_column(0, data, offs, rows, np.int32, validity_from_mask(ok))
    assert np.array_equal(t.download_column(0).astype(np.int64), O.rle_decode(data, offs, rows, np.int32).astype(np.int64))
    t.close()
    for dt in (np.int16, np.uint64):  # a column held as INT32 and one as the bits of UINT64
        vals, ok, segs = mixed_column(rng, dt, 3, 5_001)  # one row group of each codec
        t = CubitTable(ctx, len(vals))
        t.add_segment_column(0, segs, dt, validity_from_mask(ok))
        held = as_held(t.download_column(0), dt)
        want = vals.astype(np.uint64) if np.dtype(dt) == np.uint64 else vals.astype(np.int64)
        assert np.array_equal(held[ok], want[ok]), dt
        t.close()


def test_quantile_index_equals_null_stream_twin(null_ctx, delayed, tmp_path):
    ctx = delayed().ctx
    rng = np.random.default_rng(15)
    v = (rng.standard_normal(N3) * 1e6).astype(np.int64)
    ok = rng.random(N3) > 0.07
    files = []
    keys = []
    for c in (null_ctx, ctx):
        t = CubitTable(c, N3)
        t.add_column(0, v, validity_from_mask(ok))
        keys.append(t.build_index_quantiles(0, 32))
        files.append(tmp_path / f"q{len(files)}.cubitix")
        t.save_index(0, L.INDEX_RANGE, files[-1])
        if c is ctx:
            ocol = O.Column(v, validity_from_mask(ok))
            for k in (int(keys[0][3]), int(keys[0][17]) + 1):
                fs = F.TableFilterSet({0: F.ConstantFilter("<", k)})
                assert np.array_equal(t.scan(fs), O.table_scan([ocol], F.serialize(fs), N3)), k
        t.close()
    assert len(keys[0]) > 2 and np.array_equal(keys[0], keys[1])
    assert files[0].read_bytes() == files[1].read_bytes()


def test_sync_column(delayed):
    ctx = delayed().ctx
    rng = np.random.default_rng(23)
    old = rng.integers(0, 50, N3).astype(np.int64)
    ook = rng.random(N3) > 0.1
    t = CubitTable(ctx, N3, row_base=3)
    t.add_column(0, old, validity_from_mask(ook))
    t.build_index(0, L.INDEX_RANGE, [10, 20, 30, 40])
    t.build_index(0, L.INDEX_BINS, [0, 10, 20, 30, 40, 50])
    new, nok = mutate(rng, old, ook, 0.05, -5, 60)
    ch = changed_rows(old, ook, new, nok)
    n_changed, applied = t.sync_column(0, new, validity_from_mask(nok))
    assert applied and n_changed == int(ch.sum())
    want = expected_column(old, new, nok, ch)
    assert np.array_equal(t.download_column(0), want)
    ocol = O.Column(want, validity_from_mask(nok))
    for fs in (F.TableFilterSet({0: F.ConstantFilter("<", 20)}), F.TableFilterSet({0: F.ConstantFilter("=", -3)}),
               F.TableFilterSet({0: F.ConstantFilter(">", 52)}), F.TableFilterSet({0: F.IsNullFilter()}),
               F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 10), F.ConstantFilter("<", 31)])})):
        assert np.array_equal(t.scan(fs), O.table_scan([ocol], F.serialize(fs), N3, row_base=3)), fs
    t.close()


def test_device_dictionary_encode(delayed):
    ctx = delayed().ctx
    rng = np.random.default_rng(51)
    vals, pool = random_strings(rng, N, pool=300)
    vals = [None if rng.random() < 0.03 else v for v in vals]
    d = Dictionary(pool)
    want, wvalid = d.encode(vals)
    buf, offs, valid = pack_strings(vals)
    d_buf, d_offs, d_valid = ctx.upload(buf), ctx.upload(offs), ctx.upload(validity_from_mask(valid))
    d_codes = ctx.alloc(len(vals) * 4)
    d_codes.zero()
    ctx.sync()
    L.check(ctx.lib.cubit_dict_encode_device(ctx.handle, d.handle, d_buf.ptr, d_offs.ptr, len(vals), d_valid.ptr,
                                             d_codes.ptr))
    got = d_codes.download(np.int32, len(vals))
    assert np.array_equal(got[wvalid], want[wvalid]) and (got[~wvalid] == 0).all()
    assert len(np.unique(want[wvalid])) > 100  # zeros left in place would not pass for codes


# ------------------------------------------------------------------ fused sum and probes

def test_fused_sum_and_probes_with_visible_nullable_updates(delayed):
    ctx = delayed().ctx
    rng = np.random.default_rng(77)
    base = 11
    a = rng.integers(-(10 ** 12), 10 ** 12, N).astype(np.int64)
    b = np.array([-(2 ** 40) - 3, -2, 0, 5, 1000, 2 ** 35], dtype=np.int64)[rng.integers(0, 6, N)]
    key = rng.integers(0, 100, N).astype(np.int32)
    va, vb = rng.random(N) > 0.1, rng.random(N) > 0.1
    rows = np.sort(rng.choice(N, size=N // 50, replace=False)).astype(np.int64)
    upd = {}
    for c in (0, 1):
        vals = rng.integers(-(10 ** 6), 10 ** 6, len(rows)).astype(np.int64)
        vers = np.where(rng.random(len(rows)) < 0.7, np.uint64(3), np.uint64(WRITER)).astype(np.uint64)
        ok = rng.random(len(rows)) > 0.2  # False: the record sets the row NULL
        upd[c] = (rows, vals, vers, ok)
    t = CubitTable(ctx, N, row_base=base)
    t.add_column(0, a, validity_from_mask(va))
    t.add_column(1, b, validity_from_mask(vb))
    t.add_column(2, key)
    t.build_index(1, L.INDEX_RANGE)
    t.build_index(2, L.INDEX_RANGE)
    for c in (0, 1):
        t.set_updates(c, *upd[c])
    ocols = [O.Column(a, validity_from_mask(va), updates=upd[0]), O.Column(b, validity_from_mask(vb), updates=upd[1]),
             O.Column(key)]
    base_cols = [O.Column(a, validity_from_mask(va)), O.Column(b, validity_from_mask(vb)), O.Column(key)]
    fs = F.TableFilterSet({2: F.ConstantFilter("<", 30)})
    plan = F.serialize(fs)
    for txn, tx in ((None, None), (L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1)),
                    (L.Txn(10, WRITER), O.Mvcc(10, WRITER))):
        oc = ocols if txn is not None else base_cols  # no transaction: the base, no update record applied
        ref = O.table_scan(oc, plan, N, row_base=base, tx=tx)
        av, aok = O.fetch(oc[0], ref, row_base=base, tx=tx, with_valid=True)
        bv, bok = O.fetch(oc[1], ref, row_base=base, tx=tx, with_valid=True)
        both = aok & bok
        want = sum(int(x) * int(y) for x, y in zip(av[both], bv[both]))
        if txn is not None:  # the updates change what the reader sums
            assert (aok != va[ref - base]).any()
        assert t.sum_product(0, 1, fs, txn=txn) == (want, len(ref)), txn
        # row ids checked on the host before the probes read through them
        got, k, _, (d_ids, d_cnt, d_dir) = scan_tiles(ctx, t, fs, N, txn=txn, ordered=True)
        assert k == len(ref) and np.array_equal(got, ref), txn
        d_out, d_val = ctx.alloc(k * 8), ctx.alloc(((k + 63) // 64 + 1) * 8)
        for col, (xv, xok) in ((0, (av, aok)), (1, (bv, bok))):
            for b_ in (d_out, d_val):
                b_.zero()
            ctx.sync()
            t.probe(col, d_ids.addr, d_cnt.addr, k, d_out.addr, txn)
            ctx.check()
            assert np.array_equal(d_out.download(np.int64, k)[xok], xv[xok]), (txn, col)
            d_out.zero()
            ctx.sync()
            t.probe_validity(col, d_ids.addr, d_cnt.addr, k, d_out.addr, d_val.addr, txn)
            ctx.check()
            words = d_val.download(np.uint64, (k + 63) // 64)
            valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:k].astype(bool)
            assert np.array_equal(valid, xok), (txn, col)
            assert np.array_equal(d_out.download(np.int64, k), np.where(xok, xv, 0)), (txn, col)
        for b_ in (d_ids, d_cnt, d_dir, d_out, d_val):
            b_.free()
    t.close()


# ------------------------------------------------------------------ stream switches, partitions

def test_stream_switch_in_the_middle_of_a_sequence(delayed):
    """Build on stream A, switch to non-blocking B for an append and a merge, then to the null
    stream: the rows equal the oracle's after each switch."""
    d = delayed()
    ctx = d.ctx
    rng = np.random.default_rng(31)
    cols = [rng.integers(0, 50, N).astype(np.int32), rng.integers(0, 50, N).astype(np.int64)]
    sets = [F.TableFilterSet({0: F.ConstantFilter("<", 20), 1: F.ConstantFilter("=", 9)}),
            F.TableFilterSet({0: F.ConjunctionAndFilter([F.ConstantFilter(">=", 10), F.ConstantFilter("<", 45)])})]

    def check(label):
        ocols = [O.Column(c) for c in cols]
        for fs in sets:
            ref = O.table_scan(ocols, F.serialize(fs), len(cols[0]), row_base=2)
            assert len(ref) > 0 and np.array_equal(t.scan(fs), ref), (label, fs)

    t = CubitTable(ctx, N, row_base=2)
    for c, a in enumerate(cols):
        t.add_column(c, a)
    t.build_index(0, L.INDEX_RANGE)
    t.build_index(1, L.INDEX_EQUALITY)
    check("stream A")
    other = d.pool_stream()
    ctx.set_stream(other.cuda_stream)
    extra = [rng.integers(0, 50, 70_003).astype(np.int32), rng.integers(0, 50, 70_003).astype(np.int64)]
    t.append({0: extra[0], 1: extra[1]})
    cols = [np.concatenate([c, e]) for c, e in zip(cols, extra)]
    rows = np.sort(rng.choice(len(cols[0]), size=3000, replace=False)).astype(np.int64)
    vals = rng.integers(0, 50, len(rows)).astype(np.int64)
    t.set_updates(0, rows, vals, np.full(len(rows), 3, dtype=np.uint64))
    assert t.merge_updates(0, 5) == len(rows)
    cols[0][rows] = vals
    check("stream B")
    ctx.set_stream(None)
    check("null stream")
    t.close()


def test_two_partitions_one_cursor(delayed, monkeypatch):
    """DOUBLE, VARCHAR and UBIGINT columns as two partitions, each context on its own non-blocking
    stream, through one table-function cursor: row order and values exact."""
    ds = [delayed(), delayed()]
    delayed_scan_lib(monkeypatch, *ds)
    rng = np.random.default_rng(78)
    dbl = (rng.standard_normal(N3) * 100 - 400).astype(np.float64)
    dbl[rng.integers(0, N3, 50)] = math.nan
    ub = rng.integers(0, 2 ** 64 - 1, N3, dtype=np.uint64, endpoint=True)
    words = [b"", b"a", b"ab", b"b", b"\x80", b"zz"]
    strs = [words[i] for i in rng.integers(0, len(words), N3)]
    dic = Dictionary(words)
    codes, _ = dic.encode(strs)
    cuts = [0, 140_000, N3]
    tables = []
    for r, d in enumerate(ds):
        lo, hi = cuts[r], cuts[r + 1]
        t = CubitTable(d.ctx, hi - lo, row_base=lo)
        t.add_column(0, dbl[lo:hi])
        seg = np.ascontiguousarray(codes[lo:hi])
        L.check(t.lib.cubit_table_add_dict_column(t.handle, 1, dic.handle, seg.ctypes.data, None, 0))
        t.types[1] = L.TYPE_VARCHAR
        t.add_column(2, ub[lo:hi])
        t.build_index(1, L.INDEX_EQUALITY)
        tables.append(t)
    fs = F.TableFilterSet({0: F.ConstantFilter(">", -350.0), 1: F.ConstantFilter("<=", b"ab")})
    ref = O.table_scan([O.Column(dbl), O.StringColumn(strs), O.Column(ub)], F.serialize(fs), N3)
    assert ref[0] < cuts[1] <= ref[-1]  # rows of both partitions
    fn = CubitScanFunction(tables, [0, 1, 2, ROW_ID], [3, 0, 1, 2], fs)
    parts, lock = [], threading.Lock()

    def task():
        local = fn.init_local()
        while True:
            vals = fn.function(local)
            if len(vals[0]) == 0:
                return
            with lock:
                parts.append(vals)

    th = [threading.Thread(target=task) for _ in range(3)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    fn.close()
    ids = np.concatenate([p[0] for p in parts])
    assert all(np.all(np.diff(p[0]) > 0) for p in parts)  # each chunk in row order
    o = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[o], ref)
    assert np.array_equal(np.concatenate([p[1] for p in parts])[o], O.fp_bits(dbl[ref], np.float64))
    assert [dic.entry(c) for c in np.concatenate([p[2] for p in parts])[o]] == [strs[i] for i in ref]
    assert np.array_equal(np.concatenate([p[3] for p in parts])[o].view(np.uint64), ub[ref])
    for t in tables:
        t.close()
