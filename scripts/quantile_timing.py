"""Time cubit_table_build_index_quantiles at the bench's scale (612 M rows) on four columns: INT32
over a 2,526-value span (a date column: one histogram pass), INT64 over a 2^24 span, INT64 over
the full 64-bit range, and a single-valued INT64 column (every row in one LDS counter). Per column:
each histogram pass (the dispatch's own time, and the column's bytes over it), the whole call at 64
and 256 bins, build_index with the same keys given (what remains is the chooser's share), and one
K0 comparison (cubit_build_bitvector) over the same column in the same process: a pass and K0 both
stream the column once, so K0 is the yardstick for a pass.

--plain-adds times the histogram kernel without its wave-level pre-aggregation
(CUBIT_QUANTILE_PLAIN_ADDS); run both forms to see what it pays."""
import os
import sys
import time

import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--plain-adds" in sys.argv:
    os.environ["CUBIT_QUANTILE_PLAIN_ADDS"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "duckdb-cubit_amd"))
from cubit_amd import _lib as L  # noqa: E402
from cubit_amd.table import Context, CubitTable, DeviceBuffer  # noqa: E402

n = int(args[0]) if args else 612_000_000
rng = np.random.default_rng(8)
print(f"{n} rows; histogram adds: {'plain' if 'CUBIT_QUANTILE_PLAIN_ADDS' in os.environ else 'wave-aggregated'}",
      flush=True)


def columns():
    yield "INT32, 2,526-value span", rng.integers(8035, 8035 + 2526, n, dtype=np.int32)
    yield "INT64, 2^24 span", rng.integers(0, 2 ** 24, n, dtype=np.int64)
    yield "INT64, full range", rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True)
    yield "INT64, one value", np.full(n, 19_940_101, dtype=np.int64)


ctx = Context(0)
ctx.enable_timing(True)
lib = L.gpu_lib()
words = DeviceBuffer(ctx, int(lib.cubit_padded_words(n)) * 8)
for name, v in columns():
    typ = L.TYPE_INT32 if v.dtype == np.int32 else L.TYPE_INT64
    probe = int(v[n // 2])
    d_col = ctx.upload(v)
    nbytes = v.nbytes
    del v
    t = CubitTable(ctx, n)
    t.add_device_column(0, d_col.addr, typ)
    print(f"--- {name} ({nbytes / 1e9:.2f} GB)", flush=True)
    # K0 first (it also warms the clocks): five launches back to back between two synchronisations
    L.check(lib.cubit_build_bitvector(ctx.handle, d_col.ptr, typ, None, n, L.CMP_LT, probe, words.ptr))
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(5):
        L.check(lib.cubit_build_bitvector(ctx.handle, d_col.ptr, typ, None, n, L.CMP_LT, probe, words.ptr))
    ctx.sync()
    k0_ms = (time.perf_counter() - t0) * 1e3 / 5
    print(f"K0 (v < {probe}): {k0_ms:.3f} ms = {nbytes / k0_ms / 1e9:.2f} TB/s", flush=True)
    for n_bins in (64, 256):
        call_ms = given_ms = float("inf")
        for _ in range(2):  # the faster of two: the first call of a size also allocates its bitvectors
            ctx.timing_reset()
            t0 = time.perf_counter()
            keys = t.build_index_quantiles(0, n_bins)
            call_ms = min(call_ms, (time.perf_counter() - t0) * 1e3)
            passes = ctx.kernel_times_ms()
        for _ in range(2 if len(keys) else 0):
            t0 = time.perf_counter()
            t.build_index(0, L.INDEX_RANGE, keys)
            given_ms = min(given_ms, (time.perf_counter() - t0) * 1e3)
        given_ms = given_ms if len(keys) else 0.0
        print(f"n_bins {n_bins}: {len(keys)} keys, {len(passes)} passes of {sum(passes):.2f} ms in all; whole call "
              f"{call_ms:.2f} ms, build_index with the keys given {given_ms:.2f} ms, the difference (statistics, "
              f"passes, counters to the host) {call_ms - given_ms:.2f} ms", flush=True)
        for i, ms in enumerate(passes):
            print(f"  pass {i}: {ms:.3f} ms = {nbytes / ms / 1e9:.2f} TB/s; pass / K0 = {ms / k0_ms:.2f}", flush=True)
    t.close()
    d_col.free()
words.free()
ctx.close()
