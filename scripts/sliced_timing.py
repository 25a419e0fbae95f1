"""Time the bit-sliced index's kernels at the bench's scale (612 M rows, one process) against K0 over
the same column in the same run: INT32 over a 2,526-value span (a date column: 12 slices), INT64
over a 2^24 span (24 slices) and INT64 over the full 64-bit range (64 slices). Per column:
cubit_bitslice_build once beside one K0 launch; then three rounds, each timing five back-to-back
launches between two synchronisations of K0 (cubit_build_bitvector, v < c), of the one-sided
cubit_bitslice_compare (u <= c - base) and of the two-sided one (the middle half of the range), the
three alternated inside a round so drift hits them alike. Every figure comes with the bytes its
kernel has to move over its time; the spread is the range over the rounds. K0 in this run is the
yardstick, never an earlier figure. The outputs are compared word for word before anything is timed."""
import ctypes as C
import os
import sys
import time

import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "duckdb-cubit_amd"))
from cubit_amd import _lib as L  # noqa: E402
from cubit_amd.table import Context, DeviceBuffer  # noqa: E402

n = int(args[0]) if args else 612_000_000
ROUNDS, LAUNCHES = 3, 5
rng = np.random.default_rng(8)
print(f"{n} rows; {ROUNDS} rounds of {LAUNCHES} launches per kernel", flush=True)


def columns():
    yield "INT32, 2,526-value span", rng.integers(8035, 8035 + 2526, n, dtype=np.int32), 8035, 8035 + 2525
    yield "INT64, 2^24 span", rng.integers(0, 2 ** 24, n, dtype=np.int64), 0, 2 ** 24 - 1
    yield "INT64, full range", rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True), -2 ** 63, 2 ** 63 - 1


ctx = Context(0)
lib = L.gpu_lib()
pw = int(lib.cubit_padded_words(n))
words = DeviceBuffer(ctx, pw * 8)
words2 = DeviceBuffer(ctx, pw * 8)


def timed(launch):
    launch()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / LAUNCHES


for name, v, base, top in columns():
    typ = L.TYPE_INT32 if v.dtype == np.int32 else L.TYPE_INT64
    bits = int(top - base).bit_length()
    d_col = ctx.upload(v)
    col_bytes = v.nbytes
    del v
    slices = DeviceBuffer(ctx, bits * pw * 8)
    ptrs = (C.c_void_p * bits)(*[slices.addr + s * pw * 8 for s in range(bits)])
    bv_bytes = n / 8
    span = top - base
    c = base + span // 2  # K0: v < c + 1; one-sided slices: u <= c - base
    lo, hi = span // 4, span - span // 4
    print(f"--- {name}: {bits} slices, column {col_bytes / 1e9:.2f} GB, slices {bits * bv_bytes / 1e9:.2f} GB", flush=True)

    def k0():
        L.check(lib.cubit_build_bitvector(ctx.handle, d_col.ptr, typ, None, n, L.CMP_LE, c, words.ptr))

    def build():
        L.check(lib.cubit_bitslice_build(ctx.handle, d_col.ptr, typ, None, n, base, bits, ptrs))

    def one_sided():
        L.check(lib.cubit_bitslice_compare(ctx.handle, ptrs, bits, None, n, 0, c - base, 0, words2.ptr))

    def two_sided():
        L.check(lib.cubit_bitslice_compare(ctx.handle, ptrs, bits, None, n, lo, hi, 0, words2.ptr))

    # the build, beside one K0 (each: a warm-up launch, then one timed between synchronisations)
    build()
    k0()
    ctx.sync()
    t0 = time.perf_counter()
    build()
    ctx.sync()
    build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    k0()
    ctx.sync()
    one_k0_ms = (time.perf_counter() - t0) * 1e3
    passes = (bits + 15) // 16
    build_bytes = passes * col_bytes + bits * bv_bytes
    print(f"build: {build_ms:.3f} ms for {passes} pass(es), {build_bytes / 1e9:.2f} GB = {build_bytes / build_ms / 1e9:.2f} "
          f"TB/s; one K0 beside it {one_k0_ms:.3f} ms; build / K0 = {build_ms / one_k0_ms:.2f}", flush=True)
    # same answer before any timing: u <= c - base is v <= c
    one_sided()
    ctx.sync()
    same = np.array_equal(words.download(np.uint64, (n + 63) // 64), words2.download(np.uint64, (n + 63) // 64))
    print(f"one-sided compare equals K0 word for word: {same}", flush=True)
    if not same:
        sys.exit(1)
    res = {"K0": [], "sliced one-sided": [], "sliced two-sided": []}
    for r in range(ROUNDS):
        order = [("K0", k0), ("sliced one-sided", one_sided), ("sliced two-sided", two_sided)]
        for what, fn in order[r % 3:] + order[:r % 3]:
            res[what].append(timed(fn))
    moved = {"K0": col_bytes + bv_bytes, "sliced one-sided": (bits + 1) * bv_bytes, "sliced two-sided": (bits + 1) * bv_bytes}
    for what, ms in res.items():
        best = min(ms)
        print(f"{what}: {' / '.join(f'{x:.3f}' for x in ms)} ms (spread {max(ms) - min(ms):.3f}); best {best:.3f} ms = "
              f"{moved[what] / 1e9:.2f} GB at {moved[what] / best / 1e9:.2f} TB/s", flush=True)
    spread = max(max(ms) - min(ms) for ms in res.values())
    for what in ("sliced one-sided", "sliced two-sided"):
        gain = min(res["K0"]) - max(res[what])  # the slowest sliced round against the fastest K0 round
        print(f"{what} vs K0: best {min(res[what]) / min(res['K0']):.2f}x of K0's time; slowest sliced round is "
              f"{gain:+.3f} ms under the fastest K0 round (largest spread {spread:.3f} ms): "
              f"{'faster beyond the spread' if gain > spread else 'not faster beyond the spread'}", flush=True)
    slices.free()
    d_col.free()
words.free()
words2.free()
ctx.close()
