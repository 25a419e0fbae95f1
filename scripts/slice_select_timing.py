"""Time cubit_table_select at the bench's scale (612 M rows, one process) on both forced paths — the
radix select over the column's bit slices, and scan + probe + array select over the column — for a
12-bit INT32 column and a 24-bit INT64 column, at selectivities 1e-3 / 1 % / 50 % / 100 % (a filter column
with a RANGE index whose keys are the filter constants, so the program is one index leaf and no K0
pass runs inside the timed calls), for the median (quantile_disc 0.5) and the maximum (rank 0
descending). Beside them, in the same run and over the same number of slices, one
cubit_bitslice_compare pass as the byte-rate yardstick the aggregate used.
  Call time: three rounds, each timing five back-to-back calls between two synchronisations, the
paths alternated inside a round so drift hits them alike; the spread is the range over the rounds.
Kernel time: the dispatch-stamped time from the first pass's start to the last step's end (context
timing), five calls. The slice path's rate is the bytes its passes have to move,
(K + 1 + 2b - d_last + 2 (passes - 1)) n / 8, over that time. The two paths' six result words are
compared before anything is timed; a difference ends the run."""
import ctypes as C
import os
import sys
import time

import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "duckdb-cubit_amd"))
from cubit_amd import _lib as L  # noqa: E402
from cubit_amd import filters as F  # noqa: E402
from cubit_amd.table import Context, CubitTable, DeviceBuffer  # noqa: E402

n = int(args[0]) if args else 612_000_000
ROUNDS, LAUNCHES = 3, 5
CHUNK = 4
F_SPAN = 1_000_000
SELS = [("1e-3", 1_000), ("1 %", 10_000), ("50 %", 500_000), ("100 %", None)]
MODES = [("median", L.SELECT_QUANTILE, 0, 0.5), ("max", L.SELECT_RANK_DESC, 0, 0.0)]
rng = np.random.default_rng(9)
print(f"{n} rows; {ROUNDS} rounds of {LAUNCHES} calls per path", flush=True)

ctx = Context(0)
lib = L.gpu_lib()
pw = int(lib.cubit_padded_words(n))
t = CubitTable(ctx, n)
f = rng.integers(0, F_SPAN, n, dtype=np.int32)
t.add_column(0, f)
t.build_index(0, L.INDEX_RANGE, [c for _, c in SELS if c is not None])
del f
COLS = [(1, "INT32, 2,526-value span", rng.integers(8035, 8035 + 2526, n, dtype=np.int32), 8035, 8035 + 2525),
        (2, "INT64, 2^24 span", rng.integers(0, 2 ** 24, n, dtype=np.int64), 0, 2 ** 24 - 1)]
out_s, out_c = DeviceBuffer(ctx, 64), DeviceBuffer(ctx, 64)
words = DeviceBuffer(ctx, pw * 8)


def timed(launch):
    launch()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / LAUNCHES


def kernel_ms(launch):
    """Mean dispatch-stamped time of the last timed span of each call (the select's passes / the compare)."""
    ctx.enable_timing(True)
    launch()
    ctx.sync()
    ctx.timing_reset()
    for _ in range(LAUNCHES):
        launch()
    ctx.sync()
    ms = ctx.kernel_times_ms()
    ctx.enable_timing(False)
    per_call = len(ms) // LAUNCHES
    assert per_call >= 1 and len(ms) == LAUNCHES * per_call, len(ms)
    return sum(ms[per_call - 1::per_call]) / LAUNCHES


def line(what, ms, moved=None):
    rate = f" = {moved / 1e9:.2f} GB at {moved / min(ms) / 1e9:.2f} TB/s" if moved else ""
    print(f"{what}: {' / '.join(f'{x:.3f}' for x in ms)} ms (spread {max(ms) - min(ms):.3f}); best {min(ms):.3f} ms{rate}",
          flush=True)


for col, name, v, base, top in COLS:
    elem = v.dtype.itemsize
    bits = int(top - base).bit_length()
    t.add_column(col, v)
    del v
    t.build_index(col, L.INDEX_SLICED)
    assert t.index_info(col)[0] == bits
    # the yardstick's own slices, built from the table's column on the device
    d_col, typ = t.column_data(col)
    slices = DeviceBuffer(ctx, bits * pw * 8)
    ptrs = (C.c_void_p * bits)(*[slices.addr + s * pw * 8 for s in range(bits)])
    L.check(lib.cubit_bitslice_build(ctx.handle, C.c_void_p(d_col), typ, None, n, base, bits, ptrs))
    bv = n / 8
    passes = (bits + CHUNK - 1) // CHUNK
    print(f"--- {name}: {bits} slices = {passes} passes, column {elem * n / 1e9:.2f} GB, slices {bits * bv / 1e9:.2f} GB",
          flush=True)

    def compare():
        L.check(lib.cubit_bitslice_compare(ctx.handle, ptrs, bits, None, n, 0, (top - base) // 2, 0, words.ptr))

    cmp_ms = [timed(compare) for _ in range(ROUNDS)]
    cmp_kernel = kernel_ms(compare)
    line(f"bitslice_compare, one pass over {bits} slices", cmp_ms, (bits + 1) * bv)
    print(f"bitslice_compare kernel time {cmp_kernel:.3f} ms = {(bits + 1) * bv / cmp_kernel / 1e9:.2f} TB/s", flush=True)
    for sel_name, c in SELS:
        fs = F.TableFilterSet({0: F.ConstantFilter("<", c)}) if c is not None else None
        plan = F.serialize(fs, None)
        nodes = F.to_ctypes(plan.nodes)
        est = t.estimate_rows(fs)
        k_leaves = 1 if c is not None else 0
        moved = (k_leaves + 1 + 2 * bits - CHUNK + 2 * (passes - 1)) * bv  # an upper bound: empty waves skip their slices
        for mode_name, mode, k, q in MODES:

            def call(flag, out):
                L.check(lib.cubit_table_select(t.handle, nodes, len(plan.nodes), None, col, mode, k, q, flag, out.ptr))

            def from_slices():
                call(L.SELECT_FROM_SLICES, out_s)

            def from_column():
                call(L.SELECT_FROM_COLUMN, out_c)

            from_slices()
            from_column()
            ctx.sync()
            a, b = out_s.download(np.int64, 6), out_c.download(np.int64, 6)
            if not np.array_equal(a, b):
                print(f"paths differ at {sel_name} {mode_name}: slices {a} column {b}", flush=True)
                sys.exit(1)
            call(0, out_s)
            ctx.sync()
            chosen = "slices" if t.last_select()[0] else "column"
            res = {"slices": [], "column": []}
            for r in range(ROUNDS):
                order = [("slices", from_slices), ("column", from_column)]
                for what, fn in order[r % 2:] + order[:r % 2]:
                    res[what].append(timed(fn))
            k_ms = kernel_ms(from_slices)
            rows = int(a[5])
            print(f"{name}; selectivity {sel_name} ({rows} rows, estimate {est}); {mode_name} = {int(a[0])} "
                  f"(below {int(a[2])}, equal {int(a[3])}); path=None takes the {chosen}", flush=True)
            line("  from the slices", res["slices"], moved)
            line("  from the column", res["column"])
            spread = max(max(ms) - min(ms) for ms in res.values())
            print(f"  slices / column = {min(res['slices']) / min(res['column']):.2f} (largest spread {spread:.3f} ms); "
                  f"select passes {k_ms:.3f} ms = {moved / k_ms / 1e9:.2f} TB/s; "
                  f"select passes / compare kernel = {k_ms / cmp_kernel:.2f}", flush=True)
    slices.free()
words.free()
t.close()
ctx.close()
