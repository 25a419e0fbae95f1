"""Time sum(a * b) at the bench's scale (612 M rows, one process) on both forced paths of
cubit_table_sum_product — from the bit slices of both operands, and the fused gather over the columns,
which is the code the library had before the slice path and so the baseline — for a 24-slice price and
a 4-slice discount (INT64 both) under filters that keep 1e-3, 1 %, 10 %, 50 % and 98 % of the rows (a
filter column with a RANGE index whose keys are the filter constants, so the program is one index leaf
and no K0 pass runs inside the timed calls). Then the TPC-H Q1 shape: the same product per group of a
3-value and a 2-value column (cubit_table_sum_product_grouped) from the slices and from the column, at
the 98 % filter, beside one cubit_table_aggregate_grouped SUM over the 24 slices alone — the traffic
floor of the grouped call, which has to read those slices and the same group bitvectors.
  Call time: three rounds, each timing five back-to-back calls between two synchronisations, the paths
alternated inside a round so drift hits them alike; the spread is the range over the rounds. Kernel
time: the dispatch-stamped time of the fused kernel (context timing), five launches. Rates are the bytes
the byte rule charges the slice path over its time. The two paths' results are compared before anything
is timed; a difference ends the run."""
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
F_SPAN = 1_000_000
SELS = [("1e-3", 1_000), ("1 %", 10_000), ("10 %", 100_000), ("50 %", 500_000), ("98 %", 980_000)]
PRICE, DISC, FLT, FLAG, STATUS = range(5)
rng = np.random.default_rng(9)
print(f"{n} rows; {ROUNDS} rounds of {LAUNCHES} calls per path", flush=True)

ctx = Context(0)
lib = L.gpu_lib()
t = CubitTable(ctx, n)
for col, make in ((FLT, lambda: rng.integers(0, F_SPAN, n, dtype=np.int32)),
                  (PRICE, lambda: rng.integers(90_000, 90_000 + 2 ** 24, n, dtype=np.int64)),
                  (DISC, lambda: rng.integers(0, 11, n, dtype=np.int64)),
                  (FLAG, lambda: rng.integers(0, 3, n, dtype=np.int32)),
                  (STATUS, lambda: rng.integers(0, 2, n, dtype=np.int32))):
    v = make()
    if col in (PRICE, DISC):  # both ends of the span occur: the slice counts do not depend on the draw
        v[0], v[1] = (90_000, 90_000 + 2 ** 24 - 1) if col == PRICE else (0, 10)
    t.add_column(col, v)
    del v
t.build_index(FLT, L.INDEX_RANGE, [c for _, c in SELS])
t.build_index(PRICE, L.INDEX_SLICED)
t.build_index(DISC, L.INDEX_SLICED)
t.build_index(FLAG, L.INDEX_EQUALITY)
t.build_index(STATUS, L.INDEX_EQUALITY)
n_a, n_b = t.index_info(PRICE)[0], t.index_info(DISC)[0]
assert (n_a, n_b) == (24, 4), (n_a, n_b)
bv = n / 8
print(f"price {n_a} slices, discount {n_b} slices; each column {8 * n / 1e9:.2f} GB, "
      f"the slices {(n_a + n_b) * bv / 1e9:.2f} GB", flush=True)
out_s, out_c, cnt = DeviceBuffer(ctx, 64), DeviceBuffer(ctx, 64), DeviceBuffer(ctx, 16)
gout_s, gout_c = DeviceBuffer(ctx, 6 * 48), DeviceBuffer(ctx, 6 * 48)


def timed(launch):
    launch()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / LAUNCHES


def kernel_ms(launch, per_call_kernels=1):
    """Mean dispatch-stamped time per call of the call's timed kernels (the fused kernel's launches)."""
    ctx.enable_timing(True)
    launch()
    ctx.sync()
    ctx.timing_reset()
    for _ in range(LAUNCHES):
        launch()
    ctx.sync()
    ms = ctx.kernel_times_ms()
    ctx.enable_timing(False)
    assert len(ms) == LAUNCHES * per_call_kernels, (len(ms), per_call_kernels)
    return sum(ms) / LAUNCHES


def line(what, ms, moved=None):
    rate = f" = {moved / 1e9:.2f} GB at {moved / min(ms) / 1e9:.2f} TB/s" if moved else ""
    print(f"{what}: {' / '.join(f'{x:.3f}' for x in ms)} ms (spread {max(ms) - min(ms):.3f}); best {min(ms):.3f} ms{rate}",
          flush=True)


def rounds(paths):
    res = {name: [] for name, _ in paths}
    for r in range(ROUNDS):
        for name, fn in paths[r % len(paths):] + paths[:r % len(paths)]:
            res[name].append(timed(fn))
    return res


print("--- cubit_table_sum_product(price, discount)", flush=True)
for sel_name, c in SELS:
    fs = F.TableFilterSet({FLT: F.ConstantFilter("<", c)})
    plan = F.serialize(fs, None)
    nodes = F.to_ctypes(plan.nodes)
    est = t.estimate_rows(fs)

    def call(flag, out):
        L.check(lib.cubit_table_sum_product(t.handle, nodes, len(plan.nodes), None, PRICE, DISC, out.ptr, cnt.ptr, flag))

    def from_slices():
        call(L.SUM_FROM_SLICES, out_s)

    def from_column():
        call(L.SUM_FROM_COLUMN, out_c)

    from_slices()
    from_column()
    ctx.sync()
    a, b = out_s.download(np.int64, 2), out_c.download(np.int64, 2)
    if not np.array_equal(a, b):
        print(f"paths differ at {sel_name}: slices {a} column {b}", flush=True)
        sys.exit(1)
    rows = int(cnt.download(np.uint64, 1)[0])
    call(0, out_s)
    ctx.sync()
    chosen = "slices" if t.last_sum_product()[0] else "column"
    res = rounds([("slices", from_slices), ("column", from_column)])
    k_ms = kernel_ms(from_slices)
    moved = (1 + n_a + n_b) * bv
    print(f"selectivity {sel_name} ({rows} rows, estimate {est}); path=None takes the {chosen}", flush=True)
    line("  from the slices", res["slices"], moved)
    line("  from the column", res["column"])
    spread = max(max(ms) - min(ms) for ms in res.values())
    print(f"  slices / column = {min(res['slices']) / min(res['column']):.2f} (largest spread {spread:.3f} ms); "
          f"fused kernel {k_ms:.3f} ms = {moved / k_ms / 1e9:.2f} TB/s", flush=True)

print("--- the Q1 shape: per (flag, status) group, 3 x 2 groups, the 98 % filter", flush=True)
fs = F.TableFilterSet({FLT: F.ConstantFilter("<", SELS[-1][1])})
plan = F.serialize(fs, None)
nodes = F.to_ctypes(plan.nodes)
by = (C.c_int * 2)(FLAG, STATUS)


def grouped(flag, out):
    L.check(lib.cubit_table_sum_product_grouped(t.handle, nodes, len(plan.nodes), None, PRICE, DISC, by, 2, flag, out.ptr, 6))


def grouped_slices():
    grouped(L.SUM_FROM_SLICES, gout_s)


def grouped_column():
    grouped(L.SUM_FROM_COLUMN, gout_c)


def floor_sum():
    L.check(lib.cubit_table_aggregate_grouped(t.handle, nodes, len(plan.nodes), None, PRICE, by, 2,
                                              L.AGG_SUM | L.AGG_FROM_SLICES, gout_c.ptr, 6))


grouped_slices()
grouped_column()
ctx.sync()
a, b = gout_s.download(np.int64, 24), gout_c.download(np.int64, 24)
if not np.array_equal(a, b):
    print(f"grouped paths differ: slices {a} column {b}", flush=True)
    sys.exit(1)
grouped(0, gout_s)
ctx.sync()
used, launches = t.last_sum_product()
print(f"path=None takes the {'slices' if used else 'column'}; the fused kernel runs {launches if used else 2} launches",
      flush=True)
grouped_slices()
launches = t.last_sum_product()[1]
floor_sum()
floor_launches = t.last_grouped()[2]
res = rounds([("slices", grouped_slices), ("column", grouped_column), ("floor", floor_sum)])
moved = launches * (1 + n_a + n_b) * bv + (3 + 2 * 2) * bv  # two launches of 2 x 2 and 1 x 2 group leaves
floor_moved = floor_launches * (1 + n_a) * bv + (3 + 2) * bv
k_ms = kernel_ms(grouped_slices, launches)
kf_ms = kernel_ms(floor_sum, floor_launches)
line(f"  sum_product_grouped from the slices ({launches} launches)", res["slices"], moved)
line("  sum_product_grouped from the column", res["column"])
line(f"  aggregate_grouped SUM(price) from its {n_a} slices ({floor_launches} launches)", res["floor"], floor_moved)
spread = max(max(ms) - min(ms) for ms in res.values())
print(f"  slices / column = {min(res['slices']) / min(res['column']):.3f}; slices / floor = "
      f"{min(res['slices']) / min(res['floor']):.2f} (largest spread {spread:.3f} ms); fused kernels {k_ms:.3f} ms per call "
      f"= {moved / k_ms / 1e9:.2f} TB/s; floor kernels {kf_ms:.3f} ms = {floor_moved / kf_ms / 1e9:.2f} TB/s", flush=True)
for b in (out_s, out_c, cnt, gout_s, gout_c):
    b.free()
t.close()
ctx.close()
