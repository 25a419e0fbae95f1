"""Time cubit_table_select_grouped at the bench's scale (612 M rows, one process), with the method and the
synthetic data of group_agg_timing.py and slice_select_timing.py: value columns of 12 slices (INT32) and
24 slices (INT64); group layouts of a 3-value column with a 2-value column whose combination (2, 1) is
empty (6 group slots), a 7-value column alone and a 25-value column alone, each with an every-value
EQUALITY index; a filter column with a RANGE index whose keys are the filter constants, keeping about
0.1 %, 2 %, 50 % and 98 % of the rows. The measured quantity is the median (quantile_disc 0.5). In each
alternated round:
  the grouped call from the slices;
  the loop of n_groups cubit_table_select calls with the group's equality predicates ANDed into the
  filter (what a caller had to do before), each forced to the path path=None gives it;
  the grouped call from the column;
  one ungrouped cubit_table_select over the same slices.
Call time: five rounds, each timing back-to-back calls between two synchronisations, the contenders
alternated inside a round so drift hits them alike; the spread is the range over the rounds. Kernel
time: the dispatch-stamped times of one call's batches (first pass's start to last step's end), summed.
Bytes by the formulas of DESIGN.md §3: grouped, per batch (K + 1 + 2b - d_last + 2 (passes - 1) +
leaves · passes) n / 8; the loop G times the ungrouped select's bytes with one more leaf per group
column; ungrouped (K + 1 + 2b - d_last + 2 (passes - 1)) n / 8. The three grouped results (slices,
column, loop) are compared before anything is timed; a difference ends the run. The value columns are
not nullable, so no formula here carries the validity's bit. --out=PATH also writes every line to PATH
(the run recorded under profiles/)."""
import ctypes as C
import os
import sys
import time

import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = next((a[len("--out="):] for a in sys.argv[1:] if a.startswith("--out=")), None)
if out_path:
    class Tee:
        def __init__(self, *files):
            self.files = files

        def write(self, text):
            for f in self.files:
                f.write(text)

        def flush(self):
            for f in self.files:
                f.flush()

    sys.stdout = Tee(sys.stdout, open(out_path, "w"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "duckdb-cubit_amd"))
from cubit_amd import _lib as L  # noqa: E402
from cubit_amd import filters as F  # noqa: E402
from cubit_amd.table import Context, CubitTable, DeviceBuffer  # noqa: E402

n = int(args[0]) if args else 612_000_000
ROUNDS, LAUNCHES = 5, 5
CHUNK = 4  # kSelectChunk (cubit_program.hpp): slices per pass
F_SPAN = 1_000_000
SELS = [("0.1 %", 1_000), ("2 %", 20_000), ("50 %", 500_000), ("98 %", 980_000)]
MODE, RANK, Q = L.SELECT_QUANTILE, 0, 0.5
rng = np.random.default_rng(9)
print(f"{n} rows; {ROUNDS} rounds of {LAUNCHES} calls per contender; the median", flush=True)

ctx = Context(0)
lib = L.gpu_lib()
t = CubitTable(ctx, n)
f = rng.integers(0, F_SPAN, n, dtype=np.int32)
t.add_column(0, f)
t.build_index(0, L.INDEX_RANGE, sorted(c for _, c in SELS))
del f
VALUES = [(1, "INT32, 12 slices", lambda: rng.integers(8035, 8035 + 2526, n, dtype=np.int32), 12),
          (2, "INT64, 24 slices", lambda: rng.integers(0, 2 ** 24, n, dtype=np.int64), 24)]
for col, name, make, bits in VALUES:
    t.add_column(col, make())
    t.build_index(col, L.INDEX_SLICED)
    assert t.index_info(col)[0] == bits
g3 = rng.integers(0, 3, n, dtype=np.int32)
g2 = rng.integers(0, 2, n, dtype=np.int32)
g2[g3 == 2] = 0  # one combination empty
GROUP_DATA = {3: g3, 4: g2, 5: rng.integers(0, 7, n, dtype=np.int32), 6: rng.integers(0, 25, n, dtype=np.int32)}
for col, data in GROUP_DATA.items():
    t.add_column(col, data)
    t.build_index(col, L.INDEX_EQUALITY)
del g3, g2, GROUP_DATA
LAYOUTS = [("3 x 2 values, one empty", [3, 4]), ("7 values", [5]), ("25 values", [6])]
bv = n / 8


def timed(launch, launches=LAUNCHES):
    launch()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / launches


def kernel_ms(launch, per_call_spans):
    """Dispatch-stamped time of the last per_call_spans timed spans of each call, summed, mean over calls."""
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
    assert per_call >= per_call_spans and len(ms) == LAUNCHES * per_call, (len(ms), per_call_spans)
    return sum(sum(ms[i * per_call + per_call - per_call_spans:(i + 1) * per_call]) for i in range(LAUNCHES)) / LAUNCHES


def line(what, ms, moved=None):
    rate = f" = {moved / 1e9:.2f} GB at {moved / min(ms) / 1e9:.2f} TB/s" if moved else ""
    print(f"{what}: {' / '.join(f'{x:.3f}' for x in ms)} ms (spread {max(ms) - min(ms):.3f}); best {min(ms):.3f} ms{rate}",
          flush=True)


for col, name, _, bits in VALUES:
    passes = (bits + CHUNK - 1) // CHUNK
    K = 1
    select_bits = K + 1 + 2 * bits - CHUNK + 2 * (passes - 1)  # an upper bound: empty waves skip their slices
    for lay_name, by in LAYOUTS:
        groups = t.aggregate_groups(by)
        G = len(groups)
        by_arr = (C.c_int * len(by))(*by)
        out_s, out_c, out_l = (DeviceBuffer(ctx, G * 48) for _ in range(3))
        out_1 = DeviceBuffer(ctx, 64)
        for sel_name, c in SELS:
            fs = F.TableFilterSet({0: F.ConstantFilter("<", c)})
            plan = F.serialize(fs, None)
            nodes = F.to_ctypes(plan.nodes)
            # the loop's filters: the group's equality predicates ANDed in
            loop_plans = []
            for key in groups:
                p = F.serialize(F.TableFilterSet({0: F.ConstantFilter("<", c),
                                                  **{g: F.ConstantFilter("=", k) for g, k in zip(by, key)}}), None)
                loop_plans.append([F.to_ctypes(p.nodes), len(p.nodes), 0])

            def grouped(flag, out):
                L.check(lib.cubit_table_select_grouped(t.handle, nodes, len(plan.nodes), None, col, by_arr, len(by), MODE,
                                                       RANK, Q, flag, out.ptr, G))

            def from_slices():
                grouped(L.SELECT_FROM_SLICES, out_s)

            def from_column():
                grouped(L.SELECT_FROM_COLUMN, out_c)

            def loop():
                for g, (arr, cnt, flag) in enumerate(loop_plans):
                    L.check(lib.cubit_table_select(t.handle, arr, cnt, None, col, MODE, RANK, Q, flag,
                                                   C.c_void_p(out_l.addr + 48 * g)))

            def ungrouped():
                L.check(lib.cubit_table_select(t.handle, nodes, len(plan.nodes), None, col, MODE, RANK, Q,
                                               L.SELECT_FROM_SLICES, out_1.ptr))

            # each call of the loop forced to the path path=None gives it
            loop_slices = 0
            for g, lp in enumerate(loop_plans):
                L.check(lib.cubit_table_select(t.handle, lp[0], lp[1], None, col, MODE, RANK, Q, 0, C.c_void_p(out_l.addr + 48 * g)))
                took = t.last_select()[0]
                lp[2] = L.SELECT_FROM_SLICES if took else L.SELECT_FROM_COLUMN
                loop_slices += int(took)
            from_slices()
            _, _, launches, _ = t.last_select_grouped()
            from_column()
            loop()
            ctx.sync()
            a, b, d = (o.download(np.int64, G * 6) for o in (out_s, out_c, out_l))
            if not (np.array_equal(a, b) and np.array_equal(a, d)):
                print(f"results differ at {lay_name} {sel_name}: slices {a} column {b} loop {d}", flush=True)
                sys.exit(1)
            grouped(0, out_s)
            ctx.sync()
            chosen = "slices" if t.last_select_grouped()[0] else "column"
            dense = c >= 500_000
            res = {"slices": [], "column": [], "loop": [], "ungrouped": []}
            for r in range(ROUNDS):
                order = [("slices", from_slices, LAUNCHES), ("loop", loop, LAUNCHES), ("ungrouped", ungrouped, LAUNCHES),
                         ("column", from_column, 1 if dense else LAUNCHES)]
                for what, fn, k in order[r % 4:] + order[:r % 4]:
                    res[what].append(timed(fn, k))
            k_grouped = kernel_ms(from_slices, launches)
            k_ungrouped = kernel_ms(ungrouped, 1)
            # group leaves read per pass: one column, each leaf in its own batch once; two columns in one
            # launch, each column's leaves once
            assert len(by) == 1 or launches == 1
            leaves = G if len(by) == 1 else sum(len(t.aggregate_groups([g])) for g in by)
            grouped_bytes = (launches * select_bits + leaves * passes) * bv
            loop_bytes = G * (select_bits + len(by)) * bv
            rows = int(a.reshape(G, 6)[:, 5].sum())
            print(f"{name}; {lay_name} = {G} groups, {launches} batches of {passes} passes; filter keeps {sel_name} "
                  f"({rows} rows); path=None takes the {chosen}; the loop's calls take the slices in {loop_slices} of {G}",
                  flush=True)
            line("  grouped, from the slices", res["slices"], grouped_bytes)
            line("  grouped, from the column", res["column"])
            line(f"  loop of {G} selects", res["loop"], loop_bytes if loop_slices == G else None)
            line("  one ungrouped select", res["ungrouped"], select_bits * bv)
            apart = max(res["slices"]) < min(res["loop"])
            best = min(("slices", "column"), key=lambda w: min(res[w]))
            print(f"  loop / grouped = {min(res['loop']) / min(res['slices']):.2f} (byte ratio {loop_bytes / grouped_bytes:.2f}); "
                  f"the two sets {'do not overlap' if apart else 'OVERLAP'}; slices / column = "
                  f"{min(res['slices']) / min(res['column']):.2f}; path=None took the "
                  f"{'faster' if best == chosen else 'SLOWER'} path", flush=True)
            print(f"  grouped passes {k_grouped:.3f} ms = {grouped_bytes / k_grouped / 1e9:.2f} TB/s; ungrouped passes "
                  f"{k_ungrouped:.3f} ms = {select_bits * bv / k_ungrouped / 1e9:.2f} TB/s", flush=True)
        for o in (out_s, out_c, out_l, out_1):
            o.free()
t.close()
ctx.close()
