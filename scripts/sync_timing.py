"""Time cubit_table_sync_column at the bench's scale (612 M rows of INT64, a range index over 50
values) for 0.01 %, 0.1 %, 1 %, 10 % and 50 % of the rows changed: the host form (phases on stderr,
CUBIT_SYNC_TIMING: staging + H2D, diff, decode + gather, merge), the on-device form (the diff
kernel's rate against the 8 TB/s peak), and what a rebuild costs for the same change (a fresh
add_column + build_index on the new values). The last line names the largest fraction at which the
host sync is still faster than the rebuild: the shim's default (kDefaultSyncChangedFraction) is
that, rounded down to one significant digit."""
import os
import sys
import time

import numpy as np

os.environ["CUBIT_SYNC_TIMING"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "duckdb-cubit_amd"))
from cubit_amd import _lib as L  # noqa: E402
from cubit_amd.table import Context, CubitTable  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 612_000_000
rng = np.random.default_rng(5)
cur = (rng.integers(1, 51, n) * 100).astype(np.int64)
ctx = Context(0)
ctx.enable_timing(True)
tables = {}
for form in ("host", "device"):
    t = CubitTable(ctx, n)
    t.add_column(2, cur)
    t.build_index(2, L.INDEX_RANGE)
    tables[form] = t
# one small sync per table first: the context's decode scratch (tile directory, ordered-pass ids) is
# allocated on first use and kept, as it would be in a process that has scanned before
cur[0] += 100
for t in tables.values():
    assert t.sync_column(2, cur) == (1, True)
diff_bytes = n * 16 + n // 8  # old + new values read, the changed bitvector written (no validity here)
best = None
for frac in (0.0001, 0.001, 0.01, 0.1, 0.5):
    rows = rng.random(n) < frac
    new = cur.copy()
    new[rows] = np.where(cur[rows] == 5000, 100, cur[rows] + 100)  # every picked row changes, within the keys
    m = int(rows.sum())
    del rows
    print(f"--- {frac * 100:g} % of {n} rows changed ({m})", flush=True)
    sys.stderr.flush()
    t0 = time.perf_counter()
    got = tables["host"].sync_column(2, new)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert got == (m, True), got
    k_ms = ctx.last_kernel_ms()
    print(f"host form: {host_ms:.1f} ms in all; diff kernel {k_ms:.3f} ms = {diff_bytes / k_ms / 1e9:.3f} TB/s "
          f"({diff_bytes / k_ms / 1e9 / 8 * 100:.1f} % of 8 TB/s)", flush=True)
    d_new = ctx.upload(new)
    ctx.sync()
    t0 = time.perf_counter()
    got = tables["device"].sync_column(2, d_new)
    dev_ms = (time.perf_counter() - t0) * 1e3
    assert got == (m, True), got
    k_ms = ctx.last_kernel_ms()
    d_new.free()
    print(f"on-device form: {dev_ms:.1f} ms in all; diff kernel {k_ms:.3f} ms = {diff_bytes / k_ms / 1e9:.3f} TB/s "
          f"({diff_bytes / k_ms / 1e9 / 8 * 100:.1f} % of 8 TB/s)", flush=True)
    rebuilds = []
    for _ in range(2):  # the same rebuild twice: the faster one is what the sync has to beat
        t0 = time.perf_counter()
        u = CubitTable(ctx, n)
        u.add_column(2, new)
        u.build_index(2, L.INDEX_RANGE)
        ctx.sync()
        rebuilds.append((time.perf_counter() - t0) * 1e3)
        u.close()
    rebuild_ms = min(rebuilds)
    print(f"rebuild (add_column + build_index on the new values): {rebuilds[0]:.1f} and {rebuilds[1]:.1f} ms; "
          f"host sync / faster rebuild = {host_ms / rebuild_ms:.2f}", flush=True)
    if host_ms < rebuild_ms:
        best = frac
    cur = new
for form, t in tables.items():
    assert np.array_equal(t.download_column(2), cur), form
    t.close()
ctx.close()
print(f"largest measured fraction with the host sync below the rebuild: {best}")
