#!/usr/bin/env python3
"""Per-scan host times of the first N identical scans of the bench's Q6 table (development tool): the
fixed cost of an admitting scan, F of derived_chain_admit, is read from them (DESIGN.md §3,
profiles/r13_admission_cost.txt, profiles/r15_admission_cost.txt).

Every scan is cubit_table_scan with the bench's arguments, timed on the host from a synchronised stream to
a synchronised stream, so each figure carries the same launch and synchronisation overhead beside its
kernels. Printed per scan: the plan (K, passes), cubit_table_derived_stats, cubit_table_derived_chain_stats,
the decode kernel, and where the library has them the block pool, the row lists and whether the decode read
a list.

usage: admission_cost.py [--sf 100] [--scans 24] [--chain-cost BYTES]"""
import argparse
import ctypes
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT / "duckdb-cubit_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--chain-cost", type=int, default=None, help="cubit_table_set_derived_chain_cost (default: the library's)")
    ap.add_argument("--index", choices=["range+bins", "range"], default="range+bins")
    a = ap.parse_args()
    a.scaling, a.mvcc_sf, a.visible_updates = "strong", 300.0, False

    import torch

    import bench
    from cubit_amd import _lib as L
    from cubit_amd import filters as F
    from cubit_amd.table import Context

    torch.cuda.set_device(0)
    ctx = Context(0)
    w = bench.make_q6(ctx, a, 0, 1, False)
    t = w.table
    if a.chain_cost is not None:
        t.set_derived_chain_cost(a.chain_cost)
    cap = w.n // 4 + 4096
    rowids = torch.empty(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    plan = F.serialize(w.filter_set, w.residual)
    nodes = F.to_ctypes(plan.nodes)
    print(f"# sf={a.sf:g} rows={w.n} index={a.index} chain_cost={'default' if a.chain_cost is None else a.chain_cost}")
    for i in range(1, a.scans + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(ctx.lib.cubit_table_scan(t.handle, nodes, len(plan.nodes), None, rowids.data_ptr(), cap,
                                         count.data_ptr(), 0))
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6
        extra = ""
        if hasattr(t, "derived_pool_stats"):
            extra = f" pool={t.derived_pool_stats()} lists={t.row_list_stats()} from_list={int(ctx.last_decode_from_list())}"
        print(f"scan {i:3d}: {us:9.1f} us  plan={t.last_plan()} derived={t.derived_stats()} "
              f"chains={t.derived_chain_stats()} decode={ctx.last_decode_kernel()}{extra} q={int(count[0].item())}")
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
