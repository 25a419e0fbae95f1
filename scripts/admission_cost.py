#!/usr/bin/env python3
"""Per-scan host times of the first N identical scans of the bench's Q6 table (development tool): the
fixed cost of an admitting scan, F of derived_chain_admit, is read from them (DESIGN.md §3,
profiles/r13_admission_cost.txt, profiles/r15_admission_cost.txt, profiles/r19_admission_cost.txt).

Every scan is cubit_table_scan with the bench's arguments, timed on the host from a synchronised stream to
a synchronised stream, so each figure carries the same launch and synchronisation overhead beside its
kernels. Printed per scan: the plan (K, passes), cubit_table_derived_stats, cubit_table_derived_chain_stats,
the decode kernel, and where the library has them the block pool, the row lists and whether the decode read
a list.

--cycles N repeats, after that first ladder, N times: declare a column changed (every derived bitvector goes,
its block waits in the pool), then scan until the chain is kept again. Each cycle's admission takes a pooled
block. Printed per cycle: the request that admitted, that scan's time, the median of the plain scans (one pass)
of the same K before it in the cycle, and F = (admitting - plain - (k + 1) * B / rate) * rate, rate being
--byte-rate (the byte rate of the K = 3 scan's own mix, profiles/r12_q6_profile_before_after.txt). A pooled
cost that admits late (--chain-cost-pooled) leaves several plain scans before the admitting one.

usage: admission_cost.py [--sf 100] [--partition R/N] [--scans 24] [--chain-cost BYTES]
                         [--chain-cost-pooled BYTES] [--cycles N] [--byte-rate BYTES_PER_S]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT / "duckdb-cubit_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

MAX_CYCLE_SCANS = 64  # a cycle whose chain is not kept by then is reported as such


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--partition", default="0/1", help="R/N: partition R of the table split N ways by order range")
    ap.add_argument("--scans", type=int, default=24)
    ap.add_argument("--chain-cost", type=int, default=None, help="cubit_table_set_derived_chain_cost (default: the library's)")
    ap.add_argument("--chain-cost-pooled", type=int, default=None,
                    help="cubit_table_set_derived_chain_cost_pooled, after --chain-cost (default: the library's)")
    ap.add_argument("--cycles", type=int, default=0, help="pooled re-admissions after the first ladder")
    ap.add_argument("--byte-rate", type=float, default=5.97e12, help="bytes per second that turn time into F")
    ap.add_argument("--index", choices=["range+bins", "range"], default="range+bins")
    a = ap.parse_args()
    a.scaling, a.mvcc_sf, a.visible_updates = "strong", 300.0, False
    rank, world = (int(x) for x in a.partition.split("/"))

    import torch

    import bench
    from cubit_amd import _lib as L
    from cubit_amd import filters as F
    from cubit_amd.table import Context

    torch.cuda.set_device(0)
    ctx = Context(0)
    w = bench.make_q6(ctx, a, rank, world, False)
    t = w.table
    if a.chain_cost is not None:
        t.set_derived_chain_cost(a.chain_cost)
    if a.chain_cost_pooled is not None:
        t.set_derived_chain_cost_pooled(a.chain_cost_pooled)
    cap = w.n // 4 + 4096
    rowids = torch.empty(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    plan = F.serialize(w.filter_set, w.residual)
    nodes = F.to_ctypes(plan.nodes)

    def cost(x):
        return "default" if x is None else x

    print(f"# sf={a.sf:g} partition={a.partition} rows={w.n} index={a.index} chain_cost={cost(a.chain_cost)} "
          f"chain_cost_pooled={cost(a.chain_cost_pooled)}")

    def scan(label):
        """One timed scan: (µs, (K, passes), kept chains)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(ctx.lib.cubit_table_scan(t.handle, nodes, len(plan.nodes), None, rowids.data_ptr(), cap,
                                         count.data_ptr(), 0))
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6
        extra = ""
        if hasattr(t, "derived_pool_stats"):
            extra = f" pool={t.derived_pool_stats()} lists={t.row_list_stats()} from_list={int(ctx.last_decode_from_list())}"
        chains = t.derived_chain_stats()
        print(f"{label}: {us:9.1f} us  plan={t.last_plan()} derived={t.derived_stats()} "
              f"chains={chains} decode={ctx.last_decode_kernel()}{extra} q={int(count[0].item())}")
        return us, t.last_plan(), chains[0]

    for i in range(1, a.scans + 1):
        scan(f"scan {i:3d}")

    block = 0  # B: the bytes of one kept bitvector
    summary = []
    for c in range(1, a.cycles + 1):
        t.column_changed(1)
        print(f"== cycle {c}: column 1 declared changed, pool={t.derived_pool_stats()} derived={t.derived_stats()}")
        seen = []  # (µs, (K, passes)) of this cycle's scans
        admitted = None
        for i in range(1, MAX_CYCLE_SCANS + 1):
            us, p, chains = scan(f"cycle {c:2d} scan {i:3d}")
            if chains:
                admitted = i
                break
            seen.append((us, p))
        if admitted is None:
            print(f"cycle {c:2d}: no chain kept within {MAX_CYCLE_SCANS} scans")
            continue
        kept, held, _ = t.derived_stats()
        block = held // kept
        # the admitting scan read in the chain's place what the plain scans before it read: their K
        k = seen[-1][1][0] if seen else 0
        plain = [u for u, p in seen if p == (k, 1)]
        if not plain:
            print(f"cycle {c:2d}: admitted on request {admitted}: {us:.1f} us, no plain scan of K = {k} before it")
            continue
        med = statistics.median(plain)
        own_us = (k + 1) * block / a.byte_rate * 1e6
        f_bytes = (us - med - own_us) * 1e-6 * a.byte_rate
        summary.append((us, med, f_bytes))
        print(f"cycle {c:2d}: admitted on request {admitted}: {us:.1f} us; {len(plain)} plain K = {k} scans before it, "
              f"median {med:.1f} us; the bits-only pass's {(k + 1) * block} B = {own_us:.1f} us; F = {f_bytes / 1e9:.3f} GB")
    if summary:
        fs = sorted(s[2] for s in summary)
        adm, pl = statistics.median(s[0] for s in summary), statistics.median(s[1] for s in summary)
        print(f"# F from the two medians: {((adm - pl) * 1e-6 * a.byte_rate - (k + 1) * block) / 1e9:.3f} GB")
        print(f"# {len(summary)} pooled admissions: admitting scan median {statistics.median(s[0] for s in summary):.1f} us, "
              f"plain scan median {statistics.median(s[1] for s in summary):.1f} us, "
              f"F median {statistics.median(fs) / 1e9:.3f} GB, range {fs[0] / 1e9:.3f}-{fs[-1] / 1e9:.3f} GB (B = {block})")
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
