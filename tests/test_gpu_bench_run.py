"""A plain `bench.py` run end to end, at SF0.01: --steps sets the number of timed steps, the
line carries the headline alone (no --full leg), and --dump-outputs writes the last timed
step's count, row ids and tile counts — the oracle's rows for the same table."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(li001, tmp_path):
    from cubit_amd import filters as F
    from oracle import oracle as O

    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--sf", "0.01", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    cols = [O.Column(li001.l_shipdate), O.Column(li001.l_discount), O.Column(li001.l_quantity)]
    ref = O.table_scan(cols, F.serialize(F.q6_filter_set()), li001.n_rows)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "qualifying rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u64 bitvector words / int64 row ids"
    assert line["ms_per_step"] > 0
    assert line["config"]["rows_total"] == li001.n_rows
    assert line["config"]["qualifying_rows_total"] == len(ref)
    # value = qualifying rows of the timed steps over their span
    assert line["value"] == pytest.approx(len(ref) / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # what --full adds is not measured by a plain run
    for key in ("roofline", "cpu_baseline", "parity", "q6_aggregate", "typed_columns", "index_maintenance"):
        assert key not in line
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["count.npy", "row_ids.npy", "tile_counts.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["count.npy"].tolist() == [float(len(ref))]
    assert np.array_equal(got["row_ids.npy"].astype(np.int64), ref)
    assert got["tile_counts.npy"].sum() == len(ref)
