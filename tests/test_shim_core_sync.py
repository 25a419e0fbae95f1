"""The shim's update-sync decision (cubit_shim::PlanUpdateSync, shim/cubit_shim_core.hpp) through
its C test surface (csc_plan_update_sync, lib/libcubit_shim_core.so): after a committed UPDATE of an
attached column the partitions are synced in place (cubit_table_sync_column) unless row ids shrank,
a dictionary column gained a string, or there are no rows; each partition gets max_changed =
floor(fraction x its rows), never above its rows. No GPU, no DuckDB."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from conftest import PKG

RG = 122_880


@pytest.fixture(scope="module")
def core():
    subprocess.run(["make", "-s", "-C", str(PKG), "lib/libcubit_shim_core.so"], check=True)
    lib = C.CDLL(str(PKG / "lib" / "libcubit_shim_core.so"))
    lib.csc_plan_update_sync.restype = C.c_int
    lib.csc_plan_update_sync.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_uint64,
                                         C.c_void_p]
    lib.csc_default_sync_fraction.restype = C.c_double
    lib.csc_default_sync_fraction.argtypes = []
    lib.csc_split_rows.restype = C.c_uint64
    lib.csc_split_rows.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    return lib


def plan(core, gpu_rows, snap_rows, shrank=False, new_string=False, fraction=0.1, parts=None):
    """(in place?, max_changed per partition); the output array is pre-set to a sentinel, so a
    refusal that writes nothing is seen."""
    parts = np.asarray([gpu_rows] if parts is None else parts, dtype=np.uint64)
    out = np.full(len(parts), 2 ** 64 - 1, dtype=np.uint64)
    ok = core.csc_plan_update_sync(gpu_rows, snap_rows, int(shrank), int(new_string), fraction, parts.ctypes.data,
                                   len(parts), out.ctypes.data)
    return bool(ok), out.tolist()


def test_plain_update_runs_in_place(core):
    assert plan(core, 1000, 1000, fraction=0.1) == (True, [100])
    assert plan(core, 1000, 1500, fraction=0.1) == (True, [100])  # rows past the partition are appended


def test_shrunk_row_ids_rebuild(core):
    ok, out = plan(core, 1000, 1000, shrank=True)
    assert not ok and out == [2 ** 64 - 1]
    assert not plan(core, 1000, 999)[0]  # a snapshot that does not cover the partition


def test_missing_dictionary_string_rebuilds(core):
    ok, out = plan(core, 1000, 1000, new_string=True)
    assert not ok and out == [2 ** 64 - 1]


def test_zero_rows_rebuild(core):
    assert not plan(core, 0, 0)[0]
    assert not plan(core, 0, 500)[0]


def test_fraction_zero_and_one(core):
    assert plan(core, 1000, 1000, fraction=0.0) == (True, [0])  # applies only when nothing changed
    assert plan(core, 1000, 1000, fraction=1.0) == (True, [1000])
    assert plan(core, 1000, 1000, fraction=7.5) == (True, [1000])  # never above the rows
    assert plan(core, 1000, 1000, fraction=-0.5) == (True, [0])
    assert plan(core, 1000, 1000, fraction=math.nan) == (True, [0])
    assert plan(core, 3, 3, fraction=0.5) == (True, [1])  # the floor
    assert plan(core, 2 ** 40 + 1, 2 ** 40 + 1, fraction=1.0) == (True, [2 ** 40 + 1])


def test_three_way_split_gets_each_partitions_share(core):
    rows = 10 * RG + 5
    bounds = np.zeros(4, dtype=np.uint64)
    assert core.csc_split_rows(rows, 3, bounds.ctypes.data) == 3
    parts = np.diff(bounds.astype(np.int64))
    assert parts.sum() == rows and len(set(parts.tolist())) > 1  # uneven: each gets its own bound
    for fraction in (0.01, 0.1, 0.25):
        ok, out = plan(core, rows, rows, fraction=fraction, parts=parts)
        assert ok
        for m, p in zip(out, parts.tolist()):
            assert m <= p and m <= fraction * p < m + 1, (fraction, p, m)
        assert sum(out) <= fraction * rows


def test_default_fraction_is_a_fraction(core):
    f = core.csc_default_sync_fraction()
    assert 0.0 < f <= 1.0
