"""The grouped aggregate's host side, without a GPU: slot enumeration, group numbering, the split
into the kernel's batches, the path rule grouped_from_slices and the per-group combine
(duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) through tests/group_agg_core.cpp, a stand-alone
program built here with AddressSanitizer and UBSan and run as a child process; the new entry points in
the header, the library and the Python signatures."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_table_aggregate_groups", "cubit_table_aggregate_grouped", "cubit_table_last_grouped"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("group_agg_core") / "group_agg_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "group_agg_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_slots_batches_path_rule_and_combine(program):
    """Slots: keys with and without update values, duplicates between the two, the NULL slot present
    and absent, against a std::set; the numbering g = i1 * n2 + i2 and back; the 256-group limit on
    both sides with one and two columns. Batches: for 0 ... 40 x 0 ... 20 leaves and both batch sizes
    every pair of leaves lies in exactly one batch and no batch exceeds the kernel's rectangle; Q1's
    3 x 2 is one launch. Path rule: monotone in the estimated rows and in the group count, forced
    either way, never the slices without a usable index, and aggregate_from_slices itself when there
    is no group leaf. Combine: random rows in 1 ... 33 groups over slice_agg_core.cpp's bases and
    widths against __int128 sums and the extreme keys."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"group agg ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    for name, value in [("MAX_GROUP_COLS", 2), ("MAX_GROUPS", 256)]:
        assert re.search(r"^#define CUBIT_AGG_%s %d\b" % (name, value), header, flags=re.M), name
        assert getattr(L, "AGG_" + name) == value
    assert L.gpu_lib().cubit_abi_version() == 1
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name


def test_null_arguments_return_a_status():
    lib = L.gpu_lib()
    n = C.c_uint32()
    cols = (C.c_int * 1)(0)
    assert lib.cubit_table_aggregate_groups(None, cols, 1, None, None, 0, C.byref(n)) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_aggregate_grouped(None, None, 0, None, 0, cols, 1, L.AGG_SUM, None, 0) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_last_grouped(None, None, None, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
