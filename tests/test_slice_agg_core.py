"""The bit-sliced aggregate's host side, without a GPU: slice_agg_combine and the path rule
aggregate_from_slices (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) through tests/slice_agg_core.cpp,
a stand-alone program built here with AddressSanitizer and UBSan and run as a child process; the new
entry points in the header, the library and the Python signatures."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_table_aggregate", "cubit_table_last_aggregate", "cubit_bitslice_aggregate"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slice_agg_core") / "slice_agg_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "slice_agg_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_combine_and_path_rule_against_brute_force(program):
    """Combine step: bits 0, 1, 12, 31, 32, 33, 63, 64; bases 0, -17, INT64_MIN (+1, +5) and the one
    that puts the top of the range at INT64_MAX; INT64, INT32, dictionary codes and UINT64 (every value
    2^64 - 1; the full unsigned range); multiplicities 0, 1 and 2^33 at both ends and the middle of
    the range, and random groups: the 128-bit sum equals the __int128 sum of the values, min / max the
    extreme keys in column_statistics' form, unasked slots 0, and the per-slice-count form equals the
    weighted-sum form the kernel calls. UBSan turns a signed overflow into a failure. Path rule:
    monotone in the estimated rows, forced either way by its flags, never the slices without an index."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"slice agg ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 20_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    for name, value in [("SUM", 1), ("MIN", 2), ("MAX", 4), ("FROM_SLICES", 16), ("FROM_COLUMN", 32),
                        ("NO_ZONEMAP", 64)]:
        assert re.search(r"^#define CUBIT_AGG_%s %du\b" % (name, value), header, flags=re.M), name
        assert getattr(L, "AGG_" + name) == value
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name


def test_null_arguments_return_a_status():
    lib = L.gpu_lib()
    v = C.c_int()
    assert lib.cubit_table_aggregate(None, None, 0, None, 0, L.AGG_SUM, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_last_aggregate(None, C.byref(v)) == L.ERR_INVALID
    assert lib.cubit_bitslice_aggregate(None, None, 0, None, None, 0, L.TYPE_INT64, 0, L.AGG_SUM, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
