"""The grouped bit-sliced select's host side, without a GPU: a CPU model of the grouped pass sequence
and the path rule select_grouped_from_slices (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) through
tests/slice_select_grouped_core.cpp, a stand-alone program built here with AddressSanitizer and UBSan and
run as a child process; the new entry points in the header, the library and the Python signatures."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_table_select_grouped", "cubit_table_last_select_grouped", "cubit_bitslice_select_grouped"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slice_select_grouped_core") / "slice_select_grouped_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "slice_select_grouped_core.cpp"), "-o", str(exe)], check=True)
    return exe


def test_grouped_pass_sequence_and_path_rule(program):
    """Pass sequence: the grouped radix select as the kernels run it — one shared candidate set, a
    histogram and a select_step per group, narrowing by each group's own bucket, batches of groups —
    over random slice sets of 0 … 64 slices and up to 3,000 rows, 1 … 20 disjoint groups (some empty,
    one with a single value, rows in no group), NULLs, heavy ties, both directions, quantiles 0, 0.5
    and 1 and ranks found in some groups and past the end in others, against std::nth_element per
    group; the same result at every batch size 1 … 8. Path rule: select_from_slices with no group leaf
    and one launch, monotone in the estimated rows, forced either way by its flags, never the slices
    without an index, slice_bits a literal restatement of the formula over the batches."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"slice select grouped ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name
    assert "PAIRWISE DISJOINT" in header and "unspecified" in header


def test_null_arguments_return_a_status_and_the_abi_version_stays():
    lib = L.gpu_lib()
    v, n, m, p = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.cubit_table_select_grouped(None, None, 0, None, 0, None, 1, L.SELECT_RANK, 0, 0.0, 0, None,
                                          0) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_last_select_grouped(None, C.byref(v), C.byref(n), C.byref(m), C.byref(p)) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_bitslice_select_grouped(None, None, 0, None, None, None, 1, 0, L.TYPE_INT64, 0, L.SELECT_RANK, 0,
                                             0.0, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_abi_version() == 1
