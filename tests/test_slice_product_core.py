"""The sliced sum(a * b)'s host side, without a GPU: slice_product_combine and the path rules
sum_product_from_slices / sum_product_grouped_from_slices (duckdb-cubit_amd/csrc/cubit_program.hpp,
HIP-free) through tests/slice_product_core.cpp, a stand-alone program built here with AddressSanitizer
and UBSan and run as a child process; the new entry points in the header, the library and the Python
signatures."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_bitslice_sum_product", "cubit_table_sum_product_grouped", "cubit_table_last_sum_product"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slice_product_core") / "slice_product_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "slice_product_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_combine_and_path_rules_against_brute_force(program):
    """Combine step: slice counts 0, 1, 7, 8, 9, 17, 63, 64 crossed, then random 0 … 64 per side; bases
    INT64_MIN, -1, 0 (where the range fits) and INT64_MAX - span on each side; no row, a count of 0,
    multiplicities up to 2^34, INT64_MIN · INT64_MIN with and without slices: the 128-bit result equals
    the sum of the sign-extended products modulo 2^128 and is symmetric in the operands. UBSan turns a
    signed overflow into a failure. Both path rules equal a direct count in whole eighths of a byte at
    every point tried, ties included (a tie goes to the slices, with b gathered, decoded and pinned);
    n_in = kProductInner is taken automatically and kProductInner + 1 only when forced; the grouped
    launches cover every pair of group leaves once."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"slice product ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 500_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    for name, value in [("FROM_SLICES", 16), ("FROM_COLUMN", 32)]:
        assert re.search(r"^#define CUBIT_SUM_%s %du\b" % (name, value), header, flags=re.M), name
        assert getattr(L, "SUM_" + name) == value
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name
    program_hpp = (PKG / "csrc" / "cubit_program.hpp").read_text()
    assert re.search(r"^constexpr uint32_t kProductInner = \d+;", program_hpp, flags=re.M)
    assert re.search(r"^constexpr uint32_t kProductGroupBatch = \d+;", program_hpp, flags=re.M)


def test_null_arguments_return_a_status():
    lib = L.gpu_lib()
    v, n = C.c_int(), C.c_uint32()
    assert lib.cubit_bitslice_sum_product(None, None, 0, None, 0, None, 0, None, 0, None, 0, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_sum_product_grouped(None, None, 0, None, 0, 1, None, 0, 0, None, 0) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_last_sum_product(None, C.byref(v), C.byref(n)) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
