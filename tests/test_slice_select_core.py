"""The bit-sliced select's host side, without a GPU: the quantile_disc index rule, the bucket walk of
one radix step, a CPU model of the whole pass sequence and the path rule select_from_slices
(duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) through tests/slice_select_core.cpp, a stand-alone
program built here with AddressSanitizer and UBSan and run as a child process; the new entry points in
the header, the library and the Python signatures."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_table_select", "cubit_table_last_select", "cubit_bitslice_select", "cubit_table_top_n"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slice_select_core") / "slice_select_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "slice_select_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_index_rule_walk_pass_sequence_and_path_rule(program):
    """Index rule: against a literal restatement of the reference's formula for n = 0 … 2,000 and near
    2^33 and 2^47, q in {0, 1, 0.5, 1/3, 0.1, 0.9, …} and one ulp either side of j / n. Bucket walk:
    against brute force over expanded rows for d = 1 … 5, zero counts, one non-empty bucket, ranks 0,
    total - 1 and total (not found), both directions, counts past 2^32. Pass sequence: the chunked
    radix select as the kernels run it over random slice sets of 0 … 64 slices and up to 3,000 rows
    against std::nth_element, with NULLs, heavy ties, one value only, both directions and quantiles.
    Path rule: monotone in the estimated rows, forced either way by its flags, never the slices
    without an index."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"slice select ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    for name, value in [("RANK", "0"), ("RANK_DESC", "1"), ("QUANTILE", "2"), ("DESC_ROWS", "1u"),
                        ("FROM_SLICES", "16u"), ("FROM_COLUMN", "32u"), ("NO_ZONEMAP", "64u")]:
        assert re.search(r"^#define CUBIT_SELECT_%s +%s\b" % (name, value), header, flags=re.M), name
        assert getattr(L, "SELECT_" + name) == int(value.rstrip("u"))
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name


def test_null_arguments_return_a_status():
    lib = L.gpu_lib()
    v, n = C.c_int(), C.c_uint32()
    assert lib.cubit_table_select(None, None, 0, None, 0, L.SELECT_RANK, 0, 0.0, 0, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_last_select(None, C.byref(v), C.byref(n)) == L.ERR_INVALID
    assert lib.cubit_bitslice_select(None, None, 0, None, None, 0, L.TYPE_INT64, 0, L.SELECT_RANK, 0, 0.0,
                                     None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
    assert lib.cubit_table_top_n(None, None, 0, None, 0, 1, 0, None, 0, None, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
