"""The bit-sliced index's host side, without a GPU: sliced_interval (duckdb-cubit_amd/csrc/cubit_program.hpp,
HIP-free) against brute force through tests/sliced_core.cpp, a stand-alone program built here with
AddressSanitizer and UBSan and run as a child process; the new entry points in the header, the library
and the Python signatures; the shim core's `sliced` index item."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L
from test_shim_core import core_lib, split_spec

NEW = ["cubit_bitslice_build", "cubit_bitslice_compare", "cubit_table_use_sliced", "cubit_table_last_sliced"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sliced_core") / "sliced_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "sliced_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_sliced_interval_against_brute_force(program):
    """bits 0 … 6: every key of the range and every constant in [base - 3, base + 2^bits + 2] (and
    INT64_MIN / INT64_MAX), all six comparisons and the half-open interval form over every pair of
    constants, at bases 0, -17, 1000, around INT64_MIN and with the top at and just below INT64_MAX:
    membership equals the direct comparison, a miss is kFalse, a cover kAllValid, anything else an
    interval clamped to [0, 2^bits - 1]. bits 12, 31, 32, 33, 62, 63 and 64: the keys and constants at
    both ends of the range and of int64. UBSan turns a signed overflow into a failure."""
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"sliced ok (\d+) checks", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    assert re.search(r"^#define CUBIT_INDEX_SLICED 3\b", header, flags=re.M)
    assert L.INDEX_SLICED == 3
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name


def test_null_arguments_return_a_status():
    lib = L.gpu_lib()
    n = C.c_uint32()
    assert lib.cubit_table_use_sliced(None, 1) == L.ERR_INVALID
    assert lib.cubit_table_last_sliced(None, C.byref(n)) == L.ERR_INVALID
    assert lib.cubit_bitslice_build(None, None, 0, None, 0, 0, 0, None) == L.ERR_INVALID
    assert lib.cubit_bitslice_compare(None, None, 0, None, 0, 0, 0, 0, None) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()


def test_shim_core_parses_the_sliced_item():
    core = core_lib()
    assert split_spec(core, "a=sliced") == (0, [("a", L.INDEX_SLICED, [])], "")
    assert split_spec(core, " a = SLICED ;b=Sliced") == (0, [("a", L.INDEX_SLICED, []), ("b", L.INDEX_SLICED, [])], "")
    st, items, _ = split_spec(core, "l_shipdate=range~64;l_shipdate=sliced;l_discount=equality:1,2;l_tax=bins:0,4,8")
    assert st == 0 and items == [("l_shipdate", L.INDEX_RANGE, []), ("l_shipdate", L.INDEX_SLICED, []),
                                 ("l_discount", L.INDEX_EQUALITY, ["1", "2"]), ("l_tax", L.INDEX_BINS, ["0", "4", "8"])]
    # it takes no literal list and no count: reported as `a=equality~8` is
    want = split_spec(core, "x=range;a=equality~8")
    assert want[0] == 2 and want[1] == [("x", L.INDEX_RANGE, [])] and want[2] == "equality~8"
    assert split_spec(core, "x=range;a=sliced~8") == (2, [("x", L.INDEX_RANGE, [])], "sliced~8")
    assert split_spec(core, "x=range;a=sliced:1") == (2, [("x", L.INDEX_RANGE, [])], "sliced:1")
    assert split_spec(core, "a=sliced : 1,2 ")[0] == 2
