"""The row-list policy and the derived block pool (duckdb-cubit_amd/csrc/cubit_row_list.hpp, HIP-free) run
on the CPU through tests/row_list_core.cpp: a stand-alone program built here with AddressSanitizer and
UBSan and run as a child process. The policy decides which bitvectors also keep their set rows as
16-bit offsets, when the list is built, and when it goes; the pool keeps the blocks of dropped derived
bitvectors for the next admission. The device side (cubit_capi.hip, cubit_kernels.hip) only follows
them. The program ends with status 1 at the first failed check and prints it. No GPU."""
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L

NEW = ["cubit_table_use_row_lists", "cubit_table_row_list_stats", "cubit_table_derived_pool_stats",
       "cubit_ctx_last_decode_from_list"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("row_list_core") / "row_list_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "row_list_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def run(program, *args):
    r = subprocess.run([str(program), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_byte_rule_edges(program):
    """L = 2 q + 4 tiles <= B / 2: wanted at L = B / 2, not at L = B / 2 + 1 nor at the next q; an empty
    bitvector's list is its counts; SF100 Q6's kept chain (1.9 % dense) is wanted, a 3.1 % one is not."""
    assert "byte rule ok" in run(program, "rule")


def test_recurrence(program):
    """The first decode of a bitvector alone does nothing, the second builds when the rule holds and the
    room takes the list, later ones read; without room (budget 0 included) no list, and a later decode
    asks again."""
    assert "recurrence ok" in run(program, "recurrence")


def test_budget_room_and_drop_first(program):
    """Room is what the budget leaves beside bitvectors and lists; lists are shed oldest first when the
    bitvectors grow, a rebuilt list counts once, and beside the bitvector cache an eviction finds the
    lists gone before the bitvector goes."""
    assert "budget ok" in run(program, "budget")


def test_pool_reuse_bound_clear(program):
    """Blocks given back are handed out again without an allocation; the bound, another block size and a
    bound of 0 refuse or free them; clear frees all; 20,000 random operations leak and double-free nothing
    (ASan) and never hold more than the bound."""
    assert "pool ok" in run(program, "pool")


def test_offsets_round_trip(program):
    """Offsets 0, 65,535, 65,536 and 131,071 of one tile through off / lo_cnt and back, tiles all below or
    all above the half, and 50 random ascending sets."""
    assert "round trip ok" in run(program, "roundtrip")


def test_new_entry_points_are_declared_exported_and_bound():
    header = (ROOT / "include" / "cubit_gpu.h").read_text()
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in exported, name
        assert name in L.GPU_SIGNATURES, name
