"""The derived-leaf policy (duckdb-cubit_amd/csrc/cubit_derived.hpp, HIP-free) run on the CPU through
tests/derived_core.cpp: a stand-alone program built here with AddressSanitizer and UBSan and run as a
child process. The policy decides which leaf combinations a table keeps as one bitvector, when, and
which go when the budget is full; the device side (cubit_capi.hip) only follows it. The program ends
with status 1 at the first failed check and prints it. No GPU."""
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("derived_core") / "derived_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "derived_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def run(program, *args):
    r = subprocess.run([str(program), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_admission_threshold(program):
    """uses_so_far * (k - 1) >= k + 1 for k = 2 … 8, as a predicate and through the cache's counters: an
    interval (k = 2) is materialised by its fourth request, every larger group by its third; a group of
    one never; a budget of 0 or an entry larger than the budget admits and counts nothing."""
    assert "admission ok" in run(program, "admission")


def test_keys(program):
    """Every order of the same literals, and a literal met twice, give one key; a complement flip, another
    pointer, column or operator another; fewer than two distinct literals, or a bitvector both plain and
    complemented, none."""
    assert "keys ok" in run(program, "keys")


def test_lru_order_and_budget(program):
    """find makes an entry the most recently used; an admission without room evicts nothing while the plan
    is open (nor does set_budget then) and the least recently used entry at the next begin_plan; the
    waiting key is then admitted at once, the evicted one counts again from nothing; a smaller budget
    takes the cold end, 0 everything."""
    assert "lru ok" in run(program, "lru")


def test_counter_bound(program):
    """5,000 distinct keys never hold more than 1,024 counters; a key whose counter was cleared needs its
    full count again."""
    assert "counters ok" in run(program, "counters")


def test_random_traffic(program):
    """20 seeds of 4,000 plans over 12 keys of three sizes with budget changes and invalidations: the
    bytes held never exceed the budget and equal the entries' sum, no entry leaves between begin_plan
    and end_plan, and every hit returns its own live payload (a freed one is an ASan error)."""
    assert "soak ok" in run(program, "soak")
