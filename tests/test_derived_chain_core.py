"""The chain keys of the derived-leaf policy (duckdb-cubit_amd/csrc/cubit_derived.hpp, HIP-free) run on the
CPU through tests/derived_chain_core.cpp: a stand-alone program built here with AddressSanitizer and UBSan
and run as a child process. A chain names the derivable literals of one AND chain that lie on two or more
columns; it is kept by the cache that keeps the column groups, under the same budget, and bought by cost.
The program ends with status 1 at the first failed check and prints it. No GPU."""
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("derived_chain_core") / "derived_chain_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "derived_chain_core.cpp"), "-o", str(exe)], check=True)
    return exe


def run(program, *args):
    r = subprocess.run([str(program), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_cost_rule(program):
    """uses_so_far * (k - 1) * B >= (k + 1) * B + F against the same inequality in 128 bits, over k = 0 … 9,
    four sizes of B, F from 0 to 2^64 - 1 and uses up to 2^64 - 1: F = 0 is derived_admit, F = 2^64 - 1
    never admits, and an admission stays one as the uses grow. Through the cache: k is what the request
    passes, not the key's literal count; the column groups keep the count rule whatever F is; a chain
    refused under "never" is admitted at once when the cost becomes 0."""
    assert "cost ok" in run(program, "cost")


def test_chain_keys(program):
    """Every order of the literals, of the unions and a literal or union met twice give one key; a
    complement flip, another pointer, a literal or a union more or less another; a union's leaves are not
    the chain's own literals; no chain key equals the key of the same literals on any column with either
    operator; one column alone, a bitvector both plain and complemented, or a "union" that is an AND group
    or a chain give none."""
    assert "keys ok" in run(program, "keys")


def test_shared_lru(program):
    """Groups and chains in one LRU under one budget: find moves either to the front and counts chain hits
    apart; an admission without room evicts nothing while the plan is open and the least recently used
    entry of either kind at the next begin_plan; a chain outlives the eviction of the group whose literals
    it holds; a smaller budget, 0 and clear take both kinds; both kinds share the 1,024 counters."""
    assert "lru ok" in run(program, "lru")


def test_random_traffic_of_both_kinds(program):
    """20 seeds of 4,000 plans over six groups and six chains with budget changes, cost changes ("never"
    among them) and invalidations: the bytes held never exceed the budget and equal the entries' sum, the
    chain count and the two hit counters add up, no entry leaves between begin_plan and end_plan, and every
    hit returns its own live payload (a freed one is an ASan error)."""
    assert "soak ok" in run(program, "soak")
