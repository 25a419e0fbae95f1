"""The two costs of a chain's admission (duckdb-cubit_amd/csrc/cubit_derived.hpp, HIP-free) run on the CPU
through tests/derived_chain_pooled_core.cpp: a stand-alone program built here with AddressSanitizer and UBSan
and run as a child process. An admitting scan that allocates the chain's block pays kDerivedChainCost, one that
takes a block waiting in the table's pool pays kDerivedChainCostPooled, and request() is told which applies.
The program ends with status 1 at the first failed check and prints it. No GPU."""
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("derived_chain_pooled_core") / "derived_chain_pooled_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "derived_chain_pooled_core.cpp"), "-o", str(exe)], check=True)
    return exe


def run(program, *args):
    r = subprocess.run([str(program), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_pooled_selects_the_pooled_cost(program):
    """A fresh cache holds the two constants and each setter reaches the slot it names. `pooled` selects the
    pooled cost for chain keys only (the column groups keep the count rule), one counter serves both costs as
    `pooled` changes between requests, 2^64 - 1 in either slot never admits through that slot while the other
    still does, and set_chain_cost after set_chain_cost_pooled overrides it."""
    assert "select ok" in run(program, "select")


def test_three_arguments_and_set_chain_cost_as_before(program):
    """The key assertions of derived_chain_core's cost section through the new signature: a fresh cache asked
    with three arguments, or with pooled = false, buys SF100 Q6 on its 18th request; set_chain_cost(0) is the
    count rule on k, a cost of 20 B the 13th request and "never" never, whatever `pooled` says."""
    assert "compat ok" in run(program, "compat")


def test_committed_constants(program):
    """The admission request for (k = 3, B = 75,104,256) and (k = 3, B = 131,072) under either constant, derived
    from the constants by the 128-bit inequality: a 300,001-row table is not admitted within 60 requests from a
    pooled block, SF100 Q6 from a pooled block is admitted by its 8th request, and a fresh cache gives the same
    requests."""
    out = run(program, "constants")
    assert "constants ok" in out
    print(out)


def test_random_traffic_with_pooled_drawn_per_request(program):
    """20 seeds of 4,000 plans over six groups and six chains with budget changes, changes of either cost
    ("never" among them) and invalidations, `pooled` drawn at random per request: the bytes held never exceed
    the budget, no entry leaves during a plan, and no chain is admitted below the rule of the cost its request
    named (with pooled = false: the allocating rule), checked against a shadow count of each key's requests."""
    assert "soak ok" in run(program, "soak")
