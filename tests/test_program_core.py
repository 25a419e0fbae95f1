"""The filter-program compiler (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) run on the CPU through
tests/program_core.cpp: a stand-alone program built here with AddressSanitizer and UBSan and run as a
child process. The compiler decides what every eval kernel computes (leaf order, complement bits, packed
ops, CONJ / DNF / CNF form and group starts), so each emitted program is interpreted from the documented
encoding and held against the direct value of its tree. The program ends with status 1 at the first
failed check and prints it. No GPU."""
import subprocess

import pytest

from conftest import PKG, ROOT

N_TREES = 100_000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("program_core") / "program_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "program_core.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def run(program, *args):
    r = subprocess.run([str(program), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_random_and_directed_trees(program):
    """100,000 random trees (fixed seeds; constants, complemented leaves, ANDNOT, NOT above subtrees, up
    to 20 leaves) and the directed ones (a right-deep ANDNOT chain of 8: accepted, 8 deep, not for the
    kernels' four registers; a & ~b with b heavier and b a leaf; 9 leaves, and a DNF and a CNF of 9
    literals, refused; a single leaf plain and complemented). Per tree: ok exactly up to kMaxLeaves
    leaves; the nibbles, op count and one final value; the observed stack depth = max_depth; the postfix
    run and the run by eval_form's form both equal the tree; CONJ exactly for a conjunction of literals;
    fits = ok and depth <= 4. A single leaf is a conjunction of one: is_conjunction takes its program (no
    op), so eval_form gives it FORM_CONJ and it runs the K = 1 conjunction kernel, which the program
    pins. Every form must be reached by at least 1 % of the trees, and a quarter accepted."""
    out = run(program, "trees", str(N_TREES))
    w = out.splitlines()[-1].split()
    got = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert got["trees"] == N_TREES
    print(got)
    for form in ("postfix", "conj", "dnf", "cnf"):
        assert got[form] * 100 >= N_TREES, (form, got)
    assert got["accepted"] * 4 >= N_TREES, got
    assert got["postfix"] + got["conj"] + got["dnf"] + got["cnf"] == got["accepted"]
    assert got["deep"] > 0, got  # accepted programs the depth guard has to refuse were met


def test_algebra(program):
    """mk_not and mk_not twice evaluate to ~e and e; mk_bin with a constant on either side, all three
    ops, follows the truth table, and gives a constant node exactly when the value is constant."""
    assert "algebra ok" in run(program, "algebra")


def test_postfix_parser(program):
    """Random valid programs equal a direct stack evaluation; a leaf index past n_leaves, an underflow,
    more than one value left, an empty program and an opcode outside CUBIT_OP_* each have their own
    outcome. The programs are heap arrays of exact size."""
    assert "parser ok" in run(program, "parser")


def test_filter_tree_walk(program):
    """filter_subtree_end returns n_nodes for a well-formed prefix array and -1 for every proper
    truncation (heap arrays of exact size: a read past the end is seen); the node check refuses a kind
    or a cmp out of range."""
    assert "walk ok" in run(program, "walk")


def test_cmp_range(program):
    """cmp 0…5 and the between form over {INT64_MIN, INT64_MIN+1, -1, 0, 1, INT64_MAX-1, INT64_MAX}:
    membership (with neg) is the direct comparison, the intersection of two ranges their conjunction
    (!= is a complemented range, which no single range intersects into: pairs of the other six forms),
    clamp32 agrees inside INT32 and is empty when the range misses it."""
    assert "range ok" in run(program, "range")
