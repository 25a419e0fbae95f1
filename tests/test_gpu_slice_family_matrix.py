"""Every (leaf count, program form) cell the table API can produce, through every variant of the three
slice-answered kernels — eval_slice_aggregate <SUM, MINMAX>, eval_slice_aggregate_grouped <TWO, MINMAX>
and eval_slice_select — against exact integers. dispatch_k0_form compiles each of them per leaf count
and form; this is the device-side counterpart of tests/program_core.cpp, which pins the compiler alone.

A cell is a filter tree of K single-leaf literals on K different columns whose program has one form:
CONJ(1 … 8), DNF(2 … 8), CNF(3 … 8), POSTFIX(4 … 8) — 26 cells — and POSTFIX(3), which only a literal of
three leaves reaches (tree()). After every call on the slices path last_plan() and last_form() must
name the cell, so a green run proves which instantiation executed. Expected values are reductions in
Python integers / numpy over the rows the oracle returns (O.table_scan, O.fetch), through the helpers
of the three table test modules. The inputs are checked on the reference alone first: no cell may pass
by being trivial (see `reference`).

The literals: D_i ("dense") is f_i <= 6 on an even column and f_i != 3 on an odd one (a complemented
leaf), S_i ("sparse") is f_i <= 1 / f_i = 3. Even columns carry a RANGE index over every value, odd
ones an every-value EQUALITY index, and none is nullable, so each literal is exactly one index
bitvector. The middle zone of f0 holds 7 … 9 only and that of f1 never 3: D_0, S_0 and S_1 are false on
all of it, so every CONJ cell (D_0 & …) and every CNF cell ((D_0 | S_1) & …) is dead there and the
zonemap's live list is {0, 2} — a gap, and the ragged last tile on the list. (With 3 in f1's middle
zone no CNF cell would have a dead zone: S_1 keeps D_0 | S_1 alive there.)

The DNF cells are (D_0 & S_1) | (D_2 & S_3) | …, an odd K ending in the lone S_{K-1}, and the CNF cells
their duals ending in D_{K-1}. At K = 2 that recipe is the single conjunction D_0 & S_1, a CONJ program;
DNF(2) is D_0 | S_1, the only two-leaf shape the emitter makes DNF. The POSTFIX cells wrap
S_0 | (D_1 & (S_2 | S_3)) alternately as D_4 & (…), S_5 | (…), D_6 & (…), S_7 | (…)"""
import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_gpu_group_aggregate import check_groups, int_column
from test_gpu_table_aggregate import check_paths
from test_gpu_table_select import check_select, oracle_keys, want

pytestmark = pytest.mark.gpu

ZONE = 131_072
N = 2 * ZONE + 4_001  # two whole tiles and a ragged tail
TXN_START = 4611686018427388000
NF = 8
SEED = 71
V, G1, G2, H = NF, NF + 1, NF + 2, NF + 3  # the value column, the group columns and h, behind f0 … f7
CONJ, DNF, CNF, POSTFIX = L.FORM_CONJ, L.FORM_DNF, L.FORM_CNF, L.FORM_POSTFIX
NAMES = {CONJ: "conj", DNF: "dnf", CNF: "cnf", POSTFIX: "postfix"}
CELLS = ([(CONJ, k) for k in range(1, 9)] + [(DNF, k) for k in range(2, 9)] + [(CNF, k) for k in range(3, 9)]
         + [(POSTFIX, k) for k in range(3, 9)])
assert len(CELLS) == 26 + 1  # (POSTFIX, 3) is no tree of single-leaf literals: see tree()
INVERSE = {"<=": ">", ">": "<=", "!=": "=", "=": "!=", ">=": "<", "<": ">="}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ literals and trees


def literal(kind, i, flip=False):
    op, c = {("D", 0): ("<=", 6), ("D", 1): ("!=", 3), ("S", 0): ("<=", 1), ("S", 1): ("=", 3)}[(kind, i & 1)]
    return F.Cmp(i, INVERSE[op] if flip else op, c)


def tree(form, k, flip=None):
    """The cell's residual tree over the columns 0 … k-1; flip: the one literal to complement.
    (POSTFIX, 3) is the one cell no tree of single-leaf literals reaches: the single literal h >= 2 on a
    nullable column with an every-value EQUALITY index over 0 … 9, which the planner answers with the
    fewer bitvectors, valid(h) AND NOT (h = 0 OR h = 1) — an AND NOT of an OR, three leaves, postfix."""
    if (form, k) == (POSTFIX, 3):
        return F.Cmp(H, "<" if flip == 0 else ">=", 2)

    def d(i):
        return literal("D", i, flip == i)

    def s(i):
        return literal("S", i, flip == i)

    if form == CONJ:
        return d(0) if k == 1 else F.And(*[d(i) for i in range(k)])
    if form in (DNF, CNF):
        inner, outer, last = (F.And, F.Or, s) if form == DNF else (F.Or, F.And, d)
        if k == 2:
            return outer(d(0), s(1))
        groups = [inner(d(i), s(i + 1)) for i in range(0, k - 1, 2)] + ([last(k - 1)] if k & 1 else [])
        return outer(*groups)
    e = F.Or(s(0), F.And(d(1), F.Or(s(2), s(3))))  # neither a conjunction, nor an OR of them, nor an AND of ORs
    for i in range(4, k):
        e = F.Or(s(i), e) if i & 1 else F.And(d(i), e)
    return e


def negated(e):
    """NOT e with the complement pushed to the literals (De Morgan): the same leaves, every complement
    bit the other way, ANDs and ORs exchanged."""
    if isinstance(e, F.Cmp):
        return F.Cmp(e.column, INVERSE[e.comparison], e.constant)
    kids = [negated(c) for c in e.children]
    return F.Or(*kids) if isinstance(e, F.And) else F.And(*kids)


def negated_cell(form, k):
    """The cell negated(tree(form, k)) runs in: an OR of K literals is a DNF of one-literal groups, the
    dual of a DNF is a CNF and the reverse, a postfix tree stays one."""
    if form == CONJ:
        return (CONJ, 1) if k == 1 else (DNF, k)
    if form == DNF:
        return (CONJ, 2) if k == 2 else (CNF, k)
    return (DNF, k) if form == CNF else (POSTFIX, k)


def literal_columns(rng, n, dead_zone):
    """f0 … f7: INT32 over 0 … 9, not nullable; with dead_zone, rows ZONE … 2*ZONE-1 of f0 hold 7 … 9
    and those of f1 no 3."""
    fs = [rng.integers(0, 10, n).astype(np.int32) for _ in range(NF)]
    if dead_zone:
        fs[0][ZONE:2 * ZONE] = rng.integers(7, 10, ZONE)
        fs[1][ZONE:2 * ZONE] = rng.choice(np.array([0, 1, 2, 4, 5, 6, 7, 8, 9], dtype=np.int32), ZONE)
    return fs


class Data:
    """The host arrays of a table and the oracle's columns over them."""

    def __init__(self, n, seed, n_literal_cols, dead_zone, deletes=False):
        rng = np.random.default_rng(seed)
        self.n = n
        fs = literal_columns(rng, n, dead_zone)
        if not dead_zone:
            if n >= 63:  # small tables: every value in every column, so no literal folds away
                for i, f in enumerate(fs):
                    f[:10] = np.roll(np.arange(10), i)
            for f in fs:
                f[-1] = 0  # the last row qualifies under CONJ and POSTFIX
        v, vv = int_column(rng, n, np.int64, -5_000_000_000, 5_000_000_123)  # 34 slices
        self.g1 = rng.integers(0, 3, n).astype(np.int32)
        self.g2 = rng.integers(0, 2, n).astype(np.int32)
        self.g2v = rng.random(n) >= 0.1
        self.h = rng.integers(0, 10, n).astype(np.int32)
        self.hv = rng.random(n) >= 0.1
        self.cols = {i: (fs[i], None, L.INDEX_RANGE if i % 2 == 0 else L.INDEX_EQUALITY) for i in range(n_literal_cols)}
        self.cols[V] = (v, validity_from_mask(vv), L.INDEX_SLICED)
        self.cols[G1] = (self.g1, None, L.INDEX_EQUALITY)
        self.cols[G2] = (self.g2, validity_from_mask(self.g2v), L.INDEX_EQUALITY)
        self.cols[H] = (self.h, validity_from_mask(self.hv), L.INDEX_EQUALITY)
        self.ocols = [O.Column(np.zeros(n, np.int32))] * (H + 1)  # (unregistered ids: never read)
        for c, (data, vw, _) in self.cols.items():
            self.ocols[c] = O.Column(data, vw)
        self.dels = self.deleted = None
        if deletes:  # every 7th row, deleted at version 5
            self.dels = np.arange(0, n, 7, dtype=np.int64)
            self.deleted = np.full(n, np.uint64(2 ** 64 - 2), dtype=np.uint64)
            self.deleted[self.dels] = 5

    def reader(self):
        return L.Txn(10, TXN_START + 1), O.Mvcc(10, TXN_START + 1, deleted=self.deleted)

    def ids(self, residual, tx=None):
        return O.table_scan(self.ocols, F.serialize(None, residual), self.n, 0, tx)

    def upload(self, ctx):
        self.t = t = CubitTable(ctx, self.n)
        for c, (data, vw, enc) in self.cols.items():
            t.add_column(c, data, vw)
            t.build_index(c, enc)
        t.set_derived_budget(0)
        t.set_derived_chain_cost(2 ** 64 - 1)  # a repeated filter stays its K leaves
        if self.dels is not None:  # seen by a transaction only: the plain cells run without one
            t.set_deletes(self.dels, np.full(len(self.dels), 5, dtype=np.uint64))
        return self

    def close(self):
        self.t.close()


@pytest.fixture(scope="module")
def main(ctx):
    tab = Data(N, SEED, NF, dead_zone=True, deletes=True).upload(ctx)
    yield tab
    tab.close()


def not_trivial(tab, residual, what):
    ids = tab.ids(residual)
    assert 0.01 * tab.n <= len(ids) <= 0.99 * tab.n, (what, len(ids))
    assert (ids >= 2 * ZONE).any(), what
    slots = {(int(a), int(b) if ok else None) for a, b, ok in zip(tab.g1[ids], tab.g2[ids], tab.g2v[ids])}
    assert len(slots) == 9, (what, slots)
    return ids


def reference(tab, form, k):
    """The oracle's rows of the cell, after the conditions that keep it from passing trivially: 1 … 99 %
    of the rows qualify, rows of the ragged tail among them, all 9 group slots occur, and complementing
    any one literal changes the row set (no leaf, complement bit or group-start bit is idle). Also
    returns whether the middle zone is dead — it has to be for every CONJ and CNF cell."""
    ids = not_trivial(tab, tree(form, k), (form, k))
    if (form, k) == (POSTFIX, 3):  # one literal of three leaves: each leaf decides rows of the ragged tail
        tail_h, tail_hv = tab.h[2 * ZONE:], tab.hv[2 * ZONE:]
        assert (~tail_hv).any() and (tail_hv & (tail_h == 0)).any() and (tail_hv & (tail_h == 1)).any()
    for i in range(1 if (form, k) == (POSTFIX, 3) else k):
        assert not np.array_equal(tab.ids(tree(form, k, flip=i)), ids), (form, k, i)
    dead_zone = not ((ids >= ZONE) & (ids < 2 * ZONE)).any()
    assert dead_zone == (form in (CONJ, CNF) or (form, k) == (DNF, 2)), (form, k)
    return ids, dead_zone


class Ran:
    """The after-call checks: on the slices path the plan and the form name the cell; with the zonemap
    on, a cell without a row in the middle zone (dead_zone: every CONJ and CNF cell, and DNF(2), whose
    two literals are both false there) evaluates the zones {0, 2} of 3, and every other call all three."""

    def __init__(self, t, form, k, dead_zone, passes=1, exact=True):
        self.t, self.form, self.k, self.passes, self.exact, self.dead_zone = t, form, k, passes, exact, dead_zone
        self.slices_calls = 0

    def __call__(self, path, zonemap=True):
        t = self.t
        if path == "slices":
            self.slices_calls += 1
            if self.exact:
                assert t.last_plan() == (self.k, self.passes), (t.last_plan(), self.k, self.passes)
                assert t.last_form() == self.form, (t.last_form(), self.form)
            else:
                assert t.last_plan()[1] == self.passes, t.last_plan()
        assert t.last_zones() == ((2, 3) if zonemap and self.dead_zone else (3, 3)), (path, zonemap, t.last_zones())

    def zm(self, zonemap):
        return lambda path, z=None: self(path, zonemap)


# ------------------------------------------------------------------ the matrix


@pytest.mark.parametrize("form,k", CELLS, ids=[f"{NAMES[f]}{k}" for f, k in CELLS])
def test_cell_through_every_kernel_variant(main, form, k):
    tab, t = main, main.t
    residual = tree(form, k)
    ids, dead_zone = reference(tab, form, k)
    s, rows = oracle_keys(tab.ocols, V, None, residual, N)
    assert rows == len(ids)
    ran = Ran(t, form, k, dead_zone)
    for zm in (True, False):
        after = ran.zm(zm)
        assert np.array_equal(t.scan(None, residual, zonemap=zm), ids)
        assert t.count(None, residual, zonemap=zm) == len(ids)
        # the three <SUM, MINMAX> bodies of eval_slice_aggregate, then scan + probe + reduce
        for ops in (L.AGG_SUM, L.AGG_MIN | L.AGG_MAX, L.AGG_ALL):
            check_paths(t, tab.ocols, V, L.TYPE_INT64, N, None, residual, ops=ops, zonemap=zm, paths=["slices"],
                        what=(form, k, ops), after=after)
        check_paths(t, tab.ocols, V, L.TYPE_INT64, N, None, residual, ops=L.AGG_ALL, zonemap=zm, paths=["column"],
                    what=(form, k), after=after)
        # the four <TWO, MINMAX> bodies of eval_slice_aggregate_grouped
        for by in ([G1], [G1, G2]):
            for ops in (L.AGG_SUM, L.AGG_ALL):
                check_groups(t, tab.ocols, V, L.TYPE_INT64, by, N, None, residual, ops=ops, zonemap=zm,
                             paths=["slices"], what=(form, k, by, ops), after=after)
            check_groups(t, tab.ocols, V, L.TYPE_INT64, by, N, None, residual, ops=L.AGG_ALL, zonemap=zm,
                         paths=["column"], what=(form, k, by), after=after)
    # eval_slice_select and its narrow and step kernels: nine passes over the 34 slices
    check_select(t, s, rows, V, None, residual, what=(form, k), after=ran)
    assert ran.slices_calls == 2 * (3 + 4 + 17)


NEGATED = [c for c in CELLS if c != (POSTFIX, 3)]  # (NOT h >= 2 is two plain leaves, and drops the NULLs too)


@pytest.mark.parametrize("form,k", NEGATED, ids=[f"{NAMES[f]}{k}" for f, k in NEGATED])
def test_negated_cell_complements_every_leaf_the_other_way(main, form, k):
    """The DNF and CNF cells above hold no complemented leaf and the others few. NOT tree, with the
    complement pushed to the literals, reads the same K bitvectors with every complement bit the other
    way, in the dual form: between the two tests every leaf position of every form runs plain and
    complemented, and the OR of K literals opens a group at every leaf. It keeps the rows the cell drops,
    so it is as far from trivial. The slices path's eight kernel variants, zonemap on."""
    tab, t = main, main.t
    residual = negated(tree(form, k))
    ids = not_trivial(tab, residual, ("not", form, k))
    assert len(ids) == N - len(tab.ids(tree(form, k)))
    dead_zone = not ((ids >= ZONE) & (ids < 2 * ZONE)).any()
    ran = Ran(t, *negated_cell(form, k), dead_zone)
    assert np.array_equal(t.scan(None, residual), ids)
    for ops in (L.AGG_SUM, L.AGG_MIN | L.AGG_MAX, L.AGG_ALL):
        check_paths(t, tab.ocols, V, L.TYPE_INT64, N, None, residual, ops=ops, paths=["slices"],
                    what=("not", form, k, ops), after=ran)
    for by in ([G1], [G1, G2]):
        for ops in (L.AGG_SUM, L.AGG_ALL):
            check_groups(t, tab.ocols, V, L.TYPE_INT64, by, N, None, residual, ops=ops, paths=["slices"],
                         what=("not", form, k, by, ops), after=ran)
    s, rows = oracle_keys(tab.ocols, V, None, residual, N)
    check_select(t, s, rows, V, None, residual, paths=["slices"], zonemaps=(True,), ranks=[0, len(s) // 2, len(s) - 1, len(s)],
                 quantiles=[0.5], what=("not", form, k), after=ran)
    assert ran.slices_calls == 3 + 4 + 9


MVCC_CELLS = [(form, k) for k in (7, 8) for form in (CONJ, DNF, CNF, POSTFIX)]
# the visibility bitvector is AND-ed on as one more leaf: a conjunction and an AND of ORs stay what they
# are; an OR of conjunctions under an AND is neither, and runs the postfix program
MVCC_FORM = {CONJ: CONJ, DNF: POSTFIX, CNF: CNF, POSTFIX: POSTFIX}


@pytest.mark.parametrize("form,k", MVCC_CELLS, ids=[f"{NAMES[f]}{k}" for f, k in MVCC_CELLS])
def test_cell_under_a_reader_that_sees_deletes(main, form, k):
    """Every 7th row deleted at version 5, read at start time 10. Seven leaves and the visibility leaf are
    one pass of eight; eight and the visibility leaf do not fit one pass, so a part is materialised first."""
    tab, t = main, main.t
    residual = tree(form, k)
    all_ids, dead_zone = reference(tab, form, k)
    txn, tx = tab.reader()
    ids = tab.ids(residual, tx)
    assert 0 < len(ids) < len(all_ids) and not (ids % 7 == 0).any()
    ran = Ran(t, MVCC_FORM[form], 8, dead_zone) if k == 7 else Ran(t, None, None, dead_zone, passes=2, exact=False)
    assert np.array_equal(t.scan(None, residual, txn=txn), ids)
    check_paths(t, tab.ocols, V, L.TYPE_INT64, N, None, residual, txn=txn, tx=tx, ops=L.AGG_ALL,
                paths=["slices", "column"], what=(form, k), after=ran)
    s, rows = oracle_keys(tab.ocols, V, None, residual, N, tx)
    assert rows == len(ids)
    check_select(t, s, rows, V, None, residual, txn=txn, zonemaps=(True,), quantiles=[0.5], what=(form, k), after=ran)
    check_groups(t, tab.ocols, V, L.TYPE_INT64, [G1], N, None, residual, txn=txn, tx=tx, ops=L.AGG_ALL,
                 paths=["slices", "column"], what=(form, k), after=ran)
    assert ran.slices_calls == 1 + 13 + 1
    print(f"last plan {t.last_plan()} form {t.last_form()}")


# ------------------------------------------------------------------ the same forms where tails go wrong

SMALL_CELLS = [(CONJ, 3), (DNF, 3), (CNF, 3), (POSTFIX, 4)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, ZONE - 1, ZONE, ZONE + 1])
def test_forms_at_partition_sizes_around_a_word_and_a_tile(ctx, n):
    """A complemented leaf's padding bits past n are ones: a tail mask that lets them through shows in
    count_rows first. CONJ(3) and POSTFIX(4) hold one such leaf (f1 != 3), DNF(3) and CNF(3) none, so
    each tree runs negated as well (negated(): every complement bit the other way, the dual form), where
    all or all but one of the leaves are complemented. The last row's literal columns are 0, so it
    qualifies under CONJ and POSTFIX. From 63 rows on every column holds every value, so no literal
    folds away and the plan names the cell; a single row folds them all."""
    tab = Data(n, 700 + n % 1000, 4, dead_zone=False).upload(ctx)
    t = tab.t
    try:
        for form, k, residual, last_row in ([(f, k, tree(f, k), f in (CONJ, POSTFIX)) for f, k in SMALL_CELLS]
                                            + [(*negated_cell(f, k), negated(tree(f, k)), False) for f, k in SMALL_CELLS]):
            ids = tab.ids(residual)
            if last_row:
                assert len(ids) and ids[-1] == n - 1, (form, n)

            def after(path, zm=True):
                if n >= 63 and path == "slices":
                    assert (t.last_plan(), t.last_form()) == ((k, 1), form), (n, form, t.last_plan(), t.last_form())

            for path in ("slices", "column"):
                got = t.aggregate(V, None, residual, ops=L.AGG_ALL, path=path)
                assert got.count_rows == len(ids), (n, form, path, got.count_rows, len(ids))
                after(path)
            check_paths(t, tab.ocols, V, L.TYPE_INT64, n, None, residual, ops=L.AGG_ALL, paths=["slices", "column"],
                        what=(n, form), after=after)
            s, rows = oracle_keys(tab.ocols, V, None, residual, n)
            assert rows == len(ids)
            m = len(s)
            for path in ("slices", "column"):
                for rank in sorted({0, max(m - 1, 0), m}):
                    for desc in (False, True):
                        got = t.kth(V, rank, desc, None, residual, path=path)
                        assert got == want(s, rows, desc, rank), (n, form, path, rank, desc)
                        after(path)
            check_groups(t, tab.ocols, V, L.TYPE_INT64, [G1], n, None, residual, ops=L.AGG_ALL,
                         paths=["slices", "column"], what=(n, form), after=after)
    finally:
        tab.close()
