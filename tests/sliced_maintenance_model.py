"""The HIP-free half of tests/test_gpu_sliced_maintenance_fuzz.py: a model of a table whose value columns
carry bit-sliced indexes, the generator that drives a table and the model through the same random sequence
of appends, update lists, merges, syncs and delete lists, the rule by which the library refuses a forced
slice path, and the tally of what the generator reached.

`run(ctx, seed, n_ops, n0)` takes the table class as `make_table`: CubitTable on the GPU, `Stub` (which only
records the calls) for the dry run of tests/test_sliced_maintenance_model.py. Everything the tally counts is
decided here, from the model alone; `checks` (the GPU module's comparisons) is called with those decisions
and draws nothing from the generator's stream, so the dry run and the GPU run walk the same sequence.

The model keeps, per sliced column, the index's `vmin` / `vmax` / `empty` as DESIGN.md's maintenance section
states them (they only widen; a key below the base or the first valid rows rebuild from the column), because
the classes "above the top, by enough to add a slice" and "below the base" are relative to them.
"""
from collections import Counter
from types import SimpleNamespace

import numpy as np

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.datagen import validity_from_mask
from cubit_amd.table import CubitTable
from oracle import oracle as O
from test_gpu_sliced_fuzz import rand_const_filter, rand_residual  # (a GPU test module, but no HIP at import)

ZONE = 131_072
PAD_ROWS = 1_048_576  # cubit_padded_words' granule: the capacity of every table below that many rows
U64 = (1 << 64) - 1
BIAS = 1 << 63
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TXN_START = 4611686018427388000
READER, WRITER = TXN_START + 1, TXN_START + 5
NOT_DELETED = np.uint64(2 ** 64 - 2)
CMPS = ["<", "<=", ">", ">="]
N_LITERAL = 4
RANGE_KEYS = [10, 20, 30, 40]
A, B, I32, UBIG, DBL = 4, 5, 6, 7, 8
VALUE_COLS = (A, B, I32, UBIG, DBL)
FIRST_GROUP = 9
MAX_GROUP_VALUES = 13  # (13 + the NULL slot)^2 <= AGG_MAX_GROUPS
DBL_MAX_KEY = 0x7FEFFFFFFFFFFFFF  # the largest finite DOUBLE's key
DOMAIN = {L.TYPE_INT64: (I64_MIN, I64_MAX), L.TYPE_INT32: (-(1 << 31), (1 << 31) - 1), L.TYPE_UINT64: (I64_MIN, I64_MAX),
          L.TYPE_DOUBLE: (-DBL_MAX_KEY, DBL_MAX_KEY)}
DTYPE = {L.TYPE_INT64: np.int64, L.TYPE_INT32: np.int32, L.TYPE_UINT64: np.uint64, L.TYPE_DOUBLE: np.float64}
APPEND_SIZES = [1, 63, 64, 65, 1000]
N_TREES, TREES_PER_OP = 4, 2

APPEND_CLASSES = ["inside", "above", "below", "null_only", "first_valid", "growth"]
RECORD_CLASSES = ["inside", "above", "below", "to_null", "to_value", "only_null"]
REQUIRED = ([f"append:{c}" for c in APPEND_CLASSES] + [f"{op}:{c}" for op in ("merge", "sync") for c in RECORD_CLASSES]
            + ["grown:append", "grown:merge", "grown:sync", "sync:not_applied", "refusal", "new_slot", "slices:0", "slices:63+", "ubig:0", "ubig:max",
               "filter_only_visible"])


# ------------------------------------------------------------------ keys


def order_keys(typ, bits):
    """The int64 keys of a column's values given as int64 bit patterns: CubitTable._order_keys' maps."""
    return np.asarray(CubitTable._order_keys(SimpleNamespace(types={0: typ}), 0, np.ascontiguousarray(bits, dtype=np.int64)),
                      dtype=np.int64)


def as_bits(data):
    """A column's values as the int64 the C ABI carries: integers as they are, UINT64 / DOUBLE bit patterns."""
    data = np.ascontiguousarray(data)
    return data.view(np.int64) if data.dtype in (np.uint64, np.float64) else data.astype(np.int64)


def keys_of(typ, data):
    return order_keys(typ, as_bits(data))


def bits_of_keys(typ, keys):
    """The inverse of order_keys on the values this module draws (finite DOUBLEs; key 0 is +0.0)."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    if typ == L.TYPE_UINT64:
        return (keys.view(np.uint64) ^ np.uint64(BIAS)).view(np.int64)
    if typ == L.TYPE_DOUBLE:
        mag = np.abs(keys).view(np.uint64)
        return np.where(keys < 0, mag | np.uint64(BIAS), mag).view(np.int64)
    return keys


def values_of_bits(typ, bits):
    bits = np.ascontiguousarray(bits, dtype=np.int64)
    if typ == L.TYPE_UINT64:
        return bits.view(np.uint64).copy()
    if typ == L.TYPE_DOUBLE:
        return bits.view(np.float64).copy()
    return bits.astype(DTYPE[typ])


def bit_length(span):
    return int(span).bit_length()


def randint(rng, lo, hi):
    """A Python int of [lo, hi], for spans up to 2^64 - 1."""
    return lo + int(rng.integers(0, hi - lo, dtype=np.uint64, endpoint=True))


def draw_keys(rng, lo, hi, n):
    off = rng.integers(0, hi - lo, n, dtype=np.uint64, endpoint=True)
    return (off + np.uint64(lo & U64)).view(np.int64)


def reference_slices(keys, valid, vmin, n_bv, nwp):
    """[n_bv, nwp] uint64: bit r of slice k = valid[r] & (((key[r] - vmin) mod 2^64) >> k & 1), LSB first, the
    words past the last row zero. Plain numpy: the build kernel is code under test."""
    n = len(keys)
    u = np.ascontiguousarray(keys, dtype=np.int64).view(np.uint64) - np.uint64(vmin & U64)
    valid = np.asarray(valid, dtype=bool)
    out = np.zeros((n_bv, nwp * 8), dtype=np.uint8)
    for k in range(n_bv if n else 0):
        out[k, : (n + 7) // 8] = np.packbits(((u >> np.uint64(k)) & np.uint64(1)).astype(bool) & valid, bitorder="little")
    return out.view("<u8").view(np.uint64)


def product_sums(a, b, ok, labels, n_groups):
    """Per label, the exact sum of a[r] * b[r] over the rows with ok[r], as Python ints. int64 operands split
    into 32-bit limbs (a = ah 2^32 + al, ah signed, al unsigned): the four limb products fit 64 bits, and each
    is summed per label in 32-bit halves, so nothing rounds or wraps."""
    a = np.where(ok, np.ascontiguousarray(a, dtype=np.int64), 0)
    b = np.where(ok, np.ascontiguousarray(b, dtype=np.int64), 0)
    ah, al, bh, bl = a >> 32, a & 0xFFFFFFFF, b >> 32, b & 0xFFFFFFFF
    out = [0] * n_groups

    def add(x, shift):  # x: int64 (signed) or uint64 limb products
        lo = (x & x.dtype.type(0xFFFFFFFF)).astype(np.float64)
        hi = (x >> x.dtype.type(32)).astype(np.float64)  # |hi| < 2^32: sums of 2^20 rows are exact in a double
        for part, sh in ((lo, shift), (hi, shift + 32)):
            for g, v in enumerate(np.bincount(labels, weights=part, minlength=n_groups)):
                out[g] += int(v) << sh

    if n_groups:
        add(ah * bh, 64)
        add(ah * bl, 32)
        add(al * bh, 32)
        add(al.astype(np.uint64) * bl.astype(np.uint64), 0)
    return out


# ------------------------------------------------------------------ the model


class Col:
    """One column as the oracle sees it, with what the model knows of its indexes."""

    def __init__(self, typ, data, valid, nullable, enc=None, keys=None, kind="literal"):
        self.typ, self.data, self.valid, self.nullable = typ, data, valid, nullable
        self.enc, self.index_keys, self.kind = enc, keys, kind
        self.upd = None  # (rows int64, values int64 bits, versions uint64, ok bool), chronological per row
        self.empty, self.vmin, self.vmax = True, 0, 0  # the bit-sliced index's statistics
        self.home = (0, 0)  # where an all-NULL column's first valid keys are drawn
        self.gvals = None  # a group column: every value it or its records ever held

    def valid_keys(self):
        return keys_of(self.typ, self.data[self.valid])

    def n_bv(self):
        return 0 if self.empty else bit_length(self.vmax - self.vmin)

    def rebuild(self):
        k = self.valid_keys()
        self.empty = len(k) == 0
        if len(k):
            self.vmin, self.vmax = int(k.min()), int(k.max())

    def classify(self, new_keys):
        """The maintenance case of valid keys about to arrive (None: there are none)."""
        if len(new_keys) == 0:
            return None
        if self.empty:
            return "first_valid"
        lo, hi = int(new_keys.min()), int(new_keys.max())
        if lo < self.vmin:
            return "below"
        return "above" if bit_length(max(hi, self.vmax) - self.vmin) > self.n_bv() else "inside"

    def absorb(self, new_keys):
        """The index statistics after those keys arrived (the column holds them already)."""
        if len(new_keys) == 0:
            return
        if self.empty or int(new_keys.min()) < self.vmin:
            self.rebuild()
        else:
            self.vmax = max(self.vmax, int(new_keys.max()))

    def ocol(self, base=False):
        vw = validity_from_mask(self.valid) if self.nullable or not self.valid.all() else None
        upd = None if self.upd is None or base else (self.upd[0], self.upd[1], self.upd[2], self.upd[3].astype(np.uint8))
        return O.Column(self.data, vw, updates=upd)

    def visible_to(self, view):
        """Is some update record of the column visible to the transaction (the library's any_visible)?"""
        if view is None or self.upd is None or len(self.upd[0]) == 0:
            return False
        start, tid = view
        vers = self.upd[2]
        return bool((vers < np.uint64(start)).any() or (vers == np.uint64(tid)).any())


def draw_span(rng, seed):
    """(lo, span) as value_column of the family fuzz draws them: 0 ... 62 bits anywhere in int64, one seed in
    three at an int64 end."""
    bits = int(rng.integers(0, 63))
    span = (1 << bits) - 1
    lo = randint(rng, -(1 << 62), (1 << 62) - span) if rng.random() < 0.7 else [0, I64_MIN, I64_MAX - span][seed % 3]
    return lo, span


class Model:
    def __init__(self, rng, n0, seed):
        self.cols = {}
        nullable = set(int(c) for c in rng.choice(N_LITERAL, size=2, replace=False))
        kinds = [(None, None), (L.INDEX_RANGE, None), (L.INDEX_RANGE, RANGE_KEYS), (L.INDEX_EQUALITY, None)]
        for c in range(N_LITERAL):
            d = rng.integers(0, 49, n0, endpoint=True).astype(np.int32 if c % 2 == 0 else np.int64)
            valid = rng.random(n0) >= 0.1 if c in nullable else np.ones(n0, bool)
            self.cols[c] = Col(L.TYPE_INT32 if c % 2 == 0 else L.TYPE_INT64, d, valid, c in nullable, *kinds[c])
        null_operand = A if rng.random() < 0.5 else B
        for c in VALUE_COLS:
            typ = {A: L.TYPE_INT64, B: L.TYPE_INT64, I32: L.TYPE_INT32, UBIG: L.TYPE_UINT64, DBL: L.TYPE_DOUBLE}[c]
            if c in (A, B):
                lo, span = draw_span(rng, seed)
                if seed % 5 == 1 and c == A:
                    span = 0  # one distinct value: an index of 0 slices
            elif c == I32:
                span = (1 << int(rng.integers(0, 31))) - 1
                lo = randint(rng, -(1 << 31), (1 << 31) - 1 - span)
            elif c == UBIG:  # straddles 2^63 (key 0); the run takes it to 0 and 2^64 - 1
                lo, span = -randint(rng, 1, 1 << int(rng.integers(1, 40))), (1 << int(rng.integers(1, 41))) - 1
            else:  # DOUBLE: [1, 2) (52 bits of key), small magnitudes of both signs, or wide positives
                lo, span = [(0x3FF0000000000000, (1 << 52) - 1), (-0x4059000000000000, 2 * 0x4059000000000000),
                            (0x3FF0000000000000, (1 << 61) - 1)][seed % 3]
            keys = draw_keys(rng, lo, lo + span, n0)
            keys[:2] = [lo, lo + span]
            null_rate = [0.05, 0.5, 0.0][int(rng.integers(0, 3))] if c != (B if null_operand == A else A) else 0.0
            if c == null_operand:
                null_rate = max(null_rate, 0.05)
            valid = rng.random(n0) >= null_rate
            valid[:2] = True
            if (seed % 5 == 2 and c == I32) or (seed % 5 == 4 and c == UBIG):
                valid[:] = False  # some seeds start a value column all-NULL
            col = Col(typ, values_of_bits(typ, bits_of_keys(typ, keys)), valid, not valid.all(), L.INDEX_SLICED, None, "value")
            col.home = (lo, lo + span)
            col.rebuild()
            self.cols[c] = col
        self.groups = []
        n_groups = int(rng.integers(1, 3))
        null_one = int(rng.integers(0, n_groups))
        for j in range(n_groups):
            k = int(rng.integers(2, 10))
            g = (rng.integers(0, k, n0) * 3 - 7).astype(np.int32 if j == 0 else np.int64)
            g[:k] = np.arange(k) * 3 - 7
            valid = rng.random(n0) >= 0.1 if j == null_one else np.ones(n0, bool)
            valid[:k] = True
            col = Col(L.TYPE_INT32 if j == 0 else L.TYPE_INT64, g, valid, j == null_one, L.INDEX_EQUALITY, None, "group")
            col.gvals = set(int(x) for x in np.arange(k) * 3 - 7)
            self.cols[FIRST_GROUP + j] = col
            self.groups.append(FIRST_GROUP + j)
        self.inserted = np.zeros(n0, dtype=np.uint64)
        self.deleted = np.full(n0, NOT_DELETED, dtype=np.uint64)
        self.cap_rows = (n0 + PAD_ROWS - 1) // PAD_ROWS * PAD_ROWS

    @property
    def n(self):
        return len(self.inserted)

    def ocols(self, base=False):
        """The oracle's columns; base: without the update records (what a call without a transaction sees)."""
        return [self.cols[c].ocol(base) for c in sorted(self.cols)]

    def register(self, t):
        for c in sorted(self.cols):
            col = self.cols[c]
            t.add_column(c, col.data, validity_from_mask(col.valid) if col.nullable else None)
            if col.enc is not None:
                t.build_index(c, col.enc, col.index_keys)

    def merged_records(self, c, horizon):
        """(rows, value bits, ok) of each row's newest record below horizon, and the mask of the records kept."""
        rows, vals, vers, ok = self.cols[c].upd
        late = (vers >= np.uint64(horizon)).astype(np.int64)
        first = np.r_[True, rows[1:] != rows[:-1]]
        # records of a row are chronological, the merged ones its prefix: a record is merged while no
        # record of its row up to it is at or past horizon
        seen = np.cumsum(late)
        row_start = np.maximum.accumulate(np.where(first, np.arange(len(rows)), 0))
        merged = seen - (seen[row_start] - late[row_start]) == 0
        last = merged & np.r_[~merged[1:] | first[1:], True]
        return rows[last], vals[last], ok[last], ~merged


def group_value(rng, col):
    """A value for a group column: mostly one it has held, sometimes a new one (a new slot)."""
    if len(col.gvals) < MAX_GROUP_VALUES and rng.random() < 0.5:
        v = max(col.gvals) + 3
        col.gvals.add(v)
        return v
    return int(rng.choice(sorted(col.gvals)))


def beyond(rng, col, side, extreme):
    """A key past the index's top by enough to add a slice (side > 0) or below its base (side < 0); None where
    the type's range has no such key. extreme: the end of the type's range itself."""
    dmin, dmax = DOMAIN[col.typ]
    if col.empty:
        return None
    b = col.n_bv()
    if side > 0:
        need = col.vmin + (1 << b)
        if need > dmax:
            return None
        return dmax if extreme else randint(rng, need, min(dmax, need + (1 << min(b + 1, 62))))
    if col.vmin <= dmin:
        return None
    return dmin if extreme else max(dmin, col.vmin - randint(rng, 1, 1 << min(b + 1, 62)))


def draw_values(rng, col, n, mode):
    """n values of the column's dtype as (array, keys): inside the index's range, with `mode` in ("above",
    "below", "both") a few past that end. Literal and group columns: their small ranges, past both ends."""
    if col.kind == "literal":
        v = rng.integers(-6, 57, n) if mode != "inside" else rng.integers(0, 50, n)
        return v.astype(DTYPE[col.typ]), v.astype(np.int64)
    if col.kind == "group":
        pool = np.array(sorted(col.gvals))
        v = pool[rng.integers(0, len(pool), n)]
        if mode != "inside" and n:
            v[int(rng.integers(0, n))] = group_value(rng, col)
        return v.astype(DTYPE[col.typ]), v.astype(np.int64)
    lo, hi = col.home if col.empty else (col.vmin, col.vmax)
    keys = draw_keys(rng, lo, hi, n)
    for side in ([1] if mode == "above" else [-1] if mode == "below" else [1, -1] if mode == "both" else []):
        extreme = rng.random() < (0.4 if col.typ == L.TYPE_UINT64 else 0.08)
        k = beyond(rng, col, side, extreme)
        if k is None or n == 0:
            continue
        at = rng.integers(0, n, min(n, 1 + int(rng.integers(0, 3))))
        keys[at] = k
        more = rng.integers(0, n, n // 50)  # and some between the old end and the new one
        keys[more] = draw_keys(rng, min(k, hi), max(k, hi), len(more)) if side > 0 else draw_keys(rng, min(k, lo), max(k, lo), len(more))
        keys[at] = k
    return values_of_bits(col.typ, bits_of_keys(col.typ, keys)), keys


# ------------------------------------------------------------------ the tally


class Tally:
    """What the generator reached, from the model alone: `occurred` counts each class when it happens,
    `confirmed` when a forced-slices call that reads the column was answered before the column's next write. A call
    counts as answered when the library must not refuse it, also where its filter keeps no row and no kernel runs:
    the first tree of every pool keeps every row, so each round of queries has calls that do launch."""

    def __init__(self):
        self.occurred, self.confirmed, self.ops = Counter(), Counter(), Counter()
        self.forced = self.answered = self.refused_empty = 0
        self.seeds = set()

    def check(self, seeds):
        assert self.seeds == set(seeds), "run with the seeds of the module: the tally is theirs"
        missing = [c for c in REQUIRED if not self.confirmed[c]]
        assert not missing, (missing, dict(self.occurred), dict(self.confirmed))
        assert 3 * self.answered >= self.forced > 0, (self.answered, self.forced)


class Stub:
    """A table that only records what it is asked: the dry run's stand-in for CubitTable."""

    def __init__(self, ctx, n_rows, row_base=0):
        self.n_rows, self.row_base, self.calls = n_rows, row_base, Counter()
        self.ctx = SimpleNamespace(upload=lambda a: a)

    def append(self, columns, validity=None, insert_id=0):
        self.calls["append"] += 1
        self.n_rows += len(next(iter(columns.values())))

    def __getattr__(self, name):
        def record(*args, **kw):
            self.calls[name] += 1
        return record


# ------------------------------------------------------------------ the generator


def tree_columns(fs, residual):
    cols = set(fs.filters) if fs is not None else set()

    def walk(r):
        if hasattr(r, "children"):
            for k in r.children:
                walk(k)
        elif r is not None:
            cols.add(r.column)
    walk(residual)
    return cols


def make_trees(rng, m):
    """The seed's pool: every row; then random trees over the literal columns, the first of them with one more
    leaf on a value column (a constant of the range it was built with), so that a compare answered from the
    slices runs on maintained slices too."""
    trees = [(None, None)]  # every row: the slices alone decide
    while len(trees) < N_TREES:
        filters = {}
        for c in rng.choice(N_LITERAL, size=rng.integers(1, N_LITERAL + 1), replace=False):
            filters[int(c)] = rand_const_filter(rng)
        if len(trees) == 1:
            c = VALUE_COLS[int(rng.integers(0, len(VALUE_COLS)))]
            col = m.cols[c]
            v = values_of_bits(col.typ, bits_of_keys(col.typ, np.array([randint(rng, *col.home)], dtype=np.int64)))[0]
            filters[c] = F.ConstantFilter(CMPS[rng.integers(0, 4)], v if col.typ == L.TYPE_DOUBLE else int(v))
        residual = rand_residual(rng, N_LITERAL) if rng.random() < 0.5 else None
        trees.append((F.TableFilterSet(filters), residual))
    return trees


def draw_updates(rng, m, c, clock):
    """An update list for column c: chains of one to three committed versions, a writer's tail on a fifth of
    the rows, SET NULL among them, values inside and outside the index's range."""
    col = m.cols[c]
    k = int(rng.integers(1, max(2, min(m.n // 100, 400))))
    rows_u = np.sort(rng.choice(m.n, size=k, replace=False))
    nv = rng.integers(1, 4, k)
    cand = np.sort(rng.integers(1, clock + 1, (k, 3)), axis=1)
    rows, vers = [], []
    for i in range(k):
        vs = sorted(set(cand[i, : nv[i]].tolist()))
        if rng.random() < 0.2:
            vs.append(WRITER)
        rows += [int(rows_u[i])] * len(vs)
        vers += vs
    can_add = col.kind == "value" and not col.empty and col.vmin + (1 << col.n_bv()) <= DOMAIN[col.typ][1]
    modes = ["above", "above", "both", "inside", "below"] if can_add else ["inside", "above", "below", "both", "both"]
    mode = modes[int(rng.integers(0, 5))]  # (a slice can be added above the top: mostly that)
    vals, _ = draw_values(rng, col, len(rows), mode)
    ok = rng.random(len(rows)) >= (0.15 if rng.random() < 0.6 else 1.0)  # (four lists in ten: SET NULL alone)
    bits = as_bits(vals)
    bits[~ok] = 0
    return (np.array(rows, dtype=np.int64), bits, np.array(vers, dtype=np.uint64), ok)


def run(ctx, seed, n_ops, n0=None, tally=None, checks=None, make_table=CubitTable, grow_at=None):
    """Drive a table and the model through n_ops random writes, every one followed by the slice-content check
    and the queries. grow_at: the op that is an append past the table's capacity. Returns the tally."""
    rng = np.random.default_rng(9000 + seed)
    tally = tally if tally is not None else Tally()
    if n0 is None:
        n0 = ZONE + int(rng.integers(1, 131))
    m = Model(rng, n0, seed)
    t = make_table(ctx, n0, row_base=int(rng.integers(0, 1 << 30)))
    m.register(t)
    t.set_derived_budget(6 * (PAD_ROWS // 8))  # six kept bitvectors: admissions, then evictions
    t.set_derived_chain_cost(0)
    trees = make_trees(rng, m)
    clock, floor = 3, 0
    pending = {c: set() for c in m.cols}  # classes since the column's last write, not yet confirmed

    def wrote(c, classes):
        col = m.cols[c]
        classes = set(classes)
        if col.kind == "value":
            if col.n_bv() == 0 and not col.empty:
                classes.add("slices:0")
            if col.n_bv() >= 63:
                classes.add("slices:63+")
            if c == UBIG and not col.empty and col.vmin == I64_MIN:
                classes.add("ubig:0")
            if c == UBIG and not col.empty and col.vmax == I64_MAX:
                classes.add("ubig:max")
        pending[c] = classes
        for k in classes:
            tally.occurred[k] += 1

    def answered(cols):
        for c in cols:
            for k in pending[c]:
                tally.confirmed[k] += 1
            pending[c] = set()

    def apply_records(c, op, rows, bits, ok):
        """Fold records (one per row) into the model's base; returns the maintenance classes."""
        col = m.cols[c]
        classes = set()
        if len(rows) == 0:
            return classes
        was = col.valid[rows]
        new_keys = order_keys(col.typ, bits[ok])
        if (was & ~ok).any():
            classes.add(f"{op}:to_null")
        if (~was & ok).any():
            classes.add(f"{op}:to_value")
        if col.kind == "value" and was.any() and not ok.any():
            classes.add(f"{op}:only_null")  # nothing but NULLs arrive: no statistics move, the slices must
        if col.kind == "value" and len(new_keys) and not col.empty:
            if int(new_keys.min()) < col.vmin:
                classes.add(f"{op}:below")
            if bit_length(max(int(new_keys.max()), col.vmax) - col.vmin) > col.n_bv():
                classes.add(f"{op}:above")
            if ((new_keys >= col.vmin) & (new_keys <= col.vmax)).any():
                classes.add(f"{op}:inside")
        if col.kind == "group" and len(new_keys) and not np.isin(new_keys, keys_of(col.typ, col.data[col.valid])).all():
            classes.add("new_slot")
        col.data[rows] = values_of_bits(col.typ, np.where(ok, bits, 0))
        col.valid[rows] = ok
        if not ok.all():
            col.nullable = True
        if col.kind == "value":
            col.absorb(new_keys)
        return classes

    def merge(c, horizon):
        nonlocal floor
        col = m.cols[c]
        exp, classes = 0, set()
        if col.upd is not None:
            rows, bits, ok, keep = m.merged_records(c, horizon)
            exp = len(rows)
            classes = apply_records(c, "merge", rows, bits, ok)
            col.upd = tuple(a[keep] for a in col.upd) if keep.any() else None
        got = t.merge_updates(c, horizon)
        assert checks is None or got == exp, ("merge", c, horizon, got, exp)
        floor = max(floor, horizon)
        return exp, classes

    try:
        for c in VALUE_COLS:
            wrote(c, set())  # the build: a column may start at 0 slices, or at 63 and more

        grown = False  # the table crossed its capacity: every bitvector is a reallocated one
        after_growth = [str(x) for x in rng.permutation(["append", "merge", "sync"])]
        for i in range(n_ops):
            ops = ["append", "append", "updates", "updates", "merge", "merge", "sync", "sync", "deletes"]
            if any(m.cols[c].upd is not None for c in VALUE_COLS):
                ops += ["merge"] * 4  # records of a sliced column wait: fold them before they are replaced
            op = "append" if i == grow_at else str(rng.choice(ops))
            if grown:  # the writes that maintain slices, in turn, on the regrown buffers
                op = after_growth[(i - grow_at - 1) % 3]
            touched, what = {}, op  # column -> classes
            if op == "append":
                nb = int(rng.choice(APPEND_SIZES + [int(rng.integers(1, 140_001))]))
                grows = i == grow_at
                if grows:
                    nb = m.cap_rows - m.n + int(rng.integers(1, 2001))  # (across it, and no further than it takes)
                elif m.n + nb > m.cap_rows:
                    nb = m.cap_rows - m.n  # (only grow_at crosses the capacity)
                iid = int(rng.choice([0, clock, WRITER]))
                data, valid = {}, {}
                for c in sorted(m.cols):
                    col = m.cols[c]
                    mode = str(rng.choice(["inside", "inside", "inside", "above", "above", "below", "null_only"]))
                    vals, keys = draw_values(rng, col, nb, mode if mode != "null_only" else "inside")
                    ok = rng.random(nb) >= (0.1 if col.nullable else 0.0)
                    if col.kind == "value":
                        if mode == "null_only" or (col.empty and rng.random() < 0.5):
                            ok[:] = False
                        elif mode != "inside":  # the keys past the end are valid rows
                            ok[(keys < (col.home[0] if col.empty else col.vmin)) | (keys > (col.home[1] if col.empty else col.vmax))] = True
                        k_new = keys[ok]
                        cls = col.classify(k_new) or "null_only"
                        touched[c] = {f"append:{cls}"} | ({"append:growth"} if grows else set())
                    else:
                        base = keys_of(col.typ, col.data[col.valid])
                        touched[c] = {"new_slot"} if col.kind == "group" and not np.isin(keys[ok], base).all() else set()
                    data[c], valid[c] = vals, ok
                t.append(data, {c: validity_from_mask(valid[c]) for c in valid if not valid[c].all() or m.cols[c].nullable},
                         insert_id=iid)
                for c in sorted(m.cols):
                    col = m.cols[c]
                    col.data = np.concatenate([col.data, data[c]])
                    col.valid = np.concatenate([col.valid, valid[c]])
                    col.nullable |= not valid[c].all()
                    if col.kind == "value":
                        col.absorb(keys_of(col.typ, data[c][valid[c]]))
                m.inserted = np.concatenate([m.inserted, np.full(nb, iid, dtype=np.uint64)])
                m.deleted = np.concatenate([m.deleted, np.full(nb, NOT_DELETED, dtype=np.uint64)])
                if grows:
                    m.cap_rows = max((m.n + PAD_ROWS - 1) // PAD_ROWS * PAD_ROWS, m.cap_rows)
                what = (op, nb, iid, grows)
            elif op == "updates":
                c = int(rng.choice(list(range(N_LITERAL)) + list(VALUE_COLS) * 3 + m.groups))
                clock += 2
                u = draw_updates(rng, m, c, clock)
                t.set_updates(c, u[0], u[1], u[2], u[3])
                m.cols[c].upd = u
                if not u[3].all():
                    m.cols[c].nullable = True
                what = (op, c, len(u[0]))
            elif op == "merge":
                have = [c for c in m.cols if m.cols[c].upd is not None]
                have = [c for c in have if c in VALUE_COLS] * 3 + have  # (mostly a sliced column's records)
                c = int(rng.choice(have)) if have and rng.random() < 0.9 else int(rng.integers(0, len(m.cols)))
                h = int(rng.integers(floor, clock + 2)) if rng.random() < 0.5 else clock + 1
                if grown:  # a sliced column's records, every committed one (a list is set first where none waits)
                    have = [c for c in VALUE_COLS if m.cols[c].upd is not None]
                    c, h = (int(rng.choice(have)) if have else VALUE_COLS[int(rng.integers(0, len(VALUE_COLS)))]), clock + 3
                    if not have:
                        clock += 2
                        u = draw_updates(rng, m, c, clock)
                        t.set_updates(c, u[0], u[1], u[2], u[3])
                        m.cols[c].upd = u
                        m.cols[c].nullable |= not u[3].all()
                n_merged, classes = merge(c, h)
                if n_merged:
                    touched[c] = classes
                what = (op, c, h, n_merged)
            elif op == "sync":
                c = int(rng.choice(list(VALUE_COLS) * 3 + list(range(N_LITERAL)) + m.groups))
                if grown:
                    c = VALUE_COLS[int(rng.integers(0, len(VALUE_COLS)))]
                col = m.cols[c]
                classes = set()
                if col.upd is not None:  # the library refuses a sync over outstanding records: fold or clear them
                    if rng.random() < 0.5:
                        classes |= merge(c, clock + 1)[1]
                    if col.upd is not None:
                        t.set_updates(c, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint64))
                        col.upd = None
                frac = float(rng.uniform(0.001, 0.02))
                mode = ["inside", "above", "below", "both", "nulls", "nulls"][int(rng.integers(0, 6))]
                pick = np.flatnonzero(rng.random(m.n) < frac)
                new, nok = col.data.copy(), col.valid.copy()
                vals, _ = draw_values(rng, col, len(pick), mode if mode != "nulls" else "inside")
                new[pick], nok[pick] = vals, True  # (a NULL row among them: NULL -> value)
                nok[pick[rng.random(len(pick)) < 0.2]] = False  # value -> NULL
                if mode == "nulls":  # value -> NULL and nothing else
                    new, nok = col.data.copy(), col.valid.copy()
                    nok[pick] = False
                to_value = np.flatnonzero(~col.valid & (rng.random(m.n) < (10 * frac if mode != "nulls" else 0.0)))
                vals, _ = draw_values(rng, col, len(to_value), "inside")
                new[to_value], nok[to_value] = vals, True
                ob, nb_ = as_bits(col.data), as_bits(new)
                ch = np.flatnonzero((col.valid != nok) | (col.valid & nok & (ob != nb_)))
                cut = len(ch) > 0 and rng.random() < 0.25 and not grown
                on_device = rng.random() < 0.5
                vw = validity_from_mask(nok) if col.nullable or not nok.all() else None
                args = (t.ctx.upload(new), None if vw is None else t.ctx.upload(vw)) if on_device else (new, vw)
                got = t.sync_column(c, *args, max_changed=len(ch) - 1 if cut else None, on_device=on_device)
                assert checks is None or got == (len(ch), not cut), ("sync", c, got, len(ch), cut)
                if cut:
                    classes.add("sync:not_applied")
                else:
                    classes |= apply_records(c, "sync", ch, nb_[ch], nok[ch])
                touched[c] = classes
                what = (op, c, len(ch), cut, on_device, mode)
            else:
                k = int(rng.integers(0, max(1, m.n // 20)))
                rows_d = np.sort(rng.choice(m.n, size=k, replace=False)).astype(np.int64)
                ids = rng.choice(np.array([1, clock, WRITER], dtype=np.uint64), size=k)
                t.set_deletes(rows_d, ids)
                m.deleted = np.full(m.n, NOT_DELETED, dtype=np.uint64)
                m.deleted[rows_d] = ids
                what = (op, k)
            tally.ops[op] += 1
            for c, classes in touched.items():
                wrote(c, set(classes) | ({f"grown:{op}"} if grown and c in VALUE_COLS and classes else set()))
            grown |= i == grow_at

            # the slices themselves, every sliced column's: the written ones moved, the others must not have
            failed = []  # a wrong slice does not hide what it does to the queries: both are reported
            if checks is not None:
                try:
                    checks.slices(t, m, VALUE_COLS, (seed, i, what))
                except AssertionError as e:
                    failed.append(("slices", e))

            # the queries: trees drawn from the seed's pool, each under no transaction, two readers and the writer
            ocols = (m.ocols(), m.ocols(base=True)) if checks is not None else None
            views = [None, (max(floor, 2), READER), (max(clock + 1, floor), READER), (max(floor, 2), WRITER)]
            for j in rng.choice(N_TREES, size=TREES_PER_OP, replace=False):
                fs, residual = trees[int(j)]
                filter_cols = tree_columns(fs, residual)
                for view in views:
                    col = VALUE_COLS[int(rng.integers(0, len(VALUE_COLS)))]
                    draws = {"rank": float(rng.random()), "q": float(rng.random()), "k": float(rng.random()),
                             "ops": int(rng.integers(0, 8))}
                    vis = {c: m.cols[c].visible_to(view) for c in m.cols}
                    gvis = any(vis[g] for g in m.groups)
                    dead = {c: m.cols[c].empty for c in VALUE_COLS}  # an empty index answers nothing (bind_slices)
                    refuse = {"single": vis[col] or dead[col], "grouped": vis[col] or dead[col] or gvis,
                              "product": vis[A] or vis[B] or dead[A] or dead[B]}
                    refuse["product_by"] = refuse["product"] or gvis
                    reads = {"single": [col], "grouped": [col] + m.groups, "product": [A, B], "product_by": [A, B] + m.groups}
                    for kind, calls in (("single", 3), ("grouped", 1), ("product", 1), ("product_by", 1)):
                        tally.forced += calls
                        if not refuse[kind]:
                            tally.answered += calls
                            answered(reads[kind])
                            if any(vis[c] for c in filter_cols):
                                tally.occurred["filter_only_visible"] += 1
                                tally.confirmed["filter_only_visible"] += 1
                        elif any(vis[c] for c in reads[kind]):
                            for c in reads[kind]:
                                if vis[c] and c in VALUE_COLS + tuple(m.groups):
                                    pending[c].add("refusal")
                            tally.occurred["refusal"] += 1
                        else:
                            tally.refused_empty += calls
                    if checks is not None and (not failed or failed[-1][0] != "queries"):
                        try:
                            checks.queries(t, m, ocols, fs, residual, view, col, refuse, draws, (seed, i, what, int(j), view, col))
                        except AssertionError as e:
                            failed.append(("queries", e))
            assert not failed, failed
        if checks is not None:
            checks.finish(t)
    finally:
        t.close()
    tally.seeds.add(seed)
    return tally


# seed -> (ops, the op that appends past the capacity or None): what both test modules run. A growing seed crosses
# the capacity first and then appends, merges and syncs (two of the three, in a drawn order) on the grown table.
PLAN = {s: (3, 0) if s % 3 == 0 else (7, None) for s in range(24)}


def run_plan(ctx, seed, tally, checks=None, make_table=CubitTable):
    n_ops, grow_at = PLAN[seed]
    return run(ctx, seed, n_ops, None, tally, checks, make_table, grow_at)
