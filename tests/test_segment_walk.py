"""The library's segment walkers and type table (duckdb-cubit_amd/csrc/cubit_segments.hpp, HIP-free),
run on the CPU through tests/segment_walk_bounds.cpp: a stand-alone program built here with
AddressSanitizer and UBSan and run as a child process. The walkers decide what the unpack kernel may
read, so every truncation of a segment must be refused without a read past the buffer. No GPU."""
import json
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L
from oracle import oracle as O

GOLDEN = ROOT / "tests" / "golden"
SEGMENTS = (json.loads((GOLDEN / "bitpacking_reference_segments.json").read_text())["segments"] +
            json.loads((GOLDEN / "bitpacking_reference_segments_fts.json").read_text())["segments"])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("segment_walk_bounds")
    exe = d / "segment_walk_bounds"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(PKG / "csrc"), str(ROOT / "tests" / "segment_walk_bounds.cpp"), "-o", str(exe)],
                   check=True)
    return d, exe


def sweep(program, walker, raw, rows, dtype):
    """The program's output after the truncation sweep and the whole segment, both passed."""
    d, exe = program
    f = d / "segment.bin"
    f.write_bytes(raw)
    r = subprocess.run([str(exe), walker, str(f), str(rows), str(L.SEGMENT_TYPES[np.dtype(dtype).name])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"refused {len(raw)} truncations, accepted {len(raw)} bytes" in r.stdout
    return r.stdout


def runs_of(out):
    """(values as int64, end rows) from the program's "run" lines."""
    recs = [ln.split() for ln in out.splitlines() if ln.startswith("run ")]
    return np.array([int(r[1]) for r in recs], dtype=np.int64), np.array([int(r[2]) for r in recs], dtype=np.uint64)


def check_runs(out, want, rows):
    """The run ends never descend and finish at `rows`; expanded, the runs are `want` (the
    segment's values as T) widened to int64 with T's sign (uint64: the bits)."""
    vals, ends = runs_of(out)
    assert len(ends) and np.all(np.diff(ends.astype(np.int64)) >= 0) and int(ends[-1]) == rows
    lens = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    wide = want.view(np.int64) if want.dtype == np.uint64 else want.astype(np.int64)
    assert np.array_equal(np.repeat(vals, lens), wide)
    return lens


@pytest.mark.parametrize("s", SEGMENTS, ids=lambda s: s["name"].replace(" ", "_"))
def test_reference_written_segments(program, s):
    """Every segment DuckDB itself wrote (the fixtures): no truncation is accepted or read past, and
    the whole segment yields ceil(rows / 2048) groups that tile its rows, packed words in bounds (the
    program checks them); the two RLE fixtures go through the RLE walker and decode as the oracle's
    restatement does."""
    raw = bytes.fromhex(s["segment_hex"])
    dtype = s.get("dtype", "int64")
    if s.get("compression", "bitpacking") == "bitpacking":
        out = sweep(program, "bp", raw, s["count"], dtype)
        assert f": {-(-s['count'] // 2048)} groups, 0 runs" in out
    else:
        out = sweep(program, "rle", raw, s["count"], dtype)
        want = O.rle_decode(np.frombuffer(raw, np.uint8), [0], [s["count"]], dtype)
        check_runs(out, want, s["count"])


@pytest.mark.parametrize("dt,mode", [(np.int8, "for"), (np.uint16, "delta_for")], ids=["int8", "uint16"])
def test_narrow_t_moves_its_packed_runs(program, dt, mode):
    """A 1- or 2-byte T leaves packed runs off the 4-byte alignment (behind two 1-byte FOR fields,
    or three 2-byte DELTA_FOR fields): they are moved, and the program checks each lands 16-aligned
    inside the moved area."""
    rng = np.random.default_rng(3)
    v = (rng.integers(0, 100, 4101) if mode == "for" else np.cumsum(rng.integers(0, 5, 4101))).astype(dt)
    bp = O.bp_compress(v, None, "auto")
    assert set(O.bp_group_modes(bp)) == {mode}
    moved = 0
    for o, size, r in zip(bp.seg_off.tolist(), bp.seg_size.tolist(), bp.seg_count.tolist()):
        out = sweep(program, "bp", bp.data[o:o + size].tobytes(), r, dt)
        moved += int(out.rsplit("runs, ", 1)[1].split()[0])
    assert moved > 0


@pytest.mark.parametrize("dt", [np.int8, np.int16, np.int32, np.int64, np.uint64], ids=lambda d: np.dtype(d).name)
def test_rle_run_of_the_length_limit(program, dt):
    """70,000 rows: 65,535 of T's minimum (T's sign shows in the widening), which fill one run to the
    limit and leave a zero-length run behind, then T's maximum."""
    info = np.iinfo(dt)
    v = np.concatenate([np.full(O.RLE_MAX_COUNT, info.min, dtype=dt), np.full(70_000 - O.RLE_MAX_COUNT, info.max, dtype=dt)])
    data, offs, rows = O.rle_compress(v)
    assert len(offs) == 1 and int(rows[0]) == 70_000
    out = sweep(program, "rle", data.tobytes(), 70_000, dt)
    lens = check_runs(out, v, 70_000)
    assert lens.tolist() == [O.RLE_MAX_COUNT, 0, 70_000 - O.RLE_MAX_COUNT]
    vals, _ = runs_of(out)
    assert vals.tolist() == [int(info.min), int(info.min), int(np.array(info.max, dtype=dt).astype(np.int64))]


def test_rle_short_runs_with_nulls(program):
    """Runs of 1-3 rows over 5,000 rows, about 5 % NULL (a NULL row lengthens the run before it)."""
    rng = np.random.default_rng(11)
    v = np.repeat(rng.integers(-300, 300, 5_000).astype(np.int16), rng.integers(1, 4, 5_000))[:5_000]
    ok = rng.random(5_000) > 0.05
    data, offs, rows = O.rle_compress(v, ok)
    assert len(offs) == 1 and int(rows[0]) == 5_000
    out = sweep(program, "rle", data.tobytes(), 5_000, np.int16)
    lens = check_runs(out, O.rle_decode(data, offs, rows, np.int16), 5_000)
    assert len(lens) > 2_000 and lens.max() <= 8
    vals, ends = runs_of(out)
    wide = v.astype(np.int64)
    assert np.array_equal(np.repeat(vals, lens)[ok], wide[ok])  # the column's values at its valid rows


def test_type_table(program):
    """For every CUBIT_TYPE_* code what storage_of (size, column type: every code up to VARCHAR) and
    seg_type_of (size, sign, column type, tnorm: the eight integer codes) gave before the table
    replaced them, written out; FLOAT, DOUBLE and VARCHAR name no segment's T, and the codes past
    VARCHAR (the 128-bit key encodings) and unknown ones have no row."""
    T = L
    want = {  # code: size, signed, column type, tnorm, segment type
        T.TYPE_INT32: (4, 1, T.TYPE_INT32, 0, 1),
        T.TYPE_INT64: (8, 1, T.TYPE_INT64, 0, 1),
        T.TYPE_INT8: (1, 1, T.TYPE_INT32, 8 | 0x80, 1),
        T.TYPE_INT16: (2, 1, T.TYPE_INT32, 16 | 0x80, 1),
        T.TYPE_UINT8: (1, 0, T.TYPE_INT32, 8, 1),
        T.TYPE_UINT16: (2, 0, T.TYPE_INT32, 16, 1),
        T.TYPE_UINT32: (4, 0, T.TYPE_INT64, 32, 1),
        T.TYPE_UINT64: (8, 0, T.TYPE_UINT64, 0, 1),
        T.TYPE_FLOAT: (4, None, T.TYPE_FLOAT, None, 0),   # neither old function gave these a sign or a tnorm
        T.TYPE_DOUBLE: (8, None, T.TYPE_DOUBLE, None, 0),
        T.TYPE_VARCHAR: (4, None, T.TYPE_VARCHAR, None, 0),
        -1: None, T.TYPE_INT128: None, T.TYPE_UINT128: None, 13: None,
    }
    assert sorted(want) == list(range(-1, 14))
    r = subprocess.run([str(program[1]), "types"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        assert w[0] == "type"
        got[int(w[1])] = None if w[2] == "none" else tuple(int(x) for x in w[2:])
    assert sorted(got) == sorted(want)
    for code, row in want.items():
        if row is None:
            assert got[code] is None, code
        else:
            assert got[code] is not None and len(got[code]) == 5, code
            assert all(w is None or g == w for g, w in zip(got[code], row)), (code, got[code], row)
