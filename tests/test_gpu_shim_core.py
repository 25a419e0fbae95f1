"""The shim's core (shim/cubit_shim_core.hpp) end to end against the library it feeds: segments
found in a block image are planned, sized and packed by the core exactly as AttachSegmentColumn
does, registered through the entry point the core chooses, and the GPU column equals the
segments' values at every row. The reference-written segments are docs.len (BITPACKING) and
terms.docid (RLE) of tests/golden/bitpacking_reference_segments_fts.json. Adds no kernel."""
import ctypes as C

import numpy as np
import pytest

from cubit_amd import _lib as L
from cubit_amd import filters as F
from cubit_amd.table import Context, CubitTable
from oracle import oracle as O
from test_shim_core import (BLOCK, ENTRY_BITPACKED, ENTRY_MIXED, ENTRY_RLE, FTS, NAMES, P, Images, choose_entry,
                            core_lib, min_literal, plan)

pytestmark = pytest.mark.gpu

BY_NAME = {s["name"]: s for s in FTS}
LEN, DOCID = BY_NAME["docs.len"], BY_NAME["terms.docid"]
UNCOMPRESSED_AT = 65_536  # a free stretch of the block, 8-aligned
CONSTANT_STATS = "[Min: -77, Max: -77][Has Null: false, Has No Null: true]"


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def block():
    """One 262,144-byte block: the two fixture segments at their own offsets and 1,000 seeded
    int64 values as an UNCOMPRESSED segment; the values each segment holds."""
    b = np.zeros(BLOCK, dtype=np.uint8)
    for s in (LEN, DOCID):
        raw = np.frombuffer(bytes.fromhex(s["segment_hex"]), dtype=np.uint8)
        b[s["block_offset"]:s["block_offset"] + len(raw)] = raw
    plain = np.random.default_rng(17).integers(-2 ** 62, 2 ** 62, 1000, dtype=np.int64)
    plain[:4] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1]
    assert DOCID["block_offset"] + len(DOCID["segment_hex"]) // 2 <= UNCOMPRESSED_AT
    b[UNCOMPRESSED_AT:UNCOMPRESSED_AT + plain.nbytes] = plain.view(np.uint8)
    values = {"docs.len": np.array(LEN["values"], dtype=np.int64),
              "terms.docid": O.rle_decode(np.frombuffer(bytes.fromhex(DOCID["segment_hex"]), dtype=np.uint8), [0],
                                          [DOCID["count"]], np.int64).astype(np.int64),
              "plain": plain}
    assert len(values["docs.len"]) == LEN["count"] == 153 and len(values["terms.docid"]) == DOCID["count"] == 5468
    return b, values


def register(core, t, col, block, segments):
    """What AttachSegmentColumn does with the core: `segments` = (codec name, rows, block offset,
    statistics text) in row order → the entry point used (ENTRY_*)."""
    traits = (C.c_int * 6)()
    core.csc_traits(P["I64"], traits)
    seg_type, width = traits[4], traits[5]
    start = np.cumsum([0] + [s[1] for s in segments])
    codecs = plan(core, [(int(start[i]), s[1], s[0], 0, 1) for i, s in enumerate(segments)], t.n_rows)
    assert codecs is not None
    im = Images(core)
    constants = np.zeros(len(segments), dtype=np.int64)
    for i, (_, rows, at, stats) in enumerate(segments):
        if codecs[i] == L.CODEC_CONSTANT:
            lit, is_null = min_literal(core, stats)
            assert not is_null
            constants[i] = int(lit)  # the shim casts the literal through the column's type
            assert im.append(codecs[i], None, 0, 0, rows, width)
        else:
            assert im.append(codecs[i], block, at, BLOCK - at, rows, width)
    data, offs, nrows = im.bytes.copy(), im.offsets.copy(), im.rows.copy()
    im.close()
    sc = np.array(codecs, dtype=np.int32)
    entry = choose_entry(core, codecs)
    common = (t.handle, col, seg_type, data.ctypes.data, data.nbytes, offs.ctypes.data, nrows.ctypes.data)
    if entry == ENTRY_BITPACKED:
        L.check(t.lib.cubit_table_add_bitpacked_column(*common, len(offs), None))
    elif entry == ENTRY_RLE:
        L.check(t.lib.cubit_table_add_rle_column(*common, len(offs), None))
    else:
        L.check(t.lib.cubit_table_add_segment_column(*common, sc.ctypes.data, constants.ctypes.data, len(offs), None))
    t.types[col] = t.column_data(col)[1]
    return entry


def probe_all(t, col):
    vals, valid = t.fetch(col, np.arange(t.n_rows, dtype=np.int64))
    assert valid.all()
    return vals


def test_mixed_codec_column_probes_and_scans_equal(ctx, block):
    """CONSTANT, BITPACKING, RLE and UNCOMPRESSED segments in one column. The CONSTANT segment's
    2,048 rows come first, so the BITPACKING segment starts on a 2,048-row vector boundary as every
    DuckDB segment does (its group stores assume no less); RLE and UNCOMPRESSED rows have no such
    need and follow."""
    core = core_lib()
    b, values = block
    segments = [("Constant", 2048, 0, CONSTANT_STATS),
                (NAMES[0], LEN["count"], LEN["block_offset"], ""),
                (NAMES[1], DOCID["count"], DOCID["block_offset"], ""),
                ("Uncompressed", 1000, UNCOMPRESSED_AT, "")]
    want = np.concatenate([np.full(2048, -77, dtype=np.int64), values["docs.len"], values["terms.docid"],
                           values["plain"]])
    t = CubitTable(ctx, len(want))
    assert register(core, t, 0, b, segments) == ENTRY_MIXED
    assert np.array_equal(probe_all(t, 0), want)
    fs = F.TableFilterSet({0: F.ConstantFilter("<", 30)})
    ref = O.table_scan([O.Column(want)], F.serialize(fs), len(want))
    assert 0 < len(ref) < len(want)
    assert np.array_equal(t.scan(fs), ref)
    t.close()


def test_single_codec_columns_take_their_own_entry_points(ctx, block):
    core = core_lib()
    b, values = block
    for s, name, entry in ((DOCID, NAMES[1], ENTRY_RLE), (LEN, NAMES[0], ENTRY_BITPACKED)):
        t = CubitTable(ctx, s["count"])
        assert register(core, t, 0, b, [(name, s["count"], s["block_offset"], "")]) == entry
        assert np.array_equal(probe_all(t, 0), values[s["name"]])
        t.close()
