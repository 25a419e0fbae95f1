"""The DuckDB shim's engine-independent core (duckdb-cubit_amd/shim/cubit_shim_core.hpp), run here
through its C test surface (shim/cubit_shim_core_capi.cpp → lib/libcubit_shim_core.so): segment
images parsed in place out of a block, the segment plan's refusals, the CONSTANT value's literal,
the type table, int64 ↔ physical conversion, the partition and delete-list arithmetic, the index
specification's text and key order. tests/shim_core_bounds.cpp repeats the image parse under
AddressSanitizer with every truncated `room`, as a stand-alone program. No GPU, no DuckDB."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import PKG, ROOT
from cubit_amd import _lib as L
from cubit_amd.datagen import validity_from_mask

GOLDEN = ROOT / "tests" / "golden"
FTS = json.loads((GOLDEN / "bitpacking_reference_segments_fts.json").read_text())["segments"]
V64 = [s for s in json.loads((GOLDEN / "bitpacking_reference_segments.json").read_text())["segments"]
       if "block_offset" in s]
BLOCK = 262_144
RG = 122_880

# cubit_shim::Phys, in the enum's order
PHYS = ["Bool", "I8", "I16", "I32", "I64", "U8", "U16", "U32", "U64", "F32", "F64", "Varchar", "I128", "U128"]
P = {name: i for i, name in enumerate(PHYS)}
NUMPY = {"Bool": np.bool_, "I8": np.int8, "I16": np.int16, "I32": np.int32, "I64": np.int64, "U8": np.uint8,
         "U16": np.uint16, "U32": np.uint32, "U64": np.uint64, "F32": np.float32, "F64": np.float64}
NAMES = ["BitPacking", "RLE", "Constant", "Uncompressed"]  # CompressionTypeToString's spelling
CODEC = {"bitpacking": L.CODEC_BITPACKING, "rle": L.CODEC_RLE}
ENTRY_BITPACKED, ENTRY_RLE, ENTRY_MIXED = 0, 1, 2

_core = None


def core_lib():
    """lib/libcubit_shim_core.so, brought up to date by its Makefile rule: a build that fails is a
    test failure."""
    global _core
    if _core is None:
        subprocess.run(["make", "-s", "-C", str(PKG), "lib/libcubit_shim_core.so"], check=True)
        lib = C.CDLL(str(PKG / "lib" / "libcubit_shim_core.so"))
        lib.csc_load_int64.restype = C.c_int64
        lib.csc_load_int64.argtypes = [C.c_int, C.c_void_p, C.c_uint64]
        lib.csc_store_from_int64.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
        lib.csc_segment_image_size.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        lib.csc_images_new.restype = C.c_void_p
        lib.csc_images_free.argtypes = [C.c_void_p]
        lib.csc_images_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
        for f, rt in ((lib.csc_images_n_bytes, C.c_uint64), (lib.csc_images_bytes, C.c_void_p),
                      (lib.csc_images_n_segments, C.c_uint32), (lib.csc_images_offsets, C.c_void_p),
                      (lib.csc_images_rows, C.c_void_p)):
            f.restype, f.argtypes = rt, [C.c_void_p]
        lib.csc_choose_entry.argtypes = [C.c_void_p, C.c_uint32]
        lib.csc_split_rows.restype = C.c_uint64
        lib.csc_split_rows.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
        lib.csc_local_deletes.restype = None
        lib.csc_local_deletes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.c_void_p]
        lib.csc_few_distinct.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.csc_sample_rows.restype = C.c_uint64
        lib.csc_sample_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        lib.csc_row_valid.argtypes = [C.c_void_p, C.c_uint64]
        lib.csc_pack_strings.restype = C.c_uint64
        lib.csc_pack_strings.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.csc_split_index_spec.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
        lib.csc_sort_keys.restype = C.c_uint64
        lib.csc_sort_keys.argtypes = [C.c_int, C.c_void_p, C.c_uint64]
        lib.csc_sort_string_keys.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p]
        lib.csc_enough_keys.argtypes = [C.c_int, C.c_uint64]
        lib.csc_constant_min_literal.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p]
        lib.csc_plan_segments.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_void_p]
        _core = lib
    return _core


@pytest.fixture(scope="module")
def core():
    return core_lib()


class Images:
    """cubit_shim::SegmentImages behind the C surface."""

    def __init__(self, lib):
        self.lib, self.h = lib, lib.csc_images_new()

    def append(self, codec, buf, at, room, count, width) -> bool:
        """The segment at byte `at` of numpy buffer `buf` (None: no bytes, a CONSTANT segment)."""
        p = None if buf is None else buf.ctypes.data + at
        return bool(self.lib.csc_images_append(self.h, codec, p, room, count, width))

    @property
    def bytes(self) -> np.ndarray:
        n = self.lib.csc_images_n_bytes(self.h)
        return np.frombuffer(C.string_at(self.lib.csc_images_bytes(self.h), n), dtype=np.uint8) if n else \
            np.zeros(0, np.uint8)

    def _u64(self, f) -> np.ndarray:
        n = self.lib.csc_images_n_segments(self.h)
        return np.frombuffer(C.string_at(f(self.h), 8 * n), dtype=np.uint64) if n else np.zeros(0, np.uint64)

    @property
    def offsets(self) -> np.ndarray:
        return self._u64(self.lib.csc_images_offsets)

    @property
    def rows(self) -> np.ndarray:
        return self._u64(self.lib.csc_images_rows)

    def close(self):
        self.lib.csc_images_free(self.h)


def image_size(lib, codec, buf, at, room, count, width):
    """(accepted, size) of SegmentImageSize on the bytes at buf[at:]."""
    size = C.c_uint64(0)
    p = None if buf is None else buf.ctypes.data + at
    ok = lib.csc_segment_image_size(codec, p, room, count, width, C.byref(size))
    return bool(ok), int(size.value)


def choose_entry(lib, codecs) -> int:
    a = np.array(codecs, dtype=np.int32)
    return lib.csc_choose_entry(a.ctypes.data, len(a))


def blocks_of(segments):
    """{block_id: the block's 262,144 bytes} with every segment laid at its own block_offset, so the
    bytes after a segment are the next segment's, as in the file."""
    blocks = {}
    for s in sorted(segments, key=lambda s: (s["block_id"], s["block_offset"])):
        b = blocks.setdefault(s["block_id"], np.zeros(BLOCK, dtype=np.uint8))
        raw = bytes.fromhex(s["segment_hex"])
        at = s["block_offset"]
        assert at + len(raw) <= BLOCK and not b[at:at + len(raw)].any(), s["name"]  # the fixtures do not overlap
        b[at:at + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return blocks


# ------------------------------------------------------------------ segment images

@pytest.mark.parametrize("segments", [FTS, V64], ids=["fts", "storage_version"])
def test_reference_written_segments_parse_in_place(core, segments):
    """Every fixture segment, found at its offset in a block image: the size is exactly the
    segment's, and the built image is its bytes (at a 16-byte-aligned offset, rows recorded)."""
    if segments is FTS:
        assert sorted(s["compression"] for s in FTS) == ["bitpacking"] * 7 + ["rle"] * 2
        assert all("block_id" in s and "block_offset" in s for s in FTS)
    assert segments
    blocks = blocks_of(segments)
    im = Images(core)
    want_bytes = bytearray()
    for s in segments:
        raw = bytes.fromhex(s["segment_hex"])
        codec = CODEC[s.get("compression", "bitpacking")]
        width = np.dtype(s.get("dtype", "int64")).itemsize
        block, at = blocks[s["block_id"]], s["block_offset"]
        ok, size = image_size(core, codec, block, at, BLOCK - at, s["count"], width)
        assert ok and size == len(raw), (s["name"], size, len(raw))
        assert im.append(codec, block, at, BLOCK - at, s["count"], width)
        want_bytes += bytes(-len(want_bytes) % 16)
        assert int(im.offsets[-1]) == len(want_bytes) and int(im.rows[-1]) == s["count"]
        want_bytes += raw
        assert im.bytes.tobytes() == bytes(want_bytes), s["name"]
    assert len(im.offsets) == len(segments) and all(int(o) % 16 == 0 for o in im.offsets)
    im.close()


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_uncompressed_size_is_count_times_width(core, width):
    count = 1000
    buf = np.arange(count * width + 64, dtype=np.uint64).astype(np.uint8)
    assert image_size(core, L.CODEC_UNCOMPRESSED, buf, 0, len(buf), count, width) == (True, count * width)
    assert image_size(core, L.CODEC_UNCOMPRESSED, buf, 0, count * width, count, width) == (True, count * width)
    assert not image_size(core, L.CODEC_UNCOMPRESSED, buf, 0, count * width - 1, count, width)[0]
    im = Images(core)
    assert im.append(L.CODEC_UNCOMPRESSED, buf, 0, len(buf), count, width)
    assert im.bytes.tobytes() == buf[:count * width].tobytes()
    im.close()


def test_constant_segment_has_no_bytes_and_keeps_its_slot(core):
    buf = np.arange(64, dtype=np.uint8)
    assert image_size(core, L.CODEC_CONSTANT, None, 0, 0, 2048, 8) == (True, 0)
    im = Images(core)
    assert im.append(L.CODEC_UNCOMPRESSED, buf, 0, 64, 5, 4)   # 20 bytes
    assert im.append(L.CODEC_CONSTANT, None, 0, 0, 2048, 4)    # no bytes, a slot at the aligned offset
    assert im.append(L.CODEC_UNCOMPRESSED, buf, 32, 32, 3, 4)  # 12 bytes at the same offset
    assert im.offsets.tolist() == [0, 32, 32] and im.rows.tolist() == [5, 2048, 3]
    assert im.bytes.tobytes() == buf[:20].tobytes() + bytes(12) + buf[32:44].tobytes()
    assert not im.append(9, buf, 0, 64, 1, 4)  # no such codec: refused, nothing recorded
    assert len(im.offsets) == 3
    im.close()


def test_entry_point_choice(core):
    bp, rle, const, unc = L.CODEC_BITPACKING, L.CODEC_RLE, L.CODEC_CONSTANT, L.CODEC_UNCOMPRESSED
    assert choose_entry(core, [bp]) == choose_entry(core, [bp, bp, bp]) == ENTRY_BITPACKED
    assert choose_entry(core, [rle]) == choose_entry(core, [rle, rle]) == ENTRY_RLE
    for mixed in ([bp, rle], [rle, bp], [const], [unc], [bp, const], [rle, rle, unc]):
        assert choose_entry(core, mixed) == ENTRY_MIXED, mixed


# ------------------------------------------------------------------ the segment plan

def plan(lib, descs, n_rows):
    """PlanSegments over (start, count, codec name, has_updates, persistent) tuples → codecs or None."""
    n = len(descs)
    start = np.array([d[0] for d in descs], dtype=np.uint64)
    count = np.array([d[1] for d in descs], dtype=np.uint64)
    names = (C.c_char_p * max(n, 1))(*[d[2].encode() for d in descs])
    upd = np.array([d[3] for d in descs], dtype=np.uint8)
    pers = np.array([d[4] for d in descs], dtype=np.uint8)
    four = (C.c_char_p * 4)(*[x.encode() for x in NAMES])
    out = np.full(max(n, 1), -1, dtype=np.int32)
    ok = lib.csc_plan_segments(n, start.ctypes.data, count.ctypes.data, C.cast(names, C.c_void_p), upd.ctypes.data,
                               pers.ctypes.data, n_rows, C.cast(four, C.c_void_p), out.ctypes.data)
    return out[:n].tolist() if ok else None


GOOD = [(0, 100, "BitPacking", 0, 1), (100, 50, "RLE", 0, 1), (150, 2048, "Constant", 0, 1),
        (2198, 7, "Uncompressed", 0, 1)]


def test_plan_accepts_the_four_codecs(core):
    assert plan(core, GOOD, 2205) == [L.CODEC_BITPACKING, L.CODEC_RLE, L.CODEC_CONSTANT, L.CODEC_UNCOMPRESSED]
    # a CONSTANT segment has no block to be persistent in
    assert plan(core, [(0, 2048, "Constant", 0, 0), (2048, 10, "RLE", 0, 1)], 2058) == [L.CODEC_CONSTANT, L.CODEC_RLE]


def edited(i, **kw):
    keys = ["start", "count", "codec", "has_updates", "persistent"]
    d = list(GOOD)
    seg = dict(zip(keys, d[i]))
    seg.update(kw)
    d[i] = tuple(seg[k] for k in keys)
    return d


@pytest.mark.parametrize("descs,n_rows", [
    pytest.param(edited(1, start=101), 2205, id="gap"),
    pytest.param(edited(1, start=99), 2205, id="overlap"),
    pytest.param(edited(2, has_updates=1), 2205, id="has_updates"),
    pytest.param(edited(0, persistent=0), 2205, id="non-persistent-bitpacking"),
    pytest.param(edited(1, codec="Dictionary"), 2205, id="unknown-codec"),
    pytest.param(GOOD, 2206, id="short-of-n_rows"),
    pytest.param(GOOD, 2204, id="past-n_rows"),
    pytest.param([], 0, id="empty"),
])
def test_plan_refuses(core, descs, n_rows):
    assert plan(core, descs, n_rows) is None


def min_literal(lib, stats):
    lit = C.create_string_buffer(256)
    null = C.c_int(0)
    rc = lib.csc_constant_min_literal(stats.encode(), lit, 256, C.byref(null))
    assert rc in (0, 1)
    return (lit.value.decode(), bool(null.value)) if rc else None


def test_constant_min_literal(core):
    tail = "[Has Null: false, Has No Null: true]"
    assert min_literal(core, "[Min: 42, Max: 42]" + tail) == ("42", False)
    assert min_literal(core, "[Min: 1994-01-01, Max: 1994-01-01]" + tail) == ("1994-01-01", False)
    assert min_literal(core, "[Min: -12345.67, Max: -12345.67]" + tail) == ("-12345.67", False)
    assert min_literal(core, "[Min: NULL, Max: NULL][Has Null: true, Has No Null: false]") == ("NULL", True)
    assert min_literal(core, "[Has Null: false, Has No Null: true]") is None
    assert min_literal(core, " [Min: 42, Max: 42]") is None  # does not start with "[Min: "
    assert min_literal(core, "[Min: 42]") is None


# ------------------------------------------------------------------ type table

def test_type_table(core):
    """Restated from the six functions the table replaced: GpuPhysical (all 14), DictPhysical,
    WidePhysical, UploadType, SegmentType, and the width of the segments' T (asked only of a type
    with a segment type; 0 elsewhere)."""
    T = L
    want = {  # gpu, dict, wide, upload_type, segment_type, width
        "Bool": (1, 0, 0, T.TYPE_INT32, T.TYPE_INT8, 1),
        "I8": (1, 0, 0, T.TYPE_INT32, T.TYPE_INT8, 1),
        "I16": (1, 0, 0, T.TYPE_INT32, T.TYPE_INT16, 2),
        "I32": (1, 0, 0, T.TYPE_INT32, T.TYPE_INT32, 4),
        "I64": (1, 0, 1, T.TYPE_INT64, T.TYPE_INT64, 8),
        "U8": (1, 0, 0, T.TYPE_INT32, T.TYPE_UINT8, 1),
        "U16": (1, 0, 0, T.TYPE_INT32, T.TYPE_UINT16, 2),
        "U32": (1, 0, 1, T.TYPE_INT64, T.TYPE_UINT32, 4),
        "U64": (1, 0, 1, T.TYPE_UINT64, T.TYPE_UINT64, 8),
        "F32": (1, 0, 0, T.TYPE_FLOAT, -1, 0),
        "F64": (1, 0, 1, T.TYPE_DOUBLE, -1, 0),
        "Varchar": (1, 1, 0, T.TYPE_INT32, -1, 0),
        "I128": (1, 1, 0, T.TYPE_INT32, -1, 0),
        "U128": (1, 1, 0, T.TYPE_INT32, -1, 0),
    }
    assert list(want) == PHYS
    for name in PHYS:
        got = (C.c_int * 6)()
        core.csc_traits(P[name], got)
        assert tuple(got) == want[name], name
    got = (C.c_int * 6)()
    core.csc_traits(len(PHYS), got)  # Unsupported
    assert tuple(got)[:3] == (0, 0, 0)


# ------------------------------------------------------------------ conversion

def conversion_cases(name):
    dt = np.dtype(NUMPY[name])
    if name == "Bool":
        return np.array([False, True])
    if dt.kind in "iu":
        info = np.iinfo(dt)
        v = [info.min, info.max, 0, 1] + ([-1] if dt.kind == "i" else [])
        if name == "U64":
            v += [2 ** 63, 2 ** 64 - 1]
        return np.array(v, dtype=dt)
    bits = np.uint32 if name == "F32" else np.uint64
    fi = np.finfo(dt)
    nan = 0x7FC00000 if name == "F32" else 0x7FF8000000000000
    sign = 1 << (31 if name == "F32" else 63)
    pats = np.array([nan, nan | sign, 0, sign], dtype=bits).view(dt)  # both NaN signs, ±0.0
    return np.concatenate([pats, np.array([fi.min, fi.max, -1.0, np.inf, -np.inf], dtype=dt)])


@pytest.mark.parametrize("name", list(NUMPY))
def test_load_store_round_trip(core, name):
    x = conversion_cases(name)
    dt = x.dtype
    wide = np.array([core.csc_load_int64(P[name], x.ctypes.data, i) for i in range(len(x))], dtype=np.int64)
    if dt.kind == "f":  # the bit patterns, FLOAT's zero-extended
        want = x.view(np.uint32).astype(np.int64) if name == "F32" else x.view(np.int64)
    elif name == "U64":  # the bits
        want = x.view(np.int64)
    else:  # the values
        want = x.astype(np.int64)
    assert np.array_equal(wide, want)
    back = np.zeros(len(x) + 1, dtype=dt)
    guard = np.array([1], dtype=dt)[0]
    back[-1] = guard
    core.csc_store_from_int64(P[name], back.ctypes.data, wide.ctypes.data, len(x))
    assert back[:-1].tobytes() == x.tobytes() and back[-1] == guard  # bit-exact, nothing written past n


def test_uint32_loads_unsigned(core):
    x = np.array([4294967295], dtype=np.uint32)
    assert core.csc_load_int64(P["U32"], x.ctypes.data, 0) == 4294967295
    y = np.array([-1], dtype=np.int32)
    assert core.csc_load_int64(P["I32"], y.ctypes.data, 0) == -1


def test_store_narrows_as_a_cast(core):
    """The staging values are the column's own, widened; a cast back to T is the identity on them
    and wraps like a C cast otherwise (BOOL: non-zero is true)."""
    src = np.array([0, 1, 2, 256, -1], dtype=np.int64)
    out = np.zeros(5, dtype=np.uint8)
    core.csc_store_from_int64(P["U8"], out.ctypes.data, src.ctypes.data, 5)
    assert out.tolist() == [0, 1, 2, 0, 255]
    core.csc_store_from_int64(P["Bool"], out.ctypes.data, src.ctypes.data, 5)
    assert out.tolist() == [0, 1, 1, 1, 1]


def test_row_valid(core):
    words = np.array([0x8000000000000001, 0x2], dtype=np.uint64)
    got = [r for r in range(128) if core.csc_row_valid(words.ctypes.data, r)]
    assert got == [0, 63, 65]


# ------------------------------------------------------------------ partitions and deletes

def split(lib, rows, ctxs):
    bounds = np.zeros(ctxs + 2, dtype=np.uint64)
    n = lib.csc_split_rows(rows, ctxs, bounds.ctypes.data)
    return int(n), bounds[:n + 1].tolist()


@pytest.mark.parametrize("ctxs", [1, 2, 3, 8])
@pytest.mark.parametrize("rows", [0, 1, RG - 1, RG, RG + 1, 10 * RG + 5])
def test_partitions_tile_the_rows_on_row_groups(core, rows, ctxs):
    n, bounds = split(core, rows, ctxs)
    units = -(-rows // RG)
    assert n == max(1, min(ctxs, units))
    assert bounds[0] == 0 and bounds[-1] == rows and bounds == sorted(bounds)  # the ranges tile [0, rows)
    assert all(b % RG == 0 and b % 64 == 0 for b in bounds[1:-1])
    if rows:
        assert all(b > a for a, b in zip(bounds, bounds[1:]))  # no empty partition


@pytest.mark.parametrize("rows,ctxs", [(0, 2), (1, 1), (RG + 1, 2), (10 * RG + 5, 3), (10 * RG + 5, 8)])
def test_delete_lists_equal_a_brute_force_split(core, rows, ctxs):
    rng = np.random.default_rng(rows % 1000 + ctxs)
    n, bounds = split(core, rows, ctxs)
    base = np.array(bounds[:-1], dtype=np.uint64)
    n_present = max(0, rows - 7)  # the snapshot is shorter than the table: the tail is deleted too
    present = (rng.random(n_present) > 0.01).astype(np.uint8)
    if n_present > 2 * RG:
        present[RG - 3:RG + 3] = 0  # a run of deletes across a partition boundary
    out = np.zeros(max(rows, 1), dtype=np.int64)
    counts = np.zeros(n, dtype=np.uint64)
    core.csc_local_deletes(present.ctypes.data, n_present, rows, base.ctypes.data, n, out.ctypes.data,
                           counts.ctypes.data)
    gone = [r for r in range(rows) if r >= n_present or not present[r]]
    at = 0
    for p in range(n):
        want = [r - bounds[p] for r in gone if bounds[p] <= r < bounds[p + 1]]
        assert out[at:at + int(counts[p])].tolist() == want, p
        at += int(counts[p])
    assert at == len(gone)


# ------------------------------------------------------------------ small helpers

def test_few_distinct_counts_valid_rows_only(core):
    v = np.arange(600, dtype=np.int64)
    all_valid = np.full(10, ~np.uint64(0), dtype=np.uint64)
    assert core.csc_few_distinct(v.ctypes.data, all_valid.ctypes.data, 256) == 1
    assert core.csc_few_distinct(v.ctypes.data, all_valid.ctypes.data, 257) == 0
    some = all_valid.copy()
    some[4:] = 0  # rows 256 … are NULL: their values do not count
    assert core.csc_few_distinct(v.ctypes.data, some.ctypes.data, 600) == 1


def test_sample_rows(core):
    def sample(valid_mask):
        words = np.append(validity_from_mask(valid_mask), np.uint64(0))  # never empty
        out = np.zeros(4096, dtype=np.int64)
        k = core.csc_sample_rows(words.ctypes.data, len(valid_mask), out.ctypes.data)
        return out[:k].tolist()

    assert sample(np.zeros(0, bool)) == []
    assert sample(np.ones(100, bool)) == list(range(100))
    m = np.ones(5000, bool)  # stride 1: the first 4,096 valid rows
    m[10] = False
    assert sample(m) == [r for r in range(5000) if r != 10][:4096]
    m = np.ones(3 * 4096 + 5, bool)  # stride 3
    m[6] = False
    assert sample(m) == [r for r in range(0, 3 * 4096 + 5, 3) if r != 6][:4096]


def test_pack_strings(core):
    strs = [b"abc", b"", b"\xc3\xa9", b"xyz0"]
    joined = b"\x1f".join(strs)
    data = C.create_string_buffer(len(joined) + 1)
    offs = np.zeros(len(strs) + 1, dtype=np.uint64)
    assert core.csc_pack_strings(joined, len(joined), data, offs.ctypes.data) == len(strs)
    assert offs.tolist() == [0, 3, 3, 5, 9] and data.raw[:9] == b"".join(strs)


# ------------------------------------------------------------------ index specification

def split_spec(lib, spec):
    items, bad = C.create_string_buffer(4096), C.create_string_buffer(256)
    st = lib.csc_split_index_spec(spec.encode(), items, 4096, bad, 256)
    assert st >= 0
    recs = [r.split("\x1f") for r in items.value.decode().split("\x1e")] if items.value else []
    return st, [(r[0], int(r[1]), r[2:]) for r in recs], bad.value.decode()


def test_index_spec_examples_parse(core):
    st, items, _ = split_spec(core, "l_shipdate=range:1994-01-01,1995-01-01;l_shipdate=bins:1992-01-01,1993-01-01;"
                                    "l_discount=range")
    assert st == 0 and items == [("l_shipdate", L.INDEX_RANGE, ["1994-01-01", "1995-01-01"]),
                                 ("l_shipdate", L.INDEX_BINS, ["1992-01-01", "1993-01-01"]),
                                 ("l_discount", L.INDEX_RANGE, [])]
    st, items, _ = split_spec(core, "l_discount=range;l_quantity=equality")
    assert st == 0 and items == [("l_discount", L.INDEX_RANGE, []), ("l_quantity", L.INDEX_EQUALITY, [])]


def test_index_spec_tolerates_whitespace_and_empty_items(core):
    st, items, _ = split_spec(core, " ; a = RANGE : 1 , 2 ;;\tb=Bins:x,y ; ")
    assert st == 0 and items == [("a", L.INDEX_RANGE, ["1", "2"]), ("b", L.INDEX_BINS, ["x", "y"])]
    assert split_spec(core, "") == (0, [], "") and split_spec(core, " ;; ") == (0, [], "")
    # a ':' with nothing after it names no key; an empty literal between commas is kept for the cast to refuse
    assert split_spec(core, "a=range:")[1] == [("a", L.INDEX_RANGE, [])]
    assert split_spec(core, "a=range:1,,2")[1] == [("a", L.INDEX_RANGE, ["1", "", "2"])]
    # the right trim is DuckDB's StringUtil::RTrim, which also takes trailing bytes of 0x80 and above
    assert split_spec(core, "s=equality:é t ,café")[1] == [("s", L.INDEX_EQUALITY, ["é t", "caf"])]


def test_index_spec_reports_the_offending_item(core):
    st, items, bad = split_spec(core, "a=range; l_discount range ;b=bins:1,2")
    assert st == 1 and bad == "l_discount range"  # no '=': the item
    assert items == [("a", L.INDEX_RANGE, [])]  # the items before it
    st, items, bad = split_spec(core, "a=range;b= Bitmap :1,2")
    assert st == 2 and bad == "bitmap" and items == [("a", L.INDEX_RANGE, [])]  # the encoding, as the message prints it
    assert split_spec(core, "a=")[0] == 2


def sort_keys(lib, type_, keys):
    a = np.array(keys, dtype=np.int64)
    n = lib.csc_sort_keys(type_, a.ctypes.data, len(a))
    return a[:n].tolist()


def test_double_keys_sort_by_value(core):
    vals = [3.5, -2.0, 1e300, -1e300, -0.0, 0.0, 3.5, np.inf, -np.inf, 1.0]
    bits = np.array(vals, dtype=np.float64).view(np.int64).tolist()
    got = sort_keys(core, L.TYPE_DOUBLE, bits)
    back = np.array(got, dtype=np.int64).view(np.float64).tolist()
    assert back == sorted(set(vals))  # ascending by value, negatives first; 3.5 once; one zero
    # -0.0 and +0.0 share one comparison key (cubit_fp_key): they merge, and what stays is one of them
    zero = [b for b in got if b in (0, -2 ** 63)]
    assert len(zero) == 1
    # as plain integers the negative patterns would sort the other way round
    assert sort_keys(core, L.TYPE_INT64, [5, -7, 5, 0]) == [-7, 0, 5]
    nan, nan2 = 0x7FF8000000000000, 0x7FF8000000000001
    got = sort_keys(core, L.TYPE_DOUBLE, [nan, np.array([np.inf]).view(np.int64)[0], nan2])
    assert len(got) == 2 and got[1] in (nan, nan2)  # every NaN is one key, above +inf
    # UBIGINT bits sort unsigned
    assert sort_keys(core, L.TYPE_UINT64, [-1, 5, -2 ** 63, 0]) == [0, 5, -2 ** 63, -1]


def test_string_keys_sort_by_bytes(core):
    keys = [b"b", b"a", b"\xc3\xa9", b"B", b"a", b"ab", b"~"]
    joined = b"\x1f".join(keys)
    out = C.create_string_buffer(256)
    n = C.c_uint64(0)
    assert core.csc_sort_string_keys(joined, len(joined), out, 256, C.byref(n)) == 0
    assert out.raw[:n.value].split(b"\x1f") == sorted(set(keys))  # unsigned byte order


def test_bins_need_two_edges(core):
    assert core.csc_enough_keys(L.INDEX_BINS, 0) == 0 and core.csc_enough_keys(L.INDEX_BINS, 1) == 0
    assert core.csc_enough_keys(L.INDEX_BINS, 2) == 1
    assert core.csc_enough_keys(L.INDEX_RANGE, 0) == 1 and core.csc_enough_keys(L.INDEX_EQUALITY, 1) == 1


# ------------------------------------------------------------------ bounds, under AddressSanitizer

@pytest.fixture(scope="module")
def bounds_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("shim_core_bounds")
    exe = d / "shim_core_bounds"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(PKG / "shim"), str(ROOT / "tests" / "shim_core_bounds.cpp"),
                    "-o", str(exe)], check=True)
    return d, exe


@pytest.mark.parametrize("s", FTS + V64, ids=lambda s: s["name"].replace(" ", "_"))
def test_no_read_past_room(bounds_program, s):
    """tests/shim_core_bounds.cpp, a stand-alone program: SegmentImageSize on the first `room` bytes
    of the segment in a heap buffer of exactly `room` bytes, for every room from 0 to its size - 1,
    refuses (and AddressSanitizer sees no read past the buffer); with the whole segment it accepts."""
    d, exe = bounds_program
    raw = bytes.fromhex(s["segment_hex"])
    f = d / "segment.bin"
    f.write_bytes(raw)
    codec = CODEC[s.get("compression", "bitpacking")]
    width = np.dtype(s.get("dtype", "int64")).itemsize
    r = subprocess.run([str(exe), str(f), str(codec), str(s["count"]), str(width)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"refused {len(raw)} truncations, accepted {len(raw)} bytes" in r.stdout
