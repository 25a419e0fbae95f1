"""Quantile indexes without a GPU: the `column=encoding~count` items of the shim's index
specification (through the core's C surface), the Python declaration of
cubit_table_build_index_quantiles, and the header-to-export rule for the new symbol."""
import ctypes as C

import pytest

import test_abi
from cubit_amd import _lib as L
from test_shim_core import core, split_spec  # noqa: F401  (core: the fixture)

OK, MISSING_EQUALS, UNKNOWN_ENCODING, BAD_COUNT = 0, 1, 2, 3


def split_counts(lib, spec):
    """(status, each item's bin count, the offending text) from csc_split_index_spec_counts."""
    lib.csc_split_index_spec_counts.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64]
    counts = (C.c_uint32 * 16)()
    n = C.c_uint64()
    bad = C.create_string_buffer(256)
    st = lib.csc_split_index_spec_counts(spec.encode(), counts, 16, C.byref(n), bad, 256)
    assert st >= 0
    return st, [int(counts[i]) for i in range(min(16, n.value))], bad.value.decode()


def test_counts_split_beside_literal_lists(core):
    spec = "a=range~64;b=bins~8;c=range:1,2"
    assert split_counts(core, spec) == (OK, [64, 8, 0], "")
    # the record format of csc_split_index_spec is as it was: name, encoding, literals
    assert split_spec(core, spec) == (OK, [("a", L.INDEX_RANGE, []), ("b", L.INDEX_BINS, []),
                                           ("c", L.INDEX_RANGE, ["1", "2"])], "")
    assert split_counts(core, "a=range~2;b=bins~1024") == (OK, [2, 1024], "")
    assert split_counts(core, "l_discount=range;l_quantity=equality") == (OK, [0, 0], "")
    assert split_counts(core, "") == (OK, [], "")


@pytest.mark.parametrize("spec,status,bad", [
    ("a=range~1", BAD_COUNT, "1"),
    ("a=range~1025", BAD_COUNT, "1025"),
    ("a=range~x", BAD_COUNT, "x"),
    ("a=range~", BAD_COUNT, ""),
    ("a=bins~-8", BAD_COUNT, "-8"),
    ("a=bins~+8", BAD_COUNT, "+8"),
    ("a=bins~8.0", BAD_COUNT, "8.0"),
    ("a=range~99999999999999999999", BAD_COUNT, "99999999999999999999"),
    ("a=range~8:1,2", BAD_COUNT, "8:1,2"),     # a count and a literal list exclude each other
    ("a=equality~8", UNKNOWN_ENCODING, "equality~8"),  # an equality index takes no count
    ("a=bitmap~8", UNKNOWN_ENCODING, "bitmap~8"),
    ("a=~8", UNKNOWN_ENCODING, "~8"),
])
def test_bad_counts_are_reported_with_their_text(core, spec, status, bad):
    st, counts, text = split_counts(core, "z=bins~4;" + spec + ";y=range")
    assert (st, text) == (status, bad)
    assert counts == [4]  # the items before the offending one
    assert split_spec(core, "z=bins~4;" + spec)[0] == status  # both functions split alike


def test_counts_take_whitespace_and_letter_case_as_the_other_items_do(core):
    assert split_counts(core, " ; a = RANGE ~ 64 ;;\tb=Bins~\t8 ; c = range : 1 , 2 ") == (OK, [64, 8, 0], "")
    assert split_spec(core, " a = RANGE ~ 64 ")[1] == [("a", L.INDEX_RANGE, [])]
    assert split_counts(core, "a=range~064") == (OK, [64], "")
    assert split_counts(core, "a=range~6 4")[0] == BAD_COUNT
    # a '~' after the ':' belongs to a literal
    assert split_counts(core, "s=equality:a~b,~") == (OK, [0], "")
    assert split_spec(core, "s=equality:a~b,~")[1] == [("s", L.INDEX_EQUALITY, ["a~b", "~"])]


def test_python_declares_the_symbol():
    restype, argtypes = L.GPU_SIGNATURES["cubit_table_build_index_quantiles"]
    assert restype is C.c_int and len(argtypes) == 7
    assert argtypes[3] is C.c_uint32 and argtypes[5] is C.c_uint32
    fn = L.gpu_lib().cubit_table_build_index_quantiles
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert fn(None, 0, L.INDEX_RANGE, 64, None, 0, None) == L.ERR_INVALID  # a null table: a status, no GPU
    from cubit_amd.table import CubitTable
    assert callable(CubitTable.build_index_quantiles)


def test_header_declares_it_and_the_library_exports_it():
    names = test_abi.declared(test_abi.ROOT / "include" / "cubit_gpu.h")
    assert "cubit_table_build_index_quantiles" in names
    assert "cubit_table_build_index_quantiles" in L.exported_symbols(L.GPU_LIB)
    test_abi.test_every_declared_symbol_is_exported()
