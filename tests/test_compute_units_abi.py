"""The compute-unit override and the last-grid report without a GPU: the header declares the three
entry points, the library exports them, Python declares their signatures, and a null context or a null
output is a status code."""
import ctypes as C

import test_abi
from cubit_amd import _lib as L

NAMES = ["cubit_ctx_set_compute_units", "cubit_ctx_compute_units", "cubit_ctx_last_grid"]


def test_header_declares_them_and_the_library_exports_them():
    declared = test_abi.declared(test_abi.ROOT / "include" / "cubit_gpu.h")
    exported = L.exported_symbols(L.GPU_LIB)
    for name in NAMES:
        assert name in declared and name in exported, name
    assert L.gpu_lib().cubit_abi_version() == 1  # additive: the ABI version stays


def test_python_declares_the_signatures():
    assert L.GPU_SIGNATURES["cubit_ctx_set_compute_units"] == (C.c_int, [C.c_void_p, C.c_int])
    restype, argtypes = L.GPU_SIGNATURES["cubit_ctx_compute_units"]
    assert restype is C.c_int and len(argtypes) == 3
    restype, argtypes = L.GPU_SIGNATURES["cubit_ctx_last_grid"]
    assert restype is C.c_int and len(argtypes) == 3
    from cubit_amd.table import Context
    assert all(callable(getattr(Context, m)) for m in ("set_compute_units", "compute_units", "last_grid"))


def test_null_arguments_are_status_codes():
    lib = L.gpu_lib()
    a, b = C.c_int(), C.c_int()
    wg, tiles = C.c_uint32(), C.c_uint32()
    for n in (0, 1, -1):
        assert lib.cubit_ctx_set_compute_units(None, n) == L.ERR_INVALID
    assert lib.cubit_ctx_compute_units(None, C.byref(a), C.byref(b)) == L.ERR_INVALID
    assert lib.cubit_ctx_last_grid(None, C.byref(wg), C.byref(tiles)) == L.ERR_INVALID
    assert b"null" in lib.cubit_last_error()
