"""CPU: the diagnostic C ABI symbol of the resident step kernel (qs_debug_chain_resident) exists and checks its arguments."""
import ctypes as C

from quadsim_amd import _lib


def test_debug_chain_resident_rejects_null_arguments():
    lib = _lib.load()
    lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.qs_last_error.restype = C.c_char_p
    d = C.c_uint64(7)
    assert lib.qs_debug_chain_resident(None, C.byref(d)) != 0
    assert b"qs_debug_chain_resident" in lib.qs_last_error()
    assert d.value == 7
    assert lib.qs_debug_chain_resident(None, None) != 0
