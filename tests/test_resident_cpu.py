"""CPU: the diagnostic C ABI symbols of the step kernels (qs_debug_chain_resident, qs_debug_step_variant) exist and check their
arguments."""
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


def test_debug_step_variant_rejects_null_arguments():
    """qs_debug_step_variant (which step-kernel instantiation the next step launches) checks its arguments without a GPU"""
    lib = _lib.load()
    lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.qs_last_error.restype = C.c_char_p
    out = (C.c_int32 * 5)(*([7] * 5))
    assert lib.qs_debug_step_variant(None, out) != 0
    assert b"qs_debug_step_variant" in lib.qs_last_error()
    assert list(out) == [7] * 5
    assert lib.qs_debug_step_variant(None, None) != 0
    assert "qs_debug_step_variant" not in _lib.EXPORTS
