"""Context shift, the parts that need no GPU: both libraries export the new entry points, the public header declares them, and the NULL-context checks answer
without touching a device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_shift_context", "minigpt4_amd_set_context_shift")
HOOK = "minigpt4_amd_test_kv_shift"


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", txt))


def test_product_exports_and_declares_the_context_shift(lib):
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    declared = _declared("minigpt4_amd.h")
    for name in PRODUCT:
        assert name in product, name
        assert name in declared, name
    assert HOOK not in product and HOOK not in declared


def test_test_library_exports_the_kernel_hook(lib):
    test = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    assert HOOK in test
    assert HOOK in _declared("minigpt4_amd_test.h")


def test_null_context_is_refused(lib):
    L = lib.library
    assert L.minigpt4_amd_shift_context(None, 0, 1) == 1
    assert b"no context" in L.minigpt4_amd_last_error()
    assert L.minigpt4_amd_set_context_shift(None, 0) == 1
    assert L.minigpt4_amd_set_context_shift(None, -1) == 1


def test_hook_refuses_bad_shapes_without_a_device(lib):
    import numpy as np
    k = np.zeros((1, 8, 64), np.float16)
    v = np.zeros_like(k)
    kp, vp = k.ctypes.data, v.ctypes.data
    T = lib.library.minigpt4_amd_test_kv_shift
    assert T(1, 8, 64, 4, 9, 0, 1, kp, vp, None) == 1       # n_rows > n_ctx
    assert T(1, 8, 64, 4, 8, 5, 4, kp, vp, None) == 1       # n_keep + n_discard > n_rows
    assert T(1, 8, 64, 4, 8, -1, 1, kp, vp, None) == 1
    assert T(1, 8, 64, 16, 8, 0, 1, kp, vp, None) == 1      # head size 4: a 16-byte column group would span two heads
    assert T(1, 8, 64, 4, 8, 0, 1, None, vp, None) == 1
