"""Conversation fork and the prefix cache without a device: the three entry points ship in the product library and refuse a missing context with their name in the
error text, the kernel hook ships in the test library only, the headers declare each where it belongs, and the Python layers expose them."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_fork_conversation", "minigpt4_amd_set_prefix_cache", "minigpt4_amd_prefix_cache_info")
HOOK = "minigpt4_amd_test_kv_copy"


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", txt))


def test_product_exports_and_declares_the_entry_points(lib):
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    declared = _declared("minigpt4_amd.h")
    for name in PRODUCT:
        assert name in product, name
        assert name in declared, name
        assert name not in _declared("minigpt4_amd_test.h"), name
    assert HOOK not in product and HOOK not in declared
    assert not (set(PRODUCT) & _declared("minigpt4.h"))       # the reference header is untouched


def test_test_library_exports_the_kernel_hook(lib):
    assert HOOK in _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    assert HOOK in _declared("minigpt4_amd_test.h")


def test_null_context_is_refused_with_the_function_name(lib):
    L = lib.library
    dst = np.array([1], np.int32)
    out = (ctypes.c_int32 * 7)()
    assert L.minigpt4_amd_fork_conversation(None, 0, dst.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, -1) == 1
    assert b"fork_conversation" in L.minigpt4_amd_last_error()
    assert L.minigpt4_amd_set_prefix_cache(None, 256) == 1
    assert b"set_prefix_cache" in L.minigpt4_amd_last_error()
    assert L.minigpt4_amd_prefix_cache_info(None, out) == 1
    assert b"prefix_cache_info" in L.minigpt4_amd_last_error()


def test_hook_refuses_bad_arguments_without_a_device(lib):
    k = np.zeros((2, 1, 8, 64), np.float16)
    v = np.zeros_like(k)
    T = lib.library.minigpt4_amd_test_kv_copy
    I32P = ctypes.POINTER(ctypes.c_int32)

    def call(src, dst, n_rows, src_rows=0, kp=k.ctypes.data):
        d = np.array(dst, np.int32)
        return T(2, 1, 8, 64, src, d.ctypes.data_as(I32P), len(d), n_rows, src_rows, kp, v.ctypes.data, None)
    assert call(0, [0], 4) == 1                               # the source among the destinations
    assert call(0, [2], 4) == 1                               # destination out of range
    assert call(2, [1], 4) == 1                               # source out of range
    assert call(0, [1], 4, src_rows=9) == 1                   # compact source longer than the slot
    assert call(0, [1], 4, kp=None) == 1                      # only one of k / v (both NULL = the timing-only form, which needs a device)


def test_python_layers_expose_fork_and_prefix_cache():
    from minigpt4_cpp_amd import minigpt4_library as ML, serve as SV
    for name in ("amd_fork_conversation", "amd_set_prefix_cache", "amd_prefix_cache_info", "amd_test_kv_copy"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    assert inspect.signature(ML.MiniGPT4SharedLibrary.amd_fork_conversation).parameters["n_rows"].default == -1
    assert inspect.signature(SV.ReplicaServer.__init__).parameters["prefix_cache"].default == 0
