"""Scoring given tokens without a device: the two entry points ship in the product library and refuse a missing context with their name in the error text, the
kernel hook ships in the test library only and refuses every bad argument before it touches a device, the headers declare each where it belongs, and the Python layer
exposes them."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_score_tokens", "minigpt4_amd_score_batch")
HOOK = "minigpt4_amd_test_logprob_rows"
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


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
    tok, cnt, sl = np.array([1, 2], np.int32), np.array([2], np.int32), np.array([0], np.int32)
    lp = np.zeros(2, np.float32)
    assert L.minigpt4_amd_score_tokens(None, tok.ctypes.data_as(I32P), 2, lp.ctypes.data_as(F32P), None, None, None) == 1
    assert b"score_tokens" in L.minigpt4_amd_last_error()
    assert L.minigpt4_amd_score_batch(None, sl.ctypes.data_as(I32P), 1, tok.ctypes.data_as(I32P), cnt.ctypes.data_as(I32P), lp.ctypes.data_as(F32P), None, None) == 1
    assert b"score_batch" in L.minigpt4_amd_last_error()


def test_hook_refuses_bad_arguments_without_a_device(lib):
    T = lib.library.minigpt4_amd_test_logprob_rows
    lg = np.zeros((2, 8), np.float32)
    lp, gr, glp = np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(2, np.float32)

    def call(rows=2, n_vocab=8, ld=8, targets=(0, 7), logits=lg.ctypes.data_as(F32P), tp=True, lpp=lp.ctypes.data_as(F32P), grp=gr.ctypes.data_as(I32P),
             glpp=glp.ctypes.data_as(F32P)):
        t = np.array(targets, np.int32)
        return T(logits, rows, n_vocab, ld, t.ctypes.data_as(I32P) if tp else None, lpp, grp, glpp, None)
    assert call(logits=None) == 1
    assert call(tp=False) == 1
    assert call(lpp=None) == 1
    assert call(grp=None) == 1
    assert call(glpp=None) == 1
    assert call(rows=0) == 1
    assert call(n_vocab=0) == 1
    assert call(n_vocab=8, ld=7) == 1                         # ld < n_vocab
    assert call(targets=(0, 8)) == 1                          # a target of n_vocab
    assert call(targets=(-2, 0)) == 1                         # below "no target"
    assert call(n_vocab=6, targets=(0, 6)) == 1               # inside the stride, outside the vocabulary


def test_python_layer_exposes_scoring():
    from minigpt4_cpp_amd import minigpt4_library as ML
    for name in ("amd_score_tokens", "amd_score_batch", "amd_test_logprob_rows"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    assert inspect.signature(ML.MiniGPT4SharedLibrary.amd_score_tokens).parameters["want_logits"].default is False
