"""Top-N alternatives without a device: the four entry points ship in the product library and refuse a missing context with their name in the error text, the
kernel hook ships in the test library only and refuses every bad argument before it touches a device, the headers declare each where it belongs, and the Python layer
exposes them."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_token_piece", "minigpt4_amd_top_logprobs", "minigpt4_amd_end_chat_batch_top", "minigpt4_amd_score_tokens_top")
HOOK = "minigpt4_amd_test_topn_rows"
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
    tok, sl = np.array([1, 2], np.int32), np.array([0], np.int32)
    lp, rk = np.zeros(2, np.float32), np.zeros(2, np.int32)
    ti, tl = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32)
    pieces = (ctypes.c_char_p * 1)()
    ip, fp = (lambda a: a.ctypes.data_as(I32P)), (lambda a: a.ctypes.data_as(F32P))
    assert L.minigpt4_amd_token_piece(None, 0) is None
    assert L.minigpt4_amd_top_logprobs(None, ip(sl), 1, 3, None, ip(ti), fp(tl), None, None) == 1
    assert L.minigpt4_amd_last_error().startswith(b"top_logprobs")
    assert L.minigpt4_amd_end_chat_batch_top(None, ip(sl), 1, pieces, 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0, 3, ip(rk), fp(lp), ip(rk), ip(ti), fp(tl)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"end_chat_batch_top")
    assert L.minigpt4_amd_score_tokens_top(None, ip(tok), 2, 3, fp(lp), ip(rk), ip(ti), fp(tl)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"score_tokens_top")


def test_hook_refuses_bad_arguments_without_a_device(lib):
    T = lib.library.minigpt4_amd_test_topn_rows
    lg = np.zeros((3, 8), np.float32)
    ids, lps, rk, tlp = np.zeros((2, 8), np.int32), np.zeros((2, 8), np.float32), np.zeros(2, np.int32), np.zeros(2, np.float32)
    A = dict(logits=lg.ctypes.data_as(F32P), ids=ids.ctypes.data_as(I32P), lps=lps.ctypes.data_as(F32P), rk=rk.ctypes.data_as(I32P), tlp=tlp.ctypes.data_as(F32P))

    def call(buf_rows=3, rows=2, n_vocab=8, ld=8, top_n=3, targets=(0, 7), row_index=None, tp=True, **kw):
        a = dict(A, **kw)
        t = np.array(targets, np.int32)
        ri = None if row_index is None else np.array(row_index, np.int32)
        return T(a["logits"], buf_rows, n_vocab, ld, None if ri is None else ri.ctypes.data_as(I32P), rows, top_n, t.ctypes.data_as(I32P) if tp else None, a["ids"], a["lps"],
                 a["rk"], a["tlp"], None)
    for name in A:
        assert call(**{name: None}) == 1, name                # a NULL pointer
    assert call(tp=False) == 1
    assert call(rows=0) == 1
    assert call(buf_rows=0) == 1
    assert call(n_vocab=0) == 1
    assert call(n_vocab=8, ld=7) == 1                         # ld < n_vocab
    assert call(top_n=0) == 1
    assert call(top_n=65) == 1
    assert call(top_n=9) == 1                                 # inside 1..64, above n_vocab
    assert call(n_vocab=6, top_n=7) == 1                      # inside the stride, above the vocabulary
    assert call(targets=(0, 8)) == 1                          # a target of n_vocab
    assert call(targets=(-2, 0)) == 1                         # below "no target"
    assert call(n_vocab=6, targets=(0, 6)) == 1               # inside the stride, outside the vocabulary
    assert call(row_index=(0, 3)) == 1                        # a row outside the buffer
    assert call(row_index=(-1, 0)) == 1
    assert call(buf_rows=1) == 1                              # two rows of a one-row buffer, no row_index


def test_python_layer_exposes_top_logprobs():
    from minigpt4_cpp_amd import minigpt4_library as ML
    C = ML.MiniGPT4SharedLibrary
    for name in ("amd_token_piece", "amd_top_logprobs", "amd_end_chat_batch_top", "amd_test_topn_rows", "amd_score_tokens"):
        assert callable(getattr(C, name)), name
    sig = inspect.signature(C.amd_score_tokens).parameters
    assert sig["top_n"].default == 0 and sig["want_logits"].default is False
    assert inspect.signature(C.amd_top_logprobs).parameters["top_n"].default == 5
    assert inspect.signature(C.amd_top_logprobs).parameters["targets"].default is None
    assert inspect.signature(C.amd_end_chat_batch_top).parameters["top_n"].default == 5
    with pytest.raises(ValueError):
        C.amd_score_tokens(None, None, [1, 2], want_logits=True, top_n=3)   # refused before the library is touched
    from minigpt4_cpp_amd import serve as S
    assert inspect.signature(S.ReplicaServer.run).parameters["logprobs"].default == 0
