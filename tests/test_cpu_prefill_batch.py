"""minigpt4_amd_prefill_batch without a device: the symbol ships in the product library, refuses a missing context / slot list with an error text, and the Python
layers expose it (minigpt4_library.amd_prefill_batch, serve.ReplicaServer.run(batched_prefill=...))."""
import ctypes
import inspect
import os

import numpy as np


def test_prefill_batch_symbol_and_argument_checks(lib):
    L = lib.library
    assert hasattr(L, "minigpt4_amd_prefill_batch")
    slots = np.array([0, 1], np.int32)
    assert L.minigpt4_amd_prefill_batch(None, slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2) == 1
    assert b"prefill_batch" in L.minigpt4_amd_last_error()


def test_prefill_batch_declared_in_public_header_only():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "minigpt4_amd.h")).read()
    test = open(os.path.join(root, "include", "minigpt4_amd_test.h")).read()
    assert "minigpt4_amd_prefill_batch(" in pub and "minigpt4_amd_prefill_batch(" not in test
    assert "minigpt4_amd_test_attn_prefill_seg(" in test and "minigpt4_amd_test_rope_kv_seg(" in test
    assert "minigpt4_amd_test_attn_prefill_seg(" not in pub


def test_python_layers_expose_prefill_batch():
    from minigpt4_cpp_amd import minigpt4_library as ML, serve as SV
    assert callable(getattr(ML.MiniGPT4SharedLibrary, "amd_prefill_batch"))
    p = inspect.signature(SV.ReplicaServer.run).parameters["batched_prefill"]
    assert p.default is False
