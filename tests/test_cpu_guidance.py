"""Guided decoding without a device: where the entry points and the hook live, the refusals that come before anything runs (C ABI, binding, kernel hook) and the
serving layer's arguments.  The arithmetic runs on the device only: tests/test_gpu_guidance.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("minigpt4_amd_end_chat_guided", "minigpt4_amd_guided_logits", "minigpt4_amd_guidance_info")
HOOK = "minigpt4_amd_test_guide_rows"
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def _declared(header):
    return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_entry_points_and_hook_are_where_they_belong(lib):
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    test = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    for name in ENTRY:
        assert name in product and name in test and name in _declared("minigpt4_amd.h"), name
    assert HOOK in test and HOOK not in product
    assert HOOK in _declared("minigpt4_amd_test.h") and HOOK not in _declared("minigpt4_amd.h")


def test_refusals_on_a_null_context_carry_the_short_names(lib):
    L = lib.library
    a, b = np.array([0], np.int32), np.array([1], np.int32)
    toks, ids, info = (ctypes.c_char_p * 1)(), np.zeros(1, np.int32), np.zeros(4, np.int32)
    ip = lambda x: x.ctypes.data_as(I32P)
    assert L.minigpt4_amd_end_chat_guided(None, ip(a), ip(b), 1, 1.5, toks, 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0, ip(ids)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"end_chat_guided: no context")
    assert L.minigpt4_amd_guided_logits(None, ip(a), ip(b), 1, 1.5, None, ip(ids)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"guided_logits: no context")
    assert L.minigpt4_amd_guidance_info(None, ip(info)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"guidance_info: no context")
    with pytest.raises(RuntimeError, match="end_chat_guided"):
        lib.amd_end_chat_guided(None, [0], [1], 1.5)
    with pytest.raises(RuntimeError, match="guided_logits"):
        lib.amd_guided_logits(None, [0], [1], 1.5)
    with pytest.raises(RuntimeError, match="guidance_info"):
        lib.amd_guidance_info(None)


@pytest.mark.parametrize("call", ["amd_end_chat_guided", "amd_guided_logits"])
def test_binding_refuses_before_the_library_is_touched(lib, call):
    f = getattr(lib, call)
    name = call[len("amd_"):]
    for slots, neg, scale in (([0, 2], [1], 1.5),                  # unequal lengths
                              ([0, 1], [2, 1], 1.5),               # a slot in both lists
                              ([0, 0], [1, 2], 1.5),               # a slot twice in one list
                              ([], [], 1.5),                       # empty
                              ([0], [1], float("inf")), ([0], [1], float("nan")), ([0], [1], 1e39),   # not finite (1e39: not as the float the library takes)
                              ([0], [-1], 1.5),
                              (list(range(33)), list(range(33, 66)), 1.5)):
        with pytest.raises(ValueError, match=name):
            f(None, slots, neg, scale)                             # ctx None: reaching the library would raise RuntimeError instead


def test_hook_refuses_before_it_looks_for_a_device(lib):
    H = lib.library.minigpt4_amd_test_guide_rows
    lg = np.zeros((3, 40), np.float32)
    mixed, pick, val, rt = np.zeros((2, 32), np.float32), np.zeros(2, np.int32), np.zeros(2, np.float32), np.zeros(64, np.int32)
    ip, fp = (lambda x: x.ctypes.data_as(I32P)), (lambda x: x.ctypes.data_as(F32P))

    def rc(logits=lg, buf_rows=3, n_vocab=32, ld=40, pairs=(0, 1, 2, 2), scales=(1.5, 0.0), tok=(0, 1, -1, -1), n=2, pick_=pick, val_=val, rt_=rt):
        pr, sc, ti = np.array(pairs, np.int32), np.array(scales, np.float32), np.array(tok, np.int32)
        return H(None if logits is None else fp(logits), buf_rows, n_vocab, ld, ip(pr), fp(sc), ip(ti), n, fp(mixed), None if pick_ is None else ip(pick_),
                 None if val_ is None else fp(val_), None if rt_ is None else ip(rt_), None)
    for kw in (dict(logits=None), dict(pairs=(0, 3, 2, 2)), dict(pairs=(-1, 1, 2, 2)), dict(n=0), dict(n=33), dict(ld=31), dict(n_vocab=0), dict(buf_rows=0),
               dict(tok=(0, 64, -1, -1)), dict(tok=(0, 1, -2, -1)), dict(pick_=None), dict(val_=None), dict(rt_=None)):
        assert rc(**kw) == 1, kw
    assert rc() in (0, 2)                                          # well-formed: runs, or finds no device


def test_python_layer_and_serving_arguments(lib):
    from minigpt4_cpp_amd import minigpt4_library as ML
    from minigpt4_cpp_amd import serve as S
    for name in ("amd_end_chat_guided", "amd_guided_logits", "amd_guidance_info", "amd_test_guide_rows"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    sig = inspect.signature(S.ReplicaServer.run).parameters
    assert sig["guidance_scale"].default == 1.0 and sig["negative_prompt"].default is None
    srv = S.ReplicaServer.__new__(S.ReplicaServer)                 # no model: the checks come before the library is touched
    srv.lib, srv.ctx, srv.conversations = lib, None, 4
    reqs = [S.Request(np.zeros((3, 224, 224), np.float32), "hello", 4)]
    with pytest.raises(ValueError, match="guidance_scale"):
        srv.run(reqs, guidance_scale=1.5, logprobs=1)
    with pytest.raises(ValueError, match="guidance_scale"):
        srv.run(reqs, guidance_scale=1.5, num_beams=2)
    with pytest.raises(ValueError, match="guidance_scale"):
        srv.run(reqs, guidance_scale=float("nan"))
