"""A context's launch tuning (Engine::tune_, csrc/kernels.hpp: struct LaunchTuning) is read at ITS load and belongs to it: no later load, no earlier load and no
test-library setter changes it."""
import ctypes

import numpy as np
import pytest

from test_cpu_launch_tuning import DEFAULTS, FIELDS, SWITCHES

pytestmark = pytest.mark.gpu

PROMPT = [1, 17, 300, 41, 5, 260, 99, 8]                           # 8 rows: the prompt mat-mul kernels (N >= 5), one chunk
FIVE = {"MINIGPT4_ATTN_PREFILL_W8": "0", "MINIGPT4_SPLITK_XCD": "0", "MINIGPT4_ATTN_QT": "2", "MINIGPT4_F16_KS": "2", "MINIGPT4_MMQH": "1"}


def context_tuning(lib, ctx):
    f = lib.library.minigpt4_amd_test_context_tuning
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    f.restype = ctypes.c_int
    out = (ctypes.c_int * len(FIELDS))()
    assert f(ctx.ptr, out, len(FIELDS)) == len(FIELDS)
    t = dict(zip(FIELDS, out))
    assert t["cus"] > 0
    return t


def _load(lib, tiny_files):
    vp, llm = tiny_files
    return lib.minigpt4_model_load(vp, llm("q5_k"), verbosity=1, n_ctx=64, n_batch=32)


def _prompt_logits(lib, ctx):
    lib.minigpt4_reset_chat(ctx)
    lib.amd_eval_tokens(ctx, PROMPT)
    return lib.amd_logits(ctx)


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_two_live_contexts_keep_their_own_tuning(gpu_lib, tiny_files, clean_env):
    a = _load(gpu_lib, tiny_files)
    b = None
    try:
        cus = context_tuning(gpu_lib, a)["cus"]
        assert context_tuning(gpu_lib, a) == dict(DEFAULTS, cus=cus)
        before = _prompt_logits(gpu_lib, a)
        for k, v in FIVE.items():
            clean_env.setenv(k, v)
        b = _load(gpu_lib, tiny_files)
        assert context_tuning(gpu_lib, a) == dict(DEFAULTS, cus=cus)
        assert context_tuning(gpu_lib, b) == dict(DEFAULTS, cus=cus, attn_prefill_w8=0, splitk_xcd=0, attn_vit_qt=2, f16_ks=2, mmqh=1)
        lb = _prompt_logits(gpu_lib, b)
        assert np.isfinite(lb).all()
        after = _prompt_logits(gpu_lib, a)                           # after B's load AND B's prompt pass
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32)), float(np.abs(before - after).max())
    finally:
        gpu_lib.minigpt4_free(a)
        if b is not None:
            gpu_lib.minigpt4_free(b)


def test_a_switch_does_not_outlive_the_context_that_read_it(gpu_lib, tiny_files, clean_env):
    clean_env.setenv("MINIGPT4_ATTN_PREFILL_W8", "0")
    ctx = _load(gpu_lib, tiny_files)
    try:
        assert context_tuning(gpu_lib, ctx)["attn_prefill_w8"] == 0
    finally:
        gpu_lib.minigpt4_free(ctx)
    clean_env.delenv("MINIGPT4_ATTN_PREFILL_W8")
    ctx = _load(gpu_lib, tiny_files)
    try:
        assert context_tuning(gpu_lib, ctx)["attn_prefill_w8"] == 1
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_the_test_library_setters_reach_no_context(gpu_lib, tiny_files, clean_env):
    L = gpu_lib.library
    L.minigpt4_amd_test_set_gemm_arm.argtypes = [ctypes.c_int, ctypes.c_int]
    L.minigpt4_amd_test_set_gemm_arm.restype = None
    try:
        L.minigpt4_amd_test_set_gemm_arm(5, 0)
        L.minigpt4_amd_test_set_splitk_xcd(0)
        ctx = _load(gpu_lib, tiny_files)
        try:
            t = context_tuning(gpu_lib, ctx)
            assert t["gemm_arm"] == 0 and t["splitk_xcd"] == 1
            assert t == dict(DEFAULTS, cus=t["cus"])
        finally:
            gpu_lib.minigpt4_free(ctx)
    finally:
        L.minigpt4_amd_test_set_gemm_arm(0, 0)
        L.minigpt4_amd_test_set_splitk_xcd(1)
