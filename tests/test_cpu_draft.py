"""Draft verification and lookup decoding without a device: the three entry points ship in the product library and refuse a missing context with their name in the
error text, the two hooks ship in the test library only, the attention hook refuses every bad argument before it touches a device, and the host drafter follows its
rule (restated here in a few lines of Python) on random histories and on hand-made cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_set_speculation", "minigpt4_amd_verify_draft", "minigpt4_amd_decode_lookup")
HOOKS = ("minigpt4_amd_test_attn_draft", "minigpt4_amd_test_ngram_draft")
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
    for hook in HOOKS:
        assert hook not in product and hook not in declared, hook
    assert not ((set(PRODUCT) | set(HOOKS)) & _declared("minigpt4.h"))       # the reference header is untouched


def test_test_library_exports_the_hooks(lib):
    exported = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    for hook in HOOKS:
        assert hook in exported, hook
        assert hook in _declared("minigpt4_amd_test.h"), hook


def test_null_context_is_refused_with_the_function_name(lib):
    L = lib.library
    d, ids, n, rg, st = np.array([1, 3], np.int32), np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(8, np.int32), np.zeros(4, np.int32)
    ip = lambda a: a.ctypes.data_as(I32P)
    assert L.minigpt4_amd_set_speculation(None, 4) == 1
    assert L.minigpt4_amd_last_error().startswith(b"set_speculation")
    assert L.minigpt4_amd_verify_draft(None, ip(d), 2, ip(ids), ip(n), ip(rg)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"verify_draft")
    assert L.minigpt4_amd_decode_lookup(None, ip(d), 2, 8, 3, 1, 4, ip(ids), ip(n), ip(st)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"decode_lookup")


def _verify_form_max_ctx(hd):
    """The largest n_ctx (a multiple of 8) whose verify-pass attention launch fits a CU's LDS, from the layout alone: 160 KiB hold 256 bytes of static reduction arrays
    and, dynamically, n_ctx fp32 scores + n_ctx fp16 probabilities (n_ctx padded to 8), the fp16 q row [hd], 8 new key rows and 8 new value rows in fp16 [8][hd] each
    (the one-row forms keep one of each), the fp32 partial outputs [P][hd] of the P = 512 / (hd / 8) key partitions, and 64 spare bytes."""
    fixed = 256 + hd * 2 + 2 * 8 * hd * 2 + (512 // (hd // 8)) * hd * 4 + 64
    return (160 * 1024 - fixed) // (4 + 2) // 8 * 8


def test_attention_hook_refuses_bad_arguments_without_a_device(lib):
    """Every bad argument is refused (1) before a device is looked for (2 on a box without one).  The context bound is the verify form's own, derived in
    _verify_form_max_ctx from the LDS layout: at head size 128 a context of 23 792 rows is accepted as far as the device check and 23 800 is refused, although the
    one-row kernel (and with it the model load) admits 24 392; the same pair at the bound and 8 rows above it holds for head sizes 64 and 32."""
    T = lib.library.minigpt4_amd_test_attn_draft
    n_head, hd, n_ctx, n_slot = 2, 64, 16, 2
    E = n_head * hd
    q = np.zeros((8, E), np.float32)
    kc = np.zeros((n_slot, n_ctx, E), np.uint16)
    out = np.zeros((8, E), np.float32)
    fp, vp = q.ctypes.data_as(F32P), kc.ctypes.data_as(ctypes.c_void_p)
    A = dict(q=fp, k=fp, v=fp, kc=vp, vc=vp, out=out.ctypes.data_as(F32P))

    def call(mode=0, n_head=n_head, hd=hd, n_ctx=n_ctx, n_slot=n_slot, slot=1, n_past=4, R=3, **kw):
        a = dict(A, **kw)
        return T(mode, n_head, hd, n_ctx, n_slot, slot, n_past, R, 1, a["q"], a["k"], a["v"], a["kc"], a["vc"], a["out"])
    for name in A:
        assert call(**{name: None}) == 1, name                # a NULL array
    assert call(mode=2) == 1 and call(mode=-1) == 1
    assert call(hd=48) == 1 and call(hd=256) == 1 and call(hd=0) == 1
    assert call(n_head=0) == 1
    assert call(n_slot=0) == 1
    assert call(slot=2) == 1 and call(slot=-1) == 1
    assert call(R=0) == 1 and call(R=9) == 1
    assert call(n_past=-1) == 1
    assert call(n_past=14, R=3) == 1                          # the last row would sit at position n_ctx
    assert call(n_past=16, R=1) == 1
    assert call(n_ctx=1 << 24, n_past=0) == 1                 # more score rows than the kernel's LDS holds
    assert _verify_form_max_ctx(128) == 23792
    no_device = lib.amd_device_count() <= 0
    for hd_ in (128, 64, 32):
        fits = _verify_form_max_ctx(hd_)
        if no_device:
            assert call(hd=hd_, n_ctx=fits, n_past=0) == 2, (hd_, fits)       # accepted as far as the device check (the arrays are never touched)
        assert call(hd=hd_, n_ctx=fits + 8, n_past=0) == 1, (hd_, fits)       # 8 rows more: the launch would not fit


def ref_draft(h, ngram_max, ngram_min, n_draft):
    """The rule of include/minigpt4_amd.h: the longest suffix (ngram_max .. ngram_min tokens) that occurs earlier, its most recent occurrence; the tokens behind that
    occurrence up to n_draft, before any id 2, up to the end of the history."""
    n = len(h)
    for L in range(min(ngram_max, n - 1), ngram_min - 1, -1):
        for s in range(n - L - 1, -1, -1):
            if h[s:s + L] == h[n - L:]:
                out = []
                for t in h[s + L:]:
                    if len(out) >= n_draft or t == 2:
                        break
                    out.append(t)
                return out
    return []


def test_drafter_follows_the_rule_on_random_histories(lib):
    rng = np.random.default_rng(7)
    some = 0
    for case in range(200):
        h = [int(x) for x in rng.integers(0, 8, 200)]
        ngram_min = int(rng.integers(1, 4))
        ngram_max = ngram_min + int(rng.integers(0, 4))
        n_draft = int(rng.integers(1, 8))
        got = lib.amd_test_ngram_draft(h, ngram_max, ngram_min, n_draft)
        assert got == ref_draft(h, ngram_max, ngram_min, n_draft), (case, h, ngram_max, ngram_min, n_draft)
        some += bool(got)
    assert some > 100                                          # the cases exercise matches, not only misses


def test_drafter_hand_made_cases(lib):
    D = lib.amd_test_ngram_draft
    assert D([5, 6, 7], 3, 1, 4) == []                                         # no match
    assert D([], 3, 1, 4) == [] and D([5], 3, 1, 4) == []
    assert D([5, 5], 3, 1, 4) == [5]                                           # the occurrence may end right in front of the suffix
    assert D([1, 3, 9, 4, 3, 7, 5, 1, 3], 2, 1, 3) == [9, 4, 3]                # the 2-gram (1, 3) at 0 beats the more recent 1-gram (3) at 4
    assert D([1, 3, 9, 4, 3, 7, 5, 1, 3], 1, 1, 3) == [7, 5, 1]                # ... which wins when only 1-grams are tried
    assert D([1, 3, 9, 4, 3, 7, 5, 1, 3], 4, 3, 3) == []                       # ngram_min above every match
    assert D([3, 4, 0, 3, 5, 0, 3], 1, 1, 3) == [5, 0, 3]                      # the most recent among equal lengths
    assert D([3, 4, 2, 6, 3], 2, 1, 4) == [4]                                  # cut before id 2
    assert D([3, 2, 6, 3], 2, 1, 4) == []                                      # ... also when it follows at once
    assert D([3, 4, 5, 6, 3], 1, 1, 2) == [4, 5]                               # cut at n_draft
    assert D([3, 4, 5, 6, 3], 1, 1, 7) == [4, 5, 6, 3]                         # cut at the end of the history
    assert D([3, 4, 5, 6, 3], 1, 1, 0) == []
    with pytest.raises(ValueError):
        D([3, 4], 1, 2, 3)                                                     # ngram_max < ngram_min
    with pytest.raises(ValueError):
        D([3, 4], 2, 0, 3)


def test_python_layer_exposes_speculation():
    from minigpt4_cpp_amd import minigpt4_library as ML
    C = ML.MiniGPT4SharedLibrary
    for name in ("amd_set_speculation", "amd_verify_draft", "amd_decode_lookup", "amd_test_attn_draft", "amd_test_ngram_draft"):
        assert callable(getattr(C, name)), name
