"""The verify pass over several conversations without a device: the three entry points ship in the product library and refuse a missing context with their name, the
two hooks ship in the test library only and refuse every bad argument before a device is looked for, the serving loop's Python drafter equals the engine's, the numpy
reference of the epilogue (tests/draft_batch_ref.py) follows its rule on hand-made cases, and ReplicaServer.run(lookup=...) refuses what the greedy raw-logits rule
does not cover."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import draft_batch_ref as B
import greedy_ref as G
from test_cpu_draft import ref_draft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_verify_draft_batch", "minigpt4_amd_decode_lookup_batch", "minigpt4_amd_speculation_batch_info")
HOOKS = ("minigpt4_amd_test_attn_draft_batch", "minigpt4_amd_test_draft_finish_batch")
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
        assert name in product and name in declared, name
        assert name not in _declared("minigpt4_amd_test.h"), name
    for hook in HOOKS:
        assert hook not in product and hook not in declared, hook
    exported = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    for hook in HOOKS:
        assert hook in exported and hook in _declared("minigpt4_amd_test.h"), hook
    assert not ((set(PRODUCT) | set(HOOKS)) & _declared("minigpt4.h"))       # the reference header is untouched
    txt = open(os.path.join(ROOT, "include", "minigpt4_amd.h")).read()
    assert "pass_ms(N) / step_ms(n) - 1" in txt                              # the break-even formula is stated where the calls are declared


def test_null_context_is_refused_with_the_function_name(lib):
    L = lib.library
    a = np.zeros(16, np.int32)
    ip = a.ctypes.data_as(I32P)
    assert L.minigpt4_amd_verify_draft_batch(None, ip, 1, ip, ip, ip, ip, ip) == 1
    assert L.minigpt4_amd_last_error().startswith(b"verify_draft_batch")
    assert L.minigpt4_amd_decode_lookup_batch(None, ip, 1, ip, ip, 8, 3, 1, 4, ip, ip, ip) == 1
    assert L.minigpt4_amd_last_error().startswith(b"decode_lookup_batch")
    assert L.minigpt4_amd_speculation_batch_info(None, (ctypes.c_int64 * 8)()) == 1
    assert L.minigpt4_amd_last_error().startswith(b"speculation_batch_info")
    with pytest.raises(RuntimeError, match="verify_draft_batch"):
        lib.amd_verify_draft_batch(None, [0, 1], [[1], []])
    with pytest.raises(ValueError):
        lib.amd_verify_draft_batch(None, [0, 1], [[1]])                      # one draft per conversation


def test_python_layer_exposes_the_calls():
    from minigpt4_cpp_amd import minigpt4_library as ML
    from minigpt4_cpp_amd import serve as S
    for name in ("amd_verify_draft_batch", "amd_decode_lookup_batch", "amd_speculation_batch_info", "amd_test_attn_draft_batch", "amd_test_draft_finish_batch"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    assert inspect.signature(S.ReplicaServer.run).parameters["lookup"].default == 0
    assert "lookup" in inspect.getsource(S.serve)                            # serve() passes it through


def test_attention_hook_refuses_bad_arguments_without_a_device(lib):
    T = lib.library.minigpt4_amd_test_attn_draft_batch
    n_head, hd, n_ctx, n_slot = 2, 64, 32, 3
    E = n_head * hd
    q = np.zeros((64, E), np.float32)
    kc = np.zeros((n_slot, n_ctx, E), np.uint16)
    fp, vp = q.ctypes.data_as(F32P), kc.ctypes.data_as(ctypes.c_void_p)
    A = dict(q=fp, k=fp, v=fp, kc=vp, vc=vp, out=fp)
    good = [(2, 4, 3), (0, 0, 1)]

    def call(groups=good, mode=0, vs=1, n_head=n_head, hd=hd, n_ctx=n_ctx, n_slot=n_slot, n_groups=None, **kw):
        a = dict(A, **kw)
        g = None if groups is None else np.ascontiguousarray(groups, np.int32).reshape(-1)
        ng = (0 if g is None else len(g) // 3) if n_groups is None else n_groups
        return T(mode, vs, n_head, hd, n_ctx, n_slot, ng, None if g is None else g.ctypes.data_as(I32P), 1, a["q"], a["k"], a["v"], a["kc"], a["vc"], a["out"])
    for name in A:
        assert call(**{name: None}) == 1, name
    assert call(groups=None, n_groups=1) == 1
    assert call(mode=2) == 1 and call(mode=-1) == 1
    assert call(vs=3) == 1 and call(vs=0) == 1 and call(vs=8) == 1
    assert call(hd=48) == 1 and call(n_head=0) == 1 and call(n_slot=0) == 1
    assert call(n_groups=0) == 1 and call(n_groups=65, groups=[(0, 0, 1)] * 65) == 1
    assert call(groups=[(3, 0, 1)]) == 1 and call(groups=[(-1, 0, 1)]) == 1                     # a slot outside [0, n_slot)
    assert call(groups=[(1, 0, 2), (1, 8, 2)]) == 1                                               # a slot named twice
    assert call(groups=[(0, 0, 0)]) == 1 and call(groups=[(0, 0, 9)]) == 1                      # R outside 1 .. 8
    assert call(groups=[(0, -1, 2)]) == 1 and call(groups=[(0, 30, 3)]) == 1 and call(groups=[(0, 32, 1)]) == 1   # a row outside the cache
    assert call(n_slot=9, groups=[(s, 0, 8) for s in range(9)]) == 1                             # 72 rows
    assert call(n_ctx=1 << 24) == 1                                                               # more score rows than the kernel's LDS holds
    if lib.amd_device_count() <= 0:
        assert call() == 2 and call(groups=[(0, 29, 3), (2, 0, 8)], vs=4) == 2                    # accepted as far as the device check
    with pytest.raises(ValueError):
        lib.amd_test_attn_draft_batch(0, q[:4], q[:4], q[:4], kc, kc, n_head, [(0, 0, 9)])       # the wrapper turns 1 into ValueError (and checks the row count itself)


def test_epilogue_hook_refuses_bad_arguments_without_a_device(lib):
    T = lib.library.minigpt4_amd_test_draft_finish_batch
    V, n_slot = 8, 3
    lg = np.zeros((64, V), np.float32)
    st = G.start_state(n_slot, V, 1)
    res = np.zeros(129, np.int32)
    ptr = lambda a, t: a.ctypes.data_as(t)

    def call(slots=(2, 2, 0), pos=(5, 6, 0), N=None, n_vocab=V, n_slot=n_slot, **null):
        rs, rp = np.array(slots, np.int32), np.array(pos, np.int32)
        tok = np.zeros(max(len(rs), 1), np.int32)
        a = dict(logits=ptr(lg, F32P), tok=ptr(tok, I32P), rs=ptr(rs, I32P), rp=ptr(rp, I32P), n_past=ptr(st["n_past"], I32P), argmax=ptr(st["argmax"], I32P),
                 feed=ptr(st["feed"], I32P), keep=ptr(st["slot_logits"], F32P), res=ptr(res, I32P))
        a.update(null)
        return T(a["logits"], len(rs) if N is None else N, n_vocab, a["tok"], a["rs"], a["rp"], n_slot, a["n_past"], a["argmax"], a["feed"], a["keep"], a["res"])
    for name in ("logits", "tok", "rs", "rp", "n_past", "argmax", "feed", "keep", "res"):
        assert call(**{name: None}) == 1, name
    assert call(N=0) == 1 and call(slots=[0] * 8 + [1] * 8 + [2] * 8, pos=list(range(8)) * 3, N=65) == 1
    assert call(n_vocab=0) == 1 and call(n_vocab=(1 << 20) + 1) == 1
    assert call(n_slot=0) == 1 and call(n_slot=4097) == 1
    assert call(slots=(3, 0)) == 1 and call(slots=(-1, 0)) == 1                                   # a slot outside [0, n_slot)
    assert call(slots=(2, 0, 2), pos=(5, 0, 6)) == 1                                              # rows of one slot that are not adjacent
    assert call(slots=(1,) * 9, pos=tuple(range(9))) == 1                                         # a group of 9 rows
    assert call(slots=(1, 1), pos=(4, 6)) == 1 and call(slots=(1, 1), pos=(4, 4)) == 1          # positions not consecutive inside a group
    assert call(slots=(1,), pos=(-1,)) == 1
    if lib.amd_device_count() <= 0:
        assert call() == 2
    with pytest.raises(ValueError):
        lib.amd_test_draft_finish_batch(lg[:2], [0, 0], [1, 1], [4, 6], st["n_past"], st["argmax"], st["feed"], st["slot_logits"])


# ---- the serving loop's drafter -------------------------------------------------------------------------------------------------------------------------------------
def test_python_drafter_equals_the_engines_on_random_histories(lib):
    from minigpt4_cpp_amd import serve as S
    rng = np.random.default_rng(11)
    some = 0
    for case in range(200):
        h = [int(x) for x in rng.integers(0, 8, int(rng.integers(0, 200)))]
        ngram_min = int(rng.integers(1, 4))
        ngram_max = ngram_min + int(rng.integers(0, 4))
        n_draft = int(rng.integers(0, 8))
        got = S.ngram_draft(h, ngram_max, ngram_min, n_draft)
        assert got == lib.amd_test_ngram_draft(h, ngram_max, ngram_min, n_draft) == ref_draft(h, ngram_max, ngram_min, n_draft), (case, h, ngram_max, ngram_min, n_draft)
        some += bool(got)
    assert some > 100


def test_python_drafter_hand_made_cases(lib):
    from minigpt4_cpp_amd import serve as S
    cases = [([5, 6, 7], 3, 1, 4, []), ([], 3, 1, 4, []), ([5], 3, 1, 4, []), ([5, 5], 3, 1, 4, [5]),
             ([1, 3, 9, 4, 3, 7, 5, 1, 3], 2, 1, 3, [9, 4, 3]), ([1, 3, 9, 4, 3, 7, 5, 1, 3], 1, 1, 3, [7, 5, 1]), ([1, 3, 9, 4, 3, 7, 5, 1, 3], 4, 3, 3, []),
             ([3, 4, 0, 3, 5, 0, 3], 1, 1, 3, [5, 0, 3]), ([3, 4, 2, 6, 3], 2, 1, 4, [4]), ([3, 2, 6, 3], 2, 1, 4, []), ([3, 4, 5, 6, 3], 1, 1, 2, [4, 5]),
             ([3, 4, 5, 6, 3], 1, 1, 7, [4, 5, 6, 3]), ([3, 4, 5, 6, 3], 1, 1, 0, [])]
    for h, nmax, nmin, nd, want in cases:                                      # the hand-made cases of tests/test_cpu_draft.py
        assert S.ngram_draft(h, nmax, nmin, nd) == want == lib.amd_test_ngram_draft(h, nmax, nmin, nd), (h, nmax, nmin, nd)
    with pytest.raises(ValueError):
        S.ngram_draft([3, 4], 1, 2, 3)
    with pytest.raises(ValueError):
        S.ngram_draft([3, 4], 2, 0, 3)
    assert S.ngram_draft([3, 4, 5, 6, 3]) == [4, 5, 6, 3]                      # the defaults: 3 .. 1 tokens, 4 draft tokens


# ---- the numpy reference of the epilogue ----------------------------------------------------------------------------------------------------------------------------
def _rows(ids, V=8):
    """One logits row per id with a single maximum there."""
    lg = np.zeros((len(ids), V), np.float32)
    for t, i in enumerate(ids):
        lg[t, i] = 5
    return lg


def test_reference_hand_made_cases():
    V, n_slot = 8, 4
    st = G.start_state(n_slot, V, 3)
    # three groups in slot order different from row order: slot 3 (R = 4, m = 0), slot 0 (R = 3, m = R - 1 = 2), slot 2 (R = 1)
    groups = [(3, 10, 4), (0, 0, 3), (2, 7, 1)]
    rs, rp = B.pack(groups)
    assert rs.tolist() == [3, 3, 3, 3, 0, 0, 0, 2] and rp.tolist() == [10, 11, 12, 13, 0, 1, 2, 7]
    assert B.groups_of(rs) == [(0, 4), (4, 3), (7, 1)]
    ids = [1, 2, 3, 4, 5, 6, 7, 0]
    lg = _rows(ids, V)
    #      g0  d0 (wrong) d1 = ids[1]: a match behind the mismatch   | g0  d0  d1 both right | g0
    tok = [9, 7, 2, 3, 9, 5, 6, 9]
    out = B.finish_batch_ref(lg, tok, rs, rp, st)
    assert out["m_of_slot"] == {3: 0, 0: 2, 2: 0}
    assert out["res"][:8].tolist() == [0, -1, -1, -1, 2, -1, -1, 0] and (out["res"][8:64] == -1).all()
    assert out["res"][64:72].tolist() == ids and (out["res"][72:] == -1).all()
    assert out["n_past"][[3, 0, 2]].tolist() == [11, 3, 8] and out["n_past"][1] == st["n_past"][1] and out["n_past"][4] == st["n_past"][4]
    assert out["argmax"][[3, 0, 2]].tolist() == [1, 7, 0] and out["feed"][[3, 0, 2]].tolist() == [1, 7, 0]
    assert np.array_equal(out["slot_logits"][3], lg[0]) and np.array_equal(out["slot_logits"][0], lg[6]) and np.array_equal(out["slot_logits"][2], lg[7])
    for k in ("argmax", "feed", "slot_logits"):                                # the slot that is not in the pass, and the guard
        assert np.array_equal(out[k][1], st[k][1]) and np.array_equal(out[k][4], st[k][4]), k
    # a tie on the first maximum: the lower index is the row's choice, and only a draft token equal to IT is kept
    lg2 = _rows([2, 0], V)
    lg2[0, 6] = 5
    assert B.finish_batch_ref(lg2, [9, 2], [1, 1], [4, 5], st)["m_of_slot"] == {1: 1}
    assert B.finish_batch_ref(lg2, [9, 6], [1, 1], [4, 5], st)["m_of_slot"] == {1: 0}
    # a draft token equal to a LATER row's greedy id but not its own row's: not kept; nor is one equal to another group's
    lg3 = _rows([1, 2, 3, 4], V)
    assert B.finish_batch_ref(lg3, [9, 2, 2, 3], [0, 0, 0, 0], [0, 1, 2, 3], st)["m_of_slot"] == {0: 0}
    assert B.finish_batch_ref(lg3, [9, 1, 9, 3], [0, 0, 1, 1], [0, 1, 0, 1], st)["m_of_slot"] == {0: 1, 1: 1}
    assert B.finish_batch_ref(lg3, [9, 3, 9, 1], [0, 0, 1, 1], [0, 1, 0, 1], st)["m_of_slot"] == {0: 0, 1: 0}
    # toks_for builds row tokens with the wanted counts
    tok4 = B.toks_for(ids, [(0, 4, 3, False), (4, 3, 1, True), (7, 1, 0, False)])
    assert B.finish_batch_ref(lg, tok4, rs, rp, st)["m_of_slot"] == {3: 3, 0: 1, 2: 0}
    # one group alone is greedy_ref.draft_finish_ref, position set first
    one = B.finish_batch_ref(lg[:4], tok[:4], rs[:4], rp[:4], st)
    st1 = {k: np.array(v, copy=True) for k, v in st.items()}
    st1["n_past"][3] = 10
    ref = G.draft_finish_ref(lg[:4], tok[:4], 3, st1)
    for k in ("n_past", "argmax", "feed", "slot_logits"):
        assert np.array_equal(one[k], ref[k]), k
    assert one["res"][0] == ref["m"] and one["res"][64:68].tolist() == ref["ids"]


# ---- the server's refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_serving_refuses_what_the_greedy_rule_does_not_cover(lib):
    from minigpt4_cpp_amd import serve as S
    srv = S.ReplicaServer.__new__(S.ReplicaServer)                 # no model: the checks come before the library is touched
    srv.lib, srv.ctx, srv.conversations, srv._parked = lib, None, 4, {}
    reqs = [S.Request(np.zeros((3, 224, 224), np.float32), "hello", 4)]
    for kw in (dict(temp=0.8), dict(repeat_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(logit_bias={3: 1.0}), dict(regex="a+"),
               dict(logprobs=2), dict(num_beams=2), dict(guidance_scale=1.5), dict(temp=0.8, device_sampling=True), dict(sessions=[None])):
        with pytest.raises(ValueError, match="lookup"):
            srv.run(reqs, lookup=4, **kw)
    for bad in (8, -1, 2.5, True):
        with pytest.raises(ValueError, match="lookup"):
            srv.run(reqs, lookup=bad)
