"""Device-side sampling without a device: where the entry points and the hooks live, the refusals that come before anything runs (C ABI, binding, kernel hook), the
generator against the Random123 known answers and a NumPy restatement, the rule's host side (sampling.hpp: the function k_sample_rows' thread 0 runs) against float64, and the
serving layer's arguments.  The kernel and the engine run on the device: tests/test_gpu_device_sampling.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sampling_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("minigpt4_amd_end_chat_batch_sampled", "minigpt4_amd_sampled_candidates", "minigpt4_amd_conversation_seed", "minigpt4_amd_sampling_info")
HOOKS = ("minigpt4_amd_test_sample_rows", "minigpt4_amd_test_sample_rule", "minigpt4_amd_test_philox")
I32P, F32P, U64P, U32P = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32))


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def _declared(header):
    return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_entry_points_and_hooks_are_where_they_belong(lib):
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    test = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    for name in ENTRY:
        assert name in product and name in test and name in _declared("minigpt4_amd.h"), name
    for name in HOOKS:
        assert name in test and name not in product, name
        assert name in _declared("minigpt4_amd_test.h") and name not in _declared("minigpt4_amd.h"), name


def test_refusals_on_a_null_context_carry_the_short_names(lib):
    L = lib.library
    a = np.array([0], np.int32)
    toks, ids, info = (ctypes.c_char_p * 1)(), np.zeros(64, np.int32), np.zeros(6, np.uint64)
    ip = lambda x: x.ctypes.data_as(I32P)
    assert L.minigpt4_amd_end_chat_batch_sampled(None, ip(a), 1, toks, 0.8, 40, 0.9, ip(ids)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"end_chat_batch_sampled: no context")
    assert L.minigpt4_amd_sampled_candidates(None, ip(a), 1, 0.8, 40, 0.9, ip(ids), None, None, None) == 1
    assert L.minigpt4_amd_last_error().startswith(b"sampled_candidates: no context")
    assert L.minigpt4_amd_conversation_seed(None, 0, 1, 0) == 1
    assert L.minigpt4_amd_last_error().startswith(b"conversation_seed: no context")
    assert L.minigpt4_amd_sampling_info(None, 0, info.ctypes.data_as(U64P)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"sampling_info: no context")
    for call, args in (("amd_end_chat_batch_sampled", ([0],)), ("amd_sampled_candidates", ([0],)), ("amd_conversation_seed", (0, 1)), ("amd_sampling_info", ())):
        with pytest.raises(RuntimeError, match=call[len("amd_"):]):
            getattr(lib, call)(None, *args)


@pytest.mark.parametrize("call", ["amd_end_chat_batch_sampled", "amd_sampled_candidates"])
def test_binding_refuses_before_the_library_is_touched(lib, call):
    f = getattr(lib, call)
    name = call[len("amd_"):]
    ok = dict(temp=0.8, top_k=40, top_p=0.9)
    for slots, kw in (([], {}), ([0, 0], {}), ([0, -1], {}), (list(range(65)), {}),
                      ([0], dict(temp=0.0)), ([0], dict(temp=-1.0)), ([0], dict(temp=float("nan"))), ([0], dict(temp=float("inf"))), ([0], dict(temp=1e39)),
                      ([0], dict(top_k=0)), ([0], dict(top_k=65)), ([0], dict(top_k=2.5)),
                      ([0], dict(top_p=0.0)), ([0], dict(top_p=1.5)), ([0], dict(top_p=float("nan"))), ([0], dict(top_p=-0.5))):
        with pytest.raises(ValueError, match=name):
            f(None, slots, **{**ok, **kw})                         # ctx None: reaching the library would raise RuntimeError instead
    with pytest.raises(ValueError, match="conversation_seed"):
        lib.amd_conversation_seed(None, 0, -1)
    with pytest.raises(ValueError, match="conversation_seed"):
        lib.amd_conversation_seed(None, 0, 1, 1 << 64)


def test_kernel_hook_refuses_before_it_looks_for_a_device(lib):
    H = lib.library.minigpt4_amd_test_sample_rows
    lg = np.zeros((3, 40), np.float32)
    out, rt = np.zeros((2, 133), np.int32), np.zeros(64, np.int32)
    ip, fp = (lambda x: x.ctypes.data_as(I32P)), (lambda x: x.ctypes.data_as(F32P))

    def rc(logits=lg, buf_rows=3, n_vocab=32, ld=40, rows=((0, 0, 1, 0), (2, 1, 1, 0)), table=((5, 1, 0, 0), (7, 0, 0, 1)), n_table=2, n_bitmaps=1, bm_of=(-1, 0),
           params=((0.8, 0.9), (1.0, 1.0)), top_k=(4, 32), tok=(0, -1), n=2, out_=out, rt_=rt):
        rw = np.zeros((2, 8), np.int32)
        rw[:, :4] = rows
        tb, bm = np.array(table, np.int32), np.zeros((1, 4), np.uint32)
        pr, tk, sd, ti, bo = np.array(params, np.float32), np.array(top_k, np.int32), np.zeros((2, 2), np.uint64), np.array(tok, np.int32), np.array(bm_of, np.int32)
        return H(None if logits is None else fp(logits), buf_rows, n_vocab, ld, ip(rw), n, ip(tb), n_table, bm.ctypes.data_as(U32P), n_bitmaps, ip(bo), fp(pr), ip(tk),
                 sd.ctypes.data_as(U64P), ip(ti), None if rt_ is None else ip(rt_), None if out_ is None else ip(out_), None)
    for kw in (dict(logits=None), dict(out_=None), dict(rt_=None), dict(n=0), dict(ld=31), dict(n_vocab=0), dict(buf_rows=0), dict(buf_rows=2),
               dict(rows=((0, 0, 1, 0), (2, 2, 1, 0))), dict(rows=((0, 0, 3, 0), (2, 1, 1, 0))), dict(rows=((-1, 0, 1, 0), (2, 1, 1, 0))), dict(n_table=1),
               dict(table=((5, 1, 0, 0), (32, 0, 0, 1))), dict(table=((5, 1, 0, 0), (-1, 0, 0, 1))), dict(rows=((0, 0, 2, 0), (2, 1, 1, 0)), table=((5, 1, 0, 0), (5, 0, 0, 1))),
               dict(bm_of=(-1, 1)), dict(bm_of=(-2, 0)), dict(n_bitmaps=-1), dict(tok=(64, -1)), dict(tok=(0, -2)),
               dict(top_k=(0, 32)), dict(top_k=(4, 33)), dict(top_k=(65, 32)),
               dict(params=((0.0, 0.9), (1.0, 1.0))), dict(params=((float("nan"), 0.9), (1.0, 1.0))), dict(params=((float("inf"), 0.9), (1.0, 1.0))),
               dict(params=((0.8, 0.0), (1.0, 1.0))), dict(params=((0.8, 0.9), (1.0, 1.5))), dict(params=((0.8, float("nan")), (1.0, 1.0)))):
        assert rc(**kw) == 1, kw
    assert rc() in (0, 2)                                          # well-formed: runs, or finds no device


# ------------------------------------------------------------------------------------------------ the generator
def test_philox_known_answers_and_numpy_restatement(lib):
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in SR.philox4x32_10(ctr, key)) == want   # the restatement reproduces the Random123 answers ...
        assert tuple(int(x) for x in lib.amd_test_philox(ctr, key)) == want   # ... and so does the library
    rng = np.random.default_rng(11)
    ctrs, keys = rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64), rng.integers(0, 1 << 32, (200, 2), dtype=np.uint64)
    want = SR.philox4x32_10(ctrs, keys)
    for c, k, w in zip(ctrs, keys, want):
        assert np.array_equal(lib.amd_test_philox(c, k), w)
    assert SR.draw_word(0, 0) == 0x6627e8d5 and SR.draw_word((1 << 64) - 1, (1 << 64) - 1) != SR.draw_word((1 << 64) - 1, (1 << 32) - 1)   # both counter words count


# ------------------------------------------------------------------------------------------------ the rule's host side against float64
def _values(rng, n):
    return np.sort((3.0 * rng.standard_normal(n)).astype(np.float32))[::-1].copy()


def _check_rule(lib, v, temp, top_p, word, kept_exact=True):
    got, ref = lib.amd_test_sample_rule(v, temp, top_p, word), SR.rule64(v, temp, top_p, word)
    near_cut = ref["c"] is not None and np.abs(ref["c"] - float(np.float32(top_p))).min() < 1e-4
    if not near_cut:
        assert got["kept"] == ref["kept"], (temp, top_p, got["kept"], ref["kept"])
    else:
        assert abs(got["kept"] - ref["kept"]) <= 1
        ref = SR.rule64(v, temp, top_p, word, kept=got["kept"])
    k = got["kept"]
    assert np.all(np.abs(got["p"][:k] - ref["p"]) <= 2e-4 * ref["p"]) and np.all(got["p"][k:] == 0)
    assert 0 <= got["pick"] < k
    if np.abs(ref["cum"] - ref["u"]).min() >= 1e-4:
        assert got["pick"] == ref["pick"], (temp, top_p, word, got["pick"], ref["pick"])
    else:
        assert abs(got["pick"] - ref["pick"]) <= 1
    return got, ref


def test_sample_rule_against_float64(lib):
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 40, 64):
        v = _values(rng, n)
        for temp, top_p in ((0.8, 0.9), (0.25, 0.5), (1.5, 1.0), (1.0, 0.9)):
            for word in [0, 0xFFFFFFFF, 0x80000000] + [int(w) for w in rng.integers(0, 1 << 32, 24)]:
                _check_rule(lib, v, temp, top_p, word)


def test_sample_rule_edges(lib):
    rng = np.random.default_rng(6)
    v = _values(rng, 40)
    one = lib.amd_test_sample_rule(v[:1], 0.8, 0.9, 0x12345678)                  # top_k = 1: one candidate, probability exactly 1
    assert one["pick"] == 0 and one["kept"] == 1 and one["p"][0] == 1.0
    full, _ = _check_rule(lib, v, 0.8, 1.0, 0x9abcdef0)                          # top_p = 1: nothing is cut
    assert full["kept"] == 40 and abs(float(full["p"].astype(np.float64).sum()) - 1.0) < 1e-5
    peaked = v.copy()
    peaked[0] += 20.0                                                            # a top_p that keeps one candidate
    for word in (0, 0xFFFFFFFF, 0x7FFFFFFF):
        r = lib.amd_test_sample_rule(peaked, 1.0, 0.5, word)
        assert r["kept"] == 1 and r["pick"] == 0 and r["p"][0] == 1.0 and np.all(r["p"][1:] == 0)
    for temp, top_p in ((0.8, 0.9), (0.25, 0.5), (1.5, 1.0)):
        lo, hi = lib.amd_test_sample_rule(v, temp, top_p, 0), lib.amd_test_sample_rule(v, temp, top_p, 0xFFFFFFFF)
        assert lo["pick"] == 0                                                   # word 0: u = 0, t = 0, S_0 = 1 > 0
        assert 0 <= hi["pick"] < hi["kept"]                                      # the largest u: inside kept even where u * S rounds up to S
    eq = lib.amd_test_sample_rule(np.zeros(64, np.float32), 1.0, 1.0, 0xFFFFFFFF)   # 64 equal candidates, u = 1 - 2^-24: t = 64 - 2^-18, only S_63 = 64 exceeds it
    assert eq["kept"] == 64 and eq["pick"] == 63 and np.all(eq["p"] == np.float32(1 / 64))
    for bad in (dict(temp=0.0), dict(temp=float("nan")), dict(top_p=0.0), dict(values=np.zeros(65, np.float32)), dict(values=np.zeros(0, np.float32))):
        kw = {**dict(values=v, temp=0.8, top_p=0.9, word=1), **bad}
        with pytest.raises(ValueError):
            lib.amd_test_sample_rule(**kw)


# ------------------------------------------------------------------------------------------------ the python layer and the server
def test_python_layer_and_serving_arguments(lib):
    from minigpt4_cpp_amd import minigpt4_library as ML
    from minigpt4_cpp_amd import serve as S
    for name in ("amd_end_chat_batch_sampled", "amd_sampled_candidates", "amd_conversation_seed", "amd_sampling_info", "amd_test_sample_rows", "amd_test_sample_rule",
                 "amd_test_philox"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    sig = inspect.signature(S.ReplicaServer.run).parameters
    assert sig["device_sampling"].default is False and sig["seeds"].default is None
    srv = S.ReplicaServer.__new__(S.ReplicaServer)                 # no model: the checks come before the library is touched
    srv.lib, srv.ctx, srv.conversations = lib, None, 4
    reqs = [S.Request(np.zeros((3, 224, 224), np.float32), "hello", 4)]
    for kw in (dict(num_beams=2), dict(guidance_scale=1.5), dict(logprobs=2)):
        with pytest.raises(ValueError, match="device_sampling"):
            srv.run(reqs, temp=0.8, device_sampling=True, **kw)
    with pytest.raises(ValueError, match="device_sampling"):
        srv.run(reqs, temp=0.0, device_sampling=True)
    with pytest.raises(ValueError, match="device_sampling"):
        srv.run(reqs, temp=0.8, top_k=65, device_sampling=True)
    with pytest.raises(ValueError, match="seeds"):
        srv.run(reqs, temp=0.8, device_sampling=True, seeds=[1, 2])
    with pytest.raises(ValueError, match="seeds"):
        srv.run(reqs, temp=0.8, seeds=[1])
