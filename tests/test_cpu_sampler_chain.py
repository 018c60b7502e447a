"""The extended device-side sampling rule without a device (include/minigpt4_amd.h: tail-free, typical, top-p, min-p, temperature, softmax, draw over the live list; mirostat
v2 behind top-k): where the entry points and hooks live, the refusals that come before anything runs, and the rule's host side (sampling.hpp: sample_chain, the function
every thread of k_sample_rows_ex enters) against tests/sampler_chain_ref.py's float64 restatement.  The kernel and the engine run on the device:
tests/test_gpu_sampler_chain.py.

Exact: with neutral parameters the chain equals sample_rule bit for bit (pick, kept, p).  Otherwise p_j within 2e-4 relative of float64, and the decisions -- the live
list, the pick, mirostat's cut -- equal the float64 rule's except where the float64 reference alone finds a threshold too close; sampler_chain_ref.py derives each margin
from the error behind that 2e-4 bound, and an excluded decision must still be an admissible neighbour, from which the reference is continued.  Caps on the random rows:
at most 5 % of a case's rows and 1 % of its draws excluded (a seed that exceeds one is changed, never the cap).  mu': within the bound sampler_chain_ref.judge_mirostat
derives from the error of p_pick.  The constructed edge rows sit on their thresholds by construction and carry no cap."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sampler_chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("minigpt4_amd_end_chat_batch_sampled_ex", "minigpt4_amd_sampled_candidates_ex", "minigpt4_amd_conversation_mirostat", "minigpt4_amd_mirostat_info",
         "minigpt4_amd_verify_draft_sampled_ex", "minigpt4_amd_decode_lookup_sampled_ex")
HOOKS = ("minigpt4_amd_test_sample_chain", "minigpt4_amd_test_sample_rows_ex")
I32P, F32P, U64P, U32P = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32))
NEUTRAL_SETS = ((0.8, 0.9), (0.25, 0.5), (1.5, 1.0), (1.0, 0.9))             # (temp, top_p) of tests/test_cpu_device_sampling.py
BAD_CHAIN = (dict(tfs_z=0.0), dict(tfs_z=1.5), dict(tfs_z=-0.5), dict(tfs_z=float("nan")), dict(typical_p=0.0), dict(typical_p=1.01), dict(typical_p=float("nan")),
             dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(mirostat=1), dict(mirostat=3), dict(mirostat=-1), dict(mirostat=2, mirostat_tau=0.0),
             dict(mirostat_tau=float("inf")), dict(mirostat_tau=float("nan")), dict(mirostat_tau=-1.0), dict(mirostat_eta=-0.1), dict(mirostat_eta=float("nan")),
             dict(mirostat_eta=float("inf")))


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
    header = open(os.path.join(ROOT, "include", "minigpt4_amd.h")).read()
    for words in ("THE LIVE LIST", "RETURN TO VALUE ORDER", "NOT THE REFERENCE'S BEHAVIOUR", "mirostat v1 is not built", "PER-CONVERSATION"):
        assert words in header, words                                        # the header states the rule


def test_refusals_on_a_null_context_carry_the_short_names(lib):
    L = lib.library
    a, ids, info = np.array([0], np.int32), np.zeros(64, np.int32), np.zeros(4, np.float32)
    toks = (ctypes.c_char_p * 1)()
    ip = lambda x: x.ctypes.data_as(I32P)
    assert L.minigpt4_amd_end_chat_batch_sampled_ex(None, ip(a), 1, toks, 0.8, 40, 0.9, 0.95, 1.0, 0.0, 0, 5.0, 0.1, ip(ids)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"end_chat_batch_sampled_ex: no context")
    assert L.minigpt4_amd_sampled_candidates_ex(None, ip(a), 1, 0.8, 40, 0.9, 0.95, 1.0, 0.0, 0, 5.0, 0.1, ip(ids), None, None, None) == 1
    assert L.minigpt4_amd_last_error().startswith(b"sampled_candidates_ex: no context")
    assert L.minigpt4_amd_conversation_mirostat(None, 0, 3.0) == 1
    assert L.minigpt4_amd_last_error().startswith(b"conversation_mirostat: no context")
    assert L.minigpt4_amd_mirostat_info(None, 0, info.ctypes.data_as(F32P)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"mirostat_info: no context")
    assert L.minigpt4_amd_verify_draft_sampled_ex(None, ip(a), 1, 0.8, 40, 0.9, 0.95, 0.9, 0.05, ip(ids), ip(ids), ip(ids), None, None) == 1
    assert L.minigpt4_amd_last_error().startswith(b"verify_draft_sampled_ex: no context")
    assert L.minigpt4_amd_decode_lookup_sampled_ex(None, ip(a), 1, 4, 3, 1, 2, 0.8, 40, 0.9, 0.95, 0.9, 0.05, ip(ids), ip(ids), ip(ids)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"decode_lookup_sampled_ex: no context")
    for call, kw in ((lib.amd_verify_draft_sampled, dict(tfs_z=0.0)), (lib.amd_verify_draft_sampled, dict(min_p=2.0)), (lib.amd_decode_lookup_sampled, dict(typical_p=0.0))):
        with pytest.raises(ValueError):                                      # the binding: before the library is touched
            call(None, [5], **({"max_tokens": 4} if call == lib.amd_decode_lookup_sampled else {}), **kw)
    for call, args, kw in (("amd_end_chat_batch_sampled", ([0],), dict(tfs_z=0.95)), ("amd_sampled_candidates", ([0],), dict(mirostat=2)),
                           ("amd_conversation_mirostat", (0, 3.0), {}), ("amd_mirostat_info", (), {})):
        with pytest.raises(RuntimeError, match=call[len("amd_"):]):
            getattr(lib, call)(None, *args, **kw)
    with pytest.raises(RuntimeError, match="_ex: no context"):               # _extended=True reaches the _ex entry point with neutral values too
        lib.amd_end_chat_batch_sampled(None, [0], _extended=True)


@pytest.mark.parametrize("call", ["amd_end_chat_batch_sampled", "amd_sampled_candidates"])
def test_binding_refuses_before_the_library_is_touched(lib, call):
    f = getattr(lib, call)
    name = call[len("amd_"):]
    for kw in BAD_CHAIN + (dict(mirostat=1.5),):
        with pytest.raises(ValueError, match=name):
            f(None, [0], **kw)                                               # ctx None: reaching the library would raise RuntimeError instead
    with pytest.raises(ValueError, match="not built"):
        f(None, [0], mirostat=1)
    with pytest.raises(ValueError, match="conversation_mirostat"):
        lib.amd_conversation_mirostat(None, 0, float("inf"))


def test_kernel_hook_refuses_before_it_looks_for_a_device(lib):
    lg = np.zeros((1, 40), np.float32)
    rows = np.zeros((1, 8), np.int32)
    ok = [1.0, 1.0, 0.0, 0, 5.0, 0.1, float("nan")]

    def rc(chain):
        try:
            lib.amd_test_sample_rows_ex(lg, 32, rows, np.zeros((0, 4), np.int32), [(0.8, 0.9)], [4], [(1, 0)], [chain])
        except RuntimeError as e:
            return int(re.search(r"rc=(\d)", str(e)).group(1))
        return 0
    for i, bad in ((0, 0.0), (0, 1.5), (0, float("nan")), (1, 0.0), (1, 2.0), (2, -0.5), (2, 1.5), (3, 1), (3, 3), (4, 0.0), (4, float("inf")), (5, -1.0), (5, float("nan")),
                   (6, float("inf"))):
        c = list(ok)
        c[i] = bad
        assert rc(c) == 1, (i, bad)
    assert rc(ok) in (0, 2)                                                  # well-formed: runs, or finds no device
    for kw in BAD_CHAIN:
        with pytest.raises(ValueError):
            lib.amd_test_sample_chain(np.zeros(4, np.float32), 0.8, 0.9, 1, **kw)


# ------------------------------------------------------------------------------------------------ the chain's host side
def _values(rng, n, peak=0.0):
    v = np.sort((3.0 * rng.standard_normal(n)).astype(np.float32))[::-1].copy()
    v[0] += np.float32(peak)
    return v


def _words(rng, n=24):
    return [0, 0xFFFFFFFF, 0x80000000] + [int(w) for w in rng.integers(0, 1 << 32, n)]


def test_neutral_values_equal_sample_rule_bit_for_bit(lib):
    rng = np.random.default_rng(21)
    for n in (1, 2, 3, 5, 40, 64):
        v = _values(rng, n)
        for temp, top_p in NEUTRAL_SETS:
            for word in _words(rng):
                a, b = lib.amd_test_sample_rule(v, temp, top_p, word), lib.amd_test_sample_chain(v, temp, top_p, word, mu=3.25)
                assert a["pick"] == b["pick"] and a["kept"] == b["kept"], (n, temp, top_p, word)
                assert np.array_equal(a["p"].view(np.uint32), b["p"].view(np.uint32))
                assert b["mask"] == (1 << a["kept"]) - 1 and b["mu"] == np.float32(3.25) and b["observed"] == 0


CASES = {"tail_free": dict(tfs_z=0.95), "tail_free_low": dict(tfs_z=0.5), "typical": dict(typical_p=0.9), "typical_low": dict(typical_p=0.3), "top_p": dict(),
         "min_p": dict(min_p=0.05), "min_p_high": dict(min_p=0.4), "all_four": dict(tfs_z=0.95, typical_p=0.9, min_p=0.05)}


def run_case(decide, rng, kw, n_rows=24, n_words=8):
    """decide(v, temp, top_p, word, **kw) -> the library's decision; (rows, rows excluded, draws, draws excluded)"""
    rows = bad_rows = draws = bad_draws = 0
    for n in (3, 5, 17, 40, 64):
        for _ in range(n_rows):
            v = _values(rng, n, peak=1.5 if "tfs_z" in kw else 0.0)          # peaked rows keep tail-free's s, and with it its margin 3.2e-4 / s, in hand
            temp, top_p = NEUTRAL_SETS[rows % 4] if "top_p" not in kw else (0.8, kw["top_p"])
            row_ex = False
            for word in _words(rng, n_words):
                ex, near_u = CR.judge_chain(decide(v, temp, top_p, word, **kw), v, temp, top_p, word, **kw)
                row_ex |= ex
                draws += 1
                bad_draws += near_u
            rows += 1
            bad_rows += row_ex
    return rows, bad_rows, draws, bad_draws


@pytest.mark.parametrize("case", sorted(CASES))
def test_each_filter_and_all_together_against_float64(lib, case):
    rows, bad_rows, draws, bad_draws = run_case(lib.amd_test_sample_chain, np.random.default_rng(100 + sorted(CASES).index(case)), CASES[case])
    print(f"{case}: {bad_rows} of {rows} rows and {bad_draws} of {draws} draws excluded")
    assert bad_rows <= 0.05 * rows and bad_draws <= 0.01 * draws


def test_the_filters_do_cut(lib):
    """the comparison above is not vacuous: on these rows every filter shortens the list, typical sampling drops a candidate from the middle or the top, and tail-free's
    margin stays small"""
    rng = np.random.default_rng(7)
    v = _values(rng, 40, peak=1.5)
    full = (1 << 40) - 1
    for kw in (dict(tfs_z=0.95), dict(typical_p=0.9), dict(min_p=0.05)):
        assert lib.amd_test_sample_chain(v, 0.8, 1.0, 5, **kw)["mask"] != full, kw
    flat = np.float32(0.05) * np.arange(40, 0, -1, dtype=np.float32)
    flat[0] += np.float32(3.0)                                               # one likely candidate and a flat tail: the top is the least typical entry
    r = lib.amd_test_sample_chain(flat, 1.0, 1.0, 5, typical_p=0.1)
    assert CR.chain64(flat, 1.0, 1.0, 5, typical_p=0.1)["mask"] & 1 == 0 and CR.judge_chain(r, flat, 1.0, 1.0, 5, typical_p=0.1) == (False, False)
    assert r["mask"] & 1 == 0 and r["kept"] >= 1 and r["p"][0] == 0 and abs(float(r["p"].astype(np.float64).sum()) - 1) < 1e-5
    assert CR.tail_free64(v.astype(np.float64), 0.95)["s"] >= 0.3


def test_mirostat_v2_against_float64(lib):
    rng = np.random.default_rng(31)
    rows = bad_rows = draws = bad_draws = 0
    for n in (1, 2, 5, 40, 64):
        for _ in range(12):
            v = _values(rng, n)
            temp, tau, eta = ((0.8, 5.0, 0.1), (1.0, 3.0, 0.3), (1.5, 2.0, 1.0))[rows % 3]
            mu, row_ex = None, False
            for word in _words(rng, 13):                                     # a teacher-forced sequence: the library's mu' starts the next decision on both sides
                got = lib.amd_test_sample_chain(v, temp, 0.9, word, tfs_z=0.5, typical_p=0.5, min_p=0.5, mirostat=2, mirostat_tau=tau, mirostat_eta=eta, mu=mu)
                ex, near_u = CR.judge_mirostat(got, v, temp, word, tau, eta, mu)
                row_ex |= ex
                draws += 1
                bad_draws += near_u
                mu = float(got["mu"])
            rows += 1
            bad_rows += row_ex
    print(f"mirostat: {bad_rows} of {rows} rows and {bad_draws} of {draws} draws excluded")
    assert bad_rows <= 0.05 * rows and bad_draws <= 0.01 * draws


def test_edges(lib):
    rng = np.random.default_rng(41)
    C = lib.amd_test_sample_chain
    for n in (1, 2):                                                         # tail-free needs more than two candidates: a no-op
        v = _values(rng, n)
        a, b = C(v, 0.8, 1.0, 77, tfs_z=0.01), C(v, 0.8, 1.0, 77)
        assert a["mask"] == b["mask"] == (1 << n) - 1 and np.array_equal(a["p"], b["p"]) and a["pick"] == b["pick"]
    eq = np.zeros(10, np.float32)                                            # equal candidates: s = 0 <= 1e-6, d2 = 1 / 8 each, c = 2 / 8 > 0.2 at i = 1
    r = C(eq, 1.0, 1.0, 0, tfs_z=0.2)
    assert r["mask"] == 0b1 and r["kept"] == 1 and r["p"][0] == 1.0 and r["pick"] == 0
    r = C(eq, 1.0, 1.0, 0, tfs_z=0.6)                                        # c = 5 / 8 = 0.625 > 0.6 at i = 4
    assert r["mask"] == 0b1111 and np.all(r["p"][:4] == np.float32(0.25))
    r = C(eq, 1.0, 1.0, 0, tfs_z=0.999)                                      # c ends at exactly 1 > 0.999 at i = 7
    assert r["mask"] == (1 << 7) - 1
    dead = _values(rng, 6)
    dead[-1] = -np.inf                                                       # a candidate a bias sent to -inf: q = 0, typicality +inf, no NaN in H
    r = C(dead, 1.0, 1.0, 0xFFFFFFFF, typical_p=0.99)
    assert np.all(np.isfinite(r["p"])) and r["p"][5] == 0 and r["mask"] >> 5 == 0 and abs(float(r["p"].astype(np.float64).sum()) - 1) < 1e-5
    CR.judge_chain(r, dead, 1.0, 1.0, 0xFFFFFFFF, typical_p=0.99)
    r = C(dead, 1.0, 1.0, 0xFFFFFFFF, tfs_z=0.9, typical_p=0.5, min_p=0.01)
    assert np.all(np.isfinite(r["p"])) and r["p"][5] == 0
    peaked = _values(rng, 40)
    peaked[0] += 20.0                                                        # typical_p keeping one candidate: the top holds nearly all mass and is the most typical
    for word in (0, 0xFFFFFFFF):
        r = C(peaked, 1.0, 1.0, word, typical_p=0.5)
        assert r["mask"] == 1 and r["kept"] == 1 and r["pick"] == 0 and r["p"][0] == 1.0 and np.all(r["p"][1:] == 0)
    ties = np.array([2.0, 2.0, 2.0, 1.999999, 1.0, 0.0], np.float32)       # min_p = 1: only candidates tying the top survive
    r = C(ties, 0.8, 1.0, 0x80000000, min_p=1.0)
    assert r["mask"] == 0b111 and np.all(r["p"][:3] == np.float32(1 / 3)) and r["pick"] == 1
    v = _values(rng, 40)
    s0 = CR.mirostat64(v, 0.8, 0, 5.0, 0.1, 1.0)["s"][0]                     # mirostat with mu below the top's surprise: one candidate, observed 0, mu' = mu + eta * tau
    mu = np.float32(0.5 * s0)
    r = C(v, 0.8, 0.9, 0xDEADBEEF, mirostat=2, mirostat_tau=5.0, mirostat_eta=0.1, mu=mu)
    assert r["kept"] == 1 and r["mask"] == 1 and r["pick"] == 0 and r["p"][0] == 1.0 and r["observed"] == 0
    assert r["mu"] == np.float32(mu - np.float32(np.float32(0.1) * np.float32(np.float32(0.0) - np.float32(5.0))))
    a, b = C(v, 0.8, 0.9, 123456, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.2), C(v, 0.8, 0.9, 123456, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.2, mu=6.0)
    assert a["pick"] == b["pick"] and a["mask"] == b["mask"] and a["mu"] == b["mu"] and np.array_equal(a["p"], b["p"])   # unset mu is 2 * tau


# ------------------------------------------------------------------------------------------------ the python layer
def test_python_layer_arguments(lib):
    from minigpt4_cpp_amd import minigpt4_library as ML
    for name in ("amd_conversation_mirostat", "amd_mirostat_info", "amd_test_sample_chain", "amd_test_sample_rows_ex"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name)), name
    from minigpt4_cpp_amd import serve as S
    for f in (ML.MiniGPT4SharedLibrary.amd_end_chat_batch_sampled, ML.MiniGPT4SharedLibrary.amd_sampled_candidates, S.ReplicaServer.run):
        sig = inspect.signature(f).parameters
        assert [sig[k].default for k in ("tfs_z", "typical_p", "min_p", "mirostat", "mirostat_tau", "mirostat_eta")] == [1.0, 1.0, 0.0, 0, 5.0, 0.1], f
    srv = S.ReplicaServer.__new__(S.ReplicaServer)                           # no model: the checks come before the library is touched
    srv.lib, srv.ctx, srv.conversations = lib, None, 4
    reqs = [S.Request(np.zeros((3, 224, 224), np.float32), "hello", 4)]
    for kw in (dict(tfs_z=0.95), dict(typical_p=0.9), dict(min_p=0.05), dict(mirostat=2)):
        with pytest.raises(ValueError, match="device_sampling"):             # the host chain keeps its context-level mu: not through this door
            srv.run(reqs, temp=0.8, **kw)
    for kw in BAD_CHAIN:
        with pytest.raises(ValueError, match="device_sampling"):
            srv.run(reqs, temp=0.8, device_sampling=True, **kw)
