"""Repetition / frequency / presence penalties and the logit bias without a device: the host function (the one definition the kernel shares) against a numpy float32
restatement of the rules in include/minigpt4_amd.h, bit for bit; the table builder; the entry points' presence and their refusals without a context.

The reference here (`penalise_ref`) is also what tests/test_gpu_penalties.py compares the kernel and the engine with."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 13                                                                   # llama_token_nl()
PEN_REP, PEN_ALPHA, PEN_KEEP_NL = 1, 2, 4
NEUTRAL = dict(repeat_last_n=64, repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1)
PRODUCT = ("minigpt4_amd_set_penalties", "minigpt4_amd_conversation_penalties", "minigpt4_amd_set_logit_bias", "minigpt4_amd_token_history", "minigpt4_amd_penalty_info")
HOOKS = ("minigpt4_amd_test_pen_pick", "minigpt4_amd_test_penalise_host")
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


# ---------------------------------------------------------------------------------------------------------------- the reference
def window_ref(history, repeat_last_n, n_ctx):
    """the last min(len(history), W) entries; W = n_ctx if repeat_last_n < 0 else repeat_last_n, clamped to 1024"""
    W = min(n_ctx if repeat_last_n < 0 else repeat_last_n, 1024)
    n = min(len(history), W)
    return [int(t) for t in history[len(history) - n:]] if n > 0 else []


def penalise_ref(row, history, n_ctx, repeat_last_n=64, repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1, bias=()):
    """steps 1-5 in numpy float32 scalars: every operation is rounded to fp32 on its own"""
    f = np.float32
    l = np.array(row, np.float32, copy=True)
    rp, ap, af = f(repeat_penalty), f(alpha_presence), f(alpha_frequency)
    with np.errstate(all="ignore"):
        for i, b in (bias.items() if isinstance(bias, dict) else bias):
            l[i] = l[i] + f(b)
        nl = l[NL] if len(l) > NL else None
        win = window_ref(history, repeat_last_n, n_ctx)
        count = collections.Counter(t for t in win if t >= 0)
        if win and rp != f(1.0):
            for i in count:
                l[i] = l[i] * rp if l[i] <= f(0.0) else l[i] / rp
        if win and not (af == f(0.0) and ap == f(0.0)):
            for i, c in count.items():
                t = f(c) * af
                t = t + ap
                l[i] = l[i] - t
        if not penalize_nl and nl is not None:
            l[NL] = nl
    return l


def first_max(row):
    """the greedy pick: the first maximum (-0.0 == +0.0)"""
    return int(np.argmax(np.asarray(row, np.float32)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_row(n_vocab, seed):
    return (np.random.default_rng(seed).standard_normal(n_vocab) * 4).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. the host function
def _check(lib, row, history, n_ctx, **kw):
    got, table, flags = lib.amd_test_penalise_host(row, history, n_ctx, **kw)
    want = penalise_ref(row, history, n_ctx, **kw)
    assert np.array_equal(bits(got), bits(want)), (kw, np.flatnonzero(bits(got) != bits(want))[:8])
    return got, table, flags


@pytest.mark.parametrize("n_vocab", [100, 512, 513, 32001])
@pytest.mark.parametrize("penalty", [1.3, 0.8])
def test_penalise_host_matches_numpy_bit_for_bit(lib, n_vocab, penalty):
    row = make_row(n_vocab, n_vocab)
    # counts 1, 2 and 7; positive, negative, +0.0 and -0.0 logits among the penalised ids; the newline id in the window
    hist = [5] + [17] * 2 + [23] * 7 + [40, 41, 42, NL, n_vocab - 1, 60, 61]
    row[5], row[17], row[23], row[40], row[41], row[42], row[60], row[61] = 2.5, -1.75, 3.25, 0.0, -0.0, -7.0, 1e-3, -1e-3
    row[NL] = 6.0
    bias = {7: 1.5, 17: -0.25, 40: -np.inf, NL: 0.625, n_vocab - 2: 3.0}
    for alphas in (dict(), dict(alpha_presence=0.5), dict(alpha_frequency=0.3), dict(alpha_presence=-0.25, alpha_frequency=0.7)):
        for nl in (1, 0):
            for b in ({}, bias):
                _check(lib, row, hist, 2048, repeat_penalty=penalty, penalize_nl=nl, bias=b, **alphas)
    # penalty 1 with an alpha: step 3 is skipped, step 4 runs
    _check(lib, row, hist, 2048, repeat_penalty=1.0, alpha_frequency=0.3)


def test_newline_exemption_restores_the_value_after_the_bias(lib):
    row = make_row(100, 1)
    row[NL] = 4.0
    got, _, flags = _check(lib, row, [NL, NL, 3], 64, repeat_penalty=1.3, alpha_presence=1.0, penalize_nl=0, bias={NL: 0.5})
    assert got[NL] == np.float32(4.5) and flags & PEN_KEEP_NL
    got, _, flags = _check(lib, row, [NL, NL, 3], 64, repeat_penalty=1.3, alpha_presence=1.0, penalize_nl=1, bias={NL: 0.5})
    assert got[NL] == np.float32(np.float32(4.5) / np.float32(1.3)) - np.float32(1.0) and not flags & PEN_KEEP_NL


def test_small_vocabulary_has_no_newline_id(lib):
    row = make_row(10, 2)
    for nl in (0, 1):
        got, _, flags = _check(lib, row, [1, 2, 2, 9], 64, repeat_penalty=1.3, alpha_frequency=0.5, penalize_nl=nl, bias={3: -np.inf})
        assert not flags & PEN_KEEP_NL and got[3] == -np.inf
    # ids of the history that the vocabulary does not have are ignored, like -1
    got, table, _ = lib.amd_test_penalise_host(row, [1, 13, 500, -1], 64, repeat_penalty=1.3)
    assert table[:, 0].tolist() == [1]


def test_window_rules(lib):
    row = make_row(512, 3)
    hist = list(np.random.default_rng(4).integers(0, 512, 3000))
    # shorter than repeat_last_n: the whole history
    got, table, _ = _check(lib, row, hist[:10], 2048, repeat_last_n=64, repeat_penalty=1.3)
    assert table[:, 1].sum() == 10
    # repeat_last_n 0: an empty window, nothing runs, whatever the factors; a bias still applies
    got, table, flags = _check(lib, row, hist, 2048, repeat_last_n=0, repeat_penalty=1.3, alpha_presence=1.0)
    assert flags == 0 and len(table) == 0 and np.array_equal(bits(got), bits(row))
    got, table, flags = _check(lib, row, hist, 2048, repeat_last_n=0, repeat_penalty=1.3, bias={3: 1.0})
    assert flags == 0 and table[:, 0].tolist() == [3]
    # -1: n_ctx entries
    got, table, _ = _check(lib, row, hist, 100, repeat_last_n=-1, repeat_penalty=1.3, alpha_frequency=0.1)
    assert table[:, 1].sum() == 100
    # 5000 and -1 with a long context: clamped to 1024
    for rln, n_ctx in ((5000, 2048), (-1, 4096)):
        got, table, _ = _check(lib, row, hist, n_ctx, repeat_last_n=rln, repeat_penalty=1.3, alpha_frequency=0.1)
        assert table[:, 1].sum() == 1024
    # -1 entries take a place in the window and penalise nothing
    h = [7, 8, -1, -1, -1, 9]
    got, table, _ = _check(lib, row, h, 2048, repeat_last_n=4, repeat_penalty=1.3)
    assert table[:, 0].tolist() == [9]
    got, table, _ = _check(lib, row, h, 2048, repeat_last_n=5, repeat_penalty=1.3)
    assert table[:, 0].tolist() == [8, 9]
    got, table, flags = _check(lib, row, [-1] * 32, 2048, repeat_penalty=1.3)
    assert len(table) == 0 and flags == PEN_REP                            # a non-empty window of image rows: nothing to penalise
    # an empty history
    got, table, flags = _check(lib, row, [], 2048, repeat_penalty=1.3, alpha_presence=1.0)
    assert flags == 0 and len(table) == 0


def test_neutral_parameters_are_the_identity(lib):
    row = make_row(513, 5)
    got, table, flags = _check(lib, row, [1, 2, 3, 3], 2048, **NEUTRAL)
    assert flags == 0 and len(table) == 0 and np.array_equal(bits(got), bits(row))


# ---------------------------------------------------------------------------------------------------------------- 2. the table builder, presence, refusals
def test_table_builder_distinct_ids_counts_and_merge(lib):
    rng = np.random.default_rng(6)
    row = make_row(2000, 6)
    hist = [int(t) for t in rng.integers(0, 300, 1500)] + [-1] * 5
    bias = {int(i): float(v) for i, v in zip(rng.choice(2000, 256, replace=False), rng.standard_normal(256))}
    got, table, flags = _check(lib, row, hist, 2048, repeat_last_n=1024, repeat_penalty=1.1, alpha_frequency=0.2, bias=bias)
    ids = table[:, 0].tolist()
    assert len(set(ids)) == len(ids) and len(ids) <= 1024 + 256 and flags == PEN_REP | PEN_ALPHA
    count = collections.Counter(t for t in hist[-1024:] if t >= 0)
    assert set(ids) == set(count) | set(bias)
    for i, c, b, hb in table.tolist():
        assert c == count.get(i, 0)
        assert hb == (i in bias)
        if hb:
            assert np.int32(b).view(np.float32) == np.float32(bias[i])
    assert sum(1 for i in ids if i in bias and i in count) > 0              # the case has ids that both lists name: merged into one entry
    # the widest table: 1024 distinct window ids and 256 other bias ids
    hist = list(range(1024))
    bias = {i: -1.0 for i in range(1500, 1756)}
    got, table, _ = _check(lib, row, hist, 2048, repeat_last_n=-1, alpha_presence=0.5, bias=bias)
    assert len(table) == 1280 and (table[:1024, 1] == 1).all() and (table[1024:, 1] == 0).all()


def test_host_hook_refuses_bad_arguments(lib):
    L = lib.library
    row = np.zeros(16, np.float32)
    ids, val = np.array([1, 1], np.int32), np.array([0.5, 0.5], np.float32)

    def call(n_vocab=16, n_hist=0, hist=None, n_bias=0, bi=None, bv=None):
        return L.minigpt4_amd_test_penalise_host(row.ctypes.data_as(F32P), n_vocab, hist, n_hist, 64, 64, 1.3, 0.0, 0.0, 1, bi, bv, n_bias, None, 0, None)
    assert call() == 0
    assert call(n_vocab=0) == -1
    assert call(n_hist=3) == -1                                             # a history without a pointer
    assert call(n_bias=2, bi=ids.ctypes.data_as(I32P), bv=val.ctypes.data_as(F32P)) == -1      # duplicate id
    assert call(n_bias=257, bi=ids.ctypes.data_as(I32P), bv=val.ctypes.data_as(F32P)) == -1
    ids[1] = 16
    assert call(n_bias=2, bi=ids.ctypes.data_as(I32P), bv=val.ctypes.data_as(F32P)) == -1      # id outside the vocabulary
    assert L.minigpt4_amd_test_penalise_host(None, 16, None, 0, 64, 64, 1.3, 0.0, 0.0, 1, None, None, 0, None, 0, None) == -1


def test_kernel_hook_refuses_bad_arguments_before_any_device(lib):
    lg = np.zeros((2, 32), np.float32)
    rows = np.zeros((1, 8), np.int32)
    table = np.zeros((2, 4), np.int32)

    def rc(lg=lg, n_vocab=32, rows=rows, table=table):
        try:
            lib.amd_test_pen_pick(lg, n_vocab, rows, table)
        except RuntimeError as e:
            return int(re.search(r"rc=(\d+)", str(e)).group(1))
        return 0
    bad = rows.copy(); bad[0, 0] = 2
    assert rc(rows=bad) == 1                                                # buffer row out of range
    bad = rows.copy(); bad[0, 1:3] = (1, 2)
    assert rc(rows=bad) == 1                                                # table range past the table
    bad = rows.copy(); bad[0, 2] = 2
    assert rc(rows=bad) == 1                                                # duplicate id (0, 0) within one row's table
    t2 = table.copy(); t2[1, 0] = 32
    assert rc(rows=bad, table=t2) == 1                                      # id outside the vocabulary
    assert rc(n_vocab=33) == 1                                              # ld < n_vocab


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def _declared(header):
    return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


def test_entry_points_are_exported_and_declared(lib):
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    test_so = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    for name in PRODUCT:
        assert name in product and name in _declared("minigpt4_amd.h") and name not in _declared("minigpt4_amd_test.h"), name
    for hook in HOOKS:
        assert hook in test_so and hook not in product and hook in _declared("minigpt4_amd_test.h") and hook not in _declared("minigpt4_amd.h"), hook
    assert not ((set(PRODUCT) | set(HOOKS)) & _declared("minigpt4.h"))      # the reference header is untouched


def test_entry_points_refuse_a_missing_context(lib):
    L = lib.library
    err = lambda: (L.minigpt4_amd_last_error() or b"").decode()
    out = np.zeros(4, np.int32)
    assert L.minigpt4_amd_set_penalties(None, 1) == 1 and err().startswith("set_penalties: ")
    assert L.minigpt4_amd_conversation_penalties(None, 0, 64, 1.1, 0.0, 0.0, 1) == 1 and err().startswith("conversation_penalties: ")
    assert L.minigpt4_amd_set_logit_bias(None, None, None, 0) == 1 and err().startswith("set_logit_bias: ")
    assert L.minigpt4_amd_token_history(None, out.ctypes.data_as(I32P), 4) == -1 and err().startswith("token_history: ")
    assert L.minigpt4_amd_penalty_info(None, out.ctypes.data_as(I32P)) == 1 and err().startswith("penalty_info: ")


def test_documents_state_the_neutral_values_and_the_rules():
    hdr = open(os.path.join(ROOT, "include", "minigpt4_amd.h")).read()
    for needle in ("NEUTRAL VALUES ARE repeat_penalty 1.0, alpha_presence 0.0, alpha_frequency 0.0", "clamped to 1024", "minigpt4_amd_decode_loop decide on raw logits",
                   "a context shift REMOVES the", "MINIGPT4_PENALTIES=1"):
        assert needle in hdr, needle
