"""Draft verification under sampling without a device: the three entry points ship in the product library and refuse a missing context with their short name, the two
hooks ship in the test library only, and the host staging of a sampled verify pass (csrc/draft_host.hpp through minigpt4_amd_test_draft_tables) equals a NumPy
construction from the rules in include/minigpt4_amd.h: row r sees the history followed by t_0 .. t_r (t_0 = x0, t_{i + 1} = draft[i]) through the penalty window, its
constraint state is the state walked over t_0 .. t_r, and the draft is cut at the first token its state does not allow."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import constraint_ref as R
from test_cpu_penalties import NL, PEN_ALPHA, PEN_KEEP_NL, PEN_REP, window_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("minigpt4_amd_verify_draft_sampled", "minigpt4_amd_decode_lookup_sampled", "minigpt4_amd_speculation_info")
HOOKS = ("minigpt4_amd_test_draft_sample", "minigpt4_amd_test_draft_tables")
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
V, N_CTX = 512, 2048


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


def test_null_context_is_refused_with_the_short_name(lib):
    L = lib.library
    d, ids, n, nxt, st = np.array([1, 3], np.int32), np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
    ip = lambda a: a.ctypes.data_as(I32P)
    assert L.minigpt4_amd_verify_draft_sampled(None, ip(d), 2, 0.8, 40, 0.9, ip(ids), ip(n), ip(nxt), None, None) == 1
    assert L.minigpt4_amd_last_error().startswith(b"verify_draft_sampled: ")
    assert L.minigpt4_amd_decode_lookup_sampled(None, ip(d), 2, 8, 3, 1, 4, 0.8, 40, 0.9, ip(ids), ip(n), ip(st)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"decode_lookup_sampled: ")
    assert L.minigpt4_amd_speculation_info(None, (ctypes.c_int64 * 8)()) == 1
    assert L.minigpt4_amd_last_error().startswith(b"speculation_info: ")
    with pytest.raises(RuntimeError, match="verify_draft_sampled"):
        lib.amd_verify_draft_sampled(None, [1, 3])
    with pytest.raises(RuntimeError, match="speculation_info"):
        lib.amd_speculation_info(None)


# ---------------------------------------------------------------------------------------------------------------- the staging
def table_ref(history, n_ctx, n_vocab, repeat_last_n=64, repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1, bias=()):
    """(flags, [(id, count, bias bits, has_bias)]): the distinct ids the transformation touches -- the window's ids ascending with their counts (only while step 3 or 4
    runs), a bias merged into its id's entry, then the ids only the bias names, in the bias list's order"""
    f = np.float32
    win = window_ref(history, repeat_last_n, n_ctx)
    flags = 0
    if win and f(repeat_penalty) != f(1.0):
        flags |= PEN_REP
    if win and not (f(alpha_frequency) == f(0.0) and f(alpha_presence) == f(0.0)):
        flags |= PEN_ALPHA
    bias = dict(bias)
    word = lambda b: int(np.array([b], np.float32).view(np.int32)[0])
    out = []
    if flags:
        count = collections.Counter(t for t in win if 0 <= t < n_vocab)
        out = [(i, c, word(bias[i]) if i in bias else 0, int(i in bias)) for i, c in sorted(count.items())]
        if not penalize_nl and n_vocab > NL:
            flags |= PEN_KEEP_NL
    seen = {e[0] for e in out}
    out += [(i, 0, word(b), 1) for i, b in bias.items() if i not in seen]
    return flags, out


def stage_ref(history, x0, draft, n_ctx, n_vocab, pen, bias, con):
    """con = (trans, acc, pieces, state) or None -> (n_rows, cut, [(flags, table)] per row, states)"""
    toks, states, cut = [x0], [], 0
    if con:
        trans, acc, pieces, q = con
        step = lambda s, t: s if t == R.EOS else R.walk(trans, s, pieces[t])
        allowed = lambda s, t: bool(acc[s]) if t == R.EOS else (t >= 3 and len(pieces[t]) > 0 and R.walk(trans, s, pieces[t]) != R.DEAD)
        q = step(q, x0)
        states.append(q)
        for t in draft:
            if not allowed(q, t):
                break
            q = step(q, t)
            states.append(q)
            toks.append(t)
        cut = len(draft) - (len(toks) - 1)
    else:
        toks += list(draft)
        states = [0] * len(toks)
    rows = [table_ref(list(history) + toks[:r + 1], n_ctx, n_vocab, bias=bias, **pen) for r in range(len(toks))]
    return len(toks), cut, rows, states


def check(lib, history, x0, draft, pen, bias, con, n_ctx=N_CTX, n_vocab=V):
    kw = dict(trans=con[0], accept=R.accept_words(con[1]), pieces=con[2], state=con[3]) if con else {}
    got = lib.amd_test_draft_tables(history, x0, draft, n_ctx, n_vocab, bias=bias, **pen, **kw)
    n_rows, cut, rows, states = stage_ref(history, x0, draft, n_ctx, n_vocab, pen, bias, con)
    what = (len(history), x0, list(draft), pen, cut)
    assert got["n_rows"] == n_rows and got["cut"] == cut, (what, got["n_rows"], got["cut"])
    assert got["states"].tolist() == states, what
    off = 0
    f32 = lambda v: int(np.array([v], np.float32).view(np.int32)[0])
    for r, (flags, tab) in enumerate(rows):
        w = got["rows"][r]
        assert w[0] == r and w[1] == off and w[2] == len(tab) and w[3] == flags and w[7] == 0, (what, r, w.tolist(), flags, len(tab))
        assert (w[4], w[5], w[6]) == (f32(pen.get("repeat_penalty", 1.0)), f32(pen.get("alpha_frequency", 0.0)), f32(pen.get("alpha_presence", 0.0))), (what, r)
        assert got["tables"][r].tolist() == [list(e) for e in tab], (what, r)
        off += len(tab)
    return got


PENS = [dict(), dict(repeat_penalty=1.3), dict(repeat_last_n=-1, repeat_penalty=1.3, alpha_frequency=0.25, alpha_presence=0.5, penalize_nl=0),
        dict(repeat_last_n=0, repeat_penalty=1.3), dict(repeat_last_n=64, alpha_presence=0.5)]
BIAS = {90: -50.0, 41: 8.0, 51: 3.0, 7: -np.inf}


@pytest.mark.parametrize("n_hist", [0, 1, 63, 64, 65, 1100])
def test_tables_equal_the_numpy_construction(lib, n_hist):
    rng = np.random.default_rng(500 + n_hist)
    for pen in PENS:
        for bias in ({}, BIAS):
            for n_draft in (0, 1, 7):
                hist = rng.integers(0, 60, n_hist).astype(np.int32)         # few distinct ids: counts above 1, ids that leave the window as it slides
                if n_hist >= 63:
                    hist[[n_hist - 64 + 3 if n_hist >= 64 else 2, n_hist - 40, n_hist - 1]] = -1   # embedding rows inside the window: a place each, no penalty
                    hist[n_hist - 63] = NL
                draft = rng.integers(0, 60, n_draft).tolist()
                if n_draft == 7:
                    draft[2], draft[5] = 41, V - 1                             # a biased id and the last id enter through the draft
                got = check(lib, hist, int(rng.integers(0, V)), draft, pen, bias, None)
                assert got["n_rows"] == 1 + n_draft and got["cut"] == 0
    # the window slides with the row: with repeat_last_n 64 and a history of 64 distinct ids, row r has lost the r + 1 oldest ids
    hist = np.arange(100, 164)
    got = check(lib, hist, 5, [6, 7, 8], dict(repeat_penalty=1.3), {}, None)
    for r in range(4):
        ids = got["tables"][r][:, 0].tolist()
        assert ids == [5, 6, 7, 8][:r + 1] + list(range(100 + r + 1, 164)), (r, ids)


def _digits_constraint():
    from minigpt4_cpp_amd import modelgen as G
    pieces = [p for p, _ in G.synth_vocab(V)]
    trans, acc = R.compile_ref(rb"[0-9]+")
    digits = [i for i, p in enumerate(pieces) if i >= 3 and p and p.isdigit()]
    letters = [i for i, p in enumerate(pieces) if i >= 3 and p and p.isalpha()]
    assert len(digits) >= 8 and letters
    return trans, acc, pieces, digits, letters


def test_the_constraint_cuts_the_draft_and_walks_the_states(lib):
    trans, acc, pieces, digits, letters = _digits_constraint()
    rng = np.random.default_rng(9)
    hist = rng.integers(0, 60, 65)
    pen = dict(repeat_penalty=1.3)
    for place, want_rows in ((0, 1), (3, 4), (6, 7)):                           # a letter in first, middle and last place of 7
        draft = [int(d) for d in rng.choice(digits, 7)]
        draft[place] = letters[0]
        got = check(lib, hist, digits[0], draft, pen, BIAS, (trans, acc, pieces, R.START))
        assert got["n_rows"] == want_rows and got["cut"] == 7 - place
    got = check(lib, hist, digits[1], [int(d) for d in rng.choice(digits, 7)], pen, {}, (trans, acc, pieces, R.START))
    assert got["n_rows"] == 8 and got["cut"] == 0 and all(acc[s] for s in got["states"])
    # "</s>" is allowed exactly where the state accepts: behind a digit it stays (and leaves the state), from the start state it is cut; ids 0 and 1 never pass
    got = check(lib, hist, digits[2], [R.EOS, digits[3]], pen, {}, (trans, acc, pieces, R.START))
    assert got["n_rows"] == 3 and got["states"][0] == got["states"][1]
    got = check(lib, hist, R.EOS, [R.EOS, digits[3]], pen, {}, (trans, acc, pieces, R.START))     # a stuck x0 leaves the start state, which does not accept
    assert got["n_rows"] == 1 and got["cut"] == 2 and got["states"].tolist() == [R.START]
    for bad in (0, 1):
        assert check(lib, hist, digits[2], [bad], pen, {}, (trans, acc, pieces, R.START))["cut"] == 1
    # no constraint: nothing is cut and the states are 0
    got = check(lib, hist, digits[0], [letters[0], R.EOS, 0], pen, {}, None)
    assert got["n_rows"] == 4 and got["states"].tolist() == [0, 0, 0, 0]


def test_the_hook_refuses_bad_arguments(lib):
    T = lib.library.minigpt4_amd_test_draft_tables
    h, d = np.arange(4, dtype=np.int32), np.array([10, 11], np.int32)
    n_rows, cut, n_tab = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rows, tab, states = np.zeros((8, 8), np.int32), np.zeros((64, 4), np.int32), np.zeros(8, np.int32)
    ip = lambda a: a.ctypes.data_as(I32P)

    def call(hist=h, n_hist=4, x0=5, draft=d, n_draft=2, n_ctx=64, n_vocab=100, cap=64, rp=1.3):
        return T(ip(hist) if hist is not None else None, n_hist, x0, ip(draft) if draft is not None else None, n_draft, 64, rp, 0.0, 0.0, 1, None, None, 0, n_ctx, n_vocab,
                 None, None, 0, 0, None, None, ctypes.byref(n_rows), ctypes.byref(cut), ip(rows), ip(tab), cap, ctypes.byref(n_tab), ip(states))
    assert call() == 0 and n_rows.value == 3
    for kw in (dict(hist=None), dict(n_hist=-1), dict(x0=-1), dict(x0=100), dict(draft=None), dict(n_draft=8), dict(n_draft=-1), dict(n_ctx=0), dict(n_vocab=0),
               dict(draft=np.array([1, 100], np.int32)), dict(cap=-1)):
        assert call(**kw) == 1, kw
    assert call(cap=3) == 4 and n_tab.value == 5 + 6 + 7                        # rows of 5, 6 and 7 distinct ids
