"""Constrained decoding on the GPU (k_constrain_index, k_constrain_pick; minigpt4_amd_constraint_compile / _free / _set_constraint / _constraint_advance / _info / _mask).
The reference throughout is tests/constraint_ref.py -- an independent construction of the automaton, the index bits and the masked first maximum --, the patterns are
those of tests/test_cpu_constraint.py; bits and ids are compared exactly.

  1. the index kernel alone: the whole index[S][W] on the synthetic vocabularies and on a constructed one;
  2. the pick kernel alone on constructed rows, penalties and bias included;
  3. greedy decoding end to end on the tiny files: every pick against the reference pick from the same context's raw logits, the state against the reference walk;
  4. the batched step with four conversations: one launch per step, an unconstrained conversation equals a twin's, the _top report describes the raw row;
  5. temp > 0: every sampled id lies in the allowed set, the host counter moves and the launch counter does not;
  6. lifetime and refusals;
  7. the server's keyword.

Tests 3 to 5 take their reference from minigpt4_amd_get_logits of the SAME context at the SAME step, so the same bits enter both sides and no margin is involved."""
import ctypes
import os
import re

import numpy as np
import pytest

import constraint_ref as R
from test_cpu_constraint import BY_NAME, PATTERNS, ref_of
from test_cpu_penalties import first_max, make_row
from test_gpu_penalties import SHAPES, _f32_word, _head_tail

pytestmark = pytest.mark.gpu

N_CTX = 512
PROMPT = "what is in the picture?"
PEN = dict(repeat_last_n=64, repeat_penalty=1.3, alpha_presence=0.5, alpha_frequency=0.25, penalize_nl=1)


def synth_pieces(n_vocab):
    from minigpt4_cpp_amd import modelgen as G
    return [p for p, _ in G.synth_vocab(n_vocab)]


def constructed_pieces():
    """<unk> <s> </s>, the 256 byte tokens, then: an empty piece, the NUL byte again as its own piece, pieces with bytes >= 0x80, a 10-byte piece, pairs that differ in the
    last byte only, and pieces the patterns of the CPU set can take whole."""
    extra = [b"", b"\x00", b"\xc3\xa9", b"\xc3\xa9\xc3\xa9", b"\xc3", b"\xff\xfe", b"0123456789", b"yes", b"yet", b"no", b"ye", b"12", b"19", b"20", b"1.5", b"-0", b"-",
             b'{"n": ', b'{"n": 7', b', "ok": ', b"true}", b"false}", b"true", b"aaaa", b"aaab", b"ab", b"abab", b"bc", b"xx", b"zz", b"\n\t", b"\r\f", b"a]b}", b"A", b"E",
             b"2024-0", b"-12", b" ", b"a c", b"a\nc"]
    return [b"<unk>", b"<s>", b"</s>"] + [bytes([b]) for b in range(256)] + extra


# ------------------------------------------------------------------------------------------------ 1. the index kernel
@pytest.mark.parametrize("n_vocab", [100, 512, 513, 32001])
def test_index_kernel_on_the_synthetic_vocabularies(gpu_lib, n_vocab):
    pieces = synth_pieces(n_vocab)
    assert len(pieces) == n_vocab
    for name in ("empty", "number", "a_0_255"):                              # S = 2, a small automaton, the largest of the CPU set
        trans, acc = ref_of(BY_NAME[name])
        got, ms = gpu_lib.amd_test_constrain_index(pieces, trans, R.accept_words(acc))
        want = R.index_ref(pieces, trans, acc)
        print("V %d %s: S %d, W %d, %.3f ms" % (n_vocab, name, len(trans), got.shape[1], ms))
        assert got.shape == want.shape == (len(trans), R.index_words(n_vocab))
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
        assert not got[0].any()                                              # the dead row
        assert not (got[:, 0] & 3).any()                                     # ids 0 and 1
        assert np.array_equal((got[:, 0] >> 2) & 1, acc.astype(np.uint32))   # EOS iff the state accepts
        tail = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, n_vocab:]
        assert not tail.any()                                                # bits at or beyond V
    assert {len(ref_of(BY_NAME[n])[0]) for n in ("empty", "number", "a_0_255")} == {2, 7, 257}


@pytest.mark.parametrize("p", PATTERNS, ids=lambda p: p.name)
def test_index_kernel_on_the_constructed_vocabulary(gpu_lib, p):
    pieces = constructed_pieces()
    trans, acc = ref_of(p)
    got, _ = gpu_lib.amd_test_constrain_index(pieces, trans, R.accept_words(acc))
    want = R.index_ref(pieces, trans, acc)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    ids = {bytes(x): i for i, x in enumerate(pieces) if i >= 259}
    assert not np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, ids[b""]].any()   # the empty piece is never allowed
    if p.name == "yes_no":
        ok = set(R.allowed_ids(got[R.START], len(pieces)))
        assert ids[b"yes"] in ok and ids[b"ye"] in ok and ids[b"no"] in ok and ids[b"yet"] not in ok   # two pieces that differ in the last byte only
    if p.name == "class_hex":
        ok = set(R.allowed_ids(got[R.START], len(pieces)))
        assert ids[b"\xff\xfe"] in ok and 3 in ok and ids[b"\x00"] in ok and ids[b"\xc3"] not in ok   # bytes >= 0x80 are unsigned; the NUL byte is a byte (token 3)
    if p.name == "digits_1_3":
        assert ids[b"0123456789"] not in set(R.allowed_ids(got[R.START], len(pieces)))
    if p.name == "no_quote":
        assert ids[b"0123456789"] in set(R.allowed_ids(got[R.START], len(pieces)))   # the 10-byte piece


def test_index_hook_refuses_what_would_index_outside(gpu_lib):
    pieces = constructed_pieces()
    trans, acc = ref_of(BY_NAME["yes_no"])
    bad = trans.copy()
    bad[3, 7] = len(trans)
    with pytest.raises(RuntimeError):
        gpu_lib.amd_test_constrain_index(pieces, bad, R.accept_words(acc))
    with pytest.raises(RuntimeError):
        gpu_lib.amd_test_constrain_index(pieces, trans[:1], R.accept_words(acc[:1]))


# ------------------------------------------------------------------------------------------------ 2. the pick kernel
def _bitmap(n_vocab, ids):
    ok = np.zeros(R.index_words(n_vocab) * 32, bool)
    ok[list(ids)] = True
    return np.packbits(ok, bitorder="little").view(np.uint32)


def _pick_scenarios(n_vocab):
    """name -> f(row, head, tail0) -> (history, params, bias, allowed ids, expected id or None, stuck); rows arrive as N(0, 4^2) capped at 8"""
    S = {}
    most = [i for i in range(3, n_vocab) if i % 7 != 3]

    def raw_winner_disallowed(row, head, tail0):
        row[30], row[31] = 9.5, 9.0
        return [], {}, {}, [i for i in most if i != 30] + [31], 31, False
    S["raw_winner_disallowed"] = raw_winner_disallowed

    def tie_lower_allowed_id(row, head, tail0):
        row[25], row[40], row[41] = 12.0, 12.0, 12.0                          # 25 is not allowed: of the allowed 40 and 41 the lower wins
        return [], {}, {}, [i for i in most if i != 25] + [40, 41], 40, False
    S["tie_lower_allowed_id"] = tie_lower_allowed_id

    def zero_tie(row, head, tail0):                                          # -0.0 at the lower id equals +0.0: the lower id wins
        row[:] = -np.abs(row) - 1.0
        row[22], row[45] = -0.0, 0.0
        return [], {}, {}, [22, 45, 50, 51], 22, False
    S["zero_tie"] = zero_tie

    def zero_tie_penalised(row, head, tail0):                                # +0.0 * 1.3 = +0.0 at the lower, penalised id against -0.0
        row[:] = -np.abs(row) - 1.0
        row[22], row[45] = 0.0, -0.0
        return [22], dict(repeat_penalty=1.3), {}, [22, 45, 50], 22, False
    S["zero_tie_penalised"] = zero_tie_penalised

    def only_id_in_head(row, head, tail0):                                   # the only allowed id sits in the scalar head (or is id 0 of an aligned row)
        i = max(head - 1, 0)
        row[i] = -7.0
        return [], {}, {}, [i], i, False
    S["only_id_in_head"] = only_id_in_head

    def only_id_in_tail(row, head, tail0):
        i = n_vocab - 1 if tail0 >= n_vocab else tail0
        row[i] = -7.0
        return [], {}, {}, [i], i, False
    S["only_id_in_tail"] = only_id_in_tail

    def penalty_drops_below(row, head, tail0):                               # an allowed id falls below another allowed one
        row[30], row[31] = 9.5, 9.0
        return [30], dict(repeat_penalty=1.3), {}, most + [30, 31], 31, False
    S["penalty_drops_below"] = penalty_drops_below

    def penalised_id_disallowed(row, head, tail0):                           # the table names an id the constraint forbids; it must neither win nor hide another
        row[30], row[31], row[32] = 9.5, 9.25, 9.0
        return [30, 31], dict(alpha_presence=0.125), {30: 5.0}, [i for i in most if i != 30] + [31, 32], 31, False
    S["penalised_id_disallowed"] = penalised_id_disallowed

    def bias_minus_infinity(row, head, tail0):                               # a banned allowed id; the next allowed one wins
        row[30], row[31] = 9.5, 9.0
        return [], {}, {30: -np.inf}, [30, 31, 32], 31, False
    S["bias_minus_infinity"] = bias_minus_infinity

    def all_allowed_banned(row, head, tail0):                                # every allowed id at -infinity: still the first of them, not stuck
        return [], {}, {40: -np.inf, 44: -np.inf}, [40, 44], 40, False
    S["all_allowed_banned"] = all_allowed_banned

    def nothing_allowed(row, head, tail0):
        return [5, 6], dict(repeat_penalty=1.3), {7: 1.0}, [], R.EOS, True
    S["nothing_allowed"] = nothing_allowed

    def last_id_allowed(row, head, tail0):
        row[n_vocab - 1], row[0] = 8.5, 30.0                                  # id 0 towers but is not allowed
        return [n_vocab - 1], dict(alpha_frequency=0.25), {}, [n_vocab - 1, 33], n_vocab - 1, False
    S["last_id_allowed"] = last_id_allowed

    def many_entries(row, head, tail0):
        ids = [i for i in range(20, n_vocab - 8)][:64]
        return ids[:8] + ids, dict(repeat_penalty=1.1, alpha_frequency=0.25, repeat_last_n=-1), {ids[3]: 2.0}, most, None, False
    S["many_entries"] = many_entries
    return S


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_pick_kernel_against_numpy(gpu_lib, rows, n_vocab, ld):
    lib = gpu_lib
    scen = list(_pick_scenarios(n_vocab).items())
    for first in range(0, len(scen), rows):                                  # launches of `rows` rows until every scenario has run
        buf = np.full((rows, ld), 1e9, np.float32)                            # the stride's padding would win every pick if it were read
        row_words, table, bitmaps, want, names = [], [], [], [], []
        for r in range(rows):
            name, fn = scen[(first + r) % len(scen)]
            head, tail0 = _head_tail(r, n_vocab, ld)
            x = np.minimum(make_row(n_vocab, 1000 * n_vocab + first + r), np.float32(8.0))
            hist, kw, bias, allowed, pick, stuck = fn(x, head, tail0)
            buf[r, :n_vocab] = x
            _, tab, flags = lib.amd_test_penalise_host(x, hist, 4096, bias=bias, **kw)
            words = _bitmap(n_vocab, allowed)
            ref = R.pick_ref(x, words, history=hist, n_ctx=4096, bias=bias, **kw)
            if pick is not None:
                assert ref == (pick, stuck), (name, ref, pick)               # the scenario is what its name says
            p = dict(repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0)
            p.update({k: v for k, v in kw.items() if k in p})
            row_words.append([r, len(table), len(tab), flags, _f32_word(p["repeat_penalty"]), _f32_word(p["alpha_frequency"]), _f32_word(p["alpha_presence"]), 0])
            table += tab.tolist()
            bitmaps.append(words); want.append(ref); names.append(name)
        ids, stuck, ms = lib.amd_test_constrain_pick(buf, n_vocab, np.array(row_words, np.int32), np.array(table, np.int32).reshape(-1, 4), np.array(bitmaps), list(range(rows)))
        print("rows %d n_vocab %d ld %d: %d table entries, %.3f ms" % (rows, n_vocab, ld, len(table), ms))
        for r in range(rows):
            assert (int(ids[r]), bool(stuck[r])) == want[r], (names[r], r, int(ids[r]), bool(stuck[r]), want[r])


def test_pick_kernel_64_rows_with_different_states(gpu_lib):
    """One launch, 64 rows of an unaligned buffer, each under the index row of another (pattern, state): the bitmaps are the index kernel's own output."""
    n_vocab, ld = 513, 517
    pieces = synth_pieces(n_vocab)
    rows_of = []
    for name in ("json", "date", "number", "nested_counts", "word_space", "alt_in_star", "punct_escapes"):
        trans, acc = ref_of(BY_NAME[name])
        index, _ = gpu_lib.amd_test_constrain_index(pieces, trans, R.accept_words(acc))
        assert np.array_equal(index, R.index_ref(pieces, trans, acc))
        rows_of += [index[s] for s in range(len(trans))]                     # the dead rows included: they pick EOS and report stuck
    assert len(rows_of) >= 64
    bitmaps = np.array(rows_of[:64])
    buf = np.full((64, ld), 1e9, np.float32)
    want = []
    for r in range(64):
        buf[r, :n_vocab] = make_row(n_vocab, 77 + r)
        want.append(R.pick_ref(buf[r, :n_vocab], bitmaps[r]))
    words = np.array([[r, 0, 0, 0, _f32_word(1.0), 0, 0, 0] for r in range(64)], np.int32)
    ids, stuck, _ = gpu_lib.amd_test_constrain_pick(buf, n_vocab, words, np.zeros((0, 4), np.int32), bitmaps, list(range(64)))
    assert [(int(i), bool(s)) for i, s in zip(ids, stuck)] == want
    assert sum(s for _, s in want) >= 1 and len({i for i, _ in want}) > 8    # dead rows are among them; the states differ in what they allow


# ------------------------------------------------------------------------------------------------ helpers of the engine tests
def _load(lib, tiny_files, wtype="q5_k", mix="q5_k_m", conditioned=True, n_conv=1, seed=1337):
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm(wtype, mix=mix, conditioned=conditioned), verbosity=0, seed=seed, n_ctx=N_CTX, n_batch=32)
    if n_conv > 1:
        lib.amd_set_conversations(ctx, n_conv)
    return ctx


FILES = [("q5_k", "q5_k_m", True), ("f16", "none", False)]
PIECES = synth_pieces(512)                                                   # the tiny files' vocabulary
_INDEX = {}


def index_of(p):
    if p.name not in _INDEX:
        trans, acc = ref_of(p)
        _INDEX[p.name] = R.index_ref(PIECES, trans, acc)
    return _INDEX[p.name]


def ref_step(p, state, row, **kw):
    """the reference pick for a conversation in `state` and the state after it"""
    trans, _ = ref_of(p)
    tid, stuck = R.pick_ref(row, index_of(p)[state], **kw)
    assert not stuck
    return tid, state if tid == R.EOS else R.walk(trans, state, PIECES[tid])


def test_the_tiny_vocabulary_has_what_the_patterns_need():
    assert PIECES[3:259] == [bytes([b]) for b in range(256)]
    assert b"no" in PIECES and b"y" in PIECES and all(bytes([d]) in PIECES for d in b"0123456789")


# ------------------------------------------------------------------------------------------------ 3. greedy, end to end
BOUNDED = [p for p in PATTERNS if p.longest is not None]


@pytest.mark.parametrize("wtype,mix,conditioned", FILES, ids=lambda v: v if isinstance(v, str) else None)
def test_greedy_end_chat_follows_every_bounded_pattern(gpu_lib, tiny_files, wtype, mix, conditioned):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, wtype, mix, conditioned)
    try:
        launches = 0
        for p in BOUNDED:
            trans, acc = ref_of(p)
            h = lib.amd_constraint_compile(ctx, p.pattern)
            lib.minigpt4_reset_chat(ctx)
            lib.amd_set_constraint(ctx, 0, h)
            lib.minigpt4_begin_chat(ctx, PROMPT)
            state, text, ended = R.START, b"", False
            for _ in range(p.longest + 1):                                   # every piece has at least one byte: the longest match, then "</s>"
                info = lib.amd_constraint_info(ctx)
                assert (info["handle"], info["state"], info["accepting"], info["n_states"]) == (h, state, int(acc[state]), len(trans)), (p.name, info)
                assert np.array_equal(lib.amd_constraint_mask(ctx, h, state), index_of(p)[state]), p.name
                want, state = ref_step(p, state, lib.amd_logits(ctx))
                piece = lib.minigpt4_end_chat(ctx, temp=0.0)
                got = int(lib.amd_token_history(ctx)[-1])
                launches += 1
                assert got == want, (p.name, len(text), got, want)
                if got == R.EOS:
                    assert piece == "</s>"
                    ended = True
                    break
                text += PIECES[got]
            assert ended, (p.name, text)
            assert re.fullmatch(p.re_pattern, text), (p.name, text)
            assert lib.amd_constraint_info(ctx)["state"] == state and acc[state]
            lib.amd_set_constraint(ctx, 0, 0)
            lib.amd_constraint_free(ctx, h)
        info = lib.amd_constraint_info(ctx)
        assert (info["pick_launches"], info["host_rows"], info["stuck"], info["index_launches"]) == (launches, 0, 0, len(BOUNDED)), info
    finally:
        lib.minigpt4_free(ctx)


@pytest.mark.parametrize("parity", [False, True], ids=["fast", "parity"])
def test_amd_sample_picks_and_advances_the_state_in_both_modes(gpu_lib, tiny_files, parity):
    """minigpt4_amd_sample advances nothing of the conversation, but the constraint's state belongs to the sampler: it moves with every pick.  Parity mode: the same
    decision on the oracle-order logits."""
    lib = gpu_lib
    p = BY_NAME["date"]
    trans, acc = ref_of(p)
    ctx = _load(lib, tiny_files)
    try:
        lib.amd_set_parity(ctx, parity)
        h = lib.amd_constraint_compile(ctx, p.pattern)
        lib.amd_set_constraint(ctx, 0, h)
        lib.minigpt4_begin_chat(ctx, PROMPT)
        state, text, steps = R.START, b"", 0
        for _ in range(p.longest + 1):
            steps += 1
            n_past = lib.library.minigpt4_amd_n_past(ctx.ptr)
            want, state = ref_step(p, state, lib.amd_logits(ctx))
            tid = np.zeros(1, np.int32)
            assert lib.library.minigpt4_amd_sample(ctx.ptr, tid.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
            assert int(tid[0]) == want
            assert lib.library.minigpt4_amd_n_past(ctx.ptr) == n_past and lib.amd_constraint_info(ctx)["state"] == state
            if want == R.EOS:
                break
            text += PIECES[want]
            lib.amd_eval_tokens(ctx, [want])
        assert want == R.EOS and re.fullmatch(p.re_pattern, text), text
        info = lib.amd_constraint_info(ctx)
        assert (info["pick_launches"], info["host_rows"], info["stuck"]) == (steps, 0, 0)
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 4. the batched step
def _rank(row, tid):
    row = np.asarray(row, np.float32)
    return int(np.sum(row > row[tid]) + np.sum((row == row[tid])[:tid]))


def test_batched_step_one_launch_and_the_unconstrained_stay_as_they_were(gpu_lib, tiny_files):
    lib = gpu_lib
    a, b = _load(lib, tiny_files, n_conv=4), _load(lib, tiny_files, n_conv=4)
    pats = [BY_NAME["number"], BY_NAME["word_space"]]
    bias = {90: -50.0, 302: -50.0, 41: 8.0, 51: 3.0}
    slots = [0, 1, 2, 3]
    try:
        hs = [lib.amd_constraint_compile(a, p.pattern) for p in pats]
        for c in (a, b):
            lib.amd_set_penalties(c, True)
            for s in slots:
                lib.amd_select_conversation(c, s)
                lib.minigpt4_begin_chat(c, PROMPT + " " * s)
                if s in (1, 3):                                              # penalties plus a bias: once under a constraint, once without
                    lib.amd_conversation_penalties(c, s, **PEN)
                    lib.amd_set_logit_bias(c, bias)
        lib.amd_set_constraint(a, 0, hs[0])
        lib.amd_set_constraint(a, 1, hs[1])
        states, texts = [R.START, R.START], [b"", b""]
        for step in range(10):
            rows, hist = [], []
            for s in slots:
                lib.amd_select_conversation(a, s)
                rows.append(lib.amd_logits(a).copy())
                hist.append(lib.amd_token_history(a).tolist())
            before = lib.amd_constraint_info(a, 0), lib.amd_penalty_info(a)
            want0, st0 = ref_step(pats[0], states[0], rows[0])
            want1, st1 = ref_step(pats[1], states[1], rows[1], history=hist[1], n_ctx=N_CTX, bias=bias, **PEN)
            out = lib.amd_end_chat_batch_top(a, slots, top_n=5, temp=0.0)
            ids = [int(i) for i in out["ids"]]
            assert ids[:2] == [want0, want1], (step, ids, want0, want1)
            states = [st0, st1]
            for k in range(2):
                texts[k] += b"" if ids[k] == R.EOS else PIECES[ids[k]]
                assert lib.amd_constraint_info(a, k)["state"] == states[k]
            after = lib.amd_constraint_info(a, 0), lib.amd_penalty_info(a)
            assert after[0]["pick_launches"] == before[0]["pick_launches"] + 1   # ONE k_constrain_pick launch for both constrained conversations
            assert after[1]["launches"] == before[1]["launches"] + 1             # and one k_pen_pick launch: conversation 3 (conversation 1's table went to the new kernel)
            assert after[0]["host_rows"] == 0 and after[0]["stuck"] == 0
            # the twin is fed the same four ids; its own choices for the unconstrained conversations are the ids this context picked
            twin = lib.amd_eval_batch(b, slots, ids)
            assert twin[2:] == ids[2:], (step, twin, ids)
            # the report describes the RAW rows
            for k, s in enumerate(slots):
                assert int(out["top_ids"][k][0]) == first_max(rows[k])
                assert int(out["rank"][k]) == _rank(rows[k], ids[k]), (step, k)
                lse = np.log(np.sum(np.exp(rows[k].astype(np.float64) - rows[k].max()))) + rows[k].max()
                assert abs(float(out["logprob"][k]) - (float(rows[k][ids[k]]) - lse)) < 1e-3
        for k in range(2):                                                   # every prefix stayed inside its pattern
            assert R.walk(ref_of(pats[k])[0], R.START, texts[k]) == states[k] != R.DEAD
        assert any(int(i) != first_max(r) for i, r in zip(ids[:2], rows[:2])) or texts[0] != b""   # (not vacuous: see the per-step reference picks above)
        assert lib.amd_constraint_info(b, 0)["pick_launches"] == 0           # the twin never launched the kernel
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 5. temp > 0
@pytest.mark.parametrize("name", ["json", "date"])
def test_sampling_stays_inside_the_allowed_set(gpu_lib, tiny_files, name):
    lib = gpu_lib
    p = BY_NAME[name]
    trans, acc = ref_of(p)
    ctx = _load(lib, tiny_files, seed=4242)
    try:
        h = lib.amd_constraint_compile(ctx, p.pattern)
        lib.amd_set_constraint(ctx, 0, h)
        lib.minigpt4_begin_chat(ctx, PROMPT)
        state, text, steps = R.START, b"", 0
        for _ in range(p.longest + 1):
            allowed = set(R.allowed_ids(lib.amd_constraint_mask(ctx, h, state), 512))
            assert allowed == set(R.allowed_ids(index_of(p)[state], 512))
            lib.minigpt4_end_chat(ctx, temp=0.9, top_k=40, top_p=0.95)
            tid = int(lib.amd_token_history(ctx)[-1])
            steps += 1
            assert tid in allowed, (name, text, tid)
            if tid == R.EOS:
                break
            text += PIECES[tid]
            state = R.walk(trans, state, PIECES[tid])
            assert lib.amd_constraint_info(ctx)["state"] == state
        assert tid == R.EOS and re.fullmatch(p.re_pattern, text), text
        info = lib.amd_constraint_info(ctx)
        assert info["host_rows"] == steps and info["pick_launches"] == 0 and info["stuck"] == 0
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 6. lifetime and refusals
def test_off_means_off(gpu_lib, tiny_files):
    lib = gpu_lib
    a, b = _load(lib, tiny_files), _load(lib, tiny_files)
    try:
        h = lib.amd_constraint_compile(a, b"(yes|no)")                       # compiled, never assigned
        for c in (a, b):
            lib.minigpt4_begin_chat(c, PROMPT)
        ids = [[], []]
        for _ in range(12):
            for k, c in enumerate((a, b)):
                lib.minigpt4_end_chat(c, temp=0.0)
                ids[k].append(int(lib.amd_token_history(c)[-1]))
        assert ids[0] == ids[1]
        info = lib.amd_constraint_info(a)
        assert info == dict(handle=0, state=0, accepting=0, n_states=0, pick_launches=0, host_rows=0, stuck=0, index_launches=1)
        assert lib.amd_constraint_info(b) == dict(info, index_launches=0)
        lib.amd_constraint_free(a, h)
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def test_lifetime_and_refusals(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, n_conv=2)
    L = lib.library

    def refused(rc, name):
        assert rc == 1
        assert lib._err().startswith(name + ": "), lib._err()

    try:
        trans, acc = ref_of(BY_NAME["yes_no"])
        h = lib.amd_constraint_compile(ctx, "(yes|no)")
        assert h == 1
        lib.amd_set_constraint(ctx, 1, h)
        y, e, s, n, o = (PIECES.index(x) for x in (b"y", b"e", b"s", b"n", b"o"))
        lib.amd_constraint_advance(ctx, 1, [y, R.EOS, e])                    # "</s>" leaves the state where it is
        want = R.walk(trans, R.START, b"ye")
        snap = lib.amd_constraint_info(ctx, 1)
        assert (snap["handle"], snap["state"], snap["accepting"], snap["n_states"]) == (h, want, 0, 6)
        # an advance into the dead state changes nothing, whatever came before the offending token
        two = np.array([s, n], np.int32)                                       # "yes", then a byte that no longer fits
        refused(L.minigpt4_amd_constraint_advance(ctx.ptr, 1, two.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2), "constraint_advance")
        assert lib.amd_constraint_info(ctx, 1) == snap
        for bad in ([512], [-1]):
            with pytest.raises(RuntimeError, match="constraint_advance: "):
                lib.amd_constraint_advance(ctx, 1, bad)
        with pytest.raises(RuntimeError, match="constraint_advance: "):
            lib.amd_constraint_advance(ctx, 0, [y])                          # conversation 0 has no constraint
        with pytest.raises(RuntimeError, match="constraint_advance: "):
            lib.amd_constraint_advance(ctx, 2, [y])
        assert lib.amd_constraint_info(ctx, 1) == snap
        # freeing a handle in use; handles that do not exist
        with pytest.raises(RuntimeError, match="constraint_free: "):
            lib.amd_constraint_free(ctx, h)
        for bad in (0, 2, 9, -1):
            with pytest.raises(RuntimeError, match="constraint_free: "):
                lib.amd_constraint_free(ctx, bad)
            if bad:
                with pytest.raises(RuntimeError, match="set_constraint: "):
                    lib.amd_set_constraint(ctx, 0, bad)
        with pytest.raises(RuntimeError, match="set_constraint: "):
            lib.amd_set_constraint(ctx, 2, h)
        assert lib.amd_constraint_info(ctx, 1) == snap and lib.amd_constraint_info(ctx, 0)["handle"] == 0
        # the mask: a bad state, a short buffer, a bad handle
        for state, words in ((6, None), (-1, None), (2, R.index_words(512) - 1)):
            with pytest.raises(RuntimeError, match="constraint_mask: "):
                lib.amd_constraint_mask(ctx, h, state, n_words=words)
        with pytest.raises(RuntimeError, match="constraint_mask: "):
            lib.amd_constraint_mask(ctx, 2, 1)
        assert np.array_equal(lib.amd_constraint_mask(ctx, h, want), index_of(BY_NAME["yes_no"])[want])
        # refused patterns leave no handle behind; the ninth compile is refused
        for bad in (b"a+?", b"(a", b"[^\\x00-\\xff]", b"(a|b)*a(a|b){12}"):
            with pytest.raises(RuntimeError, match="constraint_compile: "):
                lib.amd_constraint_compile(ctx, bad)
        more = [lib.amd_constraint_compile(ctx, b"[0-9]{%d}" % k) for k in range(1, 8)]
        assert more == [2, 3, 4, 5, 6, 7, 8]
        with pytest.raises(RuntimeError, match="constraint_compile: .*in use"):
            lib.amd_constraint_compile(ctx, b"x")
        assert lib.amd_constraint_info(ctx, 1) == dict(snap, index_launches=8)
        lib.amd_constraint_free(ctx, 5)
        assert lib.amd_constraint_compile(ctx, b"x") == 5                    # the freed handle is the next one given out
        # reset_chat: the state returns to the start, the handle stays; a fork touches neither handle nor state
        lib.amd_select_conversation(ctx, 1)
        lib.minigpt4_reset_chat(ctx)
        info = lib.amd_constraint_info(ctx, 1)
        assert (info["handle"], info["state"]) == (h, R.START)
        lib.amd_constraint_advance(ctx, 1, [n])
        lib.amd_select_conversation(ctx, 0)
        lib.minigpt4_begin_chat(ctx, PROMPT)
        lib.amd_fork_conversation(ctx, 0, [1])
        info = lib.amd_constraint_info(ctx, 1)
        assert (info["handle"], info["state"]) == (h, R.walk(trans, R.START, b"n")) and lib.amd_constraint_info(ctx, 0)["handle"] == 0
        # the forked conversation decodes under ITS constraint from ITS state: "o", then "</s>"
        lib.amd_select_conversation(ctx, 1)
        assert lib.minigpt4_end_chat(ctx, temp=0.0) == "o" and lib.minigpt4_end_chat(ctx, temp=0.0) == "</s>"
        # set_conversations clears the assignments and keeps the handles; so does a parity switch keep both
        lib.amd_set_parity(ctx, True)
        assert lib.amd_constraint_info(ctx, 1)["handle"] == h
        lib.amd_set_parity(ctx, False)
        lib.amd_set_conversations(ctx, 2)
        assert [lib.amd_constraint_info(ctx, s)["handle"] for s in (0, 1)] == [0, 0]
        lib.amd_constraint_free(ctx, h)                                      # no conversation uses it any more
        lib.amd_set_constraint(ctx, 0, 8)                                    # the other handles are still there
        assert lib.amd_constraint_info(ctx, 0)["n_states"] == 9
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 7. the server
def test_server_regex_keyword(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G, serve as S
    from minigpt4_cpp_amd.minigpt4_library import choice_pattern
    vp, lp = os.path.join(tmpdir_models, "vision_serve_con.bin"), os.path.join(tmpdir_models, "llm_serve_con.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)                       # tests/test_gpu_serve.py's model
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3 + i), p, 24) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)           # waves of 2 + 1
    try:
        plain = srv.run(reqs, temp=0.0, ignore_eos=True)
        for pattern in (choice_pattern(["yes", "no", "n/a"]), r"(19|20)\d\d-(0[1-9]|1[0-2])", r'\{"n": [0-9]{1,2}, "ok": (true|false)\}'):
            for kw in (dict(temp=0.0), dict(temp=0.8), dict(temp=0.0, repeat_penalty=1.3, logprobs=3)):
                got = srv.run(reqs, regex=pattern, **kw)
                assert all(re.fullmatch(pattern, g) for g in got), (pattern, kw, got)
                for slot in range(2):                                        # the call leaves no assignment and no handle behind
                    assert srv.lib.amd_constraint_info(srv.ctx, slot)["handle"] == 0
                assert srv.lib.amd_constraint_compile(srv.ctx, "x") == 1
                srv.lib.amd_constraint_free(srv.ctx, 1)
        assert srv.run(reqs, temp=0.0, ignore_eos=True) == plain
        with pytest.raises(ValueError):
            srv.run(reqs, regex="a", num_beams=2)
        with pytest.raises(ValueError):
            srv.run(reqs, regex="a", guidance_scale=1.5)
        with pytest.raises(RuntimeError, match="constraint_compile: "):
            srv.run(reqs, regex="a+?")
        assert srv.lib.amd_constraint_info(srv.ctx, 0)["handle"] == 0
    finally:
        srv.close()
