"""Repetition / frequency / presence penalties and the logit bias on the GPU (k_pen_pick; minigpt4_amd_set_penalties / _conversation_penalties / _set_logit_bias /
_token_history / _penalty_info).  The reference throughout is the numpy float32 restatement in tests/test_cpu_penalties.py; ids are compared exactly, adjusted values
bit for bit.

  3. the kernel against numpy and against the host function on constructed rows;
  4. greedy decoding end to end: a context with the mode on against a twin with the mode off that is fed its ids;
  5. the batched step against twin contexts, one launch per step, the report of _end_chat_batch_top from the raw row;
  6. the host path (temp > 0);
  7. the token history after every operation that moves rows;
  8. off means off; refusals change nothing;
  9. the server's keywords.

Files.  Tests 4 and 6 run on the PLAIN tiny files (q5_k / q5_k_m and f16) with repeat_penalty 1.3, window 64: on the CPU oracle's logits 12 resp. 11 of the 24 ids after
"what is in the picture?" differ from the raw greedy id (the conditioned files' greedy decoding never repeats a token, so a penalty above 1 changes nothing there).  Both
contexts of test 4 run the same launches, so their logits rows are the same bits and no margin is involved.  Test 5 compares a batched step with single-conversation
twins, so it runs on the conditioned q5_k_m file with parameters that decide by a wide margin there (oracle: repeat_penalty 0.25 -> 14 of 16 ids differ, smallest margin
0.67; alpha_frequency -3 -> 16 of 16, 0.33; the bias {90: -50, 302: -50, 41: +8} -> 16 of 16, 2.4).  Test 9 runs on tests/test_gpu_serve.py's model with
repeat_penalty 1.3: on the oracle two of the three requests change an id within 12 tokens."""
import ctypes

import numpy as np
import pytest

from test_cpu_penalties import NL, PEN_ALPHA, PEN_KEEP_NL, PEN_REP, bits, first_max, make_row, penalise_ref

pytestmark = pytest.mark.gpu

N_CTX = 128
PROMPT = "what is in the picture?"
PEN13 = dict(repeat_last_n=64, repeat_penalty=1.3, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1)
WILD = dict(repeat_last_n=-1, repeat_penalty=5.0, alpha_presence=3.0, alpha_frequency=3.0, penalize_nl=0)
NEUTRAL = dict(repeat_last_n=64, repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1)
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def _f32_word(v):
    return int(np.float32(v).view(np.int32))


# ------------------------------------------------------------------------------------------------ 3. the kernel
SHAPES = [(1, 100, 100), (3, 512, 512), (5, 513, 520), (2, 64, 72), (64, 32000, 32000), (65, 32001, 32001)]


def _head_tail(r, n_vocab, ld):
    """Row r of a 16-byte aligned [rows][ld] fp32 buffer: the kernel's scalar head is [0, head), its scalar tail [tail0, n_vocab)."""
    head = min(n_vocab, ((16 - (r * ld * 4) % 16) % 16) // 4)
    return head, head + 4 * ((n_vocab - head) // 4)


def _others(n_vocab, k, avoid=()):
    """k distinct ids away from the ids the scenarios plant values at"""
    out = [i for i in range(20, n_vocab - 8) if i not in avoid]
    return out[:k]


def _scenarios(n_vocab):
    """name -> f(row, head, tail0) -> (history, params, bias, expected pick or None); the row arrives filled with N(0, 4^2) values below 9 and is changed in place"""
    f = np.float32
    S = {}

    def winner_penalised(row, head, tail0):                                 # the raw winner falls below the runner-up; a table of 1
        row[30], row[31] = 9.5, 9.0
        return [30], dict(repeat_penalty=1.3), {}, 31
    S["winner_penalised"] = winner_penalised

    def tie_lower_id(row, head, tail0):                                      # a penalised entry ties an unpenalised one with a LOWER id: the lower id wins
        row[40] = 12.0
        row[25] = f(12.0) / f(1.3)
        return [40], dict(repeat_penalty=1.3), {}, 25
    S["tie_lower_id"] = tie_lower_id

    def tie_higher_id(row, head, tail0):                                     # ... with a HIGHER id: the penalised entry wins
        row[25] = 12.0
        row[40] = f(12.0) / f(1.3)
        return [25], dict(repeat_penalty=1.3), {}, 25
    S["tie_higher_id"] = tie_higher_id

    def zero_tie(row, head, tail0):                                          # -0.0 (unpenalised, lower id) against +0.0 * 1.3 = +0.0: equal, the lower id wins
        row[:] = -np.abs(row) - 1.0
        row[22], row[45] = -0.0, 0.0
        return [45], dict(repeat_penalty=1.3), {}, 22
    S["zero_tie"] = zero_tie

    def zero_tie_penalised_first(row, head, tail0):                          # the penalised -0.0 * 1.3 = -0.0 has the lower id
        row[:] = -np.abs(row) - 1.0
        row[22], row[45] = -0.0, 0.0
        return [22], dict(repeat_penalty=1.3), {}, 22
    S["zero_tie_penalised_first"] = zero_tie_penalised_first

    def bias_winner(row, head, tail0):                                       # a winner only because of its bias
        row[50] = -3.0
        return [], {}, {50: 20.0}, 50
    S["bias_winner"] = bias_winner

    def all_banned(row, head, tail0):                                        # every other candidate banned (at most 256 pairs: the small vocabularies; else the raw top 256)
        keep = n_vocab // 2
        ban = [i for i in range(n_vocab) if i != keep] if n_vocab <= 257 else [int(i) for i in np.argsort(-row, kind="stable")[:256]]
        return [], {}, {i: -np.inf for i in ban}, keep if n_vocab <= 257 else None
    S["all_banned"] = all_banned

    def head_tail_last(row, head, tail0):                                    # penalised ids in the scalar head, in the scalar tail and at n_vocab - 1, all raw leaders
        ids = sorted(set([0, max(head - 1, 0), min(tail0, n_vocab - 1), n_vocab - 1]))
        for k, i in enumerate(ids):
            row[i] = 9.0 + 0.125 * k
        row[33] = 8.5
        return ids + [n_vocab - 1], dict(alpha_presence=2.0, alpha_frequency=0.5), {}, 33
    S["head_tail_last"] = head_tail_last

    def last_id_wins(row, head, tail0):                                      # the pick itself is the penalised id n_vocab - 1, first id 0 penalised away
        row[0], row[n_vocab - 1] = 45.0, 40.0                                # 45 / 1.5 - 16 = 14 against 40 / 1.5 - 8 = 18.67
        return [0, 0, n_vocab - 1], dict(repeat_penalty=1.5, alpha_frequency=8.0), {}, n_vocab - 1
    S["last_id_wins"] = last_id_wins

    def newline_exempt(row, head, tail0):                                    # the raw winner is the exempted newline id, with a bias on it
        row[NL], row[34] = 9.5, 9.25
        return [NL, NL, 34], dict(repeat_penalty=1.3, alpha_presence=1.0, penalize_nl=0), {NL: -0.125}, NL
    S["newline_exempt"] = newline_exempt

    def newline_penalised(row, head, tail0):
        row[NL], row[34] = 9.5, 9.25
        return [NL, NL], dict(repeat_penalty=1.3, alpha_presence=1.0, penalize_nl=1), {NL: -0.125}, 34
    S["newline_penalised"] = newline_penalised

    def empty_table(row, head, tail0):                                       # a neutral conversation inside the launch
        return [5, 6, 7], {}, {}, None
    S["empty_table"] = empty_table

    def table_64(row, head, tail0):
        ids = _others(n_vocab, 64)                                           # 64 distinct ids where the vocabulary has them; the first 8 twice
        return ids[:8] + ids, dict(repeat_penalty=1.1, alpha_frequency=0.25, repeat_last_n=-1), {}, None
    S["table_64"] = table_64

    if n_vocab >= 2000:
        def table_1280(row, head, tail0):                                    # 1024 distinct window ids and 256 other bias ids
            rng = np.random.default_rng(n_vocab)
            ids = [int(i) for i in rng.choice(n_vocab, 1280, replace=False)]
            return ids[:1024], dict(repeat_penalty=1.2, alpha_presence=0.5, repeat_last_n=-1), {i: float(rng.standard_normal()) for i in ids[1024:]}, None
        S["table_1280"] = table_1280
    return S


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_kernel_against_numpy_and_host(gpu_lib, rows, n_vocab, ld):
    lib = gpu_lib
    scen = list(_scenarios(n_vocab).items())
    empty = dict(scen)["empty_table"]
    per = rows - 1 if rows > 1 else 1                                        # the last row of every multi-row launch has an empty table
    for first in range(0, len(scen), per):                                   # launches of `rows` rows until every scenario has run (the two large shapes: one launch)
        buf = np.full((rows, ld), 1e9, np.float32)                            # the stride's padding would win every pick if it were read
        row_words, table, want_rows, host_rows, spans, names = [], [], [], [], [], []
        for r in range(rows):
            name, fn = ("empty_table", empty) if rows > 1 and r == rows - 1 else scen[(first + r) % len(scen)]
            head, tail0 = _head_tail(r, n_vocab, ld)
            x = np.minimum(make_row(n_vocab, 1000 * n_vocab + first + r), np.float32(8.0))
            hist, kw, bias, pick = fn(x, head, tail0)
            buf[r, :n_vocab] = x
            host, tab, flags = lib.amd_test_penalise_host(x, hist, 4096, bias=bias, **kw)
            want = penalise_ref(x, hist, 4096, bias=bias, **kw)
            assert np.array_equal(bits(host), bits(want)), name
            if pick is not None:
                assert first_max(want) == pick, (name, first_max(want), pick)   # the scenario is what its name says
            p = dict(repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0)
            p.update({k: v for k, v in kw.items() if k in p})
            row_words.append([r, len(table), len(tab), flags, _f32_word(p["repeat_penalty"]), _f32_word(p["alpha_frequency"]), _f32_word(p["alpha_presence"]), 0])
            spans.append((len(table), len(tab)))
            table += tab.tolist()
            want_rows.append(want); host_rows.append(host); names.append(name)
        tb = np.array(table, np.int32).reshape(-1, 4)
        picked, adj, ms = lib.amd_test_pen_pick(buf, n_vocab, np.array(row_words, np.int32), tb)
        print("rows %d n_vocab %d ld %d: %d table entries, %.3f ms" % (rows, n_vocab, ld, len(tb), ms))
        for r in range(rows):
            assert int(picked[r]) == first_max(want_rows[r]), (names[r], r, int(picked[r]), first_max(want_rows[r]))
            off, n = spans[r]
            ids = tb[off:off + n, 0]
            assert np.array_equal(bits(adj[off:off + n]), bits(want_rows[r][ids])), names[r]
            assert np.array_equal(bits(adj[off:off + n]), bits(host_rows[r][ids])), names[r]
        sizes = {n for _, n in spans}
        if rows >= 64:
            assert {0, 1, 64, 1280} <= sizes, sizes
        if rows > 1:
            assert 0 in sizes                                                 # an empty table inside a multi-row launch


# ------------------------------------------------------------------------------------------------ helpers of the engine tests
def _load(lib, tiny_files, wtype="q5_k", mix="q5_k_m", conditioned=False, n_conv=1, seed=1337):
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm(wtype, mix=mix, conditioned=conditioned), verbosity=0, seed=seed, n_ctx=N_CTX, n_batch=32)
    if n_conv > 1:
        lib.amd_set_conversations(ctx, n_conv)
    return ctx


def _chat_tokens(lib, ctx, s):
    """the rows minigpt4_begin_chat queues"""
    return lib.amd_tokenize(ctx, b"Human: ", True) + lib.amd_tokenize(ctx, s.encode(), True) + lib.amd_tokenize(ctx, b"### Assistant:", True)


def _image_tokens(lib, ctx, s):
    return (lib.amd_tokenize(ctx, b"Human: <Img>", True) + [-1] * 32 + lib.amd_tokenize(ctx, b"</Img> ", True) + lib.amd_tokenize(ctx, s.encode(), True)
            + lib.amd_tokenize(ctx, b"### Assistant:", True))


def _embedding(seed=7):
    from minigpt4_cpp_amd import minigpt4_library as ML
    arr = (np.random.default_rng(seed).standard_normal(32 * 4096) * 0.5).astype(np.float32)
    emb = ML.MiniGPT4Embedding()
    emb.data = arr.ctypes.data_as(F32P)
    emb.n_embeddings = arr.size
    return emb, arr                                                          # keep `arr` alive while `emb` is in use


def _sample_id(lib, ctx, temp=0.0, top_k=40):
    """minigpt4_amd_sample: the pick with the conversation's stored parameters, nothing advanced"""
    tid = np.zeros(1, np.int32)
    assert lib.library.minigpt4_amd_sample(ctx.ptr, tid.ctypes.data_as(I32P), temp, top_k, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
    return int(tid[0])


def _want(lib, ctx, hist, params, bias=()):
    """numpy's pick from the context's raw logits row"""
    return first_max(penalise_ref(lib.amd_logits(ctx), hist, N_CTX, bias=bias, **params))


_RUNS = {}


def _greedy_run(lib, tiny_files, wtype, mix):
    """Test 4's run, once per file: dict(ids: A's 24 + 6 ids, raw: B's raw greedy id at each step, info: A's counters, history: A's token history, fed: the rows fed).
    A: mode on, minigpt4_end_chat(temp 0, PEN13); B: mode off, fed A's ids; every id is checked against numpy on B's row as it is produced."""
    key = (wtype, mix)
    if key in _RUNS:
        return _RUNS[key]
    a, b = _load(lib, tiny_files, wtype, mix), _load(lib, tiny_files, wtype, mix)
    try:
        lib.amd_set_penalties(a, True)
        assert lib.amd_penalty_info(a) == dict(mode=1, launches=0, host_rows=0, last_entries=0)
        fed, ids, raw_ids = [], [], []

        def step():
            row = lib.amd_logits(b)
            want = first_max(penalise_ref(row, fed, N_CTX, **PEN13))
            lib.minigpt4_end_chat(a, temp=0.0, **PEN13)
            got = int(lib.amd_token_history(a)[-1])
            assert got == want, (len(ids), got, want)
            ids.append(got); raw_ids.append(first_max(row))
            lib.amd_eval_tokens(b, [got]); fed.append(got)
        for c in (a, b):
            lib.minigpt4_begin_chat(c, PROMPT)
        fed += _chat_tokens(lib, a, PROMPT)
        for _ in range(24):
            step()
        emb, keep = _embedding()
        for c in (a, b):
            lib.minigpt4_begin_chat_image(c, emb, "hi")
        fed += _image_tokens(lib, a, "hi")
        for _ in range(6):                                                   # the window of 64 now holds the 32 image rows
            step()
        del keep
        _RUNS[key] = dict(ids=ids, raw=raw_ids, info=lib.amd_penalty_info(a), history=lib.amd_token_history(a).tolist(), fed=list(fed),
                          info_b=lib.amd_penalty_info(b), history_b=lib.amd_token_history(b).tolist())
    finally:
        lib.minigpt4_free(a); lib.minigpt4_free(b)
    return _RUNS[key]


FILES = [("q5_k", "q5_k_m"), ("f16", "none")]


# ------------------------------------------------------------------------------------------------ 4. greedy end to end
@pytest.mark.parametrize("wtype,mix", FILES)
def test_greedy_end_to_end_against_a_fed_twin(gpu_lib, tiny_files, wtype, mix):
    run = _greedy_run(gpu_lib, tiny_files, wtype, mix)
    differ = sum(i != r for i, r in zip(run["ids"][:24], run["raw"][:24]))
    print("ids that differ from the raw greedy id: %d of 24" % differ)
    assert differ >= 3, differ                                               # not vacuous
    assert run["info"] == dict(mode=1, launches=30, host_rows=0, last_entries=run["info"]["last_entries"])   # one launch per step, no host rows
    assert 0 < run["info"]["last_entries"] <= 32                             # 64 rows of window, 32 of them image rows
    assert run["history"] == run["fed"] and run["history_b"] == run["fed"]
    assert run["info_b"] == dict(mode=0, launches=0, host_rows=0, last_entries=0)


# ------------------------------------------------------------------------------------------------ 5. batched
BATCH_PROMPTS = ["what is in the picture?", "describe it", "colour?", "how many are there?", "where is it?"]
BATCH_PARAMS = [dict(NEUTRAL, repeat_penalty=0.25), dict(NEUTRAL), dict(NEUTRAL), dict(NEUTRAL, alpha_frequency=-3.0), dict(NEUTRAL, repeat_penalty=0.25, repeat_last_n=-1, penalize_nl=0)]
BATCH_BIAS = [{}, {}, {90: -50.0, 302: -50.0, 41: 8.0}, {}, {}]             # conversation 1 is neutral, conversation 2 bias only


@pytest.mark.parametrize("B", [1, 3, 5])
def test_batched_step_equals_twins_one_launch_per_step(gpu_lib, tiny_files, B):
    lib = gpu_lib
    steps = 10
    ctx, twin = _load(lib, tiny_files, conditioned=True, n_conv=B), _load(lib, tiny_files, conditioned=True)
    try:
        lib.amd_set_penalties(ctx, True); lib.amd_set_penalties(twin, True)
        slots = list(range(B))
        for k in slots:
            lib.amd_select_conversation(ctx, k)
            lib.minigpt4_begin_chat(ctx, BATCH_PROMPTS[k])
            lib.amd_conversation_penalties(ctx, k, **BATCH_PARAMS[k])
            lib.amd_set_logit_bias(ctx, BATCH_BIAS[k])
        got = [[] for _ in slots]
        ranks = []
        for s in range(steps):
            if s == 4:                                                       # the report: log-probability and rank of the PICKED id, alternatives, all from the raw row
                want_ids = []
                for k in slots:
                    lib.amd_select_conversation(ctx, k)
                    want_ids.append(_want(lib, ctx, lib.amd_token_history(ctx), BATCH_PARAMS[k], BATCH_BIAS[k]))
                before = lib.amd_top_logprobs(ctx, slots, top_n=5, targets=want_ids)
                launches = lib.amd_penalty_info(ctx)["launches"]
                st = lib.amd_end_chat_batch_top(ctx, slots, top_n=5, temp=0.0)
                assert st["ids"].tolist() == want_ids
                assert np.array_equal(bits(st["logprob"]), bits(before["logprob"])) and np.array_equal(st["rank"], before["rank"])
                assert np.array_equal(st["top_ids"], before["top_ids"]) and np.array_equal(bits(st["top_logprobs"]), bits(before["top_logprobs"]))
                assert lib.amd_penalty_info(ctx)["launches"] == launches + 1
                ranks = st["rank"].tolist()
                for k in slots:
                    got[k].append(int(st["ids"][k]))
            else:
                lib.amd_end_chat_batch(ctx, slots, temp=0.0)
                for k in slots:
                    lib.amd_select_conversation(ctx, k)
                    got[k].append(int(lib.amd_token_history(ctx)[-1]))
        info = lib.amd_penalty_info(ctx)
        assert info["launches"] == steps and info["host_rows"] == 0, info   # one launch per step, not B
        assert ranks[0] > 0, ranks                                           # the penalised pick was not the raw greedy token: the report describes the raw row
        if B > 1:
            assert ranks[1] == 0                                             # the neutral conversation picks the raw greedy token
        for k in slots:                                                      # the same conversation alone, through minigpt4_end_chat with its parameters as arguments
            lib.minigpt4_reset_chat(twin)
            lib.amd_set_logit_bias(twin, BATCH_BIAS[k])
            lib.minigpt4_begin_chat(twin, BATCH_PROMPTS[k])
            alone = []
            for s in range(steps):
                lib.minigpt4_end_chat(twin, temp=0.0, **BATCH_PARAMS[k])
                alone.append(int(lib.amd_token_history(twin)[-1]))
            assert got[k] == alone, (k, got[k], alone)
    finally:
        lib.minigpt4_free(ctx); lib.minigpt4_free(twin)


# ------------------------------------------------------------------------------------------------ 6. host path
@pytest.mark.parametrize("wtype,mix", FILES)
def test_host_path_top_k_1_equals_the_greedy_run(gpu_lib, tiny_files, wtype, mix):
    lib = gpu_lib
    run = _greedy_run(lib, tiny_files, wtype, mix)
    a, b = _load(lib, tiny_files, wtype, mix), _load(lib, tiny_files, wtype, mix)
    try:
        lib.amd_set_penalties(a, True)
        for c in (a, b):
            lib.minigpt4_begin_chat(c, PROMPT)
        lib.amd_logits(b)                                                    # the prompt as its own pass, as A's first sample runs it (a row's bits depend on the rows of its pass)
        ids = []
        for s in range(24):
            lib.minigpt4_end_chat(a, temp=0.8, top_k=1, **PEN13)            # the chain runs; one candidate survives: deterministic
            ids.append(int(lib.amd_token_history(a)[-1]))
            lib.amd_eval_tokens(b, [ids[-1]])
            lib.amd_logits(b)                                                # evaluated row by row, like A's steps: the twins' rows are then the same bits
        assert ids == run["ids"][:24]
        assert lib.amd_penalty_info(a) == dict(mode=1, launches=0, host_rows=24, last_entries=0)
        # the cached host row stays raw: sample without advancing, then read the logits
        before = lib.amd_logits(a)
        assert _sample_id(lib, a, temp=0.8, top_k=1) == _want(lib, b, lib.amd_token_history(b), PEN13)
        assert lib.amd_penalty_info(a)["host_rows"] == 25
        after = lib.amd_logits(a)
        assert np.array_equal(bits(before), bits(after)) and np.array_equal(bits(after), bits(lib.amd_logits(b)))
    finally:
        lib.minigpt4_free(a); lib.minigpt4_free(b)


def test_host_path_mirostat_two_identical_runs(gpu_lib, tiny_files):
    lib = gpu_lib
    outs = []
    for _ in range(2):
        ctx = _load(lib, tiny_files, seed=99)
        try:
            lib.amd_set_penalties(ctx, True)
            lib.minigpt4_begin_chat(ctx, PROMPT)
            for s in range(8):
                lib.minigpt4_end_chat(ctx, temp=0.8, mirostat=2, **dict(PEN13, alpha_frequency=0.25))
            outs.append(lib.amd_token_history(ctx).tolist())
            assert lib.amd_penalty_info(ctx) == dict(mode=1, launches=0, host_rows=8, last_entries=0)
        finally:
            lib.minigpt4_free(ctx)
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ 7. state
def test_history_follows_every_operation(gpu_lib, tiny_files):
    lib = gpu_lib
    P = dict(NEUTRAL, repeat_penalty=0.25, repeat_last_n=16, alpha_frequency=-0.5)
    ctx = _load(lib, tiny_files, conditioned=True, n_conv=3)
    try:
        lib.amd_set_penalties(ctx, True)
        lib.amd_set_speculation(ctx, 3)
        for k in range(3):
            lib.amd_conversation_penalties(ctx, k, **P)
        picks = []

        def check(fed):
            """the history is `fed`, and one penalised pick agrees with numpy on this state"""
            assert lib.amd_token_history(ctx).tolist() == fed
            launches = lib.amd_penalty_info(ctx)["launches"]
            want = _want(lib, ctx, fed, P)
            assert _sample_id(lib, ctx) == want
            assert lib.amd_penalty_info(ctx)["launches"] == launches + 1
            picks.append(want != first_max(lib.amd_logits(ctx)))
        lib.minigpt4_begin_chat(ctx, PROMPT)
        fed = _chat_tokens(lib, ctx, PROMPT)
        check(fed)
        lib.minigpt4_reset_chat(ctx)                                         # reset empties it
        assert lib.amd_token_history(ctx).tolist() == []
        lib.minigpt4_begin_chat(ctx, PROMPT)
        for s in range(3):
            lib.minigpt4_end_chat(ctx, temp=0.0, **P)
        fed = fed + lib.amd_token_history(ctx).tolist()[len(fed):]
        assert len(fed) == len(_chat_tokens(lib, ctx, PROMPT)) + 3
        check(fed)
        lib.amd_fork_conversation(ctx, 0, [1], -1)                           # a full fork copies it
        lib.amd_fork_conversation(ctx, 0, [2], 10)                           # a prefix fork copies the prefix
        lib.amd_select_conversation(ctx, 1)
        check(fed)
        lib.amd_select_conversation(ctx, 2)
        assert lib.amd_token_history(ctx).tolist() == fed[:10]
        lib.amd_eval_tokens(ctx, [fed[3], fed[4], 77])
        check(fed[:10] + [fed[3], fed[4], 77])
        lib.amd_select_conversation(ctx, 0)
        lib.amd_shift_context(ctx, 4, 8)                                     # exactly the discarded rows leave; the next pick sees the shortened window
        fed = fed[:4] + fed[12:]
        check(fed)
        toks = [fed[-1], fed[-2], 300, 301, fed[-1]]
        lib.amd_score_tokens(ctx, toks)                                      # scoring appends what it evaluates
        fed = fed + toks
        check(fed)
        out = lib.amd_verify_draft(ctx, [fed[-2], 5, 6])                     # verification appends the rows it keeps
        kept = out["ids"].tolist()
        assert 1 <= len(kept) <= 4
        fed = fed + kept
        check(fed)
        lib.amd_eval_embd(ctx, np.zeros((2, 256), np.float32) + 0.25)        # embedding rows enter as -1 (queued rows count: the history call evaluates them)
        fed = fed + [-1, -1]
        check(fed)
        assert any(picks), picks                                             # at least one of those picks was not the raw greedy token
        lib.amd_set_conversations(ctx, 2)                                    # set_conversations clears
        for k in range(2):
            lib.amd_select_conversation(ctx, k)
            assert lib.amd_token_history(ctx).tolist() == []
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 8. off means off
def test_off_means_off_and_refusals_change_nothing(gpu_lib, tiny_files):
    lib, L = gpu_lib, gpu_lib.library
    ZERO = dict(launches=0, host_rows=0, last_entries=0)
    ctx = _load(lib, tiny_files, n_conv=2)
    try:
        def run(**kw):
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_begin_chat(ctx, PROMPT)
            return [lib.minigpt4_end_chat(ctx, temp=0.0, **kw) for _ in range(8)], lib.amd_token_history(ctx).tolist()
        neutral = run(**NEUTRAL)
        assert run(**WILD) == neutral                                        # the mode is off: the arguments are ignored, like the reference
        assert lib.amd_penalty_info(ctx) == dict(mode=0, **ZERO)
        lib.amd_conversation_penalties(ctx, 0, **WILD)                       # stored parameters count only while the mode is on
        assert run(**WILD) == neutral and lib.amd_end_chat_batch(ctx, [0], temp=0.0) is not None
        assert lib.amd_penalty_info(ctx) == dict(mode=0, **ZERO)
        lib.amd_set_penalties(ctx, True)
        assert run(**NEUTRAL) == neutral                                     # the mode is on, the parameters are neutral: no launch, no host row
        assert lib.amd_penalty_info(ctx) == dict(mode=1, **ZERO)
        assert run(**WILD) != neutral and lib.amd_penalty_info(ctx)["launches"] == 8
        # refusals: 1, the call's prefix, nothing changed
        lib.amd_conversation_penalties(ctx, 0, **dict(NEUTRAL, repeat_penalty=0.25))
        lib.amd_set_logit_bias(ctx, {41: 8.0, 90: -np.inf})                  # -inf is allowed
        hist = lib.amd_token_history(ctx).tolist()
        pick = _sample_id(lib, ctx)
        assert pick == _want(lib, ctx, hist, dict(NEUTRAL, repeat_penalty=0.25), {41: 8.0, 90: -np.inf})
        err = lambda: (L.minigpt4_amd_last_error() or b"").decode()
        for args in ((2, 64, 1.1, 0.0, 0.0, 1), (-1, 64, 1.1, 0.0, 0.0, 1), (0, 64, 0.0, 0.0, 0.0, 1), (0, 64, -1.0, 0.0, 0.0, 1), (0, 64, float("inf"), 0.0, 0.0, 1),
                     (0, 64, float("nan"), 0.0, 0.0, 1), (0, 64, 1.1, float("inf"), 0.0, 1), (0, 64, 1.1, 0.0, float("nan"), 1)):
            assert L.minigpt4_amd_conversation_penalties(ctx.ptr, *args) == 1 and err().startswith("conversation_penalties: "), args
        for pairs in ([(3, float("nan"))], [(3, float("inf"))], [(-1, 1.0)], [(512, 1.0)], [(3, 1.0), (4, 1.0), (3, 2.0)], [(i, 1.0) for i in range(257)]):
            with pytest.raises(RuntimeError, match="set_logit_bias failed: set_logit_bias: "):
                lib.amd_set_logit_bias(ctx, pairs)
        lib.minigpt4_end_chat(ctx, temp=0.0, **dict(NEUTRAL, repeat_penalty=-2.0))   # refused parameters are not stored: the step uses the stored ones
        assert int(lib.amd_token_history(ctx)[-1]) == pick and err().startswith("conversation_penalties: ")
        assert lib.amd_token_history(ctx).tolist() == hist + [pick]
        lib.amd_set_logit_bias(ctx, None)                                    # n = 0 clears
        hist = hist + [pick]
        assert _sample_id(lib, ctx) == _want(lib, ctx, hist, dict(NEUTRAL, repeat_penalty=0.25))
        # a bias is active whatever the mode
        lib.amd_set_penalties(ctx, False)
        lib.amd_set_logit_bias(ctx, {41: 50.0})
        assert _sample_id(lib, ctx) == 41 == _want(lib, ctx, hist, NEUTRAL, {41: 50.0})
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 9. server
def test_server_keywords(gpu_lib, tmpdir_models):
    import os
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp, lp = os.path.join(tmpdir_models, "vision_serve_pen.bin"), os.path.join(tmpdir_models, "llm_serve_pen.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)                       # tests/test_gpu_serve.py's model
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3 + i), p, 12) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)           # waves of 2 + 1
    try:
        plain = srv.run(reqs, temp=0.0, ignore_eos=True)
        got = srv.run(reqs, temp=0.0, ignore_eos=True, repeat_penalty=1.3)
        alone = [srv.run([r], temp=0.0, ignore_eos=True, repeat_penalty=1.3)[0] for r in reqs]
        assert got == alone
        assert any(a != b for a, b in zip(got, plain)), (got, plain)         # not vacuous: the keyword changes an answer
        info = srv.lib.amd_penalty_info(srv.ctx)
        assert info["mode"] == 0 and info["launches"] > 0 and info["host_rows"] == 0   # the call takes its settings back
        assert srv.run(reqs, temp=0.0, ignore_eos=True) == plain
        banned = srv.run(reqs[:1], temp=0.0, ignore_eos=True, logit_bias={i: -np.inf for i in range(0, 512, 2)})
        assert banned != plain[:1]
    finally:
        srv.close()
