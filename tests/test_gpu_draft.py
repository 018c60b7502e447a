"""Draft verification (minigpt4_amd_verify_draft) and greedy lookup decoding (minigpt4_amd_decode_lookup) on the GPU (include/minigpt4_amd.h "speculation").
The attention launch alone must be bit-identical to one launch of the batched decode kernel per row; through the C ABI a pass must keep exactly the tokens plain
greedy decoding emits (the CPU oracle's), leave the conversation where those tokens lead, and never let a rejected row leak into what follows."""
import ctypes

import numpy as np
import pytest

from conftest import observed_bar, record_observed

pytestmark = pytest.mark.gpu

TRIPLES = [("q4_0", "none"), ("q5_k", "q5_k_m"), ("f16", "none")]
PROMPT = b"what is the text in the picture?"
I32P = ctypes.POINTER(ctypes.c_int32)
N_ORACLE = 48
_ORACLE = {}


def oracle(lp, n=N_ORACLE, n_ctx=256):
    """The CPU oracle's greedy continuation after system_prompt + begin_chat(PROMPT): (ids [n], logits [n + 1][n_vocab]: row k = after ids[:k], n_past before id 0).  Once per file."""
    if lp not in _ORACLE:
        import refcpu as R
        from minigpt4_cpp_amd import modelgen as G
        c = R.OracleChat(R.OracleLLM(G.read_llm_file(lp), n_ctx=n_ctx), n_batch=32)
        c.system_prompt()
        c.begin_chat(PROMPT)
        n0, ids, logits = c.llm.n_past, [], [c.llm.logits.copy()]
        for _ in range(n):
            ids.append(int(c.end_chat(temp=0.0)[0]))
            logits.append(c.llm.logits.copy())
        lg = np.stack(logits)
        lg.setflags(write=False)
        _ORACLE[lp] = (tuple(ids), lg, n0)
    return _ORACLE[lp]


def begin(lib, ctx):
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.minigpt4_begin_chat(ctx, PROMPT.decode())


def n_past(lib, ctx):
    return lib.library.minigpt4_amd_n_past(ctx.ptr)


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
def _attn_case(lib, hd, n_ctx, R, p0, seed, computed=True):
    n_head, n_slot, slot = 2, 2, 1
    E = n_head * hd
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((R, E)).astype(np.float32) for _ in range(3))
    kc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
    new = lib.amd_test_attn_draft(0, q, k, v, kc, vc, n_head, slot, p0, computed_exp=computed)
    ref = lib.amd_test_attn_draft(1, q, k, v, kc, vc, n_head, slot, p0, computed_exp=computed)
    tag = (hd, n_ctx, R, p0, computed)
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0, tag
    assert np.array_equal(new[0], ref[0]), (tag, float(np.abs(new[0] - ref[0]).max()))
    assert np.array_equal(new[1], ref[1]) and np.array_equal(new[2], ref[2]), tag
    assert np.array_equal(new[1][0], kc[0]) and np.array_equal(new[2][0], vc[0]), tag                  # the other conversation's cache
    assert np.array_equal(new[1][1, :p0], kc[1, :p0]) and np.array_equal(new[1][1, p0 + R:], kc[1, p0 + R:]), tag   # only the R appended rows changed
    assert np.array_equal(new[2][1, :p0], vc[1, :p0]) and np.array_equal(new[2][1, p0 + R:], vc[1, p0 + R:]), tag
    assert not np.array_equal(new[1][1, p0:p0 + R], kc[1, p0:p0 + R]), tag


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_attention_launch_is_bit_identical_to_one_batched_launch_per_row(gpu_lib, hd, R):
    """n_ctx 544: positions 0, 1 (no / one cached key), 31 (inside one round of partitions), 508 / 512 / 520 around the 512 keys HD 128 prefetches (508 with 8 rows
    straddles it: the pass's own rows fall on both sides)."""
    for p0 in (0, 1, 31, 508, 512, 520):
        _attn_case(gpu_lib, hd, 544, R, p0, seed=1000 * hd + 10 * p0 + R)


@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_attention_launch_around_the_prefetch_of_head_size_64(gpu_lib, R):
    """HD 64 prefetches 1 024 keys: positions 1020 (the rows straddle it) and 1030 (behind it), n_ctx 1040."""
    for p0 in (1020, 1030):
        _attn_case(gpu_lib, 64, 1040, R, p0, seed=77 * p0 + R)


def test_attention_launch_with_the_exp_table(gpu_lib):
    """The gathered fp16 exp table instead of the computed form (MINIGPT4_COMPUTED_TABLES=0 contexts), and head size 32."""
    for hd, R, p0 in ((128, 8, 508), (64, 5, 31), (32, 8, 250), (32, 3, 0)):
        _attn_case(gpu_lib, hd, 544, R, p0, seed=5 + hd + p0, computed=False)
    _attn_case(gpu_lib, 32, 544, 8, 250, seed=9, computed=True)


# ---------------------------------------------------------------------------------------------------------------- through the C ABI
@pytest.fixture(scope="module")
def contexts(gpu_lib, tiny_files):
    """One context per file (n_ctx 256, speculation on at 7): the tests restart its conversation, so every row count's pass is captured once."""
    vp, llm = tiny_files
    made = {}

    def get(wtype, mix):
        if (wtype, mix) not in made:
            lp = llm(wtype, mix, conditioned=True)
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
            gpu_lib.amd_set_speculation(ctx, 7)
            made[(wtype, mix)] = (ctx, lp)
        return made[(wtype, mix)]
    yield get
    for ctx, _ in made.values():
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
@pytest.mark.parametrize("n_draft", [0, 1, 3, 4, 7])
def test_all_correct_drafts_are_kept_and_logits_match_the_oracle(gpu_lib, contexts, wtype, mix, n_draft):
    """Drafts taken from the oracle's own continuation: every pass keeps all of them, the ids are the oracle's, the position is the oracle's, and after every pass the
    conversation's logits are the oracle's after the same ids (1e-2 of the largest |logit|, and 2 x the recorded error)."""
    ctx, lp = contexts(wtype, mix)
    G, LG, n0 = oracle(lp)
    begin(gpu_lib, ctx)
    got, worst = [], 0.0
    while len(got) < 16:
        nd = min(n_draft, 16 - len(got) - 1)
        r = gpu_lib.amd_verify_draft(ctx, G[len(got) + 1:len(got) + 1 + nd])
        assert len(r["ids"]) == 1 + nd, (len(got), r)
        got += [int(x) for x in r["ids"]]
        assert list(r["row_greedy"][:1 + nd]) == list(G[len(got) - nd:len(got) + 1]), (len(got), r)
        assert n_past(gpu_lib, ctx) == n0 + len(got)
        want = LG[len(got)]
        err = float(np.abs(gpu_lib.amd_logits(ctx) - want).max() / np.abs(want).max())
        worst = max(worst, err)
    print(f"verify_draft {wtype}/{mix} n_draft={n_draft}: logits vs oracle {worst:.3e} of the largest |logit|")
    assert got == list(G[:16])
    key = f"verify_draft_{wtype}_{mix}"
    record_observed(key, worst)
    assert worst <= observed_bar(key), (worst, observed_bar(key))


@pytest.mark.parametrize("wtype,mix", TRIPLES)
@pytest.mark.parametrize("n_draft", [3, 7])
def test_first_wrong_token_ends_the_accepted_run(gpu_lib, contexts, wtype, mix, n_draft):
    ctx, lp = contexts(wtype, mix)
    G, _, n0 = oracle(lp)
    n_vocab = gpu_lib.library.minigpt4_amd_n_vocab(ctx.ptr)
    for j in range(n_draft):
        begin(gpu_lib, ctx)
        d = list(G[1:1 + n_draft])
        d[j] = (d[j] + 1) % n_vocab
        r = gpu_lib.amd_verify_draft(ctx, d)
        assert list(r["ids"]) == list(G[:1 + j]), (j, r)
        assert int(r["row_greedy"][j]) == G[j + 1], (j, r)                  # the token the wrong guess stood for
        assert n_past(gpu_lib, ctx) == n0 + 1 + j
        k = 1 + j
        r = gpu_lib.amd_verify_draft(ctx, G[k + 1:k + 1 + n_draft])
        assert list(r["ids"]) == list(G[k:k + 1 + n_draft]), (j, r)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_rejected_rows_do_not_reach_later_tokens(gpu_lib, tiny_files, wtype, mix):
    """Two forks get drafts that agree up to a wrong token at index 2 and differ in every later entry: equal results, equal logits, also four plain steps later (the
    rejected rows sit in the caches above n_past until those steps overwrite them)."""
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    G, _, n0 = oracle(lp)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        gpu_lib.amd_set_conversations(ctx, 3)
        gpu_lib.amd_set_speculation(ctx, 7)
        begin(gpu_lib, ctx)
        gpu_lib.amd_fork_conversation(ctx, 0, [1, 2])
        n_vocab = gpu_lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        wrong = (G[3] + 1) % n_vocab
        drafts = {1: [G[1], G[2], wrong, 7, 8, 9], 2: [G[1], G[2], wrong, 10, 11, 12]}
        out = {}
        for s in (1, 2):
            gpu_lib.amd_select_conversation(ctx, s)
            r = gpu_lib.amd_verify_draft(ctx, drafts[s])
            assert list(r["ids"]) == list(G[:3]), (s, r)
            assert n_past(gpu_lib, ctx) == n0 + 3
            out[s] = [gpu_lib.amd_logits(ctx).copy()]
        assert np.array_equal(out[1][0], out[2][0])
        for s in (1, 2):
            gpu_lib.amd_select_conversation(ctx, s)
            out[s].append([gpu_lib.minigpt4_end_chat(ctx, temp=0.0) for _ in range(4)])
            out[s].append(gpu_lib.amd_logits(ctx).copy())
        assert out[1][1] == out[2][1]
        assert np.array_equal(out[1][2], out[2][2])
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_one_row_pass_equals_the_batched_step(gpu_lib, tiny_files, wtype, mix):
    """n_draft = 0 is forward_batch at one row with the new attention launch and epilogue: bit-identical logits to a forked twin advanced by minigpt4_amd_eval_batch."""
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        gpu_lib.amd_set_conversations(ctx, 2)
        gpu_lib.amd_set_speculation(ctx, 1)
        begin(gpu_lib, ctx)
        gpu_lib.amd_fork_conversation(ctx, 0, [1])
        r = gpu_lib.amd_verify_draft(ctx, [])
        assert len(r["ids"]) == 1
        a = gpu_lib.amd_logits(ctx).copy()
        assert gpu_lib.amd_eval_batch(ctx, [1], [int(r["ids"][0])]) == [int(r["ids"][0])]
        gpu_lib.amd_select_conversation(ctx, 1)
        assert np.array_equal(gpu_lib.amd_logits(ctx), a)
        assert int(np.argmax(a)) == int(r["row_greedy"][0])
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_parity_mode_is_plain_greedy_decoding_bit_for_bit(gpu_lib, tiny_files, wtype, mix):
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    G, _, n0 = oracle(lp)
    n_vocab = 512
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    ref = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        for c in (ctx, ref):
            gpu_lib.amd_set_parity(c, True)
        gpu_lib.amd_set_speculation(ctx, 3)

        def step(draft, want_ids):
            r = gpu_lib.amd_verify_draft(ctx, draft)
            assert list(r["ids"]) == list(want_ids), r
            for _ in want_ids:
                gpu_lib.minigpt4_end_chat(ref, temp=0.0)
            assert n_past(gpu_lib, ctx) == n_past(gpu_lib, ref)
            assert np.array_equal(gpu_lib.amd_logits(ctx), gpu_lib.amd_logits(ref))
        begin(gpu_lib, ctx)
        begin(gpu_lib, ref)
        for k in range(0, 16, 4):                                               # all-correct drafts of 3
            step(G[k + 1:k + 4], G[k:k + 4])
        begin(gpu_lib, ctx)
        begin(gpu_lib, ref)
        step([G[1], (G[2] + 1) % n_vocab, G[3]], G[:2])                         # first wrong token at index 1
        step(G[3:6], G[2:6])
    finally:
        gpu_lib.minigpt4_free(ctx)
        gpu_lib.minigpt4_free(ref)


_WIDE = {}


def _wide_oracle(lp):
    if lp not in _WIDE:
        import refcpu as R
        from minigpt4_cpp_amd import modelgen as G
        c = R.OracleChat(R.OracleLLM(G.read_llm_file(lp, in_memory=True), n_ctx=512), n_batch=512)
        c.system_prompt()
        c.begin_chat(PROMPT)
        _WIDE[lp] = tuple(int(c.end_chat(temp=0.0)[0]) for _ in range(8))
    return _WIDE[lp]


@pytest.mark.parametrize("image", [False, True])
def test_13b_width_passes_take_the_batched_launches(gpu_lib, image):
    """The two-layer 13B-width k-quant file: R = 2 on the v_dot4 multi-row launches, R = 4 on the row-interleaved MFMA launches when the context has that image
    (set_conversations(2) builds it, set_speculation never does), R = 5 and 8 on the int8-MFMA set launches -- the ids are the oracle's on every path."""
    import headline as H
    vp, lp = H.headline_files("13b_l2")
    G = _wide_oracle(lp)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=64)
    try:
        if image:
            gpu_lib.amd_set_conversations(ctx, 2)
            gpu_lib.amd_set_conversations(ctx, 1)
        gpu_lib.amd_set_speculation(ctx, 7)
        for R in (2, 4, 5, 8):
            begin(gpu_lib, ctx)
            got = []
            while len(got) < 8:
                nd = min(R - 1, 8 - len(got) - 1)
                r = gpu_lib.amd_verify_draft(ctx, G[len(got) + 1:len(got) + 1 + nd])
                assert len(r["ids"]) == 1 + nd, (R, len(got), r)
                if not got:
                    path = gpu_lib.amd_batch_path(ctx)
                    assert path["rows"] == R, path
                    if R == 4:
                        assert (path["ri"] + path["ri_mix"] > 0) == image, path
                    if R >= 5:
                        assert path["sets"] > 0, path
                got += [int(x) for x in r["ids"]]
            assert got == list(G), (R, got, G)
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_edges_room_shift_and_refusals(gpu_lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as MG
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    L = gpu_lib.library
    prompt = [1] + [5 + (7 * i) % 300 for i in range(59)]
    o = R.OracleLLM(MG.read_llm_file(lp), n_ctx=128)                             # room for the continuation the 64-row context cannot hold
    o.eval_tokens(prompt)
    G = []
    for _ in range(8):
        G.append(int(np.argmax(o.logits)))
        o.eval_tokens([G[-1]])
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=32)
    ids, n_out, rg = np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(8, np.int32)
    ip = lambda a: a.ctypes.data_as(I32P)

    def refused(text, draft, n, ids_p=ip(ids), n_p=ip(n_out)):
        before, lg = n_past(gpu_lib, ctx), (gpu_lib.amd_logits(ctx).copy() if has_logits else None)
        d = np.array(draft if draft is not None else [0], np.int32)
        assert L.minigpt4_amd_verify_draft(ctx.ptr, ip(d) if draft is not None else None, n, ids_p, n_p, ip(rg)) == 1, text
        err = L.minigpt4_amd_last_error()
        assert err.startswith(b"verify_draft: ") and text in err, (text, err)
        assert n_past(gpu_lib, ctx) == before
        if has_logits:
            assert np.array_equal(gpu_lib.amd_logits(ctx), lg)
    try:
        gpu_lib.amd_eval_tokens(ctx, prompt)
        has_logits = True
        refused(b"speculation is off", G[1:3], 2)
        gpu_lib.amd_set_speculation(ctx, 7)
        # every listed refusal leaves the position and the logits alone
        refused(b"n_draft", G[1:3], -1)
        refused(b"draft is NULL", None, 2)
        refused(b"required", G[1:3], 2, ids_p=None)
        refused(b"required", G[1:3], 2, n_p=None)
        refused(b"out of range", [G[1], -1], 2)
        refused(b"out of range", [G[1], 512], 2)
        gpu_lib.amd_set_speculation(ctx, 3)
        refused(b"n_draft", G[1:5], 4)                                          # above max_draft
        gpu_lib.amd_set_speculation(ctx, 7)
        assert n_past(gpu_lib, ctx) == 60
        r = gpu_lib.amd_verify_draft(ctx, G[1:8])                               # room for 4 rows: the 7-token draft is cut to 3
        assert list(r["ids"]) == G[:4], r
        assert list(r["row_greedy"][:4]) == G[1:5] and list(r["row_greedy"][4:]) == [-1] * 4, r
        assert n_past(gpu_lib, ctx) == 64
        refused(b"context full", G[5:6], 1)
        refused(b"context full", [], 0)
        gpu_lib.amd_set_context_shift(ctx, 8)
        r = gpu_lib.amd_verify_draft(ctx, [3, 4])
        assert len(r["ids"]) >= 1 and n_past(gpu_lib, ctx) <= 64 and np.isfinite(gpu_lib.amd_logits(ctx)).all()
        gpu_lib.minigpt4_reset_chat(ctx)
        has_logits = False
        refused(b"no current logits", [3], 1)
        with pytest.raises(RuntimeError, match="set_speculation"):
            gpu_lib.amd_set_speculation(ctx, 8)
        gpu_lib.amd_set_speculation(ctx, 0)
        gpu_lib.amd_eval_tokens(ctx, prompt[:10])
        has_logits = True
        refused(b"speculation is off", [3], 1)
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_fork_after_a_rejected_pass_scores_like_the_source(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    G, _, n0 = oracle(lp)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        gpu_lib.amd_set_conversations(ctx, 2)
        gpu_lib.amd_set_speculation(ctx, 7)
        begin(gpu_lib, ctx)
        r = gpu_lib.amd_verify_draft(ctx, [G[1], (G[2] + 1) % 512, 9, 10, 11, 12, 13])     # five dead rows above n_past
        assert list(r["ids"]) == list(G[:2])
        gpu_lib.amd_fork_conversation(ctx, 0, [1])
        tokens = list(G[2:12])
        a = gpu_lib.amd_score_tokens(ctx, tokens)
        gpu_lib.amd_select_conversation(ctx, 1)
        assert n_past(gpu_lib, ctx) == n0 + 2
        b = gpu_lib.amd_score_tokens(ctx, tokens)
        assert np.array_equal(a["logprob"], b["logprob"]) and np.array_equal(a["greedy"], b["greedy"])
        assert list(a["greedy"][1:]) == tokens[1:] and int(a["greedy"][0]) == tokens[0]   # and the source continues the oracle's text
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_decode_lookup_emits_the_greedy_text_whatever_the_corpus(gpu_lib, contexts, wtype, mix):
    """48 tokens with the oracle's continuation as corpus, with no corpus, and with every third corpus token wrong: always the oracle's 48 greedy ids; passes + plain
    steps + accepted draft tokens account for every token.  (The </s> stop is not covered: no conditioned tiny file's continuation of these prompts holds id 2 within
    64 tokens on the CPU oracle -- all 64 ids are distinct.)"""
    ctx, lp = contexts(wtype, mix)
    G, _, n0 = oracle(lp)
    assert len(set(G)) == len(G) and 2 not in G
    bad = [g if i % 3 != 2 else (g + 1) % 512 for i, g in enumerate(G)]
    for name, corpus in (("exact", list(G)), ("empty", []), ("third_wrong", bad)):
        begin(gpu_lib, ctx)
        r = gpu_lib.amd_decode_lookup(ctx, corpus, N_ORACLE, ngram_max=3, ngram_min=1, n_draft=4)
        print(f"decode_lookup {wtype}/{mix} corpus={name}: {r['passes']} passes, {r['steps']} plain steps, {r['accepted']} of {r['sent']} draft tokens accepted")
        assert list(r["tokens"]) == list(G), (name, r)
        assert r["passes"] + r["steps"] + r["accepted"] == len(r["tokens"]) == N_ORACLE, (name, r)
        assert n_past(gpu_lib, ctx) == n0 + N_ORACLE
        if name == "empty":
            assert r["passes"] == 0 and r["sent"] == 0
        if name == "exact":
            assert r["accepted"] > 0 and r["passes"] + r["steps"] < N_ORACLE, r
    with pytest.raises(RuntimeError, match="decode_lookup: n_draft"):
        gpu_lib.amd_decode_lookup(ctx, [], 4, n_draft=8)


def test_speculation_is_refused_where_the_verify_attention_does_not_fit(gpu_lib, tiny_files):
    """The verify pass keeps 8 new key / value rows in the attention kernel's LDS where the decode step keeps one, so it ends at a smaller context than the load admits.
    Head size 64 (the tiny files): 160 KiB = 256 B static + 6 B per context row + q [64] + 2 x [8][64] fp16 + partial outputs [64][64] fp32 + 64 spare -> 24 160 rows.
    At that n_ctx a full 8-row pass launches (its LDS is sized by n_ctx) and keeps the oracle's tokens; 8 rows more, set_speculation refuses and the setting stays off."""
    vp, llm = tiny_files
    lp = llm("q4_0", "none", conditioned=True)
    G, _, _ = oracle(lp)
    fits = (160 * 1024 - (256 + 64 * 2 + 2 * 8 * 64 * 2 + 64 * 64 * 4 + 64)) // 6 // 8 * 8
    assert fits == 24160
    for n_ctx in (fits + 8, fits):
        ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=n_ctx, n_batch=32)
        try:
            if n_ctx > fits:
                with pytest.raises(RuntimeError, match="set_speculation: n_ctx"):
                    gpu_lib.amd_set_speculation(ctx, 7)
                begin(gpu_lib, ctx)
                with pytest.raises(RuntimeError, match="speculation is off"):
                    gpu_lib.amd_verify_draft(ctx, [G[1]])
                gpu_lib.amd_set_speculation(ctx, 0)                # switching off is never refused
            else:
                gpu_lib.amd_set_speculation(ctx, 7)
                begin(gpu_lib, ctx)
                assert list(gpu_lib.amd_verify_draft(ctx, list(G[1:8]))["ids"]) == list(G[:8])
        finally:
            gpu_lib.minigpt4_free(ctx)
