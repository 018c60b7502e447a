"""The verify pass over several conversations (minigpt4_amd_verify_draft_batch, minigpt4_amd_decode_lookup_batch, serve.ReplicaServer.run(lookup=...)) on the GPU.
The attention launch alone must be bit-identical to one launch of the single-conversation verify kernel per group and touch nothing else; the epilogue alone must follow
tests/draft_batch_ref.py; through the C ABI every conversation of a pass must keep exactly the tokens plain greedy decoding emits (the CPU oracle's), stand where those
tokens lead, and never let a rejected row -- its own or a neighbour's -- leak into what follows."""
import ctypes
import os

import numpy as np
import pytest

import draft_batch_ref as B
import greedy_ref as GR
from conftest import observed_bar, record_observed

pytestmark = pytest.mark.gpu

TRIPLES = [("q4_0", "none"), ("q5_k", "q5_k_m"), ("f16", "none")]
PROMPTS = (b"what is the text in the picture?", b"describe the image in detail", b"hello there, who are you?")
I32P = ctypes.POINTER(ctypes.c_int32)
N_ORACLE = 40
_ORACLE = {}


def oracle(lp, prompt, n=N_ORACLE, n_ctx=256):
    """The CPU oracle's greedy continuation after system_prompt + begin_chat(prompt): (ids [n], logits [n + 1][n_vocab]: row k = after ids[:k], n_past before id 0).
    Once per (file, prompt), shared and read-only."""
    if (lp, prompt) not in _ORACLE:
        import refcpu as R
        from minigpt4_cpp_amd import modelgen as G
        c = R.OracleChat(R.OracleLLM(G.read_llm_file(lp), n_ctx=n_ctx), n_batch=32)
        c.system_prompt()
        c.begin_chat(prompt)
        n0, ids, logits = c.llm.n_past, [], [c.llm.logits.copy()]
        for _ in range(n):
            ids.append(int(c.end_chat(temp=0.0)[0]))
            logits.append(c.llm.logits.copy())
        lg = np.stack(logits)
        lg.setflags(write=False)
        _ORACLE[(lp, prompt)] = (tuple(ids), lg, n0)
    return _ORACLE[(lp, prompt)]


def begin(lib, ctx, slot, prompt):
    lib.amd_select_conversation(ctx, slot)
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.minigpt4_begin_chat(ctx, prompt.decode())


def n_past(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.library.minigpt4_amd_n_past(ctx.ptr)


def logits_of(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_logits(ctx).copy()


# ---------------------------------------------------------------------------------------------------------------- the attention launch alone
def _attn_case(lib, hd, n_ctx, groups, seed, computed=True, n_slot=3, vs=(1,)):
    """groups [(slot, p0, R)] in row order; at least one slot of n_slot is in no group."""
    n_head = 2
    E = n_head * hd
    N = sum(R for _, _, R in groups)
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((N, E)).astype(np.float32) for _ in range(3))
    kc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
    tag = (hd, n_ctx, groups, computed)
    ref = lib.amd_test_attn_draft_batch(1, q, k, v, kc, vc, n_head, groups, computed_exp=computed)
    assert np.isfinite(ref[0]).all() and (np.abs(ref[0]).max(axis=1) > 0).all(), tag
    for s in vs:
        new = lib.amd_test_attn_draft_batch(0, q, k, v, kc, vc, n_head, groups, computed_exp=computed, vs=s)
        assert np.array_equal(new[0], ref[0]), (tag, s, float(np.abs(new[0] - ref[0]).max()))
        assert np.array_equal(new[1], ref[1]) and np.array_equal(new[2], ref[2]), (tag, s)
        inside = np.zeros((n_slot, n_ctx), bool)
        for slot, p0, R in groups:
            inside[slot, p0:p0 + R] = True
            assert not np.array_equal(new[1][slot, p0:p0 + R], kc[slot, p0:p0 + R]), (tag, s)         # the appended rows did change
        assert (~inside).any(axis=1).all() and (~inside.any(axis=1)).any()                             # ... and a whole conversation is in no group
        assert np.array_equal(new[1][~inside], kc[~inside]) and np.array_equal(new[2][~inside], vc[~inside]), (tag, s)   # everything else is untouched
    return ref


P0S, RS = (0, 1, 31, 508, 512, 520), (1, 2, 5, 8)


def _pairs(p0s, rs):
    """Two groups per launch, conversation 2 in front of conversation 0 (slot order is not row order; conversation 1 is in no pass): every (p0, R) once as the FIRST
    group and, through the rotation, every p0 and every R as a group that does not start at packed row 0 -- its rows' packed index is not their index in the group."""
    return [[(2, p0, R), (0, p0s[(i + len(p0s) // 2) % len(p0s)], rs[(j + 1) % len(rs)])] for i, p0 in enumerate(p0s) for j, R in enumerate(rs)]


@pytest.mark.parametrize("computed", [True, False])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_attention_launch_is_bit_identical_to_one_verify_launch_per_group(gpu_lib, hd, computed):
    """n_ctx 544: group starts at 0, 1 (no / one cached key), 31 (inside one round of partitions), 508 / 512 / 520 around the 512 keys head size 128 prefetches (508 with 8
    rows straddles it: the group's own rows fall on both sides), R mixed over 1, 2, 5, 8; the computed exp and the gathered fp16 table."""
    for groups in _pairs(P0S, RS):
        _attn_case(gpu_lib, hd, 544, groups, seed=[hd, groups[0][1], groups[0][2], int(computed)], computed=computed)


@pytest.mark.parametrize("computed", [True, False])
def test_attention_launch_around_the_prefetch_of_head_size_64(gpu_lib, computed):
    """Head size 64 prefetches 1 024 keys: group starts at 1020 (the rows straddle it) and 1030 (behind it), n_ctx 1040."""
    for groups in _pairs((1020, 1030), RS):
        _attn_case(gpu_lib, 64, 1040, groups, seed=[groups[0][1], groups[0][2], int(computed)], computed=computed)


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_one_group_alone_is_the_single_conversation_launch(gpu_lib, hd):
    n_head, n_slot, n_ctx = 2, 3, 544
    E = n_head * hd
    for p0, R in ((0, 1), (31, 5), (508, 8), (520, 2)):
        rng = np.random.default_rng([hd, p0, R])
        q, k, v = (rng.standard_normal((R, E)).astype(np.float32) for _ in range(3))
        kc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
        vc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
        new = gpu_lib.amd_test_attn_draft_batch(0, q, k, v, kc, vc, n_head, [(1, p0, R)])
        old = gpu_lib.amd_test_attn_draft(0, q, k, v, kc, vc, n_head, 1, p0)
        for a, b in zip(new, old):
            assert np.array_equal(a, b), (hd, p0, R)


@pytest.mark.parametrize("hd", [64, 128])
def test_eight_groups_of_eight_rows_and_the_value_column_splits(gpu_lib, hd):
    """64 rows: eight conversations of a nine-slot cache, listed in a permuted order, each at another position; then VS 2 and 4 against VS 1 on that launch and on a
    mixed one -- the same bits."""
    order, p0s = (5, 0, 7, 2, 8, 1, 6, 3), (508, 0, 31, 520, 1, 512, 200, 77)
    _attn_case(gpu_lib, hd, 544, [(s, p, 8) for s, p in zip(order, p0s)], seed=[hd, 64], n_slot=9, vs=(1, 2, 4))
    _attn_case(gpu_lib, hd, 544, [(2, 508, 5), (0, 31, 8), (3, 0, 1), (4, 520, 2)], seed=[hd, 16], n_slot=5, vs=(1, 2, 4), computed=False)
    _attn_case(gpu_lib, 32, 544, [(2, 510, 8), (0, 1, 2)], seed=[32, 10], vs=(1, 2, 4))


# ---------------------------------------------------------------------------------------------------------------- the epilogue alone
def _epilogue_case(lib, n_vocab, groups, counts, n_slot, seed, tie_rows=()):
    """groups [(slot, p0, R)], counts [(m, later_match)] per group; rows listed in tie_rows carry their maximum twice (the lower index is the row's choice)."""
    rs, rp = B.pack(groups)
    N = len(rs)
    rng = np.random.default_rng([n_vocab, N, seed])
    ids = [int(x) for x in rng.integers(0, n_vocab - 2, N)]
    lg = np.stack([GR.planted_row(n_vocab, 100 * seed + t, (ids[t], n_vocab - 1) if t in tie_rows else (ids[t],)) for t in range(N)])
    for t in (0, N - 1):
        ids[t] = n_vocab - 2 if t not in tie_rows else ids[t]                  # (n_vocab 32001: index 31999 lies in the last 16-byte load, 32000 only in the scalar tail)
        lg[t] = GR.planted_row(n_vocab, 100 * seed + t, (ids[t], n_vocab - 1) if t in tie_rows else (ids[t],))
    tok = B.toks_for(ids, [(t0, R, m, later) for (t0, R), (m, later) in zip(B.groups_of(rs), counts)])
    st = GR.start_state(n_slot, n_vocab, seed)
    want = B.finish_batch_ref(lg, tok, rs, rp, st)
    assert [want["m_of_slot"][s] for s, _, _ in groups] == [m for m, _ in counts] and want["ids"] == ids
    got = lib.amd_test_draft_finish_batch(lg, tok, rs, rp, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])
    tag = (n_vocab, groups, counts)
    assert np.array_equal(got["res"], want["res"]), (tag, got["res"], want["res"])
    for key in ("n_past", "argmax", "feed"):
        assert np.array_equal(got[key], want[key]), (tag, key, got[key], want[key])
    assert np.array_equal(GR.bits(got["slot_logits"]), GR.bits(want["slot_logits"])), tag
    out = [s for s in range(n_slot + 1) if s not in {g[0] for g in groups}]
    assert len(out) >= 2                                                       # conversations not in the pass, and the guard: nothing of theirs moved
    for s in out:
        assert got["n_past"][s] == st["n_past"][s] and got["argmax"][s] == st["argmax"][s] and got["feed"][s] == st["feed"][s], (tag, s)
        assert np.array_equal(GR.bits(got["slot_logits"][s]), GR.bits(st["slot_logits"][s])), (tag, s)


@pytest.mark.parametrize("n_vocab", [512, 32001])
def test_epilogue_follows_the_reference(gpu_lib, n_vocab):
    """Eight groups in a slot order that is not the row order, R from 1 to 8, m = 0, R - 1 and between, matches behind the first mismatch, ties on the first maximum in
    rows that decide a count; one group alone; two groups whose rows fill all 64."""
    groups = [(7, 100, 1), (2, 0, 2), (9, 31, 5), (0, 508, 8), (5, 17, 3), (3, 250, 8), (8, 1, 7), (4, 60, 4)]
    counts = [(0, False), (1, False), (0, True), (7, False), (1, True), (3, True), (6, False), (0, False)]
    _epilogue_case(gpu_lib, n_vocab, groups, counts, n_slot=11, seed=1, tie_rows=(1, 3, 8, 15, 16, 27))
    _epilogue_case(gpu_lib, n_vocab, [(1, 40, 8)], [(4, True)], n_slot=3, seed=2, tie_rows=(4,))
    _epilogue_case(gpu_lib, n_vocab, [(1, 40, 1)], [(0, False)], n_slot=3, seed=3)
    if n_vocab == 512:
        _epilogue_case(gpu_lib, n_vocab, [(s, 8 * s, 8) for s in (6, 1, 4, 0, 7, 3, 5, 2)], [(s, s % 2 == 0) for s in range(8)], n_slot=9, seed=4, tie_rows=(0, 63))


# ---------------------------------------------------------------------------------------------------------------- through the C ABI
@pytest.fixture(scope="module")
def contexts(gpu_lib, tiny_files):
    """One context per file (n_ctx 256, 64 activation rows, four conversations, speculation on at 7): the tests restart its conversations."""
    vp, llm = tiny_files
    made = {}

    def get(wtype, mix):
        if (wtype, mix) not in made:
            lp = llm(wtype, mix, conditioned=True)
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=64)
            gpu_lib.amd_set_conversations(ctx, 4)
            gpu_lib.amd_set_speculation(ctx, 7)
            made[(wtype, mix)] = (ctx, lp)
        return made[(wtype, mix)]
    yield get
    for ctx, _ in made.values():
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_all_correct_drafts_are_kept_and_logits_match_the_oracle(gpu_lib, contexts, wtype, mix):
    """Conversations 3, 0, 2 (slot order is not list order) with three prompts bring 0, 3 and 7 draft tokens from the oracle's own continuations: every pass keeps them
    all, ids and positions are the oracle's, and after every pass each conversation's logits are the oracle's (1e-2 of the largest |logit|, 2 x a recorded error)."""
    ctx, lp = contexts(wtype, mix)
    slots, counts = (3, 0, 2), (0, 3, 7)
    O = [oracle(lp, p) for p in PROMPTS]
    for s, p in zip(slots, PROMPTS):
        begin(gpu_lib, ctx, s, p)
    before = gpu_lib.amd_speculation_batch_info(ctx)
    got, worst = [[], [], []], 0.0
    for _ in range(4):
        drafts = [list(O[i][0][len(got[i]) + 1:len(got[i]) + 1 + counts[i]]) for i in range(3)]
        r = gpu_lib.amd_verify_draft_batch(ctx, slots, drafts)
        for i in range(3):
            G, LG, n0 = O[i]
            assert len(r["ids"][i]) == 1 + counts[i], (i, r)
            got[i] += [int(x) for x in r["ids"][i]]
            assert got[i] == list(G[:len(got[i])]), (i, r)
            assert list(r["row_greedy"][i][:1 + counts[i]]) == list(G[len(got[i]) - counts[i]:len(got[i]) + 1]) and (r["row_greedy"][i][1 + counts[i]:] == -1).all(), (i, r)
            assert n_past(gpu_lib, ctx, slots[i]) == n0 + len(got[i])
            want = LG[len(got[i])]
            worst = max(worst, float(np.abs(logits_of(gpu_lib, ctx, slots[i]) - want).max() / np.abs(want).max()))
    after = gpu_lib.amd_speculation_batch_info(ctx)
    assert [after[k] - before[k] for k in ("passes", "rows", "groups", "sent", "accepted", "plain_steps", "cut")] == [4, 52, 12, 40, 40, 0, 0]
    print(f"verify_draft_batch {wtype}/{mix}: logits vs oracle {worst:.3e} of the largest |logit|")
    key = f"verify_draft_batch_{wtype}_{mix}"
    record_observed(key, worst)
    assert worst <= observed_bar(key), (worst, observed_bar(key))


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_each_conversation_keeps_its_own_prefix_and_rejected_rows_do_not_leak(gpu_lib, contexts, wtype, mix):
    """Seven draft tokens each; the first wrong one sits at index 0 in one conversation, 3 in the next, 6 (the last) in the third, and a fourth conversation keeps all
    seven: each keeps exactly its own prefix and row_greedy is the oracle's up to the token the wrong guess stood for.  Then 8 plain greedy steps of each: the
    oracle's ids and logits -- nothing of the rejected rows above n_past, its own or a neighbour's, reaches them."""
    ctx, lp = contexts(wtype, mix)
    slots, wrong_at, prompts = (1, 3, 0, 2), (0, 3, 6, None), PROMPTS + (PROMPTS[0],)
    O = [oracle(lp, p) for p in prompts]
    for s, p in zip(slots, prompts):
        begin(gpu_lib, ctx, s, p)
    drafts = []
    for i, j in enumerate(wrong_at):
        d = list(O[i][0][1:8])
        if j is not None:
            d[j] = (d[j] + 1) % 512
        drafts.append(d)
    r = gpu_lib.amd_verify_draft_batch(ctx, slots, drafts)
    bar = observed_bar(f"verify_draft_batch_{wtype}_{mix}")
    for i, j in enumerate(wrong_at):
        G, LG, n0 = O[i]
        keep = 8 if j is None else 1 + j
        assert list(r["ids"][i]) == list(G[:keep]), (i, r)
        assert list(r["row_greedy"][i][:keep]) == list(G[1:1 + keep]), (i, r)
        assert n_past(gpu_lib, ctx, slots[i]) == n0 + keep
        gpu_lib.amd_select_conversation(ctx, slots[i])
        for k in range(keep, keep + 8):
            lg = gpu_lib.amd_logits(ctx)
            assert int(np.argmax(lg)) == G[k], (i, k)
            assert float(np.abs(lg - LG[k]).max() / np.abs(LG[k]).max()) <= bar, (i, k)
            gpu_lib.minigpt4_end_chat(ctx, temp=0.0)
        assert n_past(gpu_lib, ctx, slots[i]) == n0 + keep + 8


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_one_conversation_equals_verify_draft_and_no_draft_equals_the_batched_step(gpu_lib, tiny_files, wtype, mix):
    """Twin contexts.  n = 1: the same row count as minigpt4_amd_verify_draft with the same draft, so the same mat-vec launches, and the attention is bit-identical by
    contract: logits, ids and position array_equal, for a draft that is kept and one with a wrong token.  Every count 0: the ordinary batched step -- array_equal to
    minigpt4_amd_eval_batch of the same greedy tokens, and the counters say it took the plain step."""
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    G, _, n0 = oracle(lp, PROMPTS[0])
    a, b = (gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=64) for _ in range(2))
    try:
        for c in (a, b):
            gpu_lib.amd_set_conversations(c, 3)
            gpu_lib.amd_set_speculation(c, 7)
            for s, p in enumerate(PROMPTS):
                begin(gpu_lib, c, s, p)
        pos = 0
        for draft in (list(G[1:5]), [G[6], (G[7] + 1) % 512, G[8]], [], list(G[9:16])):             # keeps 5, 2, 1 and 8 tokens
            ra = gpu_lib.amd_verify_draft_batch(a, [0], [draft])
            gpu_lib.amd_select_conversation(b, 0)
            rb = gpu_lib.amd_verify_draft(b, draft)
            assert list(ra["ids"][0]) == list(rb["ids"]) == list(G[pos:pos + len(rb["ids"])]), (draft, ra, rb)
            assert list(ra["row_greedy"][0][:1 + len(draft)]) == list(rb["row_greedy"]), (draft, ra, rb)
            pos += len(rb["ids"])
            assert n_past(gpu_lib, a, 0) == n_past(gpu_lib, b, 0) == n0 + pos
            assert np.array_equal(logits_of(gpu_lib, a, 0), logits_of(gpu_lib, b, 0)), draft
        before = gpu_lib.amd_speculation_batch_info(a)
        greedy = [int(np.argmax(logits_of(gpu_lib, b, s))) for s in (2, 0, 1)]
        ra = gpu_lib.amd_verify_draft_batch(a, [2, 0, 1], [[], [], []])
        assert [list(x) for x in ra["ids"]] == [[g] for g in greedy]
        assert gpu_lib.amd_eval_batch(b, [2, 0, 1], greedy) == greedy
        assert [int(x[0]) for x in ra["row_greedy"]] == [int(np.argmax(logits_of(gpu_lib, b, s))) for s in (2, 0, 1)] and (ra["row_greedy"][:, 1:] == -1).all()
        for s in range(3):
            assert n_past(gpu_lib, a, s) == n_past(gpu_lib, b, s)
            assert np.array_equal(logits_of(gpu_lib, a, s), logits_of(gpu_lib, b, s)), s
        after = gpu_lib.amd_speculation_batch_info(a)
        assert after["plain_steps"] == before["plain_steps"] + 1 and after["passes"] == before["passes"] and after["rows"] == before["rows"]
    finally:
        gpu_lib.minigpt4_free(a)
        gpu_lib.minigpt4_free(b)


def test_13b_width_passes_take_the_set_launches(gpu_lib):
    """The two-layer 13B-width k-quant file: 2 conversations of 4 rows and 4 conversations of 2 rows are 8-row passes on the int8-MFMA set launches, and every
    conversation keeps the oracle's ids."""
    import headline as H
    from test_gpu_draft import PROMPT, _wide_oracle
    vp, lp = H.headline_files("13b_l2")
    G = _wide_oracle(lp)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=64)
    try:
        gpu_lib.amd_set_conversations(ctx, 4)
        gpu_lib.amd_set_speculation(ctx, 7)
        for n, R in ((2, 4), (4, 2)):
            begin(gpu_lib, ctx, 0, PROMPT)
            gpu_lib.amd_select_conversation(ctx, 0)
            assert gpu_lib.amd_logits(ctx).shape[0] > 0                        # (evaluates the queued prompt: the fork copies rows and logits)
            gpu_lib.amd_fork_conversation(ctx, 0, list(range(1, n)))
            slots = list(range(n))[::-1]
            got = 0
            while got < 8:
                r = gpu_lib.amd_verify_draft_batch(ctx, slots, [list(G[got + 1:got + R])] * n)
                path = gpu_lib.amd_batch_path(ctx)
                assert path["rows"] == n * R == 8 and path["sets"] > 0, path
                for i in range(n):
                    assert list(r["ids"][i]) == list(G[got:got + R]), (n, R, got, i, r)
                got += R
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_edges_room_shift_and_refusals(gpu_lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as MG
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    L = gpu_lib.library
    prompt = [1] + [5 + (7 * i) % 300 for i in range(63)]
    o = R.OracleLLM(MG.read_llm_file(lp), n_ctx=128)                             # room for the continuation the 64-row context cannot hold
    o.eval_tokens(prompt[:60])
    G = []
    for _ in range(8):
        G.append(int(np.argmax(o.logits)))
        o.eval_tokens([G[-1]])
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=32)
    ip = lambda a: a.ctypes.data_as(I32P)
    ids, n_out, rg = np.zeros((4, 8), np.int32), np.zeros(4, np.int32), np.zeros((4, 8), np.int32)
    live = [0, 1, 2]

    def state():
        return [(n_past(gpu_lib, ctx, s), logits_of(gpu_lib, ctx, s)) for s in live]

    def refused(text, slots, drafts, counts, n=None, **null):
        before = state()
        sl, d, c = (np.array(x if len(x) else [0], np.int32) for x in (slots, drafts, counts))
        a = dict(p_slots=ip(sl), p_drafts=ip(d), p_counts=ip(c), p_ids=ip(ids), p_n_out=ip(n_out))
        a.update(null)
        assert L.minigpt4_amd_verify_draft_batch(ctx.ptr, a["p_slots"], len(slots) if n is None else n, a["p_drafts"], a["p_counts"], a["p_ids"], a["p_n_out"], ip(rg)) == 1, text
        err = L.minigpt4_amd_last_error()
        assert err.startswith(b"verify_draft_batch: ") and text in err, (text, err)
        for (p0, l0), (p1, l1) in zip(before, state()):
            assert p0 == p1 and np.array_equal(l0, l1), text
    try:
        gpu_lib.amd_set_conversations(ctx, 4)
        for s, n in ((0, 60), (1, 64), (2, 30)):                                # conversation 1 is full; conversation 3 stays empty
            gpu_lib.amd_select_conversation(ctx, s)
            gpu_lib.amd_eval_tokens(ctx, prompt[:n])
        refused(b"speculation is off", [0, 2], G[1:3], [2, 0])
        gpu_lib.amd_set_speculation(ctx, 7)
        refused(b"bad slot list", [0, 2], G[1:3], [2, 0], p_slots=None)
        refused(b"bad slot list", [0, 2], G[1:3], [2, 0], n=0)
        refused(b"bad slot list", [0, 2], G[1:3], [2, 0], n=5)                 # more than the conversations
        refused(b"distinct and in range", [0, 0], G[1:3], [1, 1])
        refused(b"distinct and in range", [0, 4], G[1:3], [1, 1])
        refused(b"distinct and in range", [-1, 2], G[1:3], [1, 1])
        refused(b"required", [0, 2], G[1:3], [2, 0], p_counts=None)
        refused(b"required", [0, 2], G[1:3], [2, 0], p_ids=None)
        refused(b"required", [0, 2], G[1:3], [2, 0], p_n_out=None)
        refused(b"count outside", [0, 2], G[1:3], [-1, 2])
        refused(b"count outside", [0, 2], G[:8], [8, 0])
        refused(b"drafts is NULL", [0, 2], G[1:3], [2, 0], p_drafts=None)
        refused(b"out of range", [0, 2], [G[1], -1], [1, 1])
        refused(b"out of range", [0, 2], [G[1], 512], [1, 1])
        refused(b"no current logits", [0, 3], G[1:3], [2, 0])                  # conversation 3 has nothing
        gpu_lib.amd_set_speculation(ctx, 3)
        refused(b"count outside", [0, 2], G[1:5], [4, 0])                      # above max_draft
        gpu_lib.amd_set_speculation(ctx, 7)
        # a draft cut for room, next to a full conversation (left out, untouched) and one that sends none
        before = state()
        g2 = int(np.argmax(before[2][1]))
        info0 = gpu_lib.amd_speculation_batch_info(ctx)
        r = gpu_lib.amd_verify_draft_batch(ctx, [1, 0, 2], [[3, 4], G[1:8], []])
        assert list(r["ids"][0]) == [] and list(r["ids"][1]) == G[:4] and list(r["ids"][2]) == [g2], r
        assert (r["row_greedy"][0] == -1).all() and list(r["row_greedy"][1][:4]) == G[1:5] and (r["row_greedy"][1][4:] == -1).all() and (r["row_greedy"][2][1:] == -1).all(), r
        assert n_past(gpu_lib, ctx, 1) == 64 and np.array_equal(logits_of(gpu_lib, ctx, 1), before[1][1])
        assert n_past(gpu_lib, ctx, 0) == 64 and n_past(gpu_lib, ctx, 2) == 31
        info1 = gpu_lib.amd_speculation_batch_info(ctx)
        assert [info1[k] - info0[k] for k in ("passes", "rows", "groups", "sent", "accepted", "cut")] == [1, 5, 2, 3, 3, 4]   # cut: 4 of conversation 0's 7 (the conversation that is left out sends nothing and cuts nothing)
        # both full now: nothing to do, nothing changes
        before = state()
        r = gpu_lib.amd_verify_draft_batch(ctx, [0, 1], [[5], []])
        assert [list(x) for x in r["ids"]] == [[], []]
        for (p0, l0), (p1, l1) in zip(before, state()):
            assert p0 == p1 and np.array_equal(l0, l1)
        # the automatic shift makes room: against plain greedy steps of a twin context that holds the same rows and shifts the same way.  Conversation 0 (full) brings
        # the twin's next two tokens and keeps them, conversation 1 (full) a wrong one and keeps only its own token, conversation 2 (room) two right ones
        twin = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=32)
        try:
            gpu_lib.amd_set_conversations(twin, 4)
            for s, rows in ((0, prompt[:60] + G[:4]), (1, prompt[:64]), (2, prompt[:30] + [g2])):
                gpu_lib.amd_select_conversation(twin, s)
                gpu_lib.amd_eval_tokens(twin, rows)
                assert n_past(gpu_lib, twin, s) == n_past(gpu_lib, ctx, s) == len(rows)
            gpu_lib.amd_set_context_shift(twin, 8)
            tw = {}
            for s in live:                                                      # [(id, position after it, logits after it)] of three plain greedy steps
                gpu_lib.amd_select_conversation(twin, s)
                tw[s] = []
                for _ in range(3):
                    t = int(np.argmax(gpu_lib.amd_logits(twin)))
                    gpu_lib.minigpt4_end_chat(twin, temp=0.0)
                    tw[s].append((t, n_past(gpu_lib, twin, s), gpu_lib.amd_logits(twin).copy()))
        finally:
            gpu_lib.minigpt4_free(twin)
        assert tw[0][0][1] < 64 and tw[1][0][1] < 64 and tw[2][2][1] == 34     # the two full conversations did shift, the third did not
        gpu_lib.amd_set_context_shift(ctx, 8)
        r = gpu_lib.amd_verify_draft_batch(ctx, [0, 1, 2], [[tw[0][1][0], tw[0][2][0]], [(tw[1][1][0] + 1) % 512], [tw[2][1][0], tw[2][2][0]]])
        for i, (s, keep) in enumerate(((0, 3), (1, 1), (2, 3))):
            assert list(r["ids"][i]) == [x[0] for x in tw[s][:keep]], (s, r, [x[0] for x in tw[s]])
            assert n_past(gpu_lib, ctx, s) == tw[s][keep - 1][1], s
            want = tw[s][keep - 1][2]
            assert float(np.abs(logits_of(gpu_lib, ctx, s) - want).max() / np.abs(want).max()) <= 1e-2, s
        gpu_lib.amd_set_speculation(ctx, 0)
        refused(b"speculation is off", [0, 2], [3], [1, 0])
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_more_than_64_rows_are_refused(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lp = llm("q4_0", "none", conditioned=True)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=128)
    try:
        gpu_lib.amd_set_conversations(ctx, 9)
        gpu_lib.amd_set_speculation(ctx, 7)
        with pytest.raises(RuntimeError, match="verify_draft_batch: more rows in total"):
            gpu_lib.amd_verify_draft_batch(ctx, list(range(9)), [[3] * 7] * 9)              # 72 rows
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_parity_mode_is_plain_greedy_decoding_bit_for_bit(gpu_lib, tiny_files, wtype, mix):
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    O = [oracle(lp, p) for p in PROMPTS[:2]]
    ctx, ref = (gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32) for _ in range(2))
    try:
        for c in (ctx, ref):
            gpu_lib.amd_set_conversations(c, 2)
            gpu_lib.amd_set_parity(c, True)
            for s in range(2):
                begin(gpu_lib, c, s, PROMPTS[s])
        gpu_lib.amd_set_speculation(ctx, 3)
        got = [0, 0]
        for wrong in (None, 1, None):
            drafts = []
            for i in range(2):
                d = list(O[i][0][got[i] + 1:got[i] + 4])
                if wrong is not None and i == 1:
                    d[wrong] = (d[wrong] + 1) % 512
                drafts.append(d)
            r = gpu_lib.amd_verify_draft_batch(ctx, [1, 0], drafts[::-1])
            for i, ids in ((1, r["ids"][0]), (0, r["ids"][1])):
                keep = 4 if wrong is None or i == 0 else 1 + wrong
                assert list(ids) == list(O[i][0][got[i]:got[i] + keep]), (wrong, i, r)
                gpu_lib.amd_select_conversation(ref, i)
                for _ in range(keep):
                    gpu_lib.minigpt4_end_chat(ref, temp=0.0)
                got[i] += keep
                assert n_past(gpu_lib, ctx, i) == n_past(gpu_lib, ref, i)
                assert np.array_equal(logits_of(gpu_lib, ctx, i), logits_of(gpu_lib, ref, i)), (wrong, i)
    finally:
        gpu_lib.minigpt4_free(ctx)
        gpu_lib.minigpt4_free(ref)


@pytest.mark.parametrize("wtype,mix", TRIPLES)
def test_decode_lookup_batch_emits_every_conversations_greedy_text(gpu_lib, contexts, wtype, mix):
    """Three conversations with three prompts and three corpora -- none, the oracle's own continuation, that continuation with every third id wrong: each emits exactly
    its oracle's ids (up to and including a </s>), and passes + steps + accepted draft tokens account for every token of each."""
    ctx, lp = contexts(wtype, mix)
    slots = (2, 0, 3)
    O = [oracle(lp, p) for p in PROMPTS]
    corpora = [[], list(O[1][0]), [g if k % 3 != 2 else (g + 1) % 512 for k, g in enumerate(O[2][0])]]
    for s, p in zip(slots, PROMPTS):
        begin(gpu_lib, ctx, s, p)
    out = gpu_lib.amd_decode_lookup_batch(ctx, slots, corpora, N_ORACLE - 8, ngram_max=3, ngram_min=1, n_draft=4)
    for i, r in enumerate(out):
        G, _, n0 = O[i]
        want = list(G[:N_ORACLE - 8])
        if 2 in want:
            want = want[:want.index(2) + 1]
        print(f"decode_lookup_batch {wtype}/{mix} conversation {i}: {r['passes']} passes, {r['steps']} steps, {r['accepted']} of {r['sent']} draft tokens accepted")
        assert list(r["tokens"]) == want, (i, r)
        assert r["passes"] + r["steps"] + r["accepted"] == len(r["tokens"]), (i, r)
        assert n_past(gpu_lib, ctx, slots[i]) == n0 + len(want)
    assert out[0]["sent"] == 0 or len(set(O[0][0])) < len(O[0][0])              # no corpus: drafts only where the conversation's own text repeats
    assert out[1]["accepted"] > 0 and out[1]["passes"] + out[1]["steps"] < len(out[1]["tokens"]), out[1]
    with pytest.raises(RuntimeError, match="decode_lookup_batch: n_draft"):
        gpu_lib.amd_decode_lookup_batch(ctx, slots, corpora, 4, n_draft=8)
    with pytest.raises(RuntimeError, match="decode_lookup_batch: conversations must be distinct"):
        gpu_lib.amd_decode_lookup_batch(ctx, [0, 0], [[], []], 4)


@pytest.mark.parametrize("batched_prefill", [False, True])
def test_server_with_lookup_returns_the_same_answers(gpu_lib, tmpdir_models, batched_prefill):
    """ReplicaServer.run(lookup=4) at temp 0 against run(): three requests over two conversations (waves of 2 + 1), with and without the stop rule."""
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp = os.path.join(tmpdir_models, "vision_lookup.bin")
    lp = os.path.join(tmpdir_models, "llm_lookup.bin")
    if not os.path.exists(lp):
        G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)
        G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    # (the first prompt spells out most of the vocabulary's pieces, so that what the model emits occurs in the drafter's history and drafts are sent)
    reqs = [S.Request(G.synth_image(3), "what is the text in the picture? " + "".join(chr(c) for c in range(33, 127)) + " the quick brown fox jumps over the lazy dog", 48),
            S.Request(G.synth_image(5), "describe it", 17), S.Request(G.synth_image(7), "colour?", 1)]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)
    try:
        for ignore_eos in (False, True):
            plain = srv.run(reqs, temp=0.0, ignore_eos=ignore_eos, batched_prefill=batched_prefill)
            fast = srv.run(reqs, temp=0.0, ignore_eos=ignore_eos, batched_prefill=batched_prefill, lookup=4)
            assert fast == plain, (ignore_eos, fast, plain)
        assert all(len(a) > 0 for a in plain[:2])
        info = gpu_lib.amd_speculation_batch_info(srv.ctx)
        print(f"serve lookup=4 batched_prefill={batched_prefill}: {info}")
        assert info["passes"] > 0 and info["sent"] > 0, info               # drafts did go through the multi-row pass, not only plain steps
    finally:
        srv.close()
