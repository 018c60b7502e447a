"""The batched step is issued in one place (Engine::step_begin / step_launch) and its graph for B rows is shared by every entry point that advances B rows: the graph
decode_batch captured is replayed by decode_guided and beam_search, and the other way round.  One context walks through all of them (graphs, the default); its twin,
created under MINIGPT4_NO_GRAPH=1, runs every pass eagerly.  After every step both must stand at the same place."""
import numpy as np
import pytest

from test_gpu_batch import PROMPTS

pytestmark = pytest.mark.gpu

N_CTX, N_BATCH = 128, 32
BIAS = {7: 2.5, 100: -3.0}                 # conversation 2's logit bias in the penalties run


def n_past(lib, ctx):
    return lib.library.minigpt4_amd_n_past(ctx.ptr)


def load(lib, vp, lp, graphs, monkeypatch, parity, penalties):
    if not graphs:
        monkeypatch.setenv("MINIGPT4_NO_GRAPH", "1")          # read at init: around the load only
    try:
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=N_CTX, n_batch=N_BATCH)
    finally:
        monkeypatch.delenv("MINIGPT4_NO_GRAPH", raising=False)
    if parity:
        lib.amd_set_parity(ctx, True)
    lib.amd_set_conversations(ctx, 4)
    for s, p in enumerate(PROMPTS[:4]):                          # the question alone: the system prompt does not fit n_ctx 128 at this vocabulary
        lib.amd_select_conversation(ctx, s)
        lib.minigpt4_begin_chat(ctx, p.decode())
    lib.amd_select_conversation(ctx, 0)
    lib.amd_set_speculation(ctx, 3)
    if penalties:
        lib.amd_set_penalties(ctx, True)
        lib.amd_select_conversation(ctx, 2)
        lib.amd_set_logit_bias(ctx, BIAS)
        lib.amd_select_conversation(ctx, 0)
    return ctx


def steps_before_draft(lib, ctx):
    """Steps 1-3 of the sequence; yields (name, what the call returned)."""
    for _ in range(2):
        yield "end_chat_batch[0,1]", lib.amd_end_chat_batch(ctx, [0, 1], temp=0.0)
    for _ in range(2):
        yield "end_chat_guided[2|3]", lib.amd_end_chat_guided(ctx, [2], [3], 1.5, temp=0.0, with_ids=True)
    yield "beam_search[0,1]", lib.amd_beam_search(ctx, [0, 1], max_tokens=3)


def steps_from_draft(lib, ctx, draft):
    """Steps 4-6."""
    lib.amd_select_conversation(ctx, 0)
    yield "verify_draft(0)", lib.amd_verify_draft(ctx, draft)
    yield "end_chat_batch[3,2]", lib.amd_end_chat_batch(ctx, [3, 2], temp=0.0)
    yield "end_chat_batch[0,1,2,3]", lib.amd_end_chat_batch(ctx, [0, 1, 2, 3], temp=0.0)


def state(lib, ctx):
    out = []
    for s in range(4):
        lib.amd_select_conversation(ctx, s)
        out.append((n_past(lib, ctx), lib.amd_token_history(ctx).copy(), lib.amd_logits(ctx).copy()))
    lib.amd_select_conversation(ctx, 0)
    return out


def same_result(name, a, b, logit_range, exact):
    if name.startswith("end_chat_batch"):
        assert a == b, name
    elif name.startswith("end_chat_guided"):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), name
    elif name.startswith("verify_draft"):
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["row_greedy"], b["row_greedy"]), name
    else:                                                        # hypotheses: the ids; the score (length_penalty 1: the mean log-probability of the ids)
        assert len(a) == len(b) and len(a) > 0, name
        for (ia, sa), (ib, sb) in zip(a, b):
            assert np.array_equal(ia, ib), name
            # a logit error e moves a log-probability by at most 2 e, so the mean of them too; e is this file's bar on the logits (exact in parity mode)
            assert sa == sb if exact else abs(sa - sb) <= 2 * 2e-3 * logit_range, (name, sa, sb)


def same_state(name, sg, se, exact):
    for s, ((pg, hg, lg), (pe, he, le)) in enumerate(zip(sg, se)):
        assert pg == pe, (name, s, pg, pe)
        assert np.array_equal(hg, he), (name, s)
        if exact:
            assert np.array_equal(lg, le), (name, s)
        else:                                                    # test_gpu_batch.py's bar for two launch forms of the same arithmetic
            assert float(np.abs(lg - le).max() / (le.max() - le.min())) < 2e-3, (name, s)


def lookahead(lib, ctx):
    """Conversation 0's next three greedy tokens, on a context of its own that went through steps 1-3."""
    for _ in steps_before_draft(lib, ctx):
        pass
    lib.amd_select_conversation(ctx, 0)
    ids = []
    for _ in range(3):
        ids.append(int(np.argmax(lib.amd_logits(ctx))))          # the conditioned model's greedy choices are decisive: the first maximum is the only one
        lib.amd_end_chat_batch(ctx, [0], temp=0.0)                # (not minigpt4_end_chat: with the penalties mode on it would store its own penalty arguments)
    return ids


@pytest.mark.parametrize("wtype,mix,mode", [("q4_0", "none", "plain"), ("q4_0", "none", "penalties"), ("q4_0", "none", "parity"),
                                            ("q5_k", "q5_k_m", "plain"), ("q5_k", "q5_k_m", "penalties")])
def test_graph_of_one_entry_point_serves_the_others(gpu_lib, tiny_files, monkeypatch, wtype, mix, mode):
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    parity, penalties = mode == "parity", mode == "penalties"
    ctxs = []
    try:
        for graphs in (True, False, True):                       # G, E, and the context the draft is read from
            ctxs.append(load(gpu_lib, vp, lp, graphs, monkeypatch, parity, penalties))
        G, E, scout = ctxs
        V = gpu_lib.library.minigpt4_amd_n_vocab(G.ptr)
        # the draft: the token that follows conversation 0's greedy token (accepted), then an id the pass will not choose (rejected)
        g0, g1, g2 = lookahead(gpu_lib, scout)
        wrong = (g2 + 1) % V
        if wrong == 2:
            wrong += 1                                           # not </s>
        draft = [g1, wrong]

        def walk(ctx):
            yield from steps_before_draft(gpu_lib, ctx)
            yield from steps_from_draft(gpu_lib, ctx, draft)

        n_steps = 0
        for (name, rg), (_, re) in zip(walk(G), walk(E)):
            sg, se = state(gpu_lib, G), state(gpu_lib, E)
            same_result(name, rg, re, float(se[0][2].max() - se[0][2].min()), parity)
            same_state(name, sg, se, parity)
            if name.startswith("verify_draft"):                  # one draft token kept, one refused: the pass committed two of its three rows
                assert list(rg["ids"]) == [g0, g1], (rg, g0, g1, g2)
            n_steps += 1
        assert n_steps == 8
        if penalties:                                            # the shared row builder fed k_pen_pick from decode_batch and from the guided step, equally often
            ig, ie = gpu_lib.amd_penalty_info(G), gpu_lib.amd_penalty_info(E)
            assert ig["launches"] == ie["launches"] == 4, (ig, ie)         # two guided steps, two batched steps that list conversation 2
    finally:
        for c in ctxs:
            gpu_lib.minigpt4_free(c)
