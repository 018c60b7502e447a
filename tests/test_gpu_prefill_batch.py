"""Prompt rows of several conversations in one weight pass (include/minigpt4_amd.h: minigpt4_amd_prefill_batch).

1. kernels: the segmented prompt attention (one launch over every segment of a packed chunk) is bit-identical to one launch of the single-conversation kernel per
   segment, for every form the launcher can choose; k_rope_kv_seg (and its slab form) equals k_rope_kv per segment (q rows and cache bits);
2. whole pass: after amd_prefill_batch every conversation's logits / n_past / following greedy pieces equal a second context that evaluated the same prompts one
   conversation at a time (the bar of test_batch_logits_equal_single_conversation_path), across chunk boundaries, second turns and empty queues;
3. argument checks, parity mode (one flush per conversation: bit-identical), and the serve option.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROMPTS = [b"what is the text in the picture?", b"describe the colours", b"hello", b"and now something longer to shift the positions apart", b"a", b"b c d", b"zzz",
           b"tell me more"]


# ------------------------------------------------------------------------------------------------ 1. kernels
def _caches(rng, S, C, E):
    k = (rng.standard_normal((S, C, E), dtype=np.float32) * 0.5).astype(np.float16)
    v = rng.standard_normal((S, C, E), dtype=np.float32).astype(np.float16)
    return k, v


SEG_CASES = {
    "mixed": [(2, 1, 0), (0, 15, 0), (3, 16, 7), (1, 17, 40), (4, 142, 0)],
    "long": [(1, 512, 0), (0, 142, 300)],
    "second_turn": [(3, 33, 190), (0, 142, 0), (2, 5, 61)],
    "single": [(1, 142, 0)],
    "single_at_pos": [(0, 100, 45)],
}


@pytest.mark.parametrize("case", sorted(SEG_CASES))
@pytest.mark.parametrize("E,H", [(5120, 40), (256, 4), (256, 8)])      # hd 128 at the 13B width, hd 64 / 32 at tiny widths
@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
def test_segmented_attention_is_bit_identical_to_per_segment_launches(gpu_lib, case, E, H, form):
    segs = SEG_CASES[case]
    S, C = 5, 512
    rng = np.random.default_rng(E + 7 * H + len(segs))
    kc, vc = _caches(rng, S, C, E)
    N = sum(r for _, r, _ in segs)
    q = rng.standard_normal((N, E), dtype=np.float32)
    got, want, one = gpu_lib.amd_test_attn_prefill_seg(kc, vc, H, segs, q, form)
    assert one == (form != 4)                                 # the exact-f32 form runs per segment by design
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", ["mixed", "long", "second_turn"])
@pytest.mark.parametrize("E,H", [(5120, 40), (256, 4)])
def test_segmented_attention_fp16_rows_for_f16_wo(gpu_lib, case, E, H):
    """The out_h arm (fp16 attention rows for an F16 wo, taken by the engine from 512 packed rows): the segmented 8-wave launch stores the same fp16 bits as the
    8-wave launch of every segment."""
    segs = SEG_CASES[case]
    rng = np.random.default_rng(E + 3 * len(segs))
    kc, vc = _caches(rng, 5, 512, E)
    q = rng.standard_normal((sum(r for _, r, _ in segs), E), dtype=np.float32)
    _, _, one, ha, hb, wrote = gpu_lib.amd_test_attn_prefill_seg(kc, vc, H, segs, q, 1, fp16_rows=True)
    assert one and wrote == (True, True)
    assert np.abs(hb.view(np.float16).astype(np.float32)).max() > 0
    assert np.array_equal(ha, hb)


@pytest.mark.parametrize("E,H", [(256, 2), (128, 2), (64, 2)])          # hd 128 / 64 / 32
def test_prompt_attention_forms_are_bit_identical_to_each_other(gpu_lib, E, H):
    """The 8-wave form (1), the 4-wave form with 32 queries (2) and with 16 queries (3) are schedules over the same stages: for one input they return the same bits,
    launched per segment and segmented.  The segments take 1, 2, 3 and 4 key tiles (both exits of the 8-wave form's two-tile loop), row counts that are no multiple
    of 16 or 32, first positions that are no multiple of 64, and one row."""
    segs = [(0, 1, 0), (1, 17, 40), (2, 33, 60), (0, 5, 150), (1, 40, 200)]
    rng = np.random.default_rng(E + H)
    kc, vc = _caches(rng, 3, 256, E)
    q = rng.standard_normal((sum(r for _, r, _ in segs), E), dtype=np.float32)
    res = {form: gpu_lib.amd_test_attn_prefill_seg(kc, vc, H, segs, q, form) for form in (1, 2, 3)}
    assert all(one for _, _, one in res.values())
    want = res[1][1]
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    for form in (2, 3):
        assert np.array_equal(res[form][1], want), form
    for form in (1, 2, 3):
        assert np.array_equal(res[form][0], want), form


@pytest.mark.parametrize("E,H", [(5120, 40), (256, 4), (256, 8)])
@pytest.mark.parametrize("ks", [1, 3])
def test_segmented_rope_append_is_bit_identical_to_per_segment_launches(gpu_lib, E, H, ks):
    segs = [(2, 17, 0), (0, 1, 63), (1, 142, 5), (3, 16, 200)]
    S, C = 4, 512
    N = sum(r for _, r, _ in segs)
    rng = np.random.default_rng(E + ks)
    q, k, v = (rng.standard_normal((N, E), dtype=np.float32) for _ in range(3))
    (qa, ka, va), (qb, kb, vb) = gpu_lib.amd_test_rope_kv_seg(H, C, S, segs, q, k, v, ks)
    assert np.array_equal(qa, qb)
    assert np.array_equal(ka.view(np.uint16), kb.view(np.uint16)) and np.array_equal(va.view(np.uint16), vb.view(np.uint16))
    for slot, rows, pos in segs:                              # the rows landed where the segment's positions say
        assert np.abs(ka[slot, pos:pos + rows].astype(np.float32)).max() > 0
    assert not np.array_equal(qa, q)                          # q was rotated


# ------------------------------------------------------------------------------------------------ 2. whole pass against the single-conversation path
def _prompt(lib, ctx, slot, p, system=True):
    lib.amd_select_conversation(ctx, slot)
    if system:
        lib.minigpt4_reset_chat(ctx)
        lib.minigpt4_system_prompt(ctx)
    lib.minigpt4_begin_chat(ctx, p.decode())


def _state(lib, ctx, B):
    out = []
    for s in range(B):
        lib.amd_select_conversation(ctx, s)
        out.append((lib.amd_logits(ctx).copy(), lib.library.minigpt4_amd_n_past(ctx.ptr)))
    return out


def _check_against_single(lib, vp, lp, prompts, n_batch=32, extra=None, steps=8):
    """ctx: prompts queued, one amd_prefill_batch; ref: the same prompts, one conversation at a time (its own flush).  extra(lib, ctx, batched) may queue more."""
    B = len(prompts)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=n_batch)
    ref = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=n_batch)
    try:
        for c in (ctx, ref):
            lib.amd_set_conversations(c, B)
            for s, p in enumerate(prompts):
                _prompt(lib, c, s, p)
        if extra:
            extra(lib, ctx, True)
            extra(lib, ref, False)
        lib.amd_prefill_batch(ctx, list(range(B)))
        for s in range(B):                                    # the reference: each conversation evaluates its own queue
            lib.amd_select_conversation(ref, s)
            lib.amd_logits(ref)
        got, want = _state(lib, ctx, B), _state(lib, ref, B)
        for s in range(B):
            g, w = got[s][0], want[s][0]
            assert got[s][1] == want[s][1], (s, got[s][1], want[s][1])
            assert float(np.abs(g - w).max() / (w.max() - w.min())) < 2e-3, s
        pa = [lib.amd_end_chat_batch(ctx, list(range(B)), temp=0.0) for _ in range(steps)]
        pb = [lib.amd_end_chat_batch(ref, list(range(B)), temp=0.0) for _ in range(steps)]
        assert pa == pb
        return got
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


@pytest.mark.parametrize("wtype,mix", [("q4_0", "none"), ("q5_k", "q5_k_m"), ("f16", "none")])
@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_prefill_batch_equals_single_conversation_path(gpu_lib, tiny_files, wtype, mix, B):
    vp, llm = tiny_files
    _check_against_single(gpu_lib, vp, llm(wtype, mix, conditioned=True), PROMPTS[:B])


@pytest.mark.parametrize("sizes", [[1, 63, 64, 65, 200], [64, 1], [65], [1]])
def test_prefill_batch_chunks_cross_conversation_boundaries(gpu_lib, tiny_files, sizes):
    """n_batch = 64 with queues of 1, 63, 64, 65 and 200 rows: conversations continue in the next chunk at their advanced position.  [64, 1], [65] and [1] end
    with (or are) a chunk of exactly ONE packed row: the prompt form of the pass at N = 1."""
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    rng = np.random.default_rng(5 + len(sizes))
    toks = [np.ascontiguousarray(rng.integers(3, 500, n), np.int32) for n in sizes]

    def extra(lib, ctx, batched):
        for s, t in enumerate(toks):
            lib.amd_select_conversation(ctx, s)
            lib.minigpt4_reset_chat(ctx)                      # exactly len(t) queued rows
            assert lib.library.minigpt4_amd_eval_tokens(ctx.ptr, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(t)) == 0
    _check_against_single(gpu_lib, vp, lp, [b"x"] * len(sizes), n_batch=64, extra=extra)


def test_prefill_batch_second_turn_with_fresh_conversation_and_empty_queue(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    lib = gpu_lib
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=32)
    ref = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=32)
    try:
        for c in (ctx, ref):
            lib.amd_set_conversations(c, 3)
            for s in range(3):
                _prompt(lib, c, s, PROMPTS[s])
            for _ in range(4):
                lib.amd_end_chat_batch(c, [0, 1, 2], temp=0.0)
            _prompt(lib, c, 0, PROMPTS[4], system=False)     # slot 0: a second turn after decoding
            _prompt(lib, c, 1, PROMPTS[5])                     # slot 1: a fresh conversation; slot 2: nothing queued
        lib.amd_select_conversation(ctx, 2)
        before = lib.amd_logits(ctx).copy()
        lib.amd_prefill_batch(ctx, [2, 1, 0])                # out of slot order
        lib.amd_select_conversation(ctx, 2)
        assert np.array_equal(lib.amd_logits(ctx), before)   # skipped: byte for byte
        for s in (0, 1):
            lib.amd_select_conversation(ref, s)
            lib.amd_logits(ref)
        got, want = _state(lib, ctx, 3), _state(lib, ref, 3)
        for s in range(3):
            assert got[s][1] == want[s][1]
            assert float(np.abs(got[s][0] - want[s][0]).max() / (want[s][0].max() - want[s][0].min())) < 2e-3, s
        assert [lib.amd_end_chat_batch(ctx, [0, 1, 2], temp=0.0) for _ in range(8)] == [lib.amd_end_chat_batch(ref, [0, 1, 2], temp=0.0) for _ in range(8)]
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefill_batch_image_turns(gpu_lib, tiny_files):
    """Embedding rows (image turns, a different image per conversation) packed at their row offsets."""
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    lib = gpu_lib
    B = 4
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=64)
    ref = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=64)
    try:
        embs = []
        for b in range(B):
            e = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(G.synth_image(100 + b)))
            embs.append(e)
        for c in (ctx, ref):
            lib.amd_set_conversations(c, B)
            for s in range(B):
                lib.amd_select_conversation(c, s)
                lib.minigpt4_system_prompt(c)
                lib.minigpt4_begin_chat_image(c, embs[s], PROMPTS[s].decode())
        lib.amd_prefill_batch(ctx, list(range(B)))
        for s in range(B):
            lib.amd_select_conversation(ref, s)
            lib.amd_logits(ref)
        got, want = _state(lib, ctx, B), _state(lib, ref, B)
        for s in range(B):
            assert got[s][1] == want[s][1]
            assert float(np.abs(got[s][0] - want[s][0]).max() / (want[s][0].max() - want[s][0].min())) < 2e-3, s
        assert [lib.amd_end_chat_batch(ctx, list(range(B)), temp=0.0) for _ in range(8)] == [lib.amd_end_chat_batch(ref, list(range(B)), temp=0.0) for _ in range(8)]
        for e in embs:
            lib.minigpt4_free_embedding(e)
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefill_batch_one_row_chunk_after_decoding(gpu_lib, tiny_files):
    """A conversation with a one-token queue after decoding, alone in the call (a chunk of N = 1): same logits, position and continuation as its own flush()."""
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    lib = gpu_lib
    tok = np.ascontiguousarray([17], np.int32)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    ref = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        for c in (ctx, ref):
            lib.amd_set_conversations(c, 2)
            for s in range(2):
                _prompt(lib, c, s, PROMPTS[s])
            for _ in range(3):
                lib.amd_end_chat_batch(c, [0, 1], temp=0.0)
            lib.amd_select_conversation(c, 1)
            assert lib.library.minigpt4_amd_eval_tokens(c.ptr, tok.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1) == 0
        lib.amd_prefill_batch(ctx, [1])
        lib.amd_select_conversation(ref, 1)
        lib.amd_logits(ref)
        got, want = _state(lib, ctx, 2), _state(lib, ref, 2)
        for s in range(2):
            assert got[s][1] == want[s][1]
            assert float(np.abs(got[s][0] - want[s][0]).max() / (want[s][0].max() - want[s][0].min())) < 2e-3, s
        assert [lib.amd_end_chat_batch(ctx, [0, 1], temp=0.0) for _ in range(6)] == [lib.amd_end_chat_batch(ref, [0, 1], temp=0.0) for _ in range(6)]
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


@pytest.mark.parametrize("B,steps", [(2, 16), (4, 16), (8, 8)])
def test_prefill_batch_13b_width_matches_independent_oracle_chats(gpu_lib, monkeypatch, B, steps):
    """The serving geometry end to end: the 13b_l2 file (hd 128 x 40 heads, layer 0 a "more bits" layer whose K-split qkv combine is deferred into the slab RoPE form),
    B image turns with a different image each, packed into n_batch = 512 chunks by amd_prefill_batch before the first batched step.  Every conversation against ITS OWN
    independent OracleChat by the bar of test_configs3_operating_point_matches_independent_oracle_chats: free-running greedy pieces identical at every step, teacher-forced
    logits within 1e-2 of the largest |logit|, argmax identical on every step and on every decided step."""
    import os
    import headline as H
    from minigpt4_cpp_amd import modelgen as G
    vp, lp = H.headline_files("13b_l2")
    start = H.gpu_batched_start

    def start_and_prefill(lib, ctx, embeddings, prompts):                 # the helper queues the prompts; the prefill step evaluates them all at once
        start(lib, ctx, embeddings, prompts)
        lib.amd_prefill_batch(ctx, list(range(len(prompts))))
    monkeypatch.setattr(H, "gpu_batched_start", start_and_prefill)
    threads = max(1, min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8, 32))
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=512)
    try:
        embs = gpu_lib.amd_encode_images(ctx, [G.synth_image(300 + i) for i in range(B)])
        res = H.batched_vs_oracle(gpu_lib, ctx, lp, embs, H.BATCH_PROMPTS[:B], steps, n_ctx=512, threads=threads)
        assert len(set(res["prompt_tokens"])) > 1                                  # the conversations sit at different positions
        assert res["free_running_identical_min"] == steps, res
        assert res["teacher_forced_argmax_identical_min"] == steps, res
        assert res["max_logit_rel"] <= 1e-2, res
        assert res["decided_min"] >= steps * 3 // 4 and res["decided_argmax_mismatches"] == 0, res
    finally:
        gpu_lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 3. errors, parity mode, serve
def test_prefill_batch_rejects_bad_slot_lists_untouched(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lib = gpu_lib
    ctx = lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=0, n_ctx=256, n_batch=32)
    try:
        lib.amd_set_conversations(ctx, 3)
        for s in range(3):
            _prompt(lib, ctx, s, PROMPTS[s])
        n_past = []
        for s in range(3):
            lib.amd_select_conversation(ctx, s)
            n_past.append(lib.library.minigpt4_amd_n_past(ctx.ptr))
        for bad in ([0, 0], [0, 3], [-1], [0, 1, 2, 1]):
            with pytest.raises(RuntimeError, match="prefill_batch"):
                lib.amd_prefill_batch(ctx, bad)
        assert lib.library.minigpt4_amd_prefill_batch(ctx.ptr, None, 0) == 1
        assert lib.library.minigpt4_amd_last_error()
        for s in range(3):                                    # queues still there: a later evaluation sees them
            lib.amd_select_conversation(ctx, s)
            assert lib.library.minigpt4_amd_n_past(ctx.ptr) == n_past[s]
        lib.amd_prefill_batch(ctx, [0, 1, 2])
    finally:
        lib.minigpt4_free(ctx)


def test_prefill_batch_parity_mode_is_per_conversation_flush(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    lib = gpu_lib
    out = []
    for batched in (True, False):
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=32)
        try:
            lib.amd_set_parity(ctx, True)
            lib.amd_set_conversations(ctx, 3)
            for s in range(3):
                _prompt(lib, ctx, s, PROMPTS[s])
            if batched:
                lib.amd_prefill_batch(ctx, [1, 0, 2])
            out.append([x[0] for x in _state(lib, ctx, 3)])
        finally:
            lib.minigpt4_free(ctx)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_serve_batched_prefill_gives_the_same_answers(gpu_lib, tiny_files):
    from minigpt4_cpp_amd import modelgen as G, serve as SV
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    reqs = [SV.Request(image=G.synth_image(200 + i), prompt=PROMPTS[i].decode(), max_tokens=6) for i in range(6)]
    srv = SV.ReplicaServer(vp, lp, conversations=4, n_ctx=256, n_batch=64, library=gpu_lib)
    try:
        a = srv.run(reqs, temp=0.0, ignore_eos=True, batched_prefill=True)
        b = srv.run(reqs, temp=0.0, ignore_eos=True, batched_prefill=False)
    finally:
        srv.close()
    assert a == b and all(a)
