"""Reuse of cached K / V rows (include/minigpt4_amd.h: minigpt4_amd_fork_conversation, minigpt4_amd_set_prefix_cache, minigpt4_amd_prefix_cache_info).

1. kernel: launch_kv_copy (through minigpt4_amd_test_kv_copy) is bit-exact, touches nothing but the copied rows of the destinations, also from a compact source;
2. fork: whole state (logits equal, identical continuation), fork-then-different-questions and a partial fork against conversations that evaluated everything themselves;
3. prefix cache: counters, the lookup / capture rules (queue length - 1, PREFIX_MIN_ROWS = 8), what empties the store, results against a cache-off context -- in the
   single pass, under amd_prefill_batch (one copy launch per wave, chunk boundaries), in parity mode (bit-identical), at the 13B width against the CPU oracle, with a
   context shift afterwards, and through serve.ReplicaServer.
The fast-mode bar is the one of test_gpu_prefill_batch._check_against_single (|logit difference| < 2e-3 of the reference logits' range, identical greedy pieces): rows
after a copied prefix run in a pass of a different size, and the K split of the prompt mat-muls depends on that size -- the same cause that bar was set for.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROMPTS = ["what is the text in the picture?", "describe the colours", "hello", "and now something longer to shift the positions apart", "a", "b c d", "zzz", "tell me more"]
MIN_ROWS = 8          # Engine::PREFIX_MIN_ROWS


# ------------------------------------------------------------------------------------------------ 1. kernel
def _caches(rng, S, L, C, E):
    k = rng.integers(0, 0x7C00, (S, L, C, E), dtype=np.uint16).view(np.float16)     # finite bit patterns, all different
    v = rng.integers(0, 0x7C00, (S, L, C, E), dtype=np.uint16).view(np.float16)
    return k, v


@pytest.mark.parametrize("dsts", [[1], [4, 2], [0, 1, 2, 3]])
@pytest.mark.parametrize("E,L", [(5120, 3), (256, 2)])
def test_kv_copy_kernel_is_bit_exact_and_touches_nothing_else(gpu_lib, E, L, dsts):
    S, C = 5, 512
    src = 0 if 4 in dsts else 4                               # from slot 4; [4, 2] (slot 4 is a destination there) from slot 0
    rng = np.random.default_rng(E + L + len(dsts))
    k, v = _caches(rng, S, L, C, E)
    for n_rows in (1, 8, 45, 142, 511, 512):
        for src_rows in (0, max(n_rows, 200) if n_rows < 512 else 0):        # 0: the slot as laid out; else a compact source with another row count
            gk, gv, ms = gpu_lib.amd_test_kv_copy(k, v, src, dsts, n_rows, src_rows)
            for got, init in ((gk, k), (gv, v)):
                got, init = got.view(np.uint16), init.view(np.uint16)
                for s in range(S):
                    if s in dsts:
                        assert np.array_equal(got[s, :, :n_rows], init[src, :, :n_rows]), (s, n_rows, src_rows)
                        assert np.array_equal(got[s, :, n_rows:], init[s, :, n_rows:]), (s, n_rows, src_rows)
                    else:
                        assert np.array_equal(got[s], init[s]), (s, n_rows, src_rows)
            assert ms > 0


def test_kv_copy_kernel_refuses_bad_shapes_and_zero_rows_is_a_no_op(gpu_lib):
    rng = np.random.default_rng(3)
    k, v = _caches(rng, 3, 2, 64, 256)
    gk, gv, _ = gpu_lib.amd_test_kv_copy(k, v, 0, [1, 2], 0)
    assert np.array_equal(gk.view(np.uint16), k.view(np.uint16)) and np.array_equal(gv.view(np.uint16), v.view(np.uint16))
    with pytest.raises(RuntimeError, match="launch_kv_copy"):
        gpu_lib.amd_test_kv_copy(k, v, 0, [1], 65)                           # above the destination's rows
    with pytest.raises(RuntimeError, match="launch_kv_copy"):
        gpu_lib.amd_test_kv_copy(k, v, 0, [1], 33, src_rows=32)              # above the compact source's rows
    k4, v4 = _caches(rng, 2, 1, 8, 12)
    with pytest.raises(RuntimeError, match="launch_kv_copy"):
        gpu_lib.amd_test_kv_copy(k4, v4, 0, [1], 4)                          # E % 8
    with pytest.raises(RuntimeError):
        gpu_lib.amd_test_kv_copy(k, v, 0, [0], 4)                            # the source among the destinations


# ------------------------------------------------------------------------------------------------ helpers
def _load(lib, vp, lp, n_conv, n_ctx=512, n_batch=64):
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=n_ctx, n_batch=n_batch)
    if n_conv > 1:
        lib.amd_set_conversations(ctx, n_conv)
    return ctx


def _embed(lib, ctx, seeds):
    from minigpt4_cpp_amd import modelgen as G
    return lib.amd_encode_images(ctx, [G.synth_image(s) for s in seeds])


def _image_rows(lib, ctx, emb):
    """The 32 rows minigpt4_begin_chat_image takes from an embedding: its first 32 * n_embd floats (the tiny vision file projects wider than the tiny LLM)."""
    lib.amd_eval_embd(ctx, np.ascontiguousarray(emb, np.float32).ravel()[:32 * lib.library.minigpt4_amd_n_embd(ctx.ptr)])


def _image_head(lib, ctx, emb):
    """The reference's fragment order up to the end of the image: system prompt, "Human: <Img>", the 32 image rows, "</Img> "."""
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"Human: <Img>"))
    _image_rows(lib, ctx, emb)
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"</Img> "))


def _question(lib, ctx, q):
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, q.encode()))
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"### Assistant:"))


def _image_turn(lib, ctx, slot, emb, q):
    import headline as H
    lib.amd_select_conversation(ctx, slot)
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    st, keep = H.embedding_struct(emb)
    lib.minigpt4_begin_chat_image(ctx, st, q)
    del keep


def _head_run(lib, ctx):
    from minigpt4_cpp_amd import modelgen as G
    return len(lib.amd_tokenize(ctx, G.SYSTEM_PROMPT.encode())) + len(lib.amd_tokenize(ctx, b"Human: <Img>"))


def _state(lib, ctx, slots):
    out = []
    for s in slots:
        lib.amd_select_conversation(ctx, s)
        out.append((lib.amd_logits(ctx).copy(), lib.library.minigpt4_amd_n_past(ctx.ptr)))
    return out


def _close(got, want, exact=False):
    for s, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], (s, g[1], w[1])
        if exact:
            assert np.array_equal(g[0], w[0]), s
        else:
            rel = float(np.abs(g[0] - w[0]).max() / (w[0].max() - w[0].min()))
            print(f"slot {s}: max |logit difference| / range = {rel:.3e}")
            assert rel < 2e-3, (s, rel)


def _pieces(lib, ctx, slots, steps=8):
    return [lib.amd_end_chat_batch(ctx, list(slots), temp=0.0) for _ in range(steps)]


@pytest.fixture()
def files(tiny_files):
    vp, llm = tiny_files
    return vp, llm("q5_k", "q5_k_m", conditioned=True)


# ------------------------------------------------------------------------------------------------ 2. fork
def test_fork_copies_the_whole_state(gpu_lib, files):
    lib = gpu_lib
    ctx = _load(lib, *files, 4)
    try:
        emb = _embed(lib, ctx, [100])[0]
        _image_turn(lib, ctx, 0, emb, PROMPTS[0])
        lib.amd_select_conversation(ctx, 2)
        lib.minigpt4_system_prompt(ctx)                                       # a queue in a destination: dropped by the fork
        lib.amd_fork_conversation(ctx, 0, [1, 2, 3])
        st = _state(lib, ctx, range(4))
        assert st[0][1] > 70 and all(s[1] == st[0][1] for s in st)
        for s in st[1:]:
            assert np.array_equal(s[0], st[0][0])
        pieces = _pieces(lib, ctx, range(4))
        assert all(len(set(step)) == 1 for step in pieces), pieces
    finally:
        lib.minigpt4_free(ctx)


@pytest.mark.parametrize("parity", [False, True])
def test_fork_then_different_questions_equals_full_prompts(gpu_lib, files, parity):
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 4), _load(lib, *files, 4)
    try:
        emb = _embed(lib, ctx, [101])[0]
        for c in (ctx, ref):
            lib.amd_set_parity(c, parity)
        lib.amd_select_conversation(ctx, 0)
        _image_head(lib, ctx, emb)
        lib.amd_fork_conversation(ctx, 0, [1, 2, 3])
        for s in range(4):
            lib.amd_select_conversation(ctx, s)
            _question(lib, ctx, PROMPTS[s])
            lib.amd_select_conversation(ref, s)
            _image_head(lib, ref, emb)
            _question(lib, ref, PROMPTS[s])
        _close(_state(lib, ctx, range(4)), _state(lib, ref, range(4)), exact=parity)
        assert _pieces(lib, ctx, range(4)) == _pieces(lib, ref, range(4))
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_partial_fork_inside_the_token_prefix(gpu_lib, files):
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 2), _load(lib, *files, 2)
    try:
        from minigpt4_cpp_amd import modelgen as G
        emb = _embed(lib, ctx, [102])[0]
        head = lib.amd_tokenize(ctx, G.SYSTEM_PROMPT.encode()) + lib.amd_tokenize(ctx, b"Human: <Img>")
        k = len(head) - 5
        for c in (ctx, ref):
            lib.amd_select_conversation(c, 0)
            _image_head(lib, c, emb)
            _question(lib, c, PROMPTS[0])
        lib.amd_fork_conversation(ctx, 0, [1], n_rows=k)                      # slot 0's queue is longer than k: it is evaluated first
        lib.amd_select_conversation(ctx, 1)
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == k
        lib.amd_eval_tokens(ctx, head[k:])
        lib.amd_select_conversation(ref, 1)
        lib.minigpt4_reset_chat(ref)
        lib.amd_eval_tokens(ref, head)
        for c in (ctx, ref):
            lib.amd_select_conversation(c, 1)
            _image_rows(lib, c, emb)
            lib.amd_eval_tokens(c, lib.amd_tokenize(c, b"</Img> "))
            _question(lib, c, PROMPTS[1])
        _close(_state(lib, ctx, range(2)), _state(lib, ref, range(2)))
        assert _pieces(lib, ctx, range(2)) == _pieces(lib, ref, range(2))
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_fork_rejects_bad_arguments_untouched(gpu_lib, files):
    lib = gpu_lib
    ctx = _load(lib, *files, 3)
    try:
        for s in range(3):
            lib.amd_select_conversation(ctx, s)
            lib.minigpt4_system_prompt(ctx)
            lib.minigpt4_begin_chat(ctx, PROMPTS[s])
        before = _state(lib, ctx, range(3))
        bad = lambda top: ((3, [1], -1), (-1, [1], -1), (0, [3], -1), (0, [-1], -1), (0, [1, 1], -1), (0, [0], -1), (0, [], -1), (0, [1], top + 1), (0, [1], -2))  # noqa: E731
        # phase 1, empty queues: a refused call changes no slot's logits, greedy token or position
        for src, dst, rows in bad(before[0][1]):
            with pytest.raises(RuntimeError, match="fork_conversation"):
                lib.amd_fork_conversation(ctx, src, dst, rows)
        again = _state(lib, ctx, range(3))
        for s in range(3):
            assert again[s][1] == before[s][1] and np.array_equal(again[s][0], before[s][0]), s
        ref = _load(lib, *files, 3)                                           # the same sequence without any refused call: equal bit for bit at the end
        try:
            for s in range(3):
                lib.amd_select_conversation(ref, s)
                lib.minigpt4_system_prompt(ref)
                lib.minigpt4_begin_chat(ref, PROMPTS[s])
            _state(lib, ref, range(3))
            for s in range(3):
                lib.amd_select_conversation(ref, s)
                lib.minigpt4_begin_chat(ref, PROMPTS[s + 3])
            want = _state(lib, ref, range(3))
            want_pieces = _pieces(lib, ref, range(3), 4)
        finally:
            lib.minigpt4_free(ref)
        for s in range(3):                                                    # phase 2: queues that a refused call must leave alone
            lib.amd_select_conversation(ctx, s)
            lib.minigpt4_begin_chat(ctx, PROMPTS[s + 3])
        n_past = [lib.amd_select_conversation(ctx, s) or lib.library.minigpt4_amd_n_past(ctx.ptr) for s in range(3)]
        for src, dst, rows in bad(n_past[0]):
            with pytest.raises(RuntimeError, match="fork_conversation"):
                lib.amd_fork_conversation(ctx, src, dst, rows)
        assert n_past == [lib.amd_select_conversation(ctx, s) or lib.library.minigpt4_amd_n_past(ctx.ptr) for s in range(3)]
        assert all(n_past[s] > before[s][1] for s in range(3))
        after = _state(lib, ctx, range(3))                                    # evaluates the intact queues
        assert [a[1] for a in after] == n_past
        assert all(not np.array_equal(a[0], b[0]) for a, b in zip(after, before))
        for s in range(3):                                                    # cached rows, logits and greedy tokens are those of a context that never saw a refused call
            assert after[s][1] == want[s][1] and np.array_equal(after[s][0], want[s][0]), s
        assert _pieces(lib, ctx, range(3), 4) == want_pieces
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 3. prefix cache
def test_prefix_cache_single_pass_counters_and_results(gpu_lib, files):
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 1), _load(lib, *files, 1)
    try:
        embs = _embed(lib, ctx, [110, 111, 112])
        lib.amd_set_prefix_cache(ctx, 256)
        run = _head_run(lib, ctx)
        assert lib.amd_prefix_cache_info(ctx) == dict(max_rows=256, stored_rows=0, hits=0, rows_reused_total=0, captures=0, rows_reused_by_last_pass=0, hit_launches=0)
        for turn in range(3):
            for c in (ctx, ref):
                _image_turn(lib, c, 0, embs[turn], PROMPTS[turn])
            got, want = _state(lib, ctx, [0]), _state(lib, ref, [0])
            info = lib.amd_prefix_cache_info(ctx)
            assert info["captures"] == 1 and info["stored_rows"] == run and info["hits"] == turn, info
            assert info["rows_reused_by_last_pass"] == (run if turn else 0) and info["rows_reused_total"] == turn * run and info["hit_launches"] == turn, info
            _close(got, want)
            assert _pieces(lib, ctx, [0]) == _pieces(lib, ref, [0])
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefix_cache_lookup_rules(gpu_lib, files):
    """A queue equal to the stored run reuses queue length - 1 rows; a 7-row common prefix reuses nothing, an 8-row one 8."""
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 1), _load(lib, *files, 1)
    try:
        lib.amd_set_prefix_cache(ctx, 256)
        base = [1] + list(range(10, 40))                                       # 31 token rows

        def run(c, ids):
            lib.minigpt4_reset_chat(c)
            lib.amd_eval_tokens(c, ids)
            return _state(lib, c, [0])

        def both(ids):
            got, want = run(ctx, ids), run(ref, ids)
            _close(got, want)
            return lib.amd_prefix_cache_info(ctx)
        info = both(base)
        assert (info["captures"], info["stored_rows"], info["hits"]) == (1, 31, 0), info
        info = both(base)                                                      # the whole queue is stored: all rows but the last are reused, the run is captured again
        assert info["rows_reused_by_last_pass"] == 30 and info["hits"] == 1 and info["captures"] == 2 and info["stored_rows"] == 31, info
        info = both(base[:MIN_ROWS - 1] + [300 + i for i in range(5)])        # 7 common rows: no reuse (and this 12-row run replaces the store)
        assert info["rows_reused_by_last_pass"] == 0 and info["hits"] == 1 and info["captures"] == 3 and info["stored_rows"] == 12, info
        both(base)
        info = both(base[:MIN_ROWS] + [400 + i for i in range(5)])            # 8 common rows: 8 reused
        assert info["rows_reused_by_last_pass"] == MIN_ROWS and info["hits"] == 2, info
        info = both(base[:5])                                                  # a run below the minimum neither hits nor captures
        assert info["rows_reused_by_last_pass"] == 0 and info["stored_rows"] == 13 and info["hits"] == 2, info
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefix_cache_is_emptied_and_off_is_byte_identical(gpu_lib, files):
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 2), _load(lib, *files, 2)
    try:
        emb = _embed(lib, ctx, [120])[0]

        def fill():
            _image_turn(lib, ctx, 0, emb, PROMPTS[0])
            lib.amd_logits(ctx)
            assert lib.amd_prefix_cache_info(ctx)["stored_rows"] > MIN_ROWS
        lib.amd_set_prefix_cache(ctx, 100000)                                  # clamped to n_ctx
        assert lib.amd_prefix_cache_info(ctx)["max_rows"] == 512
        lib.amd_set_prefix_cache(ctx, 256)
        fill()
        lib.amd_set_conversations(ctx, 2)
        assert lib.amd_prefix_cache_info(ctx)["stored_rows"] == 0 and lib.amd_prefix_cache_info(ctx)["max_rows"] == 256
        fill()
        lib.amd_set_parity(ctx, True)
        assert lib.amd_prefix_cache_info(ctx)["stored_rows"] == 0
        fill()
        lib.amd_set_parity(ctx, False)
        assert lib.amd_prefix_cache_info(ctx)["stored_rows"] == 0
        fill()
        lib.amd_set_prefix_cache(ctx, 256)
        info = lib.amd_prefix_cache_info(ctx)
        assert info["stored_rows"] == 0 and info["captures"] == 0 and info["max_rows"] == 256
        fill()
        lib.amd_set_prefix_cache(ctx, 0)
        assert lib.amd_prefix_cache_info(ctx) == dict(max_rows=0, stored_rows=0, hits=0, rows_reused_total=0, captures=0, rows_reused_by_last_pass=0, hit_launches=0)
        for c in (ctx, ref):
            _image_turn(lib, c, 0, emb, PROMPTS[1])
        got, want = _state(lib, ctx, [0]), _state(lib, ref, [0])
        assert got[0][1] == want[0][1] and np.array_equal(got[0][0], want[0][0])
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefix_cache_under_prefill_batch(gpu_lib, files):
    """B = 4 image turns, two waves, n_batch = 64: the hits' segments start at pos0 = m and continue over chunk boundaries; one copy launch serves the wave."""
    lib = gpu_lib
    B = 4
    ctx, ref = _load(lib, *files, B), _load(lib, *files, B)
    try:
        lib.amd_set_prefix_cache(ctx, 256)
        run = _head_run(lib, ctx)
        embs = _embed(lib, ctx, range(130, 130 + 2 * B))
        for wave in range(2):
            for c in (ctx, ref):
                for s in range(B):
                    _image_turn(lib, c, s, embs[wave * B + s], PROMPTS[wave * B + s])
                lib.amd_prefill_batch(c, list(range(B)))
            info = lib.amd_prefix_cache_info(ctx)
            assert info["captures"] == 1 and info["stored_rows"] == run, info
            assert info["hits"] == wave * B and info["hit_launches"] == wave and info["rows_reused_by_last_pass"] == wave * B * run, info
            _close(_state(lib, ctx, range(B)), _state(lib, ref, range(B)))
            assert _pieces(lib, ctx, range(B)) == _pieces(lib, ref, range(B))
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefix_cache_parity_mode_is_bit_identical(gpu_lib, files):
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 1, n_ctx=256, n_batch=32), _load(lib, *files, 1, n_ctx=256, n_batch=32)
    try:
        embs = _embed(lib, ctx, [140, 141])
        for c in (ctx, ref):
            lib.amd_set_parity(c, True)
        lib.amd_set_prefix_cache(ctx, 128)
        for turn in range(2):
            for c in (ctx, ref):
                _image_turn(lib, c, 0, embs[turn], PROMPTS[turn])
            _close(_state(lib, ctx, [0]), _state(lib, ref, [0]), exact=True)
        assert lib.amd_prefix_cache_info(ctx)["hits"] == 1
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_context_shift_of_a_conversation_that_started_from_a_hit(gpu_lib, files):
    """The copied rows are ordinary cache rows: a shift moves and re-rotates them exactly as in a context that evaluated them itself (same shift on both sides)."""
    lib = gpu_lib
    ctx, ref = _load(lib, *files, 1), _load(lib, *files, 1)
    try:
        embs = _embed(lib, ctx, [150, 151])
        lib.amd_set_prefix_cache(ctx, 256)
        for turn in range(2):
            for c in (ctx, ref):
                _image_turn(lib, c, 0, embs[turn], PROMPTS[turn])
                lib.amd_logits(c)
        assert lib.amd_prefix_cache_info(ctx)["hits"] == 1
        for c in (ctx, ref):
            lib.amd_shift_context(c, 4, 20)                                    # drops rows inside the copied prefix
            lib.minigpt4_begin_chat(c, PROMPTS[5])
        _close(_state(lib, ctx, [0]), _state(lib, ref, [0]))
        assert _pieces(lib, ctx, [0]) == _pieces(lib, ref, [0])
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


def test_prefix_cache_13b_width_matches_independent_oracle_chats(gpu_lib, monkeypatch):
    """The 13b_l2 file, B = 4 image turns through amd_prefill_batch with the prefix cache on and warm, against four independent CPU oracle chats: the bars of
    test_prefill_batch_13b_width_matches_independent_oracle_chats."""
    import os
    import headline as H
    B, steps = 4, 16
    vp, lp = H.headline_files("13b_l2")
    start = H.gpu_batched_start

    def start_and_prefill(lib, ctx, embeddings, prompts):
        start(lib, ctx, embeddings, prompts)
        lib.amd_prefill_batch(ctx, list(range(len(prompts))))
    monkeypatch.setattr(H, "gpu_batched_start", start_and_prefill)
    threads = max(1, min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8, 32))
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=512)
    try:
        embs = _embed(gpu_lib, ctx, range(300, 300 + B))
        gpu_lib.amd_set_conversations(ctx, B)
        gpu_lib.amd_set_prefix_cache(ctx, 256)
        start_and_prefill(gpu_lib, ctx, embs[::-1], H.BATCH_PROMPTS[:B][::-1])   # the warm-up wave captures
        assert gpu_lib.amd_prefix_cache_info(ctx)["captures"] == 1
        res = H.batched_vs_oracle(gpu_lib, ctx, lp, embs, H.BATCH_PROMPTS[:B], steps, n_ctx=512, threads=threads)
        info = gpu_lib.amd_prefix_cache_info(ctx)
        print(res, info)
        assert info["hits"] >= 4 and info["captures"] == 1, info
        assert len(set(res["prompt_tokens"])) > 1                                  # the conversations sit at different positions
        assert res["free_running_identical_min"] == steps, res
        assert res["teacher_forced_argmax_identical_min"] == steps, res
        assert res["max_logit_rel"] <= 1e-2, res
        assert res["decided_min"] >= steps * 3 // 4 and res["decided_argmax_mismatches"] == 0, res
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("batched", [True, False])
def test_serve_with_prefix_cache_gives_the_same_answers(gpu_lib, files, batched):
    from minigpt4_cpp_amd import modelgen as G, serve as SV
    vp, lp = files
    reqs = [SV.Request(image=G.synth_image(200 + i), prompt=PROMPTS[i], max_tokens=6) for i in range(6)]
    out = []
    for rows in (256, 0):
        srv = SV.ReplicaServer(vp, lp, conversations=4, n_ctx=256, n_batch=64, library=gpu_lib, prefix_cache=rows)
        try:
            out.append(srv.run(reqs, temp=0.0, ignore_eos=True, batched_prefill=batched))
            if rows:
                # waves of 4 + 2: batched, the first wave looks up an empty store (its first conversation is captured afterwards) and the second wave's 2 hit;
                # one pass per conversation, the first conversation is captured and the other 3 + 2 hit
                assert gpu_lib.amd_prefix_cache_info(srv.ctx)["hits"] == (2 if batched else 5)
        finally:
            srv.close()
    assert out[0] == out[1] and all(out[0])
