"""Beam search on the device: k_kv_permute and k_beam_select alone, then minigpt4_amd_beam_search against the same search driven from Python with public calls only
(whole-state forks through spare conversations for the reordering, amd_eval_batch with forced tokens in the same slot order, amd_top_logprobs, tests/beam_ref.py)."""
import os

import numpy as np
import pytest

import beam_ref as R
from conftest import record_observed
from test_cpu_beam import make_cands

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- k_kv_permute alone ------------------------------------------------------------------------------------------------------------------------------------------------
def _maps(W):
    ident = list(range(W))
    swap = [1, 0] + ident[2:]
    cycle = [(i + 1) % W for i in range(W)]
    one = [W - 1] * W
    mix = [1, 1] if W == 2 else [0, 0] + [W - 1 - (i - 2) for i in range(2, W)]          # fixed point 0 (and the middle of the reversed tail), a copy, a reversal
    return dict(identity=ident, swap=swap, cycle=cycle, all_to_one=one, mix=mix)


@pytest.mark.parametrize("E", [64, 40])
@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_kv_permute_equals_fancy_indexing(gpu_lib, W, E):
    """6 conversations (9 for W = 8, which does not fit 6), W of them listed in non-ascending order, 2 layers, n_ctx 24.  E = 40: 2 * 2 * 8 * 5 = 160 pieces do not fill the
    last workgroup of 256; E = 64, all 24 rows: 768 pieces, three workgroups."""
    n_slot, n_layer, n_ctx = max(6, W + 1), 2, 24
    rng = np.random.default_rng(W * 100 + E)
    k0 = rng.integers(0, 65536, (n_slot, n_layer, n_ctx, E), dtype=np.uint16)
    v0 = rng.integers(0, 65536, (n_slot, n_layer, n_ctx, E), dtype=np.uint16)
    slots = [int(x) for x in rng.permutation(n_slot)[:W]]
    if slots == sorted(slots):
        slots = slots[::-1]
    for name, parent in _maps(W).items():
        for r0, r1 in ((3, 11), (0, n_ctx), (5, 5)):
            k, v = gpu_lib.amd_test_kv_permute(k0, v0, slots, parent, r0, r1)
            wk, wv = k0.copy(), v0.copy()
            src = [slots[q] for q in parent]
            wk[slots, :, r0:r1] = k0[src, :, r0:r1]
            wv[slots, :, r0:r1] = v0[src, :, r0:r1]
            assert np.array_equal(k, wk) and np.array_equal(v, wv), (name, r0, r1)       # unlisted conversations and rows outside the range included
            if name == "identity" or r0 == r1:
                assert np.array_equal(k, k0) and np.array_equal(v, v0)


# ---- k_beam_select alone ---------------------------------------------------------------------------------------------------------------------------------------------------
def _select_cases():
    out = []
    for W in (2, 3, 4, 5, 6, 7, 8):
        rng = np.random.default_rng(900 + W)
        out.append((W, *make_cands(rng, 4, W)))
        out.append((W, *make_cands(rng, 4, W, grid=0.5)))
        ids, lp = make_cands(rng, 4, W, grid=100.0)
        lp[lp == 0] = np.where(rng.random(int((lp == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
        out.append((W, ids, lp))
        ids, lp = make_cands(rng, 4, W, eos_at=[(1, 0, 0), (2, W - 1, 1), (3, 0, 2 * W - 1)])
        lp[1, 0, 0] = -0.01
        out.append((W, ids, lp))
        ids, lp = make_cands(rng, 3, W, eos_at=[(1, i, 0) for i in range(W)])
        lp[1, :, 0] = -0.001
        out.append((W, ids, lp))
    return out


def test_beam_select_equals_the_host_function(gpu_lib):
    for W, ids, lp in _select_cases():
        host = gpu_lib.amd_test_beam_select_host(ids, lp, length_penalty=1.0)
        scores = np.array([0.0] + [-np.inf] * (W - 1), np.float32)
        for t, want in enumerate(host["steps"]):
            got = gpu_lib.amd_test_beam_select(ids[t], lp[t], scores, 1 if t == 0 else (1 << W) - 1, n_vocab=512)
            assert np.array_equal(got["step"], want), (W, t)
            assert np.array_equal(got["row_tok"], want[8:8 + W])
            assert got["scores"].tobytes() == want[16:16 + W].tobytes()
            scores = got["scores"]


# ---- through the C ABI -----------------------------------------------------------------------------------------------------------------------------------------------------
def _open(lib, tiny_files, wtype, mix, n_conv, parity=False):
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm(wtype, mix, conditioned=True), verbosity=0, n_ctx=256, n_batch=64)
    lib.amd_set_conversations(ctx, n_conv)
    if parity:
        lib.amd_set_parity(ctx, True)
    return ctx


def _prompt(lib, ctx, slot, text="what do you see?", extra=()):
    lib.amd_select_conversation(ctx, slot)
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.minigpt4_begin_chat(ctx, text)
    if len(extra):
        lib.amd_eval_tokens(ctx, list(extra))
    lib.amd_logits(ctx)
    return lib.library.minigpt4_amd_n_past(ctx.ptr)


def _replay(lib, ctx, slots, spare, max_tokens, lpen, p, n_ctx=256):
    """The same search with public calls only.  Beam i continues beam parent[i]: every needed parent is forked (whole state) into its spare conversation, then the spares
    into the beams that change -- any map, no overlap."""
    W = len(slots)
    lib.amd_fork_conversation(ctx, slots[0], slots[1:], -1)
    s = R.Search(W, lpen, p)
    for _ in range(min(max_tokens, n_ctx - p)):
        top = lib.amd_top_logprobs(ctx, slots, top_n=2 * W)
        d = s.step(top["top_ids"], top["top_logprobs"])
        if s.full:
            break
        par = d["parent"]
        for q in sorted(set(par[i] for i in range(W) if par[i] != i)):
            lib.amd_fork_conversation(ctx, slots[q], [spare[q]], -1)
        for i in range(W):
            if par[i] != i:
                lib.amd_fork_conversation(ctx, spare[par[i]], [slots[i]], -1)
        lib.amd_eval_batch(ctx, slots, d["tok"])
    return s.finish(), s


def _compare(lib, ctx, W, name, max_tokens=12, lpen=1.0, extra=()):
    slots = [1, 0] + list(range(2, W))                                                  # non-ascending; the source is conversation 1
    spare = list(range(W, 2 * W))
    p = _prompt(lib, ctx, slots[0], extra=extra)
    got, st = lib.amd_beam_search(ctx, slots, max_tokens, lpen, with_stats=True)
    want, s = _replay(lib, ctx, slots, spare, max_tokens, lpen, p)
    diff = max([abs(float(a[1]) - float(b[1])) for a, b in zip(got, want)] + [0.0])
    print(f"{name}: W={W} steps={s.steps} stats={st} replay={s.stats} max|score diff|={diff:g} min margin={min(d['margin'] for d in s.log):g}")
    record_observed("beam_" + name, diff)                                              # expected 0: the suite's record of observed errors shows it
    assert len(got) == len(want)
    for (a, sa), (b, sb) in zip(got, want):                                             # same pass, same row order: ids, lengths, order and the scores' bits
        assert np.array_equal(a, b)
        assert np.float32(sa).tobytes() == np.float32(sb).tobytes()
    assert [st["passes"], st["permutes"], st["rows_moved"], st["finished"]] == s.stats   # passes equal steps; rows moved follow the parents and the `common` rule
    return got, st, s


@pytest.mark.parametrize("wtype,mix", [("q4_0", "none"), ("q5_k", "q5_k_m"), ("f16", "none")])
def test_beam_search_equals_the_python_replay(gpu_lib, tiny_files, wtype, mix):
    lib = gpu_lib
    ctx = _open(lib, tiny_files, wtype, mix, 10)
    try:
        for W in (2, 4, 5):                                                             # 5 rows: the int8-MFMA set launches
            _, st, s = _compare(lib, ctx, W, f"{wtype}_{mix}_w{W}")
            assert st["passes"] == s.steps == 12 or s.full
            path = lib.amd_batch_path(ctx)
            assert path["rows"] == W and (path["sets"] > 0) == (W == 5)
    finally:
        lib.minigpt4_free(ctx)


def test_beam_search_in_parity_mode_equals_the_replay_in_parity_mode(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _open(lib, tiny_files, "q5_k", "q5_k_m", 6, parity=True)
    try:
        _compare(lib, ctx, 3, "parity_w3", max_tokens=6)
    finally:
        lib.minigpt4_free(ctx)


def _eos_walk(seed=1, n_vocab=512):
    """conftest's conditioned models tie output row u to the embedding of token perm[u] (modelgen.write_llm_file, output_tie): after token perm[u] the model says u."""
    perm = np.random.default_rng(seed + 77).permutation(n_vocab)
    a = int(perm[R.EOS])
    return [int(perm[int(perm[a])]), int(perm[a]), a]                                    # ... -> perm[a] -> a -> EOS


def test_eos_finishes_hypotheses(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _open(lib, tiny_files, "f16", "none", 4)
    try:
        _, st, s = _compare(lib, ctx, 2, "eos_w2", max_tokens=8, lpen=0.7, extra=_eos_walk()[:2])   # the prompt ends two tokens before the model says </s>
        assert s.finished >= 1 and st["finished"] == s.finished
    finally:
        lib.minigpt4_free(ctx)


def test_state_after_the_call_and_continuation(gpu_lib, tiny_files):
    import ctypes
    lib = gpu_lib
    ctx = _open(lib, tiny_files, "q5_k", "q5_k_m", 5)
    try:
        p = _prompt(lib, ctx, 0)
        before = dict(logits=lib.amd_logits(ctx).copy(), hist=lib.amd_token_history(ctx).copy(), greedy=int(lib.amd_top_logprobs(ctx, [0], 1)["top_ids"][0, 0]))
        tid = ctypes.c_int32(-1)
        assert lib.library.minigpt4_amd_sample(ctx.ptr, ctypes.byref(tid), 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
        hyps = lib.amd_beam_search(ctx, [0, 1, 2], 8, 1.0)
        lib.amd_select_conversation(ctx, 0)
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == p
        assert np.array_equal(lib.amd_logits(ctx), before["logits"])
        assert np.array_equal(lib.amd_token_history(ctx), before["hist"])
        tid2 = ctypes.c_int32(-1)
        assert lib.library.minigpt4_amd_sample(ctx.ptr, ctypes.byref(tid2), 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
        assert tid2.value == tid.value == before["greedy"]
        for slot in (1, 2):                                                              # as a prefix fork leaves them: at the source's position, no logits
            lib.amd_select_conversation(ctx, slot)
            assert lib.library.minigpt4_amd_n_past(ctx.ptr) == p
            assert np.array_equal(lib.amd_token_history(ctx), before["hist"])
            assert (lib.amd_top_logprobs(ctx, [slot], 1)["top_ids"] == -1).all()
        # the chat continues from the best hypothesis exactly as a fresh fork of the source does
        best = [int(t) for t in hyps[0][0]]
        lib.amd_fork_conversation(ctx, 0, [4], -1)
        out = []
        for slot in (0, 4):
            lib.amd_select_conversation(ctx, slot)
            lib.amd_eval_tokens(ctx, best)
            out.append([lib.minigpt4_end_chat(ctx, temp=0.0) for _ in range(5)] + [lib.amd_logits(ctx).tobytes()])
        assert out[0] == out[1]
    finally:
        lib.minigpt4_free(ctx)


def test_room_is_respected_and_a_full_context_is_refused(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _open(lib, tiny_files, "q4_0", "none", 3)
    try:
        p = _prompt(lib, ctx, 0)
        lib.amd_eval_tokens(ctx, [(37 * i) % 400 + 20 for i in range(256 - 3 - p)])      # three rows from n_ctx
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == 253
        hyps, st = lib.amd_beam_search(ctx, [0, 1, 2], 12, 1.0, with_stats=True)
        assert st["passes"] == 3 and len(hyps) == 3 and all(len(h[0]) <= 3 for h in hyps)
        lib.amd_select_conversation(ctx, 0)
        lib.amd_eval_tokens(ctx, [21, 22, 23])
        logits = lib.amd_logits(ctx).copy()
        with pytest.raises(RuntimeError, match="beam_search: context full"):
            lib.amd_beam_search(ctx, [0, 1, 2], 12, 1.0)
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == 256 and np.array_equal(lib.amd_logits(ctx), logits)
        # refusals on a live context: nothing changes
        for bad in ([0, 0], [0, 3], [0, -1]):
            with pytest.raises(RuntimeError, match="beam_search: "):
                lib.amd_beam_search(ctx, bad, 4)
        lib.amd_select_conversation(ctx, 1)
        lib.minigpt4_reset_chat(ctx)
        with pytest.raises(RuntimeError, match="beam_search: the source conversation has no current logits"):
            lib.amd_beam_search(ctx, [1, 2], 4)
    finally:
        lib.minigpt4_free(ctx)


def test_a_context_that_never_searches_launches_neither_kernel(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _open(lib, tiny_files, "q5_k", "q5_k_m", 2)
    try:
        _prompt(lib, ctx, 0)
        for _ in range(3):
            lib.minigpt4_end_chat(ctx, temp=0.0)
        prof = lib.amd_profile_sites(ctx, 2)
        names = " ".join(s["kernel"] for s in prof["sites"])
        assert names and "k_beam_select" not in names and "k_kv_permute" not in names
    finally:
        lib.minigpt4_free(ctx)


# ---- serving -------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_serve_with_two_beams_returns_the_best_hypotheses(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G, serve as S
    lib = gpu_lib
    vp, lp = os.path.join(tmpdir_models, "vision_beam.bin"), os.path.join(tmpdir_models, "llm_beam.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3), "what is the text in the picture?", 6), S.Request(G.synth_image(5), "describe it", 5)]
    srv = S.ReplicaServer(vp, lp, conversations=4, n_ctx=512, n_batch=64, library=lib)
    try:
        ctx = srv.ctx
        one = srv.run(reqs, temp=0.0, ignore_eos=True)
        got = srv.run(reqs, temp=0.0, ignore_eos=True, num_beams=2)                     # two requests x two conversations: one wave
        want = []
        for r in reqs:                                                                   # the same prompt sequence, then the search called directly
            lib.amd_select_conversation(ctx, 0)
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_system_prompt(ctx)
            emb = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(r.image))
            lib.minigpt4_begin_chat_image(ctx, emb, r.prompt)
            lib.minigpt4_free_embedding(emb)
            ids = lib.amd_beam_search(ctx, [0, 1], r.max_tokens, 1.0)[0][0]
            want.append("".join(lib.amd_token_piece(ctx, int(t)) for t in ids if int(t) != 2))
        assert got == want and all(len(a) > 0 for a in got)
        assert srv.run(reqs, temp=0.0, ignore_eos=True, num_beams=1) == one              # num_beams = 1 is today's path
        stopped = srv.run(reqs, temp=0.0, num_beams=2)
        for a, b in zip(stopped, got):
            assert "###" not in a and len(a) <= len(b)
        with pytest.raises(ValueError):
            srv.run(reqs, num_beams=5)
    finally:
        srv.close()
