"""Sessions that outlive their slot (minigpt4.cpp_amd/serve.py: suspend / resume / sessions=): three two-turn sessions over a ReplicaServer with TWO conversations.
Every session is parked after its first turn and resumed -- into whatever slot its wave gives it -- for the follow-up question; each must give, greedily, the answers
of the same session run alone in a fresh server."""
import os

import pytest

pytestmark = pytest.mark.gpu


def test_three_sessions_over_two_slots_equal_each_session_alone(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp = os.path.join(tmpdir_models, "vision_state_serve.bin")
    lp = os.path.join(tmpdir_models, "llm_state_serve.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    first = [S.Request(G.synth_image(3), "what is the text in the picture?", 6), S.Request(G.synth_image(4), "describe it", 5), S.Request(G.synth_image(5), "colour?", 6)]
    second = [S.Request(None, "and the background?", 5), S.Request(None, "are you sure?", 6), S.Request(None, "why?", 4)]
    names = ["a", "b", "c"]

    def server():
        return S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)
    srv = server()
    try:
        got1 = srv.run(first, temp=0.0, ignore_eos=True, sessions=names)       # waves a b | c; all three parked afterwards
        assert sorted(srv.parked_sessions()) == names
        info = gpu_lib.amd_state_info(srv.ctx)
        assert info["saves"] == 3 and info["loads"] == 0
        got2 = srv.run(list(reversed(second)), temp=0.0, ignore_eos=True, sessions=list(reversed(names)))[::-1]   # waves c b | a: every session lands in another slot or wave
        info = gpu_lib.amd_state_info(srv.ctx)
        assert info["saves"] == 6 and info["loads"] == 3 and info["checksum_failures"] == 0
        with pytest.raises(ValueError, match="sessions"):
            srv.run([S.Request(None, "who?", 2)], temp=0.0, sessions=["nobody"])
        with pytest.raises(ValueError, match="sessions"):
            srv.run([S.Request(None, "who?", 2)], temp=0.0)
        # suspend / resume by hand: session a moves from slot 0 to slot 1 and answers a third question like a copy that stayed
        blob = srv._parked["a"]
        srv.resume(0, blob)
        srv.resume(1, srv.suspend(0))
        lib, ctx = srv.lib, srv.ctx
        answers = []
        for slot in (1, 0):
            if slot == 0:
                srv.resume(0, blob)
            lib.amd_select_conversation(ctx, slot)
            lib.minigpt4_begin_chat(ctx, "third question")
            answers.append("".join(lib.minigpt4_end_chat(ctx, temp=0.0) for _ in range(4)))
        assert answers[0] == answers[1] and answers[0]
    finally:
        srv.close()
    assert all(got1) and all(got2)
    # each session alone in a fresh server, both turns in one conversation that never leaves its slot: the reference's call sequence, no snapshot anywhere
    from minigpt4_cpp_amd import minigpt4_library as ML
    for i, name in enumerate(names):
        alone = server()
        try:
            lib, ctx = alone.lib, alone.ctx
            lib.amd_select_conversation(ctx, 0)
            lib.minigpt4_system_prompt(ctx)
            emb = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(first[i].image))
            lib.minigpt4_begin_chat_image(ctx, emb, first[i].prompt)
            lib.minigpt4_free_embedding(emb)
            one = "".join(lib.minigpt4_end_chat_image(ctx, temp=0.0) for _ in range(first[i].max_tokens))
            lib.minigpt4_begin_chat(ctx, second[i].prompt)
            two = "".join(lib.minigpt4_end_chat(ctx, temp=0.0) for _ in range(second[i].max_tokens))
            assert set(lib.amd_state_info(ctx).values()) == {0}
        finally:
            alone.close()
        assert (got1[i], got2[i]) == (one, two), name
