"""Run-time LoRA adapters on two paths test_gpu_lora.py's 256-wide files cannot reach: 1. an adapter on ffn_down alone behind a w1|w3 launch whose K-split combine is
deferred to its consumer (h1_ / h3_ must exist before the w2 site reads them); 2. ReplicaServer.run(adapters=...)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-2
TOKS = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]   # 21 tokens: chunks of 16 and 5 rows at n_batch 16


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_down_alone_behind_a_deferred_split(gpu_lib, tiny_files, tmpdir_models, monkeypatch):
    """A q4_k file 512 wide (two 256-value super-blocks per row: the narrowest a quantised prompt launch can split) with MINIGPT4_MMQ_KS=2: every prompt launch splits K and
    leaves its combine to its consumer, and silu * mul takes w1|w3's slabs without writing h1_ / h3_ unless something asks for them.  The adapter targets ffn_down alone, so
    nothing but the w2 site's own input makes the engine combine.  Logits within the whole-model 1e-2 of the oracle on the merged twin after the two prompt chunks and 4
    greedy steps.  Condition, on the oracle alone: base and twin differ by >= 0.1 of the largest |logit|."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, _ = tiny_files
    cfg = G.tiny_llm(wtype="q4_k", n_embd=512, n_layer=2, n_head=4, n_vocab=512)
    lp, ap, twin = (os.path.join(tmpdir_models, n) for n in ("llm_q4_k_512.bin", "lora_down.gguf", "lora_down_twin.bin"))
    G.write_llm_file(lp, cfg, seed=1, std=0.05, **G.TINY_CONDITIONED)
    G.write_lora_gguf(ap, cfg, rank=8, alpha=16.0, targets=("ffn_down",), seed=21, std_a=0.1, std_b=0.1)
    G.write_merged_twin(lp, ap, twin)
    ob, ot = (R.OracleLLM(G.read_llm_file(p), n_ctx=96) for p in (lp, twin))
    for o in (ob, ot):
        o.eval_tokens(TOKS[:16])
        o.eval_tokens(TOKS[16:])
    assert _rel(ob.logits, ot.logits) >= 0.1, _rel(ob.logits, ot.logits)
    monkeypatch.setenv("MINIGPT4_MMQ_KS", "2")
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=96, n_batch=16)
    try:
        gpu_lib.amd_set_adapter(ctx, 0, gpu_lib.amd_adapter_load(ctx, ap))
        gpu_lib.amd_eval_tokens(ctx, TOKS)
        errs = [_rel(gpu_lib.amd_logits(ctx), ot.logits)]
        for _ in range(4):
            t = int(ot.logits.argmax())
            gpu_lib.amd_eval_tokens(ctx, [t])
            ot.eval_tokens([t])
            errs.append(_rel(gpu_lib.amd_logits(ctx), ot.logits))
        print("lora ffn_down behind a deferred split: logit errors", ["%.2e" % e for e in errs])
        assert max(errs) <= TOL, errs
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_replica_server_routes_adapters(gpu_lib, tiny_files, tmpdir_models):
    """Three requests on two conversations (waves of 2 + 1) under adapter, none, adapter: each answer equals the request served alone under the same assignment, the
    adapter changes an answer, and a later call without adapters= answers as a server that never loaded one (the slots are detached)."""
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp, llm = tiny_files
    lp, ap = llm("f32", conditioned=True), os.path.join(tmpdir_models, "lora_serve.gguf")
    G.write_lora_gguf(ap, G.tiny_llm(wtype="f32", n_embd=256, n_layer=2, n_head=4, n_vocab=512), rank=8, alpha=16.0,
                      targets=("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down", "ffn_up"), seed=11, std_a=0.1, std_b=0.1)
    reqs = [S.Request(G.synth_image(3 + i), p, 6) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    which = [ap, None, ap]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=1024, n_batch=64, seed=5, library=gpu_lib)
    try:
        plain = srv.run(reqs, temp=0.0, ignore_eos=True)
        for batched_prefill in (False, True):
            got = srv.run(reqs, temp=0.0, ignore_eos=True, adapters=which, adapter_scale=4.0, batched_prefill=batched_prefill)
            alone = [srv.run([r], temp=0.0, ignore_eos=True, adapters=[a], adapter_scale=4.0)[0] for r, a in zip(reqs, which)]
            assert got == alone, (batched_prefill, got, alone)
        assert got[1] == plain[1] and (got[0] != plain[0] or got[2] != plain[2]), (got, plain)
        assert gpu_lib.amd_adapter_info(srv.ctx, 0)["loaded"] == 1             # one path, loaded once
        assert srv.run(reqs, temp=0.0, ignore_eos=True) == plain
    finally:
        srv.close()
