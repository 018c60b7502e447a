"""Run-time LoRA adapters on the GPU (csrc/lora.hip: k_lora_down / k_lora_up and their MFMA forms; minigpt4_amd_adapter_load / _set_adapter / _adapter_info).
1. the kernels alone against float64, both forms forced; 2. the whole tiny model against the CPU oracle on the merged twin; 3. three conversations under adapter X,
adapter Y and none in the same passes; 4. a quantised base with an adapter whose B is zero; 5. the refusals and the fork rule."""
import os

import numpy as np
import pytest

from lora_ref import lora_bound

pytestmark = pytest.mark.gpu

N_IN, TOL = 352, 1e-2
TOKS = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]   # 21 tokens: two chunks at n_batch 16


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
def _f64(mode, x, second):
    x = x.astype(np.float64)
    if mode == 1:
        return x * second.astype(np.float64) / np.sqrt((x * x).mean(axis=1, keepdims=True) + 1e-6)
    if mode == 2:
        return x / (1.0 + np.exp(-x)) * second.astype(np.float64)
    return x


@pytest.mark.parametrize("arrangement", ["one", "mixed"])
@pytest.mark.parametrize("form", [1, 2], ids=["vector", "mfma"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["plain", "rms", "silu"])
@pytest.mark.parametrize("n_out", [96, 288])
@pytest.mark.parametrize("r", [8, 24, 64])
@pytest.mark.parametrize("rows", [1, 3, 9, 33])
def test_kernels_against_float64(gpu_lib, rows, r, n_out, mode, form, arrangement):
    """Every output within lora_bound (tests/lora_ref.py) of the float64 value; rows without an adapter exactly 0.  33 rows: two MFMA tiles, one ragged; r = 24: the padding to 32;
    n_in = 352: not a multiple of the K steps; "mixed": rows alternate adapter 0, adapter 1, none inside one tile."""
    rng = np.random.default_rng(rows * 1000 + r * 10 + mode)
    x = rng.standard_normal((rows, N_IN)).astype(np.float32)
    second = None if mode == 0 else (1.0 + 0.1 * rng.standard_normal(N_IN)).astype(np.float32) if mode == 1 else rng.standard_normal((rows, N_IN)).astype(np.float32)
    ad = [((rng.standard_normal((r, N_IN)) * 0.1).astype(np.float16), (rng.standard_normal((n_out, r)) * 0.1).astype(np.float16), s) for s in (2.0, -0.75)]
    which = np.zeros(rows, np.int32) if arrangement == "one" else (np.arange(rows) % 3 - (np.arange(rows) % 3 == 2) * 3).astype(np.int32)   # 0, 1, -1, 0, 1, -1 ...
    got = gpu_lib.test_lora(x, second, ad, which, mode, form)
    f = _f64(mode, x, second)
    worst = 0.0
    for i in range(rows):
        if which[i] < 0:
            assert not got[i].any(), i
            continue
        a, b, s = (np.asarray(v, np.float64) for v in ad[which[i]])
        want = s * (b @ (a @ f[i]))
        terms = abs(s) * (np.abs(b) @ (np.abs(a) @ np.abs(f[i])))
        ratio = np.abs(got[i] - want) / lora_bound(form, N_IN, r, terms)
        worst = max(worst, float(ratio.max()))
    print(f"lora kernels rows={rows} r={r} n_out={n_out} mode={mode} form={form} {arrangement}: largest error / bound = {worst:.3g}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 2. - 4. the whole tiny model
ALL7 = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down", "ffn_up")


@pytest.fixture(scope="module")
def files(tiny_files, tmpdir_models):
    """The f32 conditioned base, two rank-8 adapters on all seven targets of both layers, their merged twins, and the oracle's logits after TOKS on each (computed once)."""
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    base = llm("f32", conditioned=True)
    cfg = G.tiny_llm(wtype="f32", n_embd=256, n_layer=2, n_head=4, n_vocab=512)
    out = {"vision": vp, "base": base, "cfg": cfg}
    for name, seed in (("x", 11), ("y", 12)):
        lp, twin = os.path.join(tmpdir_models, f"lora_{name}.gguf"), os.path.join(tmpdir_models, f"lora_{name}_twin.bin")
        G.write_lora_gguf(lp, cfg, rank=8, alpha=16.0, targets=ALL7, seed=seed, std_a=0.1, std_b=0.1)
        G.write_merged_twin(base, lp, twin)
        out[name], out[name + "_twin"] = lp, twin
    return out


def _oracle(path):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    return R.OracleLLM(G.read_llm_file(path), n_ctx=96)


def _walk(lib, ctx, o, steps, strict):
    """ctx and oracle o have evaluated the same rows: `steps` greedy steps on the oracle's ids; the errors, the ids, how many choices were decisive.  strict: the ids
    must be equal at every step, else wherever the oracle's top-2 margin exceeds the tolerance."""
    got, want = lib.amd_logits(ctx), o.logits
    errs, ids, decided = [_rel(got, want)], [], 0
    for _ in range(steps):
        srt = np.sort(want)
        margin = (srt[-1] - srt[-2]) / (np.abs(want).max() + 1e-30)
        decided += int(margin > 2 * TOL)
        gid, oid = int(got.argmax()), int(want.argmax())
        if strict or margin > TOL:
            assert gid == oid, (len(ids), gid, oid)
        ids.append(oid)
        lib.amd_eval_tokens(ctx, [oid])
        want = o.eval_tokens([oid])
        got = lib.amd_logits(ctx)
        errs.append(_rel(got, want))
    return errs, ids, decided


def test_whole_model_against_merged_twin(gpu_lib, files):
    """21 prompt tokens at n_batch 16 (the MFMA forms at 16 rows, the vector forms at 5), then 8 greedy steps (vector forms, captured graph): logits within 1e-2 of the
    largest |logit| of the oracle on the merged twin.  Condition, on the oracle alone: base and twin differ by >= 0.1 of the largest |logit| -- an ignored adapter fails."""
    ob, ot = _oracle(files["base"]), _oracle(files["x_twin"])
    for o in (ob, ot):
        o.eval_tokens(TOKS[:16])
        o.eval_tokens(TOKS[16:])
    assert _rel(ob.logits, ot.logits) >= 0.1, _rel(ob.logits, ot.logits)
    ctx = gpu_lib.minigpt4_model_load(files["vision"], files["base"], verbosity=0, n_ctx=96, n_batch=16)
    try:
        h = gpu_lib.amd_adapter_load(ctx, files["x"])
        gpu_lib.amd_set_adapter(ctx, 0, h)
        gpu_lib.amd_eval_tokens(ctx, TOKS)
        errs, _, _ = _walk(gpu_lib, ctx, ot, 8, strict=False)
        print("lora whole model: logit errors", ["%.2e" % e for e in errs])
        assert max(errs) <= TOL, errs
        info = gpu_lib.amd_adapter_info(ctx, 0)
        assert (info["handle"], info["scale_micro"], info["rank"], info["target_mask"], info["loaded"]) == (h, 1000000, 8, 127, 1) and info["down_launches"] == info["up_launches"] > 0
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_whole_model_at_a_multi_slab_width(gpu_lib, tiny_files, tmpdir_models):
    """n_embd 1024, one layer, 8 heads: n_ff = 2816, so the vector forms sum 2 (n_embd) and 6 (ffn_down) K slabs and the MFMA form 2 at ffn_down; one rank-64 adapter on all
    seven targets (192 rows of A at q | k | v).  37 prompt tokens at n_batch 64 (two MFMA row tiles, the second with 5 rows), then 8 greedy steps on the vector forms:
    logits within 1e-2 of the largest |logit| of the oracle on the merged twin.  Condition, on the oracle alone: base and twin differ by >= 0.1 of the largest |logit|."""
    from minigpt4_cpp_amd import modelgen as G
    vp, _ = tiny_files
    cfg = G.tiny_llm(wtype="f32", n_embd=1024, n_layer=1, n_head=8, n_vocab=512)
    assert cfg.n_ff == 2816
    base, lp, twin = (os.path.join(tmpdir_models, n) for n in ("llm_f32_1024.bin", "lora_1024.gguf", "lora_1024_twin.bin"))
    G.write_llm_file(base, cfg, seed=1, std=0.05, **G.TINY_CONDITIONED)
    G.write_lora_gguf(lp, cfg, rank=64, alpha=64.0, targets=ALL7, seed=31, std_a=0.05, std_b=0.05)
    G.write_merged_twin(base, lp, twin)
    toks = TOKS[:10] + list(range(301, 328))
    assert len(toks) == 37
    ob, ot = _oracle(base), _oracle(twin)
    for o in (ob, ot):
        o.eval_tokens(toks)
    assert _rel(ob.logits, ot.logits) >= 0.1, _rel(ob.logits, ot.logits)
    ctx = gpu_lib.minigpt4_model_load(vp, base, verbosity=0, n_ctx=96, n_batch=64)
    try:
        gpu_lib.amd_set_adapter(ctx, 0, gpu_lib.amd_adapter_load(ctx, lp))
        gpu_lib.amd_eval_tokens(ctx, toks)
        errs, _, _ = _walk(gpu_lib, ctx, ot, 8, strict=False)
        print("lora whole model, 1024 wide: logit errors", ["%.2e" % e for e in errs])
        assert max(errs) <= TOL, errs
        info = gpu_lib.amd_adapter_info(ctx, 0)
        assert (info["rank"], info["target_mask"]) == (64, 127) and info["down_launches"] == info["up_launches"] >= 8   # four site groups: the prompt pass, the decode step
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("form", [0, 2], ids=["by_rows", "mfma"])
def test_routing_three_conversations(gpu_lib, files, monkeypatch, form):
    """Conversations under adapter X, adapter Y and none share amd_prefill_batch's packed chunks and 4 amd_eval_batch steps; each stays within 1e-2 of its own oracle."""
    if form:
        monkeypatch.setenv("MINIGPT4_LORA_FORM", str(form))
    prompts = [TOKS, TOKS[:13], [1] + TOKS[12:20]]
    oracles = [_oracle(files["x_twin"]), _oracle(files["y_twin"]), _oracle(files["base"])]
    ctx = gpu_lib.minigpt4_model_load(files["vision"], files["base"], verbosity=0, n_ctx=96, n_batch=16)
    try:
        gpu_lib.amd_set_conversations(ctx, 3)
        for s, name in enumerate(("x", "y")):
            gpu_lib.amd_set_adapter(ctx, s, gpu_lib.amd_adapter_load(ctx, files[name]))
        for s, p in enumerate(prompts):
            gpu_lib.amd_select_conversation(ctx, s)
            gpu_lib.amd_eval_tokens(ctx, p)
            oracles[s].eval_tokens(p)
        gpu_lib.amd_prefill_batch(ctx, [0, 1, 2])
        for step in range(5):
            for s, o in enumerate(oracles):
                gpu_lib.amd_select_conversation(ctx, s)
                assert _rel(gpu_lib.amd_logits(ctx), o.logits) <= TOL, (step, s, _rel(gpu_lib.amd_logits(ctx), o.logits))
            if step < 4:
                ids = [int(o.logits.argmax()) for o in oracles]
                gpu_lib.amd_eval_batch(ctx, [0, 1, 2], ids)
                for o, t in zip(oracles, ids):
                    o.eval_tokens([t])
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_quantised_base_with_zero_b(gpu_lib, tiny_files, tmpdir_models):
    """q4_k base + a q, v adapter whose B is zero: what test_gpu_parity.py::test_llm_logits_and_greedy_tokens asserts without an adapter, and the kernels did run."""
    from conftest import observed_bar
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp, ap = llm("q4_k", "none", conditioned=True), os.path.join(tmpdir_models, "lora_zero_b.gguf")
    G.write_lora_gguf(ap, G.tiny_llm(wtype="q4_k", n_embd=256, n_layer=2, n_head=4, n_vocab=512), rank=8, alpha=16.0, targets=("attn_q", "attn_v"), seed=3, std_a=0.05, std_b=0.0)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=96, n_batch=16)
    try:
        gpu_lib.amd_set_adapter(ctx, 0, gpu_lib.amd_adapter_load(ctx, ap))
        o = _oracle(lp)
        gpu_lib.amd_eval_tokens(ctx, TOKS)
        o.eval_tokens(TOKS[:16])
        o.eval_tokens(TOKS[16:])
        errs, ids, decided = _walk(gpu_lib, ctx, o, 24, strict=True)
        assert max(errs) <= observed_bar("llm_logits/q4_k_none", TOL), (max(errs), errs)
        assert decided >= 20 and len(set(ids)) >= 12, (decided, ids)
        info = gpu_lib.amd_adapter_info(ctx, 0)
        assert info["down_launches"] > 0 and info["up_launches"] > 0 and info["target_mask"] == 5
    finally:
        gpu_lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 5. refusals, fork
def _refused(lib, call):
    with pytest.raises(RuntimeError):
        call()
    assert lib._err()


@pytest.mark.parametrize("case", ["cached_rows", "parity_on", "set_parity", "free_in_use", "ninth_load"])
def test_refusals(gpu_lib, files, case):
    lib = gpu_lib
    ctx = lib.minigpt4_model_load(files["vision"], files["base"], verbosity=0, n_ctx=96, n_batch=16)
    try:
        h = lib.amd_adapter_load(ctx, files["x"])
        if case == "cached_rows":
            lib.amd_eval_tokens(ctx, TOKS[:4])
            lib.amd_logits(ctx)
            _refused(lib, lambda: lib.amd_set_adapter(ctx, 0, h))
        elif case == "parity_on":
            lib.amd_set_parity(ctx, True)
            _refused(lib, lambda: lib.amd_set_adapter(ctx, 0, h))
        elif case == "set_parity":
            lib.amd_set_adapter(ctx, 0, h)
            _refused(lib, lambda: lib.amd_set_parity(ctx, True))
        elif case == "free_in_use":
            lib.amd_set_adapter(ctx, 0, h)
            _refused(lib, lambda: lib.amd_adapter_free(ctx, h))
            lib.amd_set_adapter(ctx, 0, 0)
            lib.amd_adapter_free(ctx, h)
        else:
            assert [lib.amd_adapter_load(ctx, files["y"]) for _ in range(7)] == list(range(2, 9))
            _refused(lib, lambda: lib.amd_adapter_load(ctx, files["y"]))
    finally:
        lib.minigpt4_free(ctx)


def test_fork_copies_the_assignment(gpu_lib, files):
    lib = gpu_lib
    ctx = lib.minigpt4_model_load(files["vision"], files["base"], verbosity=0, n_ctx=96, n_batch=16)
    try:
        lib.amd_set_conversations(ctx, 3)
        h = lib.amd_adapter_load(ctx, files["x"])
        lib.amd_set_adapter(ctx, 0, h, 0.5)
        lib.amd_eval_tokens(ctx, TOKS[:6])
        lib.amd_fork_conversation(ctx, 0, [2])
        assert [(lib.amd_adapter_info(ctx, s)["handle"], lib.amd_adapter_info(ctx, s)["scale_micro"]) for s in range(3)] == [(h, 500000), (0, 0), (h, 500000)]
        lib.amd_select_conversation(ctx, 0)
        a = lib.amd_logits(ctx)
        lib.amd_select_conversation(ctx, 2)
        assert np.array_equal(a, lib.amd_logits(ctx))
        ids = lib.amd_eval_batch(ctx, [0, 2], [7, 7])                        # both advance under the same adapter
        assert ids[0] == ids[1]
        lib.amd_select_conversation(ctx, 0)
        a = lib.amd_logits(ctx)
        lib.amd_select_conversation(ctx, 2)
        assert np.array_equal(a, lib.amd_logits(ctx))
    finally:
        lib.minigpt4_free(ctx)
