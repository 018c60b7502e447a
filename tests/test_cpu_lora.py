"""LoRA adapter files on the host: minigpt4_amd_adapter_peek (csrc/formats.cpp: AdapterFile) and modelgen.write_merged_twin.  No GPU."""
import os

import numpy as np
import pytest

from minigpt4_cpp_amd import modelgen as G, quants as Q

CFG = G.tiny_llm(wtype="q4_0", n_embd=256, n_layer=2, n_head=4, n_vocab=512)


def _write(tmp_path, **kw):
    p = os.path.join(str(tmp_path), "adapter.gguf")
    args = dict(rank=8, alpha=12.0, targets=("attn_q", "attn_v", "ffn_down"), seed=5, std_a=0.05, std_b=0.05)
    args.update(kw)
    G.write_lora_gguf(p, CFG, **args)
    return p


def test_peek_good_file(lib, tmp_path):
    info = lib.amd_adapter_peek(_write(tmp_path, layers=[1]))
    assert (info["refusal"], info["rank"], info["alpha_milli"], info["n_tensors"], info["n_layers"]) == (0, 8, 12000, 6, 1)
    assert info["target_mask"] == sum(1 << lib.ADAPTER_TARGETS.index(t) for t in ("attn_q", "attn_v", "ffn_down"))
    n_ff = CFG.n_ff
    assert info["device_bytes"] == 2 * 16 * ((256 + 256) * 2 + n_ff + 256) and info["any_f32"] == 0


@pytest.mark.parametrize("kw,code", [
    (dict(general_type="model"), 1),
    (dict(omit=("blk.1.attn_v.weight.lora_b",)), 2),
    (dict(n_in_of={"attn_v": 128}), 3),
    (dict(rank=72), 4),
    (dict(rank_of={"attn_v": 4}), 4),
    (dict(gtype=Q.GGML_Q8_0), 5),
    (dict(gtype=30), 5),                                # ggml type 30: BF16
], ids=["general_type", "unpaired", "shape", "rank_above_64", "mixed_ranks", "quantised", "bf16"])
def test_peek_refusals(lib, tmp_path, kw, code):
    info = lib.amd_adapter_peek(_write(tmp_path, **kw))
    assert info["refusal"] == code and lib._err().startswith("adapter file: ")


def test_merged_twin_is_w_plus_sba(tmp_path):
    src, twin = os.path.join(str(tmp_path), "base.bin"), os.path.join(str(tmp_path), "twin.bin")
    G.write_llm_file(src, CFG, seed=1, std=0.05)
    lp = _write(tmp_path, gtype=Q.GGML_F32)
    G.write_merged_twin(src, lp, twin, scale=0.5)
    base, merged = G.read_llm_file(src), G.read_llm_file(twin)
    alpha, t = G.read_lora_gguf(lp)
    a, b = (t["blk.1.ffn_down.weight.lora_" + k].astype(np.float16).astype(np.float64) for k in "ab")
    want = base.f64("layers.1.feed_forward.w2.weight") + (alpha / 8 * 0.5) * (b @ a)
    got = merged.f64("layers.1.feed_forward.w2.weight")
    assert merged.tensors["layers.1.feed_forward.w2.weight"].gtype == Q.GGML_F32 and np.array_equal(got, want.astype(np.float32).astype(np.float64))
    assert np.abs(got - base.f64("layers.1.feed_forward.w2.weight")).max() > 1e-4
    for name in ("layers.1.attention.wk.weight", "tok_embeddings.weight"):   # not targeted: byte for byte
        assert np.array_equal(merged.raw(name), base.raw(name)) and merged.tensors[name].gtype == base.tensors[name].gtype
