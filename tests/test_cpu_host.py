"""CPU-only tier: oracle vs independent float64 math, file formats, host logic of the product (tokenizer, sampler, loaders) through the
C-ABI, and the drop-in ABI surface (every declared symbol exported; no compute calls without a GPU)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_QTYPES = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q2_k", "q4_k", "q5_k", "q6_k", "f16"]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ block formats
def test_hand_computed_block_vectors():
    """Known-answer blocks built by hand from the layouts of SURVEY.md 2.5 (one block each, known d / scales / nibbles)."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    # Q4_0: d = 0.5, qs[j] = j | ((15-j) << 4)  ->  y[j] = (j-8)*0.5, y[16+j] = (7-j)*0.5
    b = np.zeros(18, np.uint8)
    b[0:2] = np.frombuffer(np.float16(0.5).tobytes(), np.uint8)
    b[2:] = [j | ((15 - j) << 4) for j in range(16)]
    want = np.array([(j - 8) * 0.5 for j in range(16)] + [(7 - j) * 0.5 for j in range(16)])
    assert np.array_equal(R.dequantize_row(Q.GGML_Q4_0, b, 32), want.astype(np.float32))
    assert np.array_equal(Q.dequantize(Q.GGML_Q4_0, b, 32), want)
    # Q8_0: d = 0.25, qs = -16..15
    b = np.zeros(34, np.uint8)
    b[0:2] = np.frombuffer(np.float16(0.25).tobytes(), np.uint8)
    b[2:] = np.arange(-16, 16, dtype=np.int8).view(np.uint8)
    assert np.array_equal(R.dequantize_row(Q.GGML_Q8_0, b, 32), (np.arange(-16, 16) * 0.25).astype(np.float32))
    # Q5_K: d = 1, dmin = 0.5; sub-block s: scale s+1, min s; every weight of sub-block s has q = 16 + s (high bit set, low nibble s)
    b = np.zeros(176, np.uint8)
    b[0:2] = np.frombuffer(np.float16(1.0).tobytes(), np.uint8)
    b[2:4] = np.frombuffer(np.float16(0.5).tobytes(), np.uint8)
    sc, mn = np.arange(1, 9), np.arange(0, 8)
    for j in range(4):
        b[4 + j] = (sc[j] & 63) | ((sc[j + 4] >> 4) << 6)
        b[4 + j + 4] = (mn[j] & 63) | ((mn[j + 4] >> 4) << 6)
        b[4 + j + 8] = (sc[j + 4] & 15) | ((mn[j + 4] & 15) << 4)
    b[16:48] = 0xFF
    for j in range(4):
        b[48 + 32 * j:48 + 32 * j + 32] = (2 * j) | ((2 * j + 1) << 4)
    want = np.concatenate([np.full(32, (s + 1) * (16 + s) - 0.5 * s) for s in range(8)])
    assert np.array_equal(R.dequantize_row(Q.GGML_Q5_K, b, 256), want.astype(np.float32))
    assert np.array_equal(Q.dequantize(Q.GGML_Q5_K, b, 256), want)
    # Q6_K: d = 2; 16 sub-blocks with scale s-8; all weights q = 33 (ql nibble 1, qh bits 10b) -> (33-32) * 2 * (s-8)
    b = np.zeros(210, np.uint8)
    b[0:128] = 0x11
    b[128:192] = 0xAA
    b[192:208] = np.arange(-8, 8, dtype=np.int8).view(np.uint8)
    b[208:210] = np.frombuffer(np.float16(2.0).tobytes(), np.uint8)
    want = np.repeat(2.0 * np.arange(-8, 8), 16)
    assert np.array_equal(R.dequantize_row(Q.GGML_Q6_K, b, 256), want.astype(np.float32))
    assert np.array_equal(Q.dequantize(Q.GGML_Q6_K, b, 256), want)


@pytest.mark.parametrize("wtype", ALL_QTYPES)
def test_quantisers_roundtrip_and_agree_with_oracle(wtype):
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    x = (0.02 * np.random.default_rng(3).standard_normal(256 * 6)).astype(np.float32)
    raw = Q.quantize(t, x)
    assert raw.nbytes == Q.nbytes(t, x.size) == R.lib().orc_type_bytes(t) * x.size // R.lib().orc_type_block(t)
    d_np, d_c = Q.dequantize(t, raw, x.size), R.dequantize_row(t, raw, x.size)
    assert np.abs(d_np - d_c).max() <= 1e-7 * np.abs(d_np).max()
    bound = {"q4_0": 0.12, "q4_1": 0.08, "q5_0": 0.06, "q5_1": 0.04, "q8_0": 0.01, "q2_k": 0.4, "q4_k": 0.08, "q5_k": 0.04, "q6_k": 0.03, "f16": 1e-3}[wtype]
    assert _rel(d_np, x) < bound


@pytest.mark.parametrize("wtype", ALL_QTYPES + ["f32"])
def test_oracle_mul_mat_vs_float64(wtype):
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(11)
    w = (0.05 * rng.standard_normal((40, 512))).astype(np.float32)
    raw = Q.quantize(t, w)
    x = rng.standard_normal((3, 512)).astype(np.float32)
    y = R.mul_mat(t, raw, 512, 40, x)
    ref = x.astype(np.float64) @ Q.dequantize(t, raw, w.size).reshape(40, 512).T
    assert _rel(y, ref) < (2e-2 if wtype not in ("f16", "f32") else 2e-3)
    # linearity in the weights' scale is exact for the integer-dot types when scaling by a power of two
    if wtype in ("q4_0", "q8_0"):
        raw2 = Q.quantize(t, w * 2.0)
        assert np.array_equal(R.mul_mat(t, raw2, 512, 40, x), 2.0 * y)


# ------------------------------------------------------------------------------------------------ models (oracle vs float64)
@pytest.mark.parametrize("wtype,mix", [("q4_0", "none"), ("q5_k", "q5_k_m"), ("f16", "none")])
def test_oracle_llama_vs_float64(tiny_files, wtype, mix):
    import f64ref as F
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    _, llm = tiny_files
    f = G.read_llm_file(llm(wtype, mix))
    o, ref = R.OracleLLM(f, n_ctx=64), F.LlamaF64(f)
    toks = [1, 5, 300, 44, 270, 99, 400]
    lo, lr = o.eval_tokens(toks, all_logits=True), ref.eval(tokens=toks)
    tol = 2e-3 if wtype == "f16" else 6e-2
    assert _rel(lo, lr) < tol
    assert _rel(o.eval_tokens([17]), ref.eval(tokens=[17])[0]) < tol
    # chunked prefill == one-shot prefill (KV cache semantics), bit-exact inside the oracle
    o2 = R.OracleLLM(f, n_ctx=64)
    o2.eval_tokens(toks[:3])
    o2.eval_tokens(toks[3:])
    o2.eval_tokens([17])
    assert _rel(o2.logits, o.logits) < 1e-5


def test_oracle_sensitivity(tiny_files):
    """Documents why whole-model parity is a tolerance, not bit-exactness: with ggml's int8 activation quantisation a 1e-6 relative input
    perturbation (the size of fp32 summation-order noise) moves the oracle's OWN logits by up to ~1e-2 of their range."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    _, llm = tiny_files
    f = G.read_llm_file(llm("q4_0"))
    tt = f.tensors["tok_embeddings.weight"]
    table = R.dequantize_row(tt.gtype, f.raw("tok_embeddings.weight"), 512 * 256).reshape(512, 256)
    toks = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302]

    def run(eps):
        o = R.OracleLLM(f, n_ctx=64)
        e = table[toks] * (1 + eps * np.random.default_rng(1).standard_normal((len(toks), 256))).astype(np.float32)
        return o.eval_embd(e)
    base = run(0.0)
    amp = [(_rel(run(eps), base), eps) for eps in (1e-6, 3e-6, 1e-5, 3e-5)]
    assert all(d < 5e-2 for d, _ in amp), amp
    assert any(d > 50 * eps for d, eps in amp), amp      # rounding flips amplify the perturbation by orders of magnitude


def test_oracle_vision_vs_float64(tiny_files):
    import f64ref as F
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, _ = tiny_files
    vf = G.read_vision_file(vp)
    ov, img = R.OracleVision(vf), G.synth_image(42)
    for st in (1, 2, 3):
        _, s = ov.encode(img, st)
        assert _rel(s, F.vision_f64(vf, img, st)) < 3e-3, st
    assert _rel(ov.encode(img), F.vision_f64(vf, img, 0)) < 3e-3


# ------------------------------------------------------------------------------------------------ file formats
def test_vision_file_layout_matches_convert_py(tiny_files):
    """Byte layout of the reference writer (convert.py:146-180, 74-144): header, config JSON, 5 models in order, page-aligned payloads,
    reversed shapes, F16 only for >=2-D `weight` tensors outside query_tokens / ln_vision."""
    from minigpt4_cpp_amd import modelgen as G, quants as Q
    vp, _ = tiny_files
    raw = open(vp, "rb").read()
    assert raw[:4] == b"ggml" and struct.unpack_from("ii", raw, 4) == (1, 0)
    vf = G.read_vision_file(vp)
    assert list(vf.models) == ["visual_encoder", "ln_vision", "query_tokens", "Qformer", "llama_proj"]
    assert vf.config["Qformer"]["encoder_width"] == 176 and vf.config["Qformer"]["query_length"] == 32
    for m, ts in vf.models.items():
        for n, t in ts.items():
            assert t.offset % 4096 == 0
            want16 = m not in ("query_tokens", "ln_vision") and n.endswith("weight") and len(t.ne) >= 2
            assert t.gtype == (Q.GGML_F16 if want16 else Q.GGML_F32), (m, n)
    assert vf.models["visual_encoder"]["pos_embed"].ne == (176, 257)
    assert vf.models["visual_encoder"]["patch_embed.proj.weight"].ne == (14, 14, 3, 176)
    assert vf.models["query_tokens"]["weight"].ne == (768, 32)
    last = max((t.offset + t.nbytes) for ts in vf.models.values() for t in ts.values())
    assert last == len(raw)


def test_llm_file_layout_and_bytes_per_token(tiny_files):
    from minigpt4_cpp_amd import modelgen as G, quants as Q
    _, llm = tiny_files
    f = G.read_llm_file(llm("q5_k", "q5_k_m"))
    assert f.hparams["n_embd"] == 256 and f.hparams["n_layer"] == 2 and len(f.vocab) == 512
    assert all(t.offset % 32 == 0 for t in f.tensors.values())
    assert f.tensors["output.weight"].gtype == Q.GGML_Q6_K and f.tensors["norm.weight"].gtype == Q.GGML_F32
    assert f.tensors["layers.1.attention.wv.weight"].gtype == Q.GGML_Q6_K   # use_more_bits(1, 2)
    # the BASELINE figures: 9.117 GB (13B Q5_K_M) and 3.751 GB (7B Q4_0, output Q6_K) streamed per token
    assert abs(G.llm_weight_bytes_per_token(G.llm_13b()) / 1e9 - 9.117) < 0.001
    assert abs(G.llm_weight_bytes_per_token(G.llm_7b()) / 1e9 - 3.751) < 0.001


def test_kquant_fallback_types_of_the_real_vicuna_v0_vocabulary(tmp_path):
    """llama.cpp's k-quant quantiser cannot give a k-quant type to a tensor with a dimension that is not a multiple of 256: with Vicuna-v0's n_vocab = 32001 the file the
    reference's README names (ggml-vicuna-13B-v0-q5_k.bin) has output.weight in F16 and tok_embeddings in Q4_0 -> 9.310 GB streamed per token.  The
    generator applies that rule, the product's host-side loader and the oracle read such a file, and the oracle evaluates it."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G, quants as Q
    cfg, _ = G.headline_llm("13b_v32001")
    t = G.llm_tensor_types(cfg)
    assert t["output.weight"] == Q.GGML_F16 and t["tok_embeddings.weight"] == Q.GGML_Q4_0
    assert t["layers.0.attention.wv.weight"] == Q.GGML_Q6_K and t["layers.5.attention.wv.weight"] == Q.GGML_Q5_K and t["layers.5.feed_forward.w1.weight"] == Q.GGML_Q5_K
    assert abs(G.llm_weight_bytes_per_token(cfg) / 1e9 - 9.310) < 0.001
    for name, want in (("7b_q8_0", 7.021), ("7b_q4_1", 4.130)):
        assert abs(G.llm_weight_bytes_per_token(G.headline_llm(name)[0]) / 1e9 - want) < 0.001
    # an explicit type still wins; a vocabulary that IS a multiple of 256 keeps the k-quant types
    assert G.llm_tensor_types(G.tiny_llm(wtype="q5_k", n_embd=256, n_vocab=513, mix="q5_k_m", output_type="q8_0"))["output.weight"] == Q.GGML_Q8_0
    assert G.llm_tensor_types(G.tiny_llm(wtype="q5_k", n_embd=256, n_vocab=512, mix="q5_k_m"))["output.weight"] == Q.GGML_Q6_K
    small = G.tiny_llm(wtype="q5_k", n_embd=256, n_layer=1, n_head=4, n_vocab=513, mix="q5_k_m")
    lp = str(tmp_path / "oddv.bin")
    G.write_llm_file(lp, small, seed=5, std=0.05)
    f = G.read_llm_file(lp)
    assert f.tensors["output.weight"].gtype == Q.GGML_F16 and f.tensors["output.weight"].ne == (256, 513) and f.tensors["tok_embeddings.weight"].gtype == Q.GGML_Q4_0
    logits = R.OracleLLM(f, n_ctx=16).eval_tokens([1, 5, 512])          # 512: the last row of the odd vocabulary
    assert logits.shape == (513,) and np.isfinite(logits).all()


def test_product_loaders_parse_both_files_without_gpu(lib, tiny_files, tmp_path):
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m")
    nv, nl, wb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert lib.library.minigpt4_amd_inspect_files(vp.encode(), lp.encode(), ctypes.byref(nv), ctypes.byref(nl), ctypes.byref(wb)) == 0
    vf, lf = G.read_vision_file(vp), G.read_llm_file(lp)
    assert nv.value == sum(len(m) for m in vf.models.values()) and nl.value == len(lf.tensors)
    assert wb.value == G.llm_weight_bytes_per_token(G.tiny_llm(wtype="q5_k", n_embd=256, n_layer=2, n_head=4, n_vocab=512, mix="q5_k_m"))
    # malformed inputs -> the reference's error codes, never a crash
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"gguf" + open(vp, "rb").read()[4:200])
    assert lib.library.minigpt4_amd_inspect_files(str(bad).encode(), None, None, None, None) == 1      # LoadModelFileHeader
    bad.write_bytes(b"ggml" + struct.pack("i", 0) + open(vp, "rb").read()[8:200])
    assert lib.library.minigpt4_amd_inspect_files(str(bad).encode(), None, None, None, None) == 2      # LoadModelFileVersion
    bad.write_bytes(open(vp, "rb").read()[:5000])
    assert lib.library.minigpt4_amd_inspect_files(str(bad).encode(), None, None, None, None) == 1      # truncated payload
    bad.write_bytes(open(lp, "rb").read()[:3000])
    assert lib.library.minigpt4_amd_inspect_files(None, str(bad).encode(), None, None, None) == 4      # LoadLanguageModel
    assert lib.library.minigpt4_amd_inspect_files(b"/nonexistent", None, None, None, None) == 17       # PathDoesNotExist
    # corrupt counts / shapes must be refused before they size an allocation (found by fuzzing the parsers under ASAN: a tensor count of 2^31 - 1,
    # a vocabulary larger than the file, dimensions whose product overflows)
    raw = bytearray(open(vp, "rb").read()[:20000])
    clen = struct.unpack_from("i", raw, 12)[0]
    mname_len = struct.unpack_from("i", raw, 16 + clen)[0]
    struct.pack_into("i", raw, 16 + clen + 4 + mname_len, 0x7FFFFFFF)                                   # tensor count of the first model
    bad.write_bytes(bytes(raw))
    assert lib.library.minigpt4_amd_inspect_files(str(bad).encode(), None, None, None, None) == 1
    raw = bytearray(open(lp, "rb").read()[:20000])
    struct.pack_into("I", raw, 8, 1 << 24)                                                             # n_vocab far beyond the file
    bad.write_bytes(bytes(raw))
    assert lib.library.minigpt4_amd_inspect_files(None, str(bad).encode(), None, None, None) == 4
    full = bytearray(open(lp, "rb").read())
    lf2 = G.read_llm_file(lp)
    first = min(lf2.tensors.values(), key=lambda t: t.offset)
    hdr = bytes(full).rfind(first.name.encode(), 0, first.offset)                                      # its header: nd, name_len, type, ne[nd], name
    nd = len(first.ne)
    struct.pack_into("II", full, hdr - 4 * nd, 0xFFFFFFFF, 0xFFFFFFFF) if nd == 2 else struct.pack_into("I", full, hdr - 4, 0xFFFFFFFF)
    bad.write_bytes(bytes(full))
    assert lib.library.minigpt4_amd_inspect_files(None, str(bad).encode(), None, None, None) == 4


def test_oracle_simd_dots_equal_scalar():
    """The AVX2 dot products of the oracle (the timed CPU baseline) against its scalar restatement: bit-identical, on quantised Gaussian weights and on arbitrary
    block bytes (every bit pattern of the quant fields, sane fp16 scales), for activations of very different magnitudes."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    L = R.lib()
    rng = np.random.default_rng(11)
    n_in, n_out = 2048, 48
    try:
        for name in ("q4_0", "q4_k", "q5_k", "q6_k"):
            t = Q.NAME_TO_TYPE[name]
            be, bb = Q.BLOCK[t]
            raws = [Q.quantize(t, (0.05 * rng.standard_normal((n_out, n_in))).astype(np.float32))]
            arb = rng.integers(0, 256, (n_in // be * n_out, bb), dtype=np.uint8)
            f16 = (rng.standard_normal((arb.shape[0], 2)) * 0.01).astype(np.float16).view(np.uint8).reshape(-1, 4)
            if name == "q4_0":
                arb[:, 0:2] = f16[:, 0:2]
            elif name == "q6_k":
                arb[:, 208:210] = f16[:, 0:2]
            else:
                arb[:, 0:4] = f16
            raws.append(arb.reshape(-1))
            x = (rng.standard_normal((4, n_in)) * np.array([1.0, 37.0, 1e-3, 0.0])[:, None]).astype(np.float32)
            for raw in raws:
                L.orc_set_simd(1)
                a = R.mul_mat(t, raw, n_in, n_out, x)
                L.orc_set_simd(0)
                b = R.mul_mat(t, raw, n_in, n_out, x)
                assert np.array_equal(a, b), name
    finally:
        L.orc_set_simd(1)


def test_oracle_accumulation_orders(tiny_files):
    """The oracle's two fp32 accumulation orders (oracle/refcpu.c): order 0 = ONE fma chain per output (what the GPU's parity mode reproduces bit for bit), order 1 = ggml's
    own x86 structure as best recalled (eight lane partials per row, fmadd per block, hsum at the end; the k-quant min term in a separate four-lane accumulator).  Same
    integers, different fp32 additions: every dot product of the two agrees to <= 1e-5 of the row's largest value and the results differ in their last bits; the AVX2 form of
    order 1 is bit-identical to its scalar lane-by-lane restatement; a whole tiny model evaluates in both orders to logits within 1e-3 of each other."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G, quants as Q
    L = R.lib()
    rng = np.random.default_rng(23)
    n_in, n_out = 2048 + 32, 64               # + 32: a 32-element tail for the F16 / F32 rows' vector loop; k-quants use 2048
    try:
        for name in ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q4_k", "q5_k", "q6_k", "f16", "f32"):
            t = Q.NAME_TO_TYPE[name]
            k = 2048 if Q.BLOCK[t][0] == 256 else (n_in + 7 if name in ("f16", "f32") else n_in)    # f16 / f32: 7 leftover elements go through the double tail
            raw = Q.quantize(t, (0.05 * rng.standard_normal((n_out, k))).astype(np.float32))
            x = (rng.standard_normal((3, k)) * np.array([1.0, 37.0, 1e-3])[:, None]).astype(np.float32)
            L.orc_set_order(0)
            a = R.mul_mat(t, raw, k, n_out, x)
            L.orc_set_order(1)
            b = R.mul_mat(t, raw, k, n_out, x)
            L.orc_set_simd(0)
            c = R.mul_mat(t, raw, k, n_out, x)
            L.orc_set_simd(1)
            assert np.array_equal(b, c), name                                   # AVX2 lanes == scalar lanes
            scale = np.abs(a).max(axis=1, keepdims=True)
            assert (np.abs(a - b) <= 1e-5 * scale).all(), (name, float((np.abs(a - b) / scale).max()))
            assert not np.array_equal(a, b), name                               # ... and the orders are really different additions
        _, llm = tiny_files
        f = G.read_llm_file(llm("q5_k", "q5_k_m", conditioned=True))
        toks = [1, 5, 300, 44, 270, 99, 400, 17]
        L.orc_set_order(0)
        l0 = R.OracleLLM(f, n_ctx=32).eval_tokens(toks)
        L.orc_set_order(1)
        l1 = R.OracleLLM(f, n_ctx=32).eval_tokens(toks)
        spread = float(np.abs(l0 - l1).max() / np.abs(l0).max())
        assert 0.0 < spread < 1e-3, spread
    finally:
        L.orc_set_order(0)
        L.orc_set_simd(1)


# ------------------------------------------------------------------------------------------------ tokenizer / sampler / templating
def test_tokenizer_matches_oracle(lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    _, llm = tiny_files
    lp = llm("q4_0")
    vocab = G.read_llm_file(lp).vocab
    v = lib.library.minigpt4_amd_vocab_load(lp.encode())
    assert v and lib.library.minigpt4_amd_vocab_size(v) == 512
    texts = [G.SYSTEM_PROMPT.encode(), b"Human: <Img>", b"</Img> ", b"### Assistant:", b"Human: ", b"what is the text in the picture?", b"", b" ", b"###",
             "héllo 世界 \U0001F600".encode(), bytes(range(1, 128)), b"aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", b"the the  the   the"]
    for t in texts:
        for bos in (True, False):
            out = (ctypes.c_int32 * (len(t) + 4))()
            n = lib.library.minigpt4_amd_vocab_tokenize(v, t, int(bos), out, len(t) + 4)
            want = R.tokenize(vocab, t, bos)
            assert list(out[:n]) == want, t
            # decoding the pieces gives back the text (byte-fallback ids are byte + 3)
            dec = b"".join(vocab[i][0] for i in want if i != 1 or not bos)
            assert dec == t
    # llama_tokenize returns nothing for an empty text, BOS included (llama.cpp master-31cfbb1: `if (text.empty()) return output;` precedes the BOS push)
    out = (ctypes.c_int32 * 4)()
    assert lib.library.minigpt4_amd_vocab_tokenize(v, b"", 1, out, 4) == 0 and R.tokenize(vocab, b"", True) == []
    lib.library.minigpt4_amd_vocab_free(v)


def test_greedy_and_sampler_chain_match_oracle(lib):
    import refcpu as R
    rng = np.random.default_rng(0)
    for trial in range(6):
        logits = (2.5 * rng.standard_normal(512)).astype(np.float32)
        assert lib.amd_sample_logits(logits, seed=1, temp=0.0) == int(np.argmax(logits))
        logits[[7, 100]] = logits.max() + 1.0      # tie: first maximum wins (llama_sample_token_greedy)
        assert lib.amd_sample_logits(logits, seed=1, temp=-1.0) == 7
        logits[100] -= 0.5                         # (ties inside std::sort are implementation-defined: keep the chain comparison tie-free)
        for kw in (dict(temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0), dict(temp=1.3, top_k=0, top_p=0.5, tfs_z=1.0, typical_p=1.0),
                   dict(temp=0.7, top_k=50, top_p=1.0, tfs_z=0.9, typical_p=1.0), dict(temp=1.0, top_k=20, top_p=0.95, tfs_z=1.0, typical_p=0.8)):
            seed = 1337 + trial
            got = lib.amd_sample_logits(logits, seed=seed, **kw)
            want = R.sample(logits, R.MT19937(seed), kw["temp"], kw["top_k"], kw["top_p"], kw["tfs_z"], kw["typical_p"])
            assert got == want, (trial, kw)
    # a full-size vocabulary through the whole-vocabulary sort (top_k = 0: every candidate is ordered; >= 1024 entries take the radix passes): negative values, +-0,
    # denormals and exact TIES -- equal logits keep their token order, the oracle's (stable) rule
    big = (2.5 * rng.standard_normal(32000)).astype(np.float32)
    big[5] = 0.0; big[6] = -0.0; big[7] = np.float32(1e-41); big[8] = np.float32(-1e-41)
    top = np.argsort(-big)[:6]
    big[top[1]] = big[top[0]]; big[top[3]] = big[top[2]]            # ties among the most probable tokens
    big[31999] = big[top[4]]
    for seed, kw in ((11, dict(temp=1.3, top_k=0, top_p=0.5, tfs_z=1.0, typical_p=1.0)), (12, dict(temp=0.9, top_k=0, top_p=0.97, tfs_z=1.0, typical_p=1.0)),
                     (13, dict(temp=1.0, top_k=0, top_p=1.0, tfs_z=0.95, typical_p=1.0)), (14, dict(temp=2.0, top_k=32000, top_p=0.999, tfs_z=1.0, typical_p=1.0))):
        for s2 in range(4):
            got = lib.amd_sample_logits(big, seed=seed * 10 + s2, **kw)
            want = R.sample(big, R.MT19937(seed * 10 + s2), kw["temp"], kw["top_k"], kw["top_p"], kw["tfs_z"], kw["typical_p"])
            assert got == want, (seed, s2, kw)
    # mirostat paths run and return a valid id
    lg = (2.5 * rng.standard_normal(512)).astype(np.float32)
    for m in (1, 2):
        assert 0 <= lib.amd_sample_logits(lg, seed=3, temp=0.8, mirostat=m) < 512


def test_mt19937_restatement_matches_numpy_stream():
    import refcpu as R
    r = R.MT19937(1337)
    rs = np.random.RandomState(1337)
    assert [r.u32() for _ in range(4)] == [int(x) for x in rs.randint(0, 2 ** 32, 4, dtype=np.uint64)]


# ------------------------------------------------------------------------------------------------ ABI surface
def _declared_symbols(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", txt)))


def _exported(so):
    return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))


def test_library_exports_every_declared_symbol(lib):
    """libminigpt4.so (what ships) exports EXACTLY what include/minigpt4.h + include/minigpt4_amd.h declare -- the reference's 18 functions and the serving / measurement /
    multi-GPU hooks -- and none of the kernel-level test hooks, micro-benchmarks or probes; those are include/minigpt4_amd_test.h, exported by libminigpt4_test.so only."""
    product = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so"))
    test = _exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    ref = _declared_symbols("minigpt4.h")
    assert len(ref) == 18, ref                       # the reference exports exactly 18 functions (minigpt4.h:97-114)
    declared = set(ref + _declared_symbols("minigpt4_amd.h"))
    hooks = set(_declared_symbols("minigpt4_amd_test.h")) - declared
    assert product == declared, (sorted(declared - product), sorted(product - declared))
    assert len(hooks) >= 20 and not (hooks & product), sorted(hooks & product)
    assert test == declared | hooks, (sorted((declared | hooks) - test), sorted(test - (declared | hooks)))
    assert not [s for s in product if "_test_" in s or "_probe_" in s or "_bench_" in s]


def test_abi_struct_layouts_and_constants(lib):
    from minigpt4_cpp_amd import minigpt4_library as ML
    assert ctypes.sizeof(ML.MiniGPT4Image) == 24 and ctypes.sizeof(ML.MiniGPT4Embedding) == 16
    assert ML.MiniGPT4Image.format.offset == 20 and ML.MiniGPT4Embedding.n_embeddings.offset == 8
    names = ["None", "LoadModelFileHeader", "LoadModelFileVersion", "LoadModelMiniGPT4DataType", "LoadLanguageModel", "OpenImage", "ImageSize", "MmapSupport",
             "FailedToAddString", "LLamaProjectionEmbeddingInvalidSize", "FailedToAddEmbedding", "EosToken", "Eos", "ImageNot224_244_3", "ImageNotF32",
             "ImageChannelsExpectedRGB", "ImageFormatExpectedU8", "PathDoesNotExist", "DumpModelFileOpen", "OpenCVNotLinked"]
    assert [lib.minigpt4_error_code_to_string(i) for i in range(20)] == names
    assert lib.minigpt4_contains_eos_token("##") and not lib.minigpt4_contains_eos_token("###") and not lib.minigpt4_contains_eos_token("a##")
    assert lib.minigpt4_is_eos("hello###") and not lib.minigpt4_is_eos("hello##") and not lib.minigpt4_is_eos("")
    assert lib.library.minigpt4_contains_eos_token(b"##") == 11 and lib.library.minigpt4_is_eos(b"x###") == 12
    img = ML.MiniGPT4Image()
    assert lib.library.minigpt4_image_load_from_file(None, b"x.png", ctypes.byref(img), 0) == 17     # native loader (tests/test_cpu_image.py): missing file
    assert lib.library.minigpt4_preprocess_image(None, ctypes.byref(img), ctypes.byref(img), 0) == 6  # no pixel data
    assert lib.library.minigpt4_quantize_model(b"/nonexistent", b"/tmp/o", 4) == 17
    assert lib.library.minigpt4_free(None) == 0


def test_model_load_fails_loudly_without_gpu_or_files(lib, tiny_files):
    vp, llm = tiny_files
    assert not lib.library.minigpt4_model_load(b"/nonexistent", llm("q4_0").encode(), 0, 1, 64, 32, False)
    if lib.amd_device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device|failed"):
            lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=0)


def test_reference_binding_binds_unmodified(lib):
    """Drop-in check: every symbol the reference's own ctypes wrapper declares (tests/golden/reference_binding.json) resolves against this library
    and answers through the wrapper's declarations (tests/ref_abi.py, equal to the recorded ones: tests/test_cpu_refwrapper.py)."""
    import json
    import ref_abi
    decl = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_binding.json")))["declarations"]
    so = os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so")
    raw = ctypes.cdll.LoadLibrary(so)
    for name in decl:
        assert getattr(raw, name) is not None, name
    wrapper = ref_abi.bind(so)
    assert wrapper.minigpt4_contains_eos_token(ref_abi.cstr("##")) and wrapper.minigpt4_is_eos(ref_abi.cstr("abc###"))
    # (the reference's own minigpt4_error_code_to_string wrapper calls .decode() on a POINTER(c_char) and raises; use the raw symbol)
    assert ctypes.cast(wrapper.minigpt4_error_code_to_string(19), ctypes.c_char_p).value == b"OpenCVNotLinked"


def test_request_sharding_is_disjoint_and_complete():
    from minigpt4_cpp_amd import dist
    for world in (1, 2, 8):
        seen = []
        for r in range(world):
            seen += dist.shard_requests(32, r, world)
        assert sorted(seen) == list(range(32))
    assert dist.shard_requests(32, 3, 8) == [3, 11, 19, 27]


def test_bench_line_is_reproducible_from_committed_profiles():
    """Round-1 verdict item 5: the roofline fraction of the bench line must be recomputable from profiles/.  The committed rocprofv3 --kernel-trace --stats summary of
    the eager decode run and the bench line's own kernel table (per-dispatch event pairs) must agree on the dominant kernel's average duration, the traffic record
    must name its source, and the per-kernel table must add up to the step time."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = json.loads([l for l in open(os.path.join(root, "profiles", "r02_bench_n1.json")) if l.lstrip().startswith("{")][-1])
    roof = bench["roofline"]
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "roofline_from_profile.py"), "stats", os.path.join(root, "profiles", "r02_decode_kernel_stats.csv"),
                          os.path.join(root, "profiles", "r02_bench_n1.json")], capture_output=True, text=True, check=True).stdout
    row = [l for l in out.splitlines() if l.startswith(roof["kernel"])][0].split("|")[0].split()
    frac_rocprof = float(row[-1])
    assert abs(frac_rocprof - roof["frac"]) < 0.05 * roof["frac"], (frac_rocprof, roof["frac"])
    assert roof["timing"] == "dispatch" and roof["bound"] == "hbm" and abs(roof["achieved"] / roof["peak"] - roof["frac"]) < 1e-9
    traffic = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    # (the bench line read the record of the previous FETCH_SIZE pass; passes agree to 0.01 %)
    assert "FETCH_SIZE" in traffic["command"] and abs(traffic["kernels"][roof["kernel"]]["bytes_per_launch"] / roof["traffic"] - 1.0) < 1e-3
    assert 0.98 < roof["traffic"] / roof["bytes_per_launch"] < 1.05                       # measured HBM bytes vs algorithmic bytes: no re-reads
    assert abs(roof["kernel_sum_ms_per_token"] - bench["ms_per_step"]) < 0.06 * bench["ms_per_step"]
    assert bench["parity"]["oracle_self_noise"]["mean_logit_rel_range"] * 1.5 >= bench["parity"]["mean_logit_rel_range"]


def test_pmc_summary_mfma_busy_is_per_xcd(tmp_path):
    """tools/pmc_summary.py: SQ_VALU_MFMA_BUSY_CYCLES is summed over the 1024 SIMDs, GRBM_GUI_ACTIVE over the 8 XCDs (round 1 forgot the / 8 and printed utilisations
    8 x too small); FETCH_SIZE is in KB and counts half of the streamed bytes on gfx950."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, dst = tmp_path / "cc.csv", tmp_path / "out.csv"
    rows = ["Kernel_Name,Counter_Name,Counter_Value"]
    for _ in range(3):
        rows += ['"void mg4::k(int)",GRBM_GUI_ACTIVE,80000', '"void mg4::k(int)",SQ_VALU_MFMA_BUSY_CYCLES,2560000', '"void mg4::k(int)",FETCH_SIZE,1000']
    src.write_text("\n".join(rows) + "\n")
    subprocess.run([sys.executable, os.path.join(root, "tools", "pmc_summary.py"), str(src), str(dst), "test"], check=True, capture_output=True)
    line = [l for l in dst.read_text().splitlines() if l.startswith('"void')][0].split(",")
    head = [l for l in dst.read_text().splitlines() if l.startswith("kernel,")][0].split(",")
    rec = dict(zip(head, line))
    assert abs(float(rec["mfma_busy_frac"]) - 2560000 / (80000 / 8 * 1024)) < 1e-4          # = 0.25
    assert abs(float(rec["avg_hbm_read_MB_corrected"]) - 1000 * 1024 * 2 / 1e6) < 1e-2
